"""The constitutive kernels against the long-double restatement of the material law (constitutive_reference.py), on an
MI355X, at the states of constitutive_cases.py: large volumetric strain on both sides of every branch of fd_log, the
identity limit, rotated stretch and shear, a rigid motion, curved elements, nearly incompressible and lambda = 0
materials, a material table, bodies of size 1e-3 and 1e3 and far from the origin -- linear tetrahedra, 10-node
tetrahedra at 4, 5 and 27 points, 8-node bricks, both models.

Every assembly strategy the element type takes, the separate entry points, the state export, the results (strain
energy, nodal stress) and the geometric stiffness product evaluate the law in their own algebra (fem_device.h,
gather_device.h, kernels_quad.hip, kernels_gather10.hip, kernels_results.hip, kernels_buckling.hip); each is compared
with the same reference, by a yardstick that a small quantity cannot hide behind a large one:

  K        every entry against the largest entry of the reference's block row
  f        every entry against its cancellation scale: the sum of |terms| the entry is the difference of
  F, g     against their own largest entry at the Gauss point;  det J against itself
  sigma    against the stress scale of the Gauss point (largest entry of the entrywise sum of |terms|)
  W        against sum vol0 |Psi terms|
  nodal    the volume-weighted average against the same average of the stress scale
  K_s v    every entry against (|K_sigma| |v|); at the stress-free states, where that is rounding, against the
           cancellation scale of K_sigma times |v|

Tolerance, for every comparison: 100 times the float64-to-long-double gap of the restatement for that quantity, that
case and that yardstick, at least 1e-13, at most 1e-10 (tests/test_gpu_pcg.py's rule).  Nothing is measured against
the code under test.  The reference of a case is computed once (constitutive_cases.reference) and the tests of a case
run together (a module-scoped parametrised fixture), about 0.5 s per test."""
import numpy as np
import pytest

import constitutive_cases as cc
import constitutive_reference as cr
import feahip

pytestmark = pytest.mark.gpu

NH, A5 = feahip.MODEL_COMPRESSIBLE_NEOHOOKEAN, feahip.MODEL_A5
ELE = {"tet4": feahip.TETRAHEDRA4, "tet10": feahip.TETRAHEDRA10, "hex8": feahip.HEXAHEDRA8}
STRATEGIES = {"auto": feahip.ASM_AUTO, "rowowner": feahip.ASM_ROWOWNER, "atomic": feahip.ASM_ATOMIC,
              "staged": feahip.ASM_STAGED, "shared": feahip.ASM_SHARED, "gather": feahip.ASM_GATHER}
SIG6 = ((0, 0), (1, 1), (2, 2), (0, 1), (1, 2), (0, 2))
CASES = [(kind, G, model, name) for kind, G in cc.ELEMENT_TYPES for model in (NH, A5) for name in cc.STATES]


def required_strategies(kind, G, table):
    """What test_gpu_parity.check_assembly runs on this element type -- its default pair, the staged visits and the
    gather kernel for linear tetrahedra with one point, the shared-state and the gather kernel for 10-node ones
    (a material table takes neither the staged visits nor the shared-state kernel: both are refused with one) -- and
    AUTO.  Every case asserts it of itself, so a selection of cases (-k) asserts as much as the whole file."""
    need = {feahip.ASM_AUTO, feahip.ASM_ROWOWNER, feahip.ASM_ATOMIC}
    if kind == "tet4" and G == 1:
        need |= {feahip.ASM_GATHER} | (set() if table else {feahip.ASM_STAGED})
    if kind == "tet10":
        need |= {feahip.ASM_GATHER} | (set() if table else {feahip.ASM_SHARED})
    return need


def case_id(p):
    return f"{p[0]}-{p[1]}-{'nh' if p[2] == NH else 'a5'}-{cc.FAMILY_OF[p[3]]}-{p[3]}"


@pytest.fixture(scope="module", params=CASES, ids=case_id)
def case(request):
    """(the cached reference of the case, a context at its state); the tests of one case run one after the other."""
    c = cc.reference(*request.param)
    st = c.st
    kw = dict(materials=st.materials, element_material=st.ids) if st.table else dict(parameters=list(st.materials[0]))
    deck = feahip.Deck(nodes=st.X0, elements=st.conn, ele_type=ELE[c.kind], gauss_nodes_count=c.G, model=c.model, **kw)
    s = feahip.FeaSolver(deck)
    s.set_nodes(st.x)
    yield c, s
    s.close()


def dense(s):
    off, idx, val = s.matrix_yale()
    K = np.zeros((s.ndof, s.ndof))
    K[np.repeat(np.arange(s.ndof), np.diff(off)), idx] = val
    return K


def held(what, err, gap):
    tol = cr.tolerance(gap)
    print(f"{what}: error {err:.2e}, gap {gap:.1e}, tolerance {tol:.1e}, ratio {err / tol:.2f}")
    return err <= tol


def check_k(c, s, what):
    return held(f"{what} K", cr.err_block_rows(dense(s), c.hi.K), c.gap["K"])


def check_f(c, s, what):
    return held(f"{what} f", cr.err_scaled(s.forces(), c.hi.f, c.hi.fscale), c.gap["f"])


def test_k_and_f_by_every_strategy(case):
    c, s = case
    ran, bad = set(), []
    for sname, strat in STRATEGIES.items():
        s.set_assembly(strat)
        try:
            s.create_stiffness_and_residual()
        except feahip.FeaHipError as e:                       # a strategy this element type / material form does not take
            print(f"{sname}: refused ({e})")
            continue
        used = s.assembly_in_use()
        assert strat == feahip.ASM_AUTO or used == strat, (sname, used)
        ran |= {strat}
        print(f"{sname}: ran strategy {used}")
        if not check_k(c, s, sname) or not check_f(c, s, sname):
            bad.append(sname)
    s.set_assembly(feahip.ASM_AUTO)
    need = required_strategies(c.kind, c.G, c.st.table)
    assert need <= ran, (sorted(need), sorted(ran))
    assert not bad, bad


def test_separate_entry_points(case):
    """create_stiffness and create_residual_forces: the residual-only records are other code (DOK = false), and the
    residual alone falls back from the shared-state kernel to the generic visits."""
    c, s = case
    ran, bad = set(), []
    generic = {feahip.ASM_ROWOWNER, feahip.ASM_ATOMIC}
    for sname, strat in STRATEGIES.items():
        s.set_assembly(strat)
        try:
            s.create_stiffness()
        except feahip.FeaHipError as e:
            print(f"{sname}: refused ({e})")
            continue
        used = s.assembly_in_use()
        assert strat == feahip.ASM_AUTO or used == strat, (sname, used)
        ran |= {strat}
        k_ok = check_k(c, s, f"{sname} create_stiffness (strategy {used})")
        s.set_forces(np.full(s.ndof, np.nan))                 # nothing of an earlier assembly is left to be read
        s.create_residual_forces()
        fused = s.assembly_in_use()
        assert fused == used or (used == feahip.ASM_SHARED and fused in generic), (sname, used, fused)
        if not k_ok or not check_f(c, s, f"{sname} create_residual_forces (strategy {fused})"):
            bad.append(sname)
    s.set_assembly(feahip.ASM_AUTO)
    need = required_strategies(c.kind, c.G, c.st.table)
    assert need <= ran, (sorted(need), sorted(ran))
    assert not bad, bad


def test_state_export(case):
    c, s = case
    el = c.hi.el
    g, dj = s.shape_gradients()
    ok = [held("F", cr.err_own_max(s.graddefs(), el.F, 2), c.gap["F"]),
          held("sigma", cr.err_scaled(s.stresses(), el.sig, c.sig_scale), c.gap["sigma"]),
          held("shape gradients", cr.err_own_max(np.swapaxes(g, -1, -2), el.g, 2), c.gap["g"]),
          held("det J", cr.err_scaled(dj, el.detJ, np.abs(el.detJ)), c.gap["detJ"])]
    assert all(ok), ok


def test_results(case):
    c, s = case
    ok = [held("strain energy", cr.err_scaled(s.strain_energy(), c.hi.W, c.hi.Wscale), c.gap["W"])]
    for m, _ in cc.selections(c.st):
        ref, scale, wt = c.nodal[m]
        sig6, _, weight = s.nodal_stresses(m)
        ref6 = np.stack([ref[:, i, j] for i, j in SIG6], axis=1)
        ok.append(held(f"nodal stress, material {m}", cr.err_scaled(sig6, ref6, scale[:, :, 0]), c.gap["nodal", m]))
        ok.append(held(f"nodal weight, material {m}", cr.err_scaled(weight, wt, np.where(wt > 0, wt, 1)), c.gap["detJ"]))
    assert all(ok), ok


def test_geometric_stiffness_product(case):
    c, s = case
    key, scale = ("Ksigma_c", c.ksv_cscale) if c.name in cc.KSIGMA_NOT_ADMITTED else ("Ksigma", c.ksv_scale)
    ok = [held(f"K_sigma v{k} ({key})", cr.err_scaled(s.geometric_spmv(c.v[k]), c.ksv[k], scale[k]), c.gap[key])
          for k in range(cc.VECTORS)]
    assert all(ok), ok

"""The long-double restatement of the material law (constitutive_reference.py) checked on the CPU, at every state of
constitutive_cases.py and every element type, before test_gpu_constitutive.py holds the kernels to it:

  oracle       its float64 run is the project's law: the oracle's element stiffness, residual, F and sigma
  gap          its float64 run against its long-double run, by every yardstick the kernels are measured with; printed,
               and small enough for the state to be admitted (100 x gap under 1e-10, every Gauss point the right way round)
  closed form  the volumetric states' stress in long double
  objectivity  K(Qx) = Q K(x) Q' blockwise, f(Qx) = Q f(x), in long double
  tangent      Neo-Hookean: K is the central difference of f in long double

Tolerances.  Oracle: the rule of the GPU tests, 100 x gap clamped to [1e-13, 1e-10] -- the oracle is float64 arithmetic
in another order, as a kernel is.  Closed form: 1e-17 relative (about 100 long-double eps); at J = 1 -+ 1e-9, where the
stress is itself a difference of O(mu) terms, 1e-17 of the stress scale; on element-local coordinates for every
element type (the undifferenced 10-node sums lose |x| / cell = 30 of their digits and sit at 1e-17 .. 3e-17).  Objectivity: both sides are
long-double runs, whose rounding is the float64 run's scaled by eps_ld / eps_64 = 4.9e-4; so the rule again, 100 x gap
x 4.9e-4 of the row scale / the residual's cancellation scale, at least 1e-17 (100 long-double eps).  The offset states
are turned about their own translation (Q does not leave the translation alone).  Tangent: 1e-8 of the block row's largest
entry, on the assembled matrices; the central difference with h = 1e-9 cell has a truncation error of h^2 and a
rounding error of eps / h = 1e-10 of the residual's scale in long double.  The differences are taken on element-local
coordinates (every element's nodes minus its first, exact in long double: the law does not see a translation), or the
|x| / cell digits the undifferenced sums lose would be lost to the quotient as well."""
import numpy as np
import pytest

import constitutive_cases as cc
import constitutive_reference as cr
import feahip
from oracle_binding import OracleSolver

NH, A5 = feahip.MODEL_COMPRESSIBLE_NEOHOOKEAN, feahip.MODEL_A5
assert (NH, A5) == (cr.NH, cr.A5)
ELE = {"tet4": feahip.TETRAHEDRA4, "tet10": feahip.TETRAHEDRA10, "hex8": feahip.HEXAHEDRA8}
LD = np.longdouble
CLOSED_TOL, OBJECTIVE_FLOOR, TANGENT_TOL = 1e-17, 1e-17, 1e-8
EPS_RATIO = float(np.finfo(LD).eps) / np.finfo(np.float64).eps      # 4.9e-4: a long-double run's rounding beside a float64 run's

etype = pytest.mark.parametrize("kind,G", cc.ELEMENT_TYPES, ids=[f"{k}-{g}" for k, g in cc.ELEMENT_TYPES])
models = pytest.mark.parametrize("model", [NH, A5], ids=["nh", "a5"])


def test_every_family_has_every_element_type():
    kinds = {k for k, _ in cc.ELEMENT_TYPES}
    assert kinds == {"tet4", "tet10", "hex8"}
    assert all(len(names) >= 1 for names in cc.FAMILIES.values()) and len(cc.STATES) == 23
    for name in cc.STATES:                                    # no state is built for fewer types than that
        for kind in kinds:
            assert cc.state(kind, name).x.shape == cc.block(kind)[0].shape


def test_gauss_rules_are_the_host_library_s():
    """The points read back from the host tables reproduce its derivative table through the written-out derivatives."""
    for kind, G in cc.ELEMENT_TYPES:
        import oracle_binding as ob
        w, pts = ob.gauss_rule(kind, G)
        _, _, dforms = feahip.element_tables(ELE[kind], G)
        mine = cr.shape_derivatives(kind, pts, np.float64)
        assert np.abs(mine - dforms).max() <= 4e-16 * np.abs(dforms).max(), (kind, G)
        assert abs(w.sum() - (1.0 if kind == "hex8" else 1 / 6)) < 1e-15


def oracle_assembly(st, kind, G, model):
    """(K dense, f, F, sigma) from the oracle's element matrices, every element by the solver of its material."""
    solvers = []
    for lam, mu in st.materials:
        d = feahip.Deck(nodes=st.X0, elements=st.conn, ele_type=ELE[kind], gauss_nodes_count=G, model=model,
                        parameters=[lam, mu])
        o = OracleSolver(d)
        o.set_nodes(st.x)
        assert o.update_state() == 0
        solvers.append(o)
    N = len(st.X0)
    K, f = np.zeros((3 * N, 3 * N)), np.zeros(3 * N)
    F, S = np.empty_like(solvers[0].graddefs()), np.empty_like(solvers[0].stresses())
    dofs = cr.dofs_of(st.conn)
    for e in range(len(st.conn)):
        o = solvers[st.ids[e]]
        kc, ks = o.element_stiffness(e)
        K[np.ix_(dofs[e], dofs[e])] += kc + ks
        f[dofs[e]] += o.element_residual(e)
        F[e], S[e] = o.graddefs()[e], o.stresses()[e]
    grads, detj = solvers[0].grads().copy(), solvers[0].detj().copy()
    for o in solvers:
        o.close()
    return K, f, F, S, grads, detj


@pytest.mark.parametrize("name", cc.STATES)
@models
@etype
def test_float64_run_is_the_oracle_and_the_state_is_admitted(kind, G, model, name):
    c = cc.reference(kind, G, model, name)
    st, hi, lo = c.st, c.hi, c.lo
    print(f"gap {kind}/{G} {'nh' if model == NH else 'a5'} {name}: " + " ".join(f"{k}={v:.1e}" for k, v in c.gap.items())
          + f" | det J min {c.detJ_min:.3g} det F [{c.detF_min:.4g}, {c.detF_max:.4g}]")
    allowed = ({"Ksigma"} if name in cc.KSIGMA_NOT_ADMITTED else set()) | \
              ({"sigma"} if (kind, model, name) in cc.SIGMA_OVER_CEILING else set())
    bad = cc.not_admitted(c)
    assert bad <= allowed and ("Ksigma" in bad) == ("Ksigma" in allowed), (bad, c.gap, c.detJ_min, c.detF_min)
    K, f, F, S, grads, detj = oracle_assembly(st, kind, G, model)
    gap = c.gap
    if kind == "tet4":
        # The oracle sums the formulas undifferenced; the linear tetrahedron's restatement subtracts first, as its
        # kernels do.  So the oracle is met by the undifferenced form of the restatement, with that form's own gap,
        # and the two forms are the same law: they agree in long double to that gap scaled by eps_ld / eps_64.
        lo, hu = (cr.run(kind, G, st.conn, st.X0, st.x, st.materials, st.ids, model, dt, local=False) for dt in (np.float64, LD))
        gap = {"K": cr.err_block_rows(lo.K, hu.K), "f": cr.err_scaled(lo.f, hu.f, hu.fscale),
               "F": cr.err_own_max(lo.el.F, hu.el.F, 2), "g": cr.err_own_max(lo.el.g, hu.el.g, 2),
               "detJ": cr.err_scaled(lo.el.detJ, hu.el.detJ, np.abs(hu.el.detJ)),
               "sigma": cr.err_scaled(lo.el.sig, hu.el.sig, c.sig_scale)}
        same = {"K": cr.err_block_rows(hu.K, hi.K), "f": cr.err_scaled(hu.f, hi.f, hi.fscale),
                "sigma": cr.err_scaled(hu.el.sig, hi.el.sig, c.sig_scale)}
        for k, e in same.items():
            bound = max(100.0 * gap[k] * EPS_RATIO, OBJECTIVE_FLOOR)
            print(f"  differenced against undifferenced, long double, {k}: {e:.1e} (bound {bound:.1e})")
            assert e <= bound, (k, e, bound)
    got = {"K": cr.err_block_rows(K, lo.K), "f": cr.err_scaled(f, lo.f, cr.f64(hi.fscale)),
           "F": cr.err_own_max(F, lo.el.F, 2), "g": cr.err_own_max(np.swapaxes(grads, -1, -2), lo.el.g, 2),
           "detJ": cr.err_scaled(detj, lo.el.detJ, np.abs(lo.el.detJ)),
           "sigma": cr.err_scaled(S, lo.el.sig, cr.f64(c.sig_scale))}
    for k, e in got.items():
        tol = cr.tolerance(gap[k])
        print(f"  oracle {k}: {e:.2e} (gap {gap[k]:.1e}, tolerance {tol:.1e})")
        assert e <= tol, (k, e, tol)


VOLUMETRIC = cc.FAMILIES["volumetric"] + [n for n in cc.STATES if n.startswith("mat_1e6_1_J")]


@pytest.mark.parametrize("name", VOLUMETRIC)
@models
@etype
def test_volumetric_stress_is_the_closed_form(kind, G, model, name):
    st = cc.state(kind, name, LD)
    r = cr.run(kind, G, st.conn, st.X0, st.x, st.materials, st.ids, model, LD, need_k=False, local=True)
    lam, mu = LD(st.materials[0][0]), LD(st.materials[0][1])
    c = np.cbrt(LD(cc.VOLUMETRIC_J[name.split("_")[-1]]))     # F = c I
    J = c * c * c
    if model == NH:
        p = (mu * (c * c - 1) + lam * np.log(J)) / J
    else:
        p = c * c * (3 * lam + 2 * mu) * (c * c - 1) / 2 / J  # F (lambda tr E + 2 mu E) F' / J, E = (c^2 - 1)/2 I
    identity_limit = name in ("J1-1e-9", "J1+1e-9")
    scale = cc.point_scale(r.el.sscale) if identity_limit else abs(p)
    err = cr.err_scaled(r.el.sig, p * np.eye(3, dtype=LD), scale)
    print(f"{kind}/{G} model {model} {name}: sigma = {float(p):.6e} I, error {err:.1e} "
          f"{'of the stress scale' if identity_limit else 'relative'}")
    assert err <= CLOSED_TOL


@pytest.mark.parametrize("name", cc.STATES)
@models
@etype
def test_objectivity_in_long_double(kind, G, model, name):
    st = cc.state(kind, name, LD)
    if name == "offset":                                      # turn about the translation, not about the origin
        shift = LD(cc.OFFSET[kind])
        st = cc.State(kind, name, st.conn, st.X0 - shift, st.x - shift, st.materials, st.ids)
    sq, Q = cc.rotated(st)
    a = cr.run(kind, G, st.conn, st.X0, st.x, st.materials, st.ids, model, LD)
    b = cr.run(kind, G, sq.conn, sq.X0, sq.x, sq.materials, sq.ids, model, LD)
    N = a.N
    Ka = a.K.reshape(N, 3, N, 3)
    QKQ = np.einsum("ik,akbl,jl->aibj", Q, Ka, Q)             # (object-loop einsum: plain long-double sums, no BLAS)
    ek = cr.err_block_rows(b.K, QKQ.reshape(3 * N, 3 * N))
    Qf = cc.apply(Q, a.f.reshape(N, 3)).ravel()
    scale = np.maximum(a.fscale.reshape(N, 3).max(axis=1), b.fscale.reshape(N, 3).max(axis=1))
    ef = cr.err_scaled(b.f.reshape(N, 3), Qf.reshape(N, 3), scale[:, None])
    gap = cc.reference(kind, G, model, name).gap
    tk, tf = (max(100.0 * gap[q] * EPS_RATIO, OBJECTIVE_FLOOR) for q in ("K", "f"))
    print(f"{kind}/{G} model {model} {name}: K(Qx) - Q K Q' {ek:.1e} of the row (tolerance {tk:.1e}), "
          f"f(Qx) - Q f {ef:.1e} of its scale (tolerance {tf:.1e})")
    assert ek <= tk and ef <= tf


@pytest.mark.parametrize("name", cc.STATES)
@etype
def test_neo_hookean_tangent_is_the_derivative_of_the_residual(kind, G, name):
    """K = -df/dx by central differences in long double: one local dof of every element at a time, the element
    quotients assembled and compared with the assembled K."""
    st = cc.state(kind, name)
    conn = st.conn
    Xe, xe = np.asarray(st.X0, dtype=LD)[conn], np.asarray(st.x, dtype=LD)[conn]
    Xe, xe = Xe - Xe[:, :1, :], xe - xe[:, :1, :]
    lam, mu = st.materials[st.ids, 0], st.materials[st.ids, 1]
    Ke = cr.evaluate(kind, G, Xe, xe, lam, mu, NH, LD).Ke                                    # [E][a][i][b][j]
    h = LD(1e-9) * LD(st.cell)
    npe = conn.shape[1]
    De = np.empty_like(Ke)
    for b in range(npe):
        for j in range(3):
            xp, xm = xe.copy(), xe.copy()
            xp[:, b, j] += h
            xm[:, b, j] -= h
            fp = cr.evaluate(kind, G, Xe, xp, lam, mu, NH, LD, need_k=False).fe
            fm = cr.evaluate(kind, G, Xe, xm, lam, mu, NH, LD, need_k=False).fe
            De[:, :, :, b, j] = -(fp - fm) / (2 * h)
    n = 3 * len(st.X0)
    d = cr.dofs_of(conn)
    rows, cols = np.repeat(d, 3 * npe, axis=1).ravel(), np.tile(d, (1, 3 * npe)).ravel()
    K, D = np.zeros((n, n), dtype=LD), np.zeros((n, n), dtype=LD)
    np.add.at(K, (rows, cols), Ke.reshape(-1))
    np.add.at(D, (rows, cols), De.reshape(-1))
    err = cr.err_block_rows(D, K)
    print(f"{kind}/{G} {name}: |K + df/dx| = {err:.1e} of the block row's largest entry")
    assert err <= TANGENT_TOL

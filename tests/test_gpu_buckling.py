"""Linear buckling on the MI355X (kernels_buckling.hip): the geometric stiffness of k_geom_elements / k_geom_blocks against
the oracle's dense K_sigma, feahip_solve_buckling against scipy.linalg.eigh on the oracle's (K_sigma, K)
(tests/buckling_reference.py), a load path under a dead traction, both preconditioners, what the solve leaves alone and
what it refuses, and the (buckling ...) section of a deck through feasolver_hip.

Rayleigh-Ritz steps for six modes to 1e-8 under block-Jacobi, MI355X beside the float64 emulation (EMULATED): see the
output of test_eigenvalues_match_the_dense_reference and DESIGN.md section 17."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import buckling_reference as br
import feahip
import mesh
from hetero_reference import MATERIALS, layered_ids, with_materials
from modal_reference import ModalReference
from test_gpu_modal import _fan_deck

pytestmark = pytest.mark.gpu

TOL, MAX_IT, N_MODES = 1e-8, 2000, 6
KINDS = ("tet4", "hex8", "tet10")
EMULATED = {"tet4": 157, "hex8": 161, "tet10": 183}        # steps of BucklingReference.emulate (test_buckling_reference_cpu)


@functools.lru_cache(maxsize=None)
def solved(kind):
    """One load increment of full Newton on the library, the float64 reference at the nodes it reached, and one buckling
    solve of six modes there: computed once per deck and read-only."""
    deck = br.column_deck(kind)
    s = feahip.FeaSolver(deck)
    done, _, _ = s.solve(load_increments=1)
    assert done == 1
    x = s.nodes()
    fac, nu, res, it = s.solve_buckling(N_MODES, TOL, MAX_IT)
    phi = s.buckling_modes()
    s.close()
    ref = br.BucklingReference(deck, x)
    print(kind, "nodes against the oracle's Newton state", np.abs(x - br.column_reference(kind)[1]).max())
    for a in (fac, nu, res, phi, ref.nu, ref.Phi, ref.K, ref.Ksig):
        a.setflags(write=False)
    return dict(fac=fac, nu=nu, res=res, it=it, phi=phi, ref=ref)


def check_eigenvalues(fac, nu, res, ref, tol=TOL):
    n = len(nu)
    want = ref.nu[:n]
    print("nu", nu, "rel err", np.abs(nu - want) / np.abs(want), "factor", fac, "resid", res)
    assert np.all(want < 0)
    assert np.all(np.abs(nu - want) <= 1e-6 * np.abs(want))
    assert np.all(np.abs(fac - (1.0 - 1.0 / want)) <= 1e-6 * np.abs(1.0 - 1.0 / want))
    assert np.all(res <= tol)
    assert np.all(np.diff(nu) >= 0)


GEOM_CASES = {
    "tet4": lambda: (br.column_deck("tet4"), None, None),
    "tet4-a5": lambda: (br.column_deck("tet4", model=feahip.MODEL_A5), None, None),
    "hex8": lambda: (br.column_deck("hex8"), None, None),
    "tet10": lambda: (br.column_deck("tet10"), None, None),
    "tet10-layered": lambda: (lambda d: (with_materials(d, MATERIALS, layered_ids(d, 3)), MATERIALS, layered_ids(d, 3)))(br.column_deck("tet10")),
    "fan": lambda: (_fan_deck(), None, None),
}


@pytest.mark.parametrize("case", sorted(GEOM_CASES))
def test_geometric_stiffness_against_the_oracle(case):
    """Per row |y - ref| <= 1e-12 (|Ksig_ref| |x|) + 1e-12 max|Ksig_ref|: the scale test_gpu_parity.py holds K to.  Each
    rigid translation is within the absolute part of zero (the row sums vanish: sum_b g_b = 0).  Two calls: the same bits."""
    deck, mats, ids = GEOM_CASES[case]()
    x = mesh.deformed_state(deck.nodes, k1=1.03)
    _, Ks, _, _ = br.dense_pair(deck, x, mats, ids)
    s = feahip.FeaSolver(deck)
    if mats is not None:
        assert s.materials()[0].shape == (3, 2)
    s.set_nodes(x)
    if case == "fan":
        s.create_stiffness_and_residual()
        assert np.diff(s.matrix_yale()[0]).max() == 3 * 143                  # a row longer than a chunk tile of 128 blocks
    absolute = 1e-12 * np.abs(Ks).max()
    assert absolute > 0
    X = np.random.default_rng(31).normal(size=(6, s.ndof))
    worst = 0.0
    for v in X:
        y = s.geometric_spmv(v)
        err, bound = np.abs(y - Ks @ v), 1e-12 * (np.abs(Ks) @ np.abs(v)) + absolute
        worst = max(worst, float((err / bound).max()))
        assert np.all(err <= bound), (case, float((err / bound).max()))
    for j in range(3):
        t = np.zeros((s.N, 3))
        t[:, j] = 1.0
        y = s.geometric_spmv(t)
        assert np.abs(y).max() <= absolute, (case, j, np.abs(y).max(), absolute)
    print(case, "worst error / bound", worst, "max |Ksig|", np.abs(Ks).max())
    assert np.array_equal(s.geometric_spmv(X[0]), s.geometric_spmv(X[0]))
    s.close()


@pytest.mark.parametrize("kind", KINDS)
def test_eigenvalues_match_the_dense_reference(kind):
    r = solved(kind)
    print(kind, "steps", r["it"], "emulation", EMULATED[kind])
    assert r["it"] > 0
    assert r["ref"].min_eig_K > 0
    check_eigenvalues(r["fac"], r["nu"], r["res"], r["ref"])


@pytest.mark.parametrize("kind", KINDS)
def test_modes_are_k_orthonormal_vanish_on_the_supports_and_satisfy_the_reference_pencil(kind):
    """Never vector against vector (HEX8 has degenerate pairs): each wanted mode must be an eigenvector of the REFERENCE
    pencil to ten times the tolerance."""
    r = solved(kind)
    phi, ref = r["phi"], r["ref"]
    assert phi.shape == (feahip.MODAL_COLS, len(ref.mask))
    G = phi @ ref.K @ phi.T
    print("K-orthonormality", np.abs(G - np.eye(len(G))).max())
    assert np.abs(G - np.eye(len(G))).max() <= 1e-10                      # all eight columns, the guards included
    assert not phi[:, ref.mask].any()
    for j in range(N_MODES):
        rr = ref.residual_ratio(r["nu"][j], phi[j])
        print("mode", j, "reference residual", rr)
        assert rr <= 10 * TOL


def test_load_path_under_a_dead_traction():
    """A clamped-free column taken to its full compressive traction by FeaSolver.solve (the magnitude is checked on the
    CPU: test_traction_column_is_a_stable_equilibrium_on_the_load_path), held against the reference at the nodes reached."""
    deck = br.traction_column()
    s = feahip.FeaSolver(deck)
    done, _, _ = s.solve(load_increments=1)
    assert done == 1 and s.load_factor() == 1.0
    x = s.nodes()
    fac, nu, res, it = s.solve_buckling(N_MODES, TOL, MAX_IT)
    s.close()
    ref = br.BucklingReference(deck, x)
    print("steps", it, "min eig K", ref.min_eig_K, "critical traction", fac[0] * br.TRACTION)
    assert ref.min_eig_K > 0 and it > 0
    assert x[:, 1].max() < 8.0                                             # compressed
    check_eigenvalues(fac, nu, res, ref)


def test_multigrid_preconditioner_gives_the_same_eigenvalues():
    """Preconditioner 1 needs more than 200 block rows to coarsen (the three columns have 81 or fewer and are refused by
    feahip_set_preconditioner), so this is the TET4 column of the same body in (3, 12, 3) cells, 208 nodes."""
    deck = br.column_deck("tet4", dims=(3, 12, 3))
    s = feahip.FeaSolver(deck)
    done, _, _ = s.solve(load_increments=1)
    assert done == 1
    ref = br.BucklingReference(deck, s.nodes())
    fac0, nu0, res0, it0 = s.solve_buckling(N_MODES, TOL, MAX_IT)
    s.set_preconditioner(1)
    fac1, nu1, res1, it1 = s.solve_buckling(N_MODES, TOL, MAX_IT)
    s.close()
    print("kind 0 steps", it0, "kind 1 steps", it1)
    check_eigenvalues(fac0, nu0, res0, ref)
    check_eigenvalues(fac1, nu1, res1, ref)


def test_buckling_leaves_the_context_alone_and_is_reproducible():
    deck = br.column_deck("tet4")
    rho = 1.5
    s = feahip.FeaSolver(deck)
    with pytest.raises(feahip.FeaHipError, match="no mass"):
        s.mass_spmv(np.ones(s.ndof))
    done, _, _ = s.solve(load_increments=1)
    assert done == 1
    fac_a, nu_a, res_a, it_a = s.solve_buckling(N_MODES, TOL, MAX_IT)      # no mass on the context
    phi_a = s.buckling_modes()
    s.set_mass(rho)
    v = np.random.default_rng(3).normal(size=s.ndof)
    mv = s.mass_spmv(v)
    before = (s.nodes(), s.solution(), s.load_factor())
    fac_b, nu_b, res_b, it_b = s.solve_buckling(N_MODES, TOL, MAX_IT)
    after = (s.nodes(), s.solution(), s.load_factor())
    for u, w in zip(before, after):
        assert np.array_equal(u, w)
    assert np.array_equal(mv, s.mass_spmv(v))
    assert it_a == it_b and np.array_equal(nu_a, nu_b) and np.array_equal(fac_a, fac_b) and np.array_equal(res_a, res_b)
    assert np.array_equal(phi_a, s.buckling_modes())
    # a modal solve on the same context: its own reference check, and the buckling modes are gone
    lam, res, _ = s.solve_modes(N_MODES, TOL, 1000)
    want = ModalReference(deck, rho, x=before[0]).lam[:N_MODES]
    assert np.all(np.abs(lam - want) <= 1e-6 * want) and np.all(res <= TOL)
    with pytest.raises(feahip.FeaHipError, match="no buckling modes held"):
        s.buckling_modes()
    s.solve_buckling(2, TOL, MAX_IT)
    with pytest.raises(feahip.FeaHipError, match="no modes held"):
        s.modes()
    s.close()


def _refused(s, code, fn):
    with pytest.raises(feahip.FeaHipError) as e:
        fn()
    prefix = f"libfeahip error {code}: "
    msg = str(e.value)
    assert msg.startswith(prefix) and len(msg) > len(prefix) + 5, msg      # the code and a non-empty feahip_last_error
    return msg


def test_refusals():
    deck = br.column_deck("tet4")
    s = feahip.FeaSolver(deck)
    assert "no buckling modes held" in _refused(s, feahip.ESTATE, lambda: s.buckling_modes())
    for bad in (0, 9):
        assert "n_modes" in _refused(s, feahip.EINVAL, lambda: s.solve_buckling(bad))
    assert "tolerance" in _refused(s, feahip.EINVAL, lambda: s.solve_buckling(2, tolerance=0.0))
    assert "max_iterations" in _refused(s, feahip.EINVAL, lambda: s.solve_buckling(2, max_iterations=-1))
    assert s._lib.feahip_solve_buckling(s._ctx, 2, 1e-8, 10, None, None, None, None) == feahip.EINVAL
    assert b"null factor" in s._lib.feahip_last_error(s._ctx)
    s.set_nodes(br.column_reference("tet4")[1])
    s.solve_buckling(2, 1e-6, MAX_IT)
    assert s.buckling_modes(6, 2).shape == (2, s.ndof)
    for first, count in ((7, 2), (-1, 1), (0, 9)):
        assert "outside" in _refused(s, feahip.EINVAL, lambda: s.buckling_modes(first, count))
    s.set_row_shard(0, 2)
    assert "row-sharded" in _refused(s, feahip.EINVAL, lambda: s.solve_buckling(2))
    assert "row-sharded" in _refused(s, feahip.EINVAL, lambda: s.geometric_spmv(np.ones(s.ndof)))
    s.close()
    s = feahip.FeaSolver(br.column_deck("tet4", dims=(1, 1, 1), size=(1.0, 1.0, 1.0), end_motion=None))   # 12 free dofs
    assert "free dofs" in _refused(s, feahip.EINVAL, lambda: s.solve_buckling(1))
    s.close()
    r = feahip.RankSolver(deck, 0, 2)
    assert "feahip_create_rank" in _refused(r, feahip.EINVAL, lambda: r.solve_buckling(2))
    assert "feahip_create_rank" in _refused(r, feahip.EINVAL, lambda: r.geometric_spmv(np.ones(r.ndof)))
    r.close()
    g = feahip.FeaGroup(deck, 2)
    m = g.ranks[0]
    assert "transport" in _refused(m, feahip.EINVAL, lambda: m.solve_buckling(2))
    g.close()
    s = feahip.FeaSolver(mesh.bar_deck(dims=(6, 36, 6)))                     # large enough for the multigrid kinds
    s.set_preconditioner(2)
    assert "preconditioner 2" in _refused(s, feahip.EINVAL, lambda: s.solve_buckling(2))
    s.close()


def test_timing_hooks_run_without_a_mass():
    s = feahip.FeaSolver(br.column_deck("tet10"))
    s.set_nodes(br.column_reference("tet10")[1])
    for what in (18, 19):
        assert s.time_kernel(what, 1, 2) > 0
    s.close()


def test_feasolver_hip_runs_the_buckling_section_of_a_deck(tmp_path):
    """(buckling :modes 3): one log line per mode whose factor is solve_buckling's at the state reached, and one
    "Buckling mode k" section per mode shape in the .msh file."""
    deck = br.column_deck("tet4", buckling_modes=3, load_increments_count=1)
    path = tmp_path / "column.sexp"
    deck.save(str(path))
    s = feahip.FeaSolver(feahip.Deck.load(str(path)))
    done, _, _ = s.solve()
    assert done == 1
    fac, nu, _, _ = s.solve_buckling(3, deck.buckling_tolerance, deck.buckling_max)
    s.close()
    exe = os.path.join(os.path.dirname(feahip.LIB_PATH), "feasolver_hip")
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert re.search(r"^Buckling analysis finished: 3 modes, \d+ steps$", out.stdout, re.M), out.stdout
    got = re.findall(r"^Buckling mode (\d+): factor = (\S+), nu = (\S+)$", out.stdout, re.M)
    assert [int(g[0]) for g in got] == [1, 2, 3]
    # (the executable reaches its state by the host's Newton loop, this test by feahip_solve: equal to their tolerance)
    assert np.all(np.abs(np.array([float(g[1]) for g in got]) - fac) <= 1e-6 * np.abs(fac))
    assert np.all(np.abs(np.array([float(g[2]) for g in got]) - nu) <= 1e-6 * np.abs(nu))
    text = (tmp_path / "column.msh").read_text()
    assert [int(k) for k in re.findall(r'^"Buckling mode (\d+)"$', text, re.M)] == [1, 2, 3]
    assert text.count("$NodeData") == text.count('"Displacements"') + 3

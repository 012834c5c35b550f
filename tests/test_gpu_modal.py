"""Modal analysis on the MI355X (kernels_modal.hip): feahip_solve_modes against scipy.linalg.eigh on the oracle's K and a
float64 consistent mass (tests/modal_reference.py), the block product k_spmm_km against float64 products, pre-stress,
a material table, both preconditioners, reproducibility and warm restarts, what the solve refuses, and that it leaves
the context's state alone."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import feahip
import mesh
from dynamics_reference import DENSITIES, dense_mass, loaded_bar
from hetero_reference import MATERIALS, layered_ids, with_materials
from modal_reference import ModalReference

pytestmark = pytest.mark.gpu

RHO, TOL, MAX_IT, N_MODES = 1.5, 1e-8, 1000, 6


def _fan_deck(m=140):
    """A fan of tetrahedra pairs around one node: its block row has m + 3 = 143 blocks, more than the 128-block tile of
    the products (the long-row path of k_spmm_km runs)."""
    ang = 2 * np.pi * np.arange(m) / m
    ring = np.stack([np.cos(ang), np.sin(ang), np.zeros(m)], axis=1)
    nodes = np.vstack([[0.0, 0.0, 0.0], ring, [0.0, 0.0, 0.7], [0.0, 0.0, -0.7]])
    top, bot = m + 1, m + 2
    el = []
    for i in range(m):
        a, b = 1 + i, 1 + (i + 1) % m
        el.append([0, a, b, top])
        el.append([0, b, a, bot])
    return feahip.Deck(nodes=nodes, elements=np.array(el, dtype=np.int32), ele_type=feahip.TETRAHEDRA4, gauss_nodes_count=1,
                       presc_node=[top, bot, 1], presc_type=[7, 7, 2], presc_values=np.zeros((3, 3)))


DECKS = {
    "tet4": lambda: loaded_bar("tet4", (3, 8, 3)),
    "tet10": lambda: loaded_bar("tet10", (2, 4, 2)),
    "hex8": lambda: loaded_bar("hex8", (3, 8, 3)),
    "fan": _fan_deck,
}
KINDS = sorted(DECKS)


@functools.lru_cache(maxsize=None)
def reference(kind):
    """The float64 eigenpairs of a deck at its own nodes, computed once and read-only."""
    ref = ModalReference(DECKS[kind](), RHO)
    for a in (ref.lam, ref.Phi, ref.K, ref.M):
        a.setflags(write=False)
    return ref


def solver(deck, rho=RHO):
    s = feahip.FeaSolver(deck)
    s.set_mass(rho)
    return s


@functools.lru_cache(maxsize=None)
def solved(kind):
    """One cold solve of six modes per deck, shared by the tests that read it."""
    s = solver(DECKS[kind]())
    lam, res, it = s.solve_modes(N_MODES, TOL, MAX_IT)
    phi = s.modes()
    s.close()
    for a in (lam, res, phi):
        a.setflags(write=False)
    return lam, res, it, phi


def check_eigenvalues(lam, ref_lam, res, tol=TOL):
    n = len(lam)
    print("lambda", lam, "rel err", np.abs(lam - ref_lam[:n]) / ref_lam[:n], "resid", res)
    assert np.all(np.abs(lam - ref_lam[:n]) <= 1e-6 * ref_lam[:n])
    assert np.all(res <= tol)
    assert np.all(np.diff(lam) >= 0)


@pytest.mark.parametrize("kind", KINDS)
def test_eigenvalues_match_the_dense_reference(kind):
    """|lambda_j - ref_j| <= 1e-6 ref_j: the first-order residual bound is 2 tol sqrt(cond M), about 1e-7 on these
    meshes.  hex8's square section has a degenerate bending pair, the fan's ring several."""
    lam, res, it, _ = solved(kind)
    print(kind, "steps", it)
    assert it > 0
    check_eigenvalues(lam, reference(kind).lam, res)


@pytest.mark.parametrize("kind", KINDS)
def test_modes_are_m_orthonormal_vanish_on_the_supports_and_satisfy_the_reference_pencil(kind):
    """Modes are never compared vector against vector (degenerate pairs rotate): each must be an eigenvector of the
    REFERENCE pencil on the free dofs to ten times the tolerance."""
    lam, _, _, phi = solved(kind)
    ref = reference(kind)
    assert phi.shape == (feahip.MODAL_COLS, len(ref.mask))
    G = phi @ ref.M @ phi.T
    print("orthonormality", np.abs(G - np.eye(len(G))).max())
    assert np.abs(G - np.eye(len(G))).max() <= 1e-10                     # all eight columns, the guards included
    assert not phi[:, ref.mask].any()
    for j in range(N_MODES):
        r = ref.residual_ratio(lam[j], phi[j])
        print("mode", j, "reference residual", r)
        assert r <= 10 * TOL


@pytest.mark.parametrize("kind", KINDS)
def test_spmm_km_against_float64_products(kind):
    """The fixed-order bound of test_spmv2_against_a_float64_product per row: nterms 2^-52 (|A| |x|), for K X and for
    M X (one term per block there); M X is zero on the prescribed dofs, and a zero column stays exactly zero.  As K is
    the library's own (feahip_get_matrix_yale), so that the bound holds the PRODUCT and not the assembly, M is the
    library's own as well: column b of the scalar mass is feahip_mass_spmv of a unit vector (m_ab x 1 plus zeros, exact);
    it is tied to the float64 mass of tests/dynamics_reference.py separately."""
    deck = DECKS[kind]()
    s = solver(deck)
    s.set_nodes(mesh.deformed_state(deck.nodes, k1=1.03))
    s.create_stiffness_and_residual()
    off, idx, val = s.matrix_yale()
    K = sp.csr_matrix((val, idx, off), shape=(s.ndof, s.ndof))
    absK = sp.csr_matrix((np.abs(val), idx, off), shape=(s.ndof, s.ndof))
    nterms = np.diff(off)
    if kind == "fan":
        assert nterms.max() == 3 * 143                                    # the long-row path runs
    m = np.zeros((s.N, s.N))
    for b in range(s.N):
        e = np.zeros(s.ndof)
        e[3 * b] = 1.0
        m[:, b] = s.mass_spmv(e)[0::3]
    M = np.kron(m, np.eye(3))
    M_ref = dense_mass(deck, RHO)
    assert np.abs(M - M_ref).max() <= 1e-13 * np.abs(M_ref).max()
    mask = reference(kind).mask
    x8 = np.random.default_rng(23).normal(size=(8, s.ndof))
    x8[3] = 0.0
    y8, z8 = s.spmm_km(x8)
    for c in range(8):
        bk = nterms * 2.0 ** -52 * (absK @ np.abs(x8[c]))
        ek = np.abs(y8[c] - K @ x8[c])
        assert np.all(ek <= bk), (kind, c, "K", float((ek / np.maximum(bk, 1e-300)).max()))
        bm = (nterms // 3) * 2.0 ** -52 * (np.abs(M) @ np.abs(x8[c]))
        em = np.abs(z8[c] - np.where(mask, 0.0, M @ x8[c]))
        assert np.all(em <= bm), (kind, c, "M", float((em / np.maximum(bm, 1e-300)).max()))
    assert not y8[3].any() and not z8[3].any()
    assert not z8[:, mask].any() and z8[:, ~mask].any()
    y8b, z8b = s.spmm_km(x8)
    assert np.array_equal(y8, y8b) and np.array_equal(z8, z8b)
    s.close()


def test_modes_of_a_stretched_bar():
    """K is the tangent at the CURRENT nodes: after five increments of end motion lambda matches the reference built at
    s.nodes(), and the first frequency has moved by more than 1 % against the unstretched bar."""
    deck = loaded_bar("tet4", (2, 4, 2), end_motion=0.02)
    s = solver(deck)
    done, _, _ = s.solve(load_increments=5)
    assert done == 5
    x = s.nodes()
    lam, res, it = s.solve_modes(N_MODES, TOL, MAX_IT)
    assert np.array_equal(s.nodes(), x)
    s.close()
    check_eigenvalues(lam, ModalReference(deck, RHO, x=x).lam, res)
    lam0 = ModalReference(deck, RHO).lam[0]
    print("lambda_1 stretched", lam[0], "unstretched", lam0)
    assert abs(lam[0] - lam0) > 0.01 * lam0


def test_modes_of_a_body_of_two_materials():
    base = loaded_bar("tet4", (2, 4, 2))
    ids = layered_ids(base, 2)
    deck = with_materials(base, MATERIALS[:2], ids)
    s = solver(deck, DENSITIES[:2])
    lam, res, it = s.solve_modes(N_MODES, TOL, MAX_IT)
    s.close()
    check_eigenvalues(lam, ModalReference(deck, DENSITIES[:2], materials=MATERIALS[:2], ids=ids).lam, res)


def test_multigrid_preconditioner_gives_the_same_eigenvalues():
    """Kind 1 (one W-cycle per column and step) against kind 0, 1e-6 relative; no iteration counts are compared."""
    s = solver(mesh.bar_deck(dims=(3, 12, 3)))
    lam0, res0, it0 = s.solve_modes(N_MODES, TOL, MAX_IT)
    s.set_preconditioner(1)
    lam1, res1, it1 = s.solve_modes(N_MODES, TOL, MAX_IT)
    s.close()
    print("kind 0", lam0, it0, "kind 1", lam1, it1)
    assert np.all(res0 <= TOL) and np.all(res1 <= TOL)
    assert np.all(np.abs(lam1 - lam0) <= 1e-6 * lam0)


@pytest.mark.parametrize("n_modes", [1, 8])
def test_one_mode_and_all_eight(n_modes):
    s = solver(DECKS["tet4"]())
    lam, res, it = s.solve_modes(n_modes, TOL, MAX_IT)
    assert lam.shape == (n_modes,)
    s.close()
    print("n_modes", n_modes, "steps", it)
    check_eigenvalues(lam, reference("tet4").lam, res)


def test_reproducible_and_warm_restarts():
    deck = DECKS["tet4"]()
    s = solver(deck)
    lam_a, res_a, it_a = s.solve_modes(N_MODES, TOL, MAX_IT)
    phi_a = s.modes()
    lam_b, res_b, it_b = s.solve_modes(N_MODES, TOL, MAX_IT)               # cold again: the same bits
    assert it_a == it_b and np.array_equal(lam_a, lam_b) and np.array_equal(res_a, res_b)
    assert np.array_equal(phi_a, s.modes())
    lam_c, res_c, it_c = s.solve_modes(N_MODES, TOL, MAX_IT, warm=True)    # converged already: nothing moves
    assert it_c == 0
    assert np.array_equal(lam_a, lam_c) and np.array_equal(res_a, res_c) and np.array_equal(phi_a, s.modes())
    # the sign is arbitrary but fixed: another context gives the same bits as well
    t = solver(deck)
    lam_t, _, _ = t.solve_modes(N_MODES, TOL, MAX_IT)
    assert np.array_equal(lam_a, lam_t) and np.array_equal(phi_a, t.modes())
    t.close()
    # the nodes move by half a percent: the modes held are a start within 1 % of the answer
    x = mesh.deformed_state(deck.nodes, k1=1.005)
    s.set_nodes(x)
    lam_w, res_w, it_w = s.solve_modes(N_MODES, TOL, MAX_IT, warm=True)
    s.close()
    print("cold", it_a, "warm after the move", it_w)
    assert 0 < it_w < it_a
    check_eigenvalues(lam_w, ModalReference(deck, RHO, x=x).lam, res_w)


def test_not_converged_leaves_finite_ascending_eigenvalues():
    s = solver(DECKS["tet4"]())
    with pytest.raises(feahip.FeaHipError, match=f"error {feahip.ENOTCONVERGED}"):
        s.solve_modes(N_MODES, TOL, 2)
    lam, res, it, rc = s.solve_modes(N_MODES, TOL, 2, check=False)
    assert rc == feahip.ENOTCONVERGED and it == 2
    assert np.all(np.isfinite(lam)) and np.all(np.diff(lam) >= 0) and lam[0] > 0
    assert np.all(np.isfinite(res)) and res.max() > TOL
    phi = s.modes(0, N_MODES)                                              # the modes as they stand
    assert phi.shape == (N_MODES, s.ndof) and np.all(np.isfinite(phi))
    s.close()


def _refused(s, code, fn):
    with pytest.raises(feahip.FeaHipError) as e:
        fn()
    prefix = f"libfeahip error {code}: "
    msg = str(e.value)
    assert msg.startswith(prefix) and len(msg) > len(prefix) + 5, msg      # the code and a non-empty feahip_last_error
    return msg


def test_refusals():
    deck = DECKS["tet4"]()
    s = feahip.FeaSolver(deck)
    assert "no mass" in _refused(s, feahip.ESTATE, lambda: s.solve_modes(2))
    s.set_mass(RHO)
    assert "no modes held" in _refused(s, feahip.ESTATE, lambda: s.modes())
    for bad in (0, 9):
        assert "n_modes" in _refused(s, feahip.EINVAL, lambda: s.solve_modes(bad))
    assert "tolerance" in _refused(s, feahip.EINVAL, lambda: s.solve_modes(2, tolerance=0.0))
    assert "max_iterations" in _refused(s, feahip.EINVAL, lambda: s.solve_modes(2, max_iterations=-1))
    assert s._lib.feahip_solve_modes(s._ctx, 2, 1e-8, 10, 0, None, None, None) == feahip.EINVAL
    assert b"null lambda" in s._lib.feahip_last_error(s._ctx)
    s.solve_modes(2, 1e-6, 200)
    assert s.modes(6, 2).shape == (2, s.ndof)
    for first, count in ((7, 2), (-1, 1), (0, 9)):
        assert "outside" in _refused(s, feahip.EINVAL, lambda: s.modes(first, count))
    s.set_preconditioner(0)
    s.set_row_shard(0, 2)
    assert "row-sharded" in _refused(s, feahip.EINVAL, lambda: s.solve_modes(2))
    s.close()
    # a per-material mass after the material count changed
    ids = layered_ids(deck, 2)
    s = solver(with_materials(deck, MATERIALS[:2], ids), DENSITIES[:2])
    s.set_materials(MATERIALS, layered_ids(deck, 3))
    assert "material count changed" in _refused(s, feahip.ESTATE, lambda: s.solve_modes(2))
    s.close()
    # fewer than 24 free dofs: a single cell clamped on one face has 12
    s = solver(loaded_bar("tet4", (1, 1, 1)))
    assert "free dofs" in _refused(s, feahip.EINVAL, lambda: s.solve_modes(1))
    s.close()
    # a member of a group, a rank context, the coarse level across the ranks
    g = feahip.FeaGroup(deck, 2)
    g.set_mass(RHO)
    m = g.ranks[0]
    assert "transport" in _refused(m, feahip.EINVAL, lambda: m.solve_modes(2))
    g.close()
    r = feahip.RankSolver(deck, 0, 2)
    assert "feahip_create_rank" in _refused(r, feahip.EINVAL, lambda: r.solve_modes(2))
    r.close()
    s = solver(mesh.bar_deck(dims=(6, 36, 6)))                               # large enough for the multigrid kinds
    s.set_preconditioner(2)
    assert "preconditioner 2" in _refused(s, feahip.EINVAL, lambda: s.solve_modes(2))
    s.close()


def test_timing_hooks_are_refused_without_a_mass_and_run_with_one():
    s = feahip.FeaSolver(DECKS["tet4"]())
    s.create_stiffness_and_residual()
    for what in (13, 14, 15):
        assert "no mass" in _refused(s, feahip.EINVAL, lambda: s.time_kernel(what, 1, 1))
    s.set_mass(RHO)
    for what in (13, 14, 15):
        assert s.time_kernel(what, 1, 2) > 0
    s.close()


def test_solve_modes_leaves_the_state_of_the_context_alone():
    """x, u, the velocities and the accelerations are untouched, the next assembly rebuilds K, and two Newmark steps
    after a modal solve give the bits they give on a context that never solved modes."""
    deck = loaded_bar("tet4", (2, 4, 2))

    def fresh():
        s = solver(deck)
        rng = np.random.default_rng(7)
        s.set_velocities(0.01 * rng.normal(size=(s.N, 3)))
        s.set_accelerations(0.1 * rng.normal(size=(s.N, 3)))
        s.set_load_factor(1.0)
        return s

    def steps(s):
        done, its, _ = s.solve_dynamic(2, 0.01, 0.25, 0.5, 0.0)
        assert done == 2
        return s.nodes(), s.velocities(), s.accelerations(), its

    a, b = fresh(), fresh()
    b.create_stiffness_and_residual()
    k_before = b.matrix_yale()[2]
    before = (b.nodes(), b.solution(), b.velocities(), b.accelerations(), b.load_factor(), b.time())
    lam, res, it = b.solve_modes(N_MODES, TOL, MAX_IT)
    after = (b.nodes(), b.solution(), b.velocities(), b.accelerations(), b.load_factor(), b.time())
    for u, v in zip(before, after):
        assert np.array_equal(u, v, equal_nan=True)
    b.create_stiffness_and_residual()                                       # every assembly rebuilds K
    assert np.array_equal(k_before, b.matrix_yale()[2])
    for u, v in zip(steps(a), steps(b)):
        assert np.array_equal(u, v)
    a.close()
    b.close()

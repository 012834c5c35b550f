"""Sharded modal analysis on the MI355X (feahip_solve_modes_sharded, feahip_group_spmm_km): the lowest modes over row
shards and rank contexts of an in-process group against scipy.linalg.eigh on the oracle's K and a float64 consistent
mass (tests/modal_reference.py), the sharded block product against float64 products, the overlap of the block exchange
with the interior product under FEAHIP_TEST_POISON_HALO, reproducibility and warm restarts, one RCCL rank against the
unsharded solve, the multigrid preconditioner, what the solve refuses, and that it leaves the group's PCG alone.

The decks are the small ones of tests/test_gpu_modal.py.  With three ranks the row shard of the tet4 bar leaves rank 0
without rows (two supers of chunks): the solve must carry a rank that owns nothing."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import feahip
import mesh
from dynamics_reference import loaded_bar
from test_gpu_modal import DECKS, MAX_IT, N_MODES, RHO, TOL, _refused, check_eigenvalues, reference

pytestmark = pytest.mark.gpu

BARS = ["hex8", "tet10", "tet4"]


def group(deck, n, rank_contexts=False, rho=RHO):
    g = feahip.FeaGroup(deck, n, rank_contexts=rank_contexts)
    if rho is not None:
        g.set_mass(rho)
    return g


@functools.lru_cache(maxsize=None)
def solved(kind, n, rank_contexts):
    """One cold sharded solve of six modes per (deck, ranks, context kind), shared by the tests that read it: lam,
    resid, steps, the stitched modes, and every rank's own modes() with the dofs it owns (in that context's order)."""
    g = group(DECKS[kind](), n, rank_contexts)
    lam, res, it = g.solve_modes(N_MODES, TOL, MAX_IT)
    phi = g.modes()
    per_rank = []
    for r, nd in zip(g.ranks, g.nodes):
        own = np.arange(r.n_own) if rank_contexts else nd
        per_rank.append((r.modes(), (3 * np.asarray(own)[:, None] + np.arange(3)[None, :]).ravel()))
    g.close()
    for a in (lam, res, phi):
        a.setflags(write=False)
    return lam, res, it, phi, per_rank


@functools.lru_cache(maxsize=None)
def unsharded_steps(kind):
    s = feahip.FeaSolver(DECKS[kind]())
    s.set_mass(RHO)
    it = s.solve_modes(N_MODES, TOL, MAX_IT)[2]
    s.close()
    return it


@pytest.mark.parametrize("kind", BARS)
@pytest.mark.parametrize("rank_contexts", [False, True])
@pytest.mark.parametrize("n", [2, 3])
def test_eigenvalues_match_the_dense_reference(n, rank_contexts, kind):
    """|lambda_j - ref_j| <= 1e-6 ref_j, the bound tests/test_gpu_modal.py derives (2 tol sqrt(cond M), about 1e-7 on
    these meshes): the cut changes the order of the sums and, on rank contexts, the start block, not the pencil."""
    lam, res, it, _, _ = solved(kind, n, rank_contexts)
    print(kind, "ranks", n, "rank contexts" if rank_contexts else "row shards", "steps", it, "unsharded steps", unsharded_steps(kind))
    assert it > 0
    check_eigenvalues(lam, reference(kind).lam, res)


@pytest.mark.parametrize("kind", BARS)
@pytest.mark.parametrize("rank_contexts", [False, True])
@pytest.mark.parametrize("n", [2, 3])
def test_modes_are_m_orthonormal_over_the_whole_mesh_and_each_rank_holds_its_own_rows(n, rank_contexts, kind):
    lam, _, _, phi, per_rank = solved(kind, n, rank_contexts)
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
    assert len(per_rank) == n
    for p, own in per_rank:                                              # authoritative on its rows, zero on all others
        off = np.ones(p.shape[1], dtype=bool)
        off[own] = False
        assert not p[:, off].any()
        assert p[:, own].any() or len(own) == 0


def group_matrices(g, deck):
    """K and the scalar mass m of the group's own ranks, in the deck's dof / node order: every rank's owned rows of its
    Yale matrix, and column b of m as feahip_mass_spmv of a unit vector on every rank that holds node b (m_ab x 1 plus
    zeros: exact) -- so that the bounds below hold the PRODUCT, as in test_spmm_km_against_float64_products."""
    N = len(deck.nodes)
    rows, cols, vals = [], [], []
    m = np.zeros((N, N))
    for r, nd in zip(g.ranks, g.nodes):
        off, idx, val = r.matrix_yale()
        Kl = sp.csr_matrix((val, idx, off), shape=(r.ndof, r.ndof)).tocoo()
        ng = r.node_global.astype(np.int64) if g.rank_contexts else np.arange(N)
        gd = (3 * ng[:, None] + np.arange(3)[None, :]).ravel()               # the context's dof -> the deck's dof
        own = np.zeros(r.ndof, dtype=bool)
        own_nodes = np.arange(r.n_own) if g.rank_contexts else nd
        own[(3 * np.asarray(own_nodes)[:, None] + np.arange(3)[None, :]).ravel()] = True
        keep = own[Kl.row]
        assert not Kl.data[~keep].any()                                      # nothing outside the owned rows
        rows.append(gd[Kl.row[keep]]); cols.append(gd[Kl.col[keep]]); vals.append(Kl.data[keep])
        for lb in range(r.N if len(own_nodes) else 0):
            e = np.zeros(r.ndof)
            e[3 * lb] = 1.0
            m[ng[own_nodes], ng[lb]] = r.mass_spmv(e)[0::3][own_nodes]
    K = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(3 * N, 3 * N))
    K.sum_duplicates(); K.sort_indices()
    return K, m


@pytest.mark.parametrize("rank_contexts", [False, True])
@pytest.mark.parametrize("kind,n", [("hex8", 3), ("tet10", 3), ("tet4", 3), ("fan", 2)])
def test_group_spmm_km_against_float64_products(kind, n, rank_contexts):
    """The check of test_spmm_km_against_float64_products on the sharded product: per row nterms 2^-52 (|A| |x|) for K X
    and for M X; M X zero on the prescribed dofs; a zero column stays exactly zero; the same bits twice.  With three ranks
    the middle one has two peers; the fan's hub row (143 blocks) takes the long-row path and is a halo row of the
    other rank.  A rank's result is zero off its own rows."""
    deck = DECKS[kind]()
    g = group(deck, n, rank_contexts)
    x = mesh.deformed_state(deck.nodes, k1=1.03)
    for r in g.ranks:
        r.set_nodes(x[r.node_global] if rank_contexts else x)
    g.each("create_stiffness_and_residual")
    K, m = group_matrices(g, deck)
    absK = abs(K)
    nterms = np.diff(K.indptr)
    if kind == "fan":
        assert nterms.max() == 3 * 143                                    # the long-row path runs
        assert all(len(nd) < len(deck.nodes) for nd in g.nodes)
    M = np.kron(m, np.eye(3))
    mask = reference(kind).mask
    x8 = np.random.default_rng(23).normal(size=(8, 3 * len(deck.nodes)))
    x8[3] = 0.0
    y8, z8, ys, zs = g.spmm_km(x8, per_rank=True)
    for c in range(8):
        bk = nterms * 2.0 ** -52 * (absK @ np.abs(x8[c]))
        ek = np.abs(y8[c] - K @ x8[c])
        assert np.all(ek <= bk), (kind, c, "K", float((ek / np.maximum(bk, 1e-300)).max()))
        bm = (nterms // 3) * 2.0 ** -52 * (np.abs(M) @ np.abs(x8[c]))
        em = np.abs(z8[c] - np.where(mask, 0.0, M @ x8[c]))
        assert np.all(em <= bm), (kind, c, "M", float((em / np.maximum(bm, 1e-300)).max()))
    assert not y8[3].any() and not z8[3].any()
    assert not z8[:, mask].any() and z8[:, ~mask].any()
    for r, nd, yr, zr in zip(g.ranks, g.nodes, ys, zs):
        off = np.ones(r.N, dtype=bool)
        off[np.arange(r.n_own) if rank_contexts else nd] = False
        assert not yr.reshape(8, -1, 3)[:, off].any() and not zr.reshape(8, -1, 3)[:, off].any()
    y8b, z8b = g.spmm_km(x8)
    assert np.array_equal(y8, y8b) and np.array_equal(z8, z8b)
    g.close()


@pytest.mark.parametrize("rank_contexts", [False, True])
@pytest.mark.parametrize("n", [2, 3])
def test_block_exchange_overlap_never_reads_a_halo_row(n, rank_contexts, monkeypatch):
    """test_interior_product_never_reads_a_halo_row for the block exchange: with FEAHIP_TEST_POISON_HALO the halo rows
    of the block vector are NaN from exchange_block_begin on and the copies wait until everything enqueued up to
    exchange_block_end has run.  Were a halo column among the interior chunks, or an event dependency missing, NaN
    would reach the products and the sums: the solve, and separately the product, must give the bits of the
    unpoisoned run."""
    deck = DECKS["tet4"]()
    x8 = np.random.default_rng(5).normal(size=(8, 3 * len(deck.nodes)))

    def run():
        g = group(deck, n, rank_contexts)
        g.each("create_stiffness_and_residual")
        y8, z8 = g.spmm_km(x8)
        lam, res, it = g.solve_modes(N_MODES, TOL, MAX_IT)
        phi = g.modes()
        g.close()
        return y8, z8, lam, res, it, phi

    monkeypatch.delenv("FEAHIP_TEST_POISON_HALO", raising=False)
    clean = run()
    monkeypatch.setenv("FEAHIP_TEST_POISON_HALO", "1")
    poisoned = run()
    for a in poisoned:
        assert np.all(np.isfinite(a))
    assert poisoned[4] == clean[4] > 0
    for a, b in zip(poisoned, clean):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("rank_contexts", [False, True])
def test_reproducible_and_warm_restart(rank_contexts):
    deck = DECKS["tet4"]()
    a = group(deck, 2, rank_contexts)
    lam_a, res_a, it_a = a.solve_modes(N_MODES, TOL, MAX_IT)
    phi_a = a.modes()
    b = group(deck, 2, rank_contexts)                                      # a fresh group: the same bits
    lam_b, res_b, it_b = b.solve_modes(N_MODES, TOL, MAX_IT)
    assert it_a == it_b > 0 and np.array_equal(lam_a, lam_b) and np.array_equal(res_a, res_b)
    assert np.array_equal(phi_a, b.modes())
    b.close()
    lam_c, res_c, it_c = a.solve_modes(N_MODES, TOL, MAX_IT, warm=True)    # converged already: nothing moves
    assert it_c == 0
    assert np.array_equal(lam_a, lam_c) and np.array_equal(res_a, res_c) and np.array_equal(phi_a, a.modes())
    lam_d, res_d, it_d = a.solve_modes(N_MODES, TOL, MAX_IT)               # cold again on the same group
    assert it_d == it_a and np.array_equal(lam_a, lam_d) and np.array_equal(phi_a, a.modes())
    a.close()


def test_one_rccl_rank_gives_the_bits_of_the_unsharded_solve():
    """The RCCL transport with one rank (all one process can host here): the block exchange with no peer, the vector
    all-reduce of one rank, and the launches on the owned rows -- all rows -- must reproduce feahip_solve_modes."""
    deck = DECKS["tet4"]()
    s = feahip.FeaSolver(deck)
    s.comm_init(0, 1, feahip.comm_unique_id())
    s.set_mass(RHO)
    s.set_preconditioner(0)
    lam, res, it = s.solve_modes_sharded(N_MODES, TOL, MAX_IT)
    phi = s.modes()
    s.close()
    t = feahip.FeaSolver(deck)
    t.set_mass(RHO)
    lam_t, res_t, it_t = t.solve_modes(N_MODES, TOL, MAX_IT)
    assert it == it_t > 0 and np.array_equal(lam, lam_t) and np.array_equal(res, res_t)
    assert np.array_equal(phi, t.modes())
    t.close()


def test_multigrid_preconditioner_gives_the_same_eigenvalues():
    """Kind 1 (one W-cycle per column on each rank's own diagonal block) against kind 0: each is within 1e-6 of the
    same spectrum, so they agree within 2e-6 relative; no iteration counts are compared."""
    g = group(mesh.bar_deck(dims=(6, 36, 6)), 2)
    lam0, res0, it0 = g.solve_modes(N_MODES, TOL, MAX_IT)
    g.each("set_preconditioner", 1)
    lam1, res1, it1 = g.solve_modes(N_MODES, TOL, MAX_IT)
    g.close()
    print("kind 0", lam0, it0, "kind 1", lam1, it1)
    assert np.all(res0 <= TOL) and np.all(res1 <= TOL)
    assert np.all(np.diff(lam0) >= 0) and np.all(np.diff(lam1) >= 0)
    assert np.all(np.abs(lam1 - lam0) <= 2e-6 * lam0)


def _group_refused(g, code, fn):
    with pytest.raises(feahip.FeaHipError) as e:
        fn()
    msg = str(e.value)
    assert msg.startswith(f"libfeahip group error {code}: "), msg
    return msg


def test_refusals():
    deck = DECKS["tet4"]()
    # no transport: the unsharded entry is the one to call
    s = feahip.FeaSolver(deck)
    s.set_mass(RHO)
    msg = _refused(s, feahip.EINVAL, lambda: s.solve_modes_sharded(2))
    assert "solve_modes_sharded: " in msg and "no transport" in msg and "feahip_solve_modes" in msg
    s.close()
    # no mass on any rank, then on one rank only
    g = group(deck, 2, rho=None)
    assert "solve_modes_sharded: no mass" in _group_refused(g, feahip.ESTATE, lambda: g.solve_modes(2))
    g.ranks[0].set_mass(RHO)
    assert "solve_modes_sharded: no mass" in _group_refused(g, feahip.ESTATE, lambda: g.solve_modes(2))
    g.ranks[1].set_mass(RHO)
    # the argument refusals of feahip_solve_modes, behind the new prefix
    for bad in (0, 9):
        assert "solve_modes_sharded: n_modes must be in [1, 8]" in _group_refused(g, feahip.EINVAL, lambda: g.solve_modes(bad))
    assert "solve_modes_sharded: tolerance must be positive" in _group_refused(g, feahip.EINVAL, lambda: g.solve_modes(2, tolerance=0.0))
    assert "solve_modes_sharded: max_iterations must not be negative" in _group_refused(g, feahip.EINVAL, lambda: g.solve_modes(2, max_iterations=-1))
    m = g.ranks[1]
    assert m._lib.feahip_solve_modes_sharded(m._ctx, 2, 1e-8, 10, 0, None, None, None) == feahip.EINVAL
    assert b"solve_modes_sharded: null lambda" in m._lib.feahip_last_error(m._ctx)
    assert "no modes held" in _refused(m, feahip.ESTATE, lambda: m.modes())
    # the unsharded solve still refuses a member of a group, and a sharded solve from any member drives the group
    assert "transport" in _refused(m, feahip.EINVAL, lambda: m.solve_modes(2))
    lam, res, it = m.solve_modes_sharded(2, 1e-6, 200)
    assert it > 0 and np.all(res <= 1e-6) and g.modes().shape == (feahip.MODAL_COLS, 3 * len(deck.nodes))
    g.close()
    # fewer than 24 free dofs over all ranks: a single cell clamped on one face has 12 (and rank 0 owns no row at all)
    g = group(loaded_bar("tet4", (1, 1, 1)), 2)
    assert "solve_modes_sharded: 12 free dofs, fewer than the 24" in _group_refused(g, feahip.EINVAL, lambda: g.solve_modes(1))
    g.close()
    # preconditioner 2, and members whose kinds differ
    g = group(mesh.bar_deck(dims=(6, 36, 6)), 2)                              # large enough for the multigrid kinds
    g.ranks[0].set_preconditioner(1)
    assert "solve_modes_sharded: the ranks' preconditioner kinds differ" in _group_refused(g, feahip.EINVAL, lambda: g.solve_modes(2))
    g.each("set_preconditioner", 2)
    assert "solve_modes_sharded: preconditioner 2" in _group_refused(g, feahip.EINVAL, lambda: g.solve_modes(2))
    g.close()


def test_group_spmm_km_needs_a_stiffness_matrix_and_a_mass():
    deck = DECKS["tet4"]()
    x8 = np.zeros((8, 3 * len(deck.nodes)))
    g = group(deck, 2, rho=None)
    g.each("create_stiffness_and_residual")
    assert "no mass" in _group_refused(g, feahip.ESTATE, lambda: g.spmm_km(x8))
    g.close()
    g = group(deck, 2)
    assert "no stiffness matrix" in _group_refused(g, feahip.ESTATE, lambda: g.spmm_km(x8))
    g.close()


@pytest.mark.parametrize("rank_contexts", [False, True])
def test_a_group_that_solved_modes_solves_the_linear_system_to_the_same_bits(rank_contexts):
    """The PCG's halo buffers, events and scratch are untouched: the first Newton solve after a modal solve gives the
    iteration count, the residual and the displacement increment of a group that never solved modes."""
    deck = DECKS["tet4"]()

    def linear_solve(g):
        g.each("update_nodes_with_bc", 1.0); g.each("create_stiffness_and_residual"); g.each("apply_prescribed_bc", 0.0)
        it, res = g.solve_slae(feahip.PCG_ILU, 1e-14, 5000)
        return it, res, g.gather("solution"), g.energy()

    a, b = group(deck, 2, rank_contexts), group(deck, 2, rank_contexts)
    lam, res, it = b.solve_modes(N_MODES, TOL, MAX_IT)
    assert it > 0
    ra, rb = linear_solve(a), linear_solve(b)
    assert ra[0] == rb[0] > 0 and ra[1] == rb[1] and np.array_equal(ra[2], rb[2]) and ra[3] == rb[3]
    a.close(); b.close()

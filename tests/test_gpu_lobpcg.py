"""The eigenvalue iteration of kernels_modal.hip against its restatement (lobpcg_reference.py), step by step, on an MI355X.

A solve capped at k with tolerance 1e-300 returns the block after k Rayleigh-Ritz steps.  The converged answer cannot tell
a wrong Gram block, a drifting K P, a residual formed with another column's theta or a reused column id from a right
one -- the iteration corrects itself and arrives some steps later (test_lobpcg_reference_cpu.py seeds each and measures
it); the k-th iterate can.  So theta, the eight residual ratios and the subspace of modes() after k steps are compared
with the long-double restatement: on one context for every (case, k) of lobpcg_cases.py, with the multigrid
preconditioner, over row shards and rank contexts, on the smallest body the solve accepts, and on a bar of 41^3 nodes,
the first in the suite to run the grid-stride loops of k_modal_gram and k_modal_residual.

K is the context's own (feahip_get_matrix_yale after the masked assembly: the assembly is pinned elsewhere), M the
float64 mass of dynamics_reference.py.  Tolerance, per quantity: 100 times the gap between the float64 and the
long-double restatement of that very solve, at least 1e-13 (the floor of the PCG pin); both are computed here.  The
subspace is measured as |1 - the smallest singular value of X_gpu' M X_ref|, never column against column.  Measured:
the largest error / tolerance is 0.069 for theta, 0.065 for the ratios (tet10 at k = 22) and 0.013 for the subspace.

Step counts are compared only where every comparison of a ratio with the tolerance that decides them lies outside
[1/3, 3] of it (the rule of lobpcg_cases.py).  Block-Jacobi gains a factor of 1.5 per step near a stop and the multigrid
on the 208-node bar a factor of 2, so no stop of theirs qualifies, and no locked solve that was tried does (DESIGN.md
section 15 has the search).  So the stop semantics are checked on the smallest body, whose stop does qualify, and the
locked solves of test_locked_sweeps are held to everything but their counts."""
import functools
import time

import numpy as np
import pytest
import scipy.linalg
import scipy.sparse as sp

import amg_reference as ar
import feahip
import lobpcg_cases as lc
import lobpcg_reference as lr
import mesh
from dynamics_reference import dense_mass
from pcg_cases import AMG_ENV

pytestmark = pytest.mark.gpu

BAND = (1.0 / 3.0, 3.0)
GM_MIN = 1e-10
NEVER = 1e-300                                                            # a tolerance no ratio meets: the cap ends the solve
QUANTITIES = ("theta", "ratios", "subspace")


def solver(deck, rho, kind=0):
    s = feahip.FeaSolver(deck)
    s.set_mass(rho)
    if kind:
        s.set_preconditioner(kind)
    return s


def masked_stiffness(s):
    """K as feahip_solve_modes makes it (assembled at the current nodes, the prescribed dofs masked), scalar CSR"""
    s.create_stiffness()
    s.apply_prescribed_bc(0.0)
    off, idx, val = s.matrix_yale()
    return sp.csr_matrix((val, idx, off), shape=(s.ndof, s.ndof))


def pencil_of(deck, rho, ids=None):
    """(K dense, M dense, mask, library id of every node) for a deck: K from a context of its own"""
    s = solver(deck, rho)
    K = masked_stiffness(s).toarray()
    keys = s.node_numbering().astype(np.int64)
    s.close()
    out = (K, dense_mass(deck, rho, ids), lc.prescribed_mask(deck), keys)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def pencil(name):
    deck = lc.deck_of(name)
    return pencil_of(deck, lc.density(name), lc.layered_ids(deck, 2) if name == "tet4_two_materials" else None)


def in_band(log):
    d = np.asarray(log, dtype=np.float64)
    return int(((d >= BAND[0]) & (d <= BAND[1])).sum())


def restated(K, M, mask, X0, want, tol, cap, **kw):
    """the float64 and the long-double restatement of one solve, and that they took the same way"""
    lo = lr.run(K, M, mask, X0, want, tol, cap, np.float64, **kw)
    hi = lr.run(K, M, mask, X0, want, tol, cap, np.longdouble, **kw)
    assert lo.branches == hi.branches and lo.code == hi.code and lo.steps == hi.steps
    assert min(lo.gm_log) >= GM_MIN and min(hi.gm_log) >= GM_MIN
    assert in_band(lo.decide_log) == 0 and in_band(hi.decide_log) == 0
    return lo, hi


@functools.lru_cache(maxsize=None)
def capped(name, k):
    K, M, mask, keys = pencil(name)
    X0 = lr.hash_block(keys, mask)
    return restated(K, M, mask, X0, lr.COLS, NEVER, k)


def compare(what, lam, res, phi, lo, hi, M):
    """theta, the ratios and the subspace of a solve against the long-double restatement; prints error / tolerance"""
    tol = lr.tolerances(lo, hi, M)
    err = (lr.rel(lam, hi.theta[:len(lam)]), lr.rel(res, hi.ratio[:len(res)]), lr.subspace_gap(phi.T, hi.X, M))
    print(f"LOBPCG {what}: " + ", ".join(f"{q} {e:.2e} / {t:.1e} = {e / t:.3f}" for q, e, t in zip(QUANTITIES, err, tol)))
    for q, e, t in zip(QUANTITIES, err, tol):
        assert e <= t, (what, q, e, t)


@pytest.mark.parametrize("name,k", lc.PAIRS)
def test_iterates_on_one_context(name, k):
    """The block after k steps, k in {0, 1, 2, 3, 5, 8, 22}: k = 0 is the hash through ritz_on_x, k = 22 passes the
    renewal.  The fan has 143 nodes (the last Gram tile holds 13 dofs) and a block row of 143 blocks."""
    K, M, mask, _ = pencil(name)
    lo, hi = capped(name, k)
    s = solver(lc.deck_of(name), lc.density(name))
    lam, res, it, rc = s.solve_modes(8, NEVER, k, check=False)
    phi = s.modes()
    s.close()
    assert rc == feahip.ENOTCONVERGED and it == k == hi.steps and hi.code == lr.OUT_OF_STEPS
    assert not phi[:, mask].any()
    compare(f"{name} k={k}", lam, res, phi, lo, hi, M)


def test_the_smallest_body_the_solve_accepts_and_what_its_stop_reports():
    """n_free == 24: a bar of 12 nodes, 4 of them clamped.  [X, W, P] has as many columns as there are free dofs: the
    second step's basis is the whole space, so the third stop test finds all eight ratios at rounding level (1e-14,
    seven orders below the tolerance 1e-8) where the two before were seven orders above.  The guards hold (scaled G_M
    >= 2e-3, no stop test within [1/3, 3] of the tolerance), so this is the stop whose step the device must share: j = 2.
    A cap above j and at j: j steps and FEAHIP_OK, the eight eigenvalues those of scipy.linalg.eigh on the same pencil
    to 1e-6 and the restatement's theta under the tolerance rule (ratios that are rounding noise are not compared), and
    a warm call after it touches nothing.  A cap one below: j - 1 steps, ENOTCONVERGED, and theta, `resid` -- the ratios
    on fresh products -- and the subspace are the restatement's.  What this stop does not reach: it ends because the
    basis fills the space, so the must_step continuation and a stop on a long recurrence with P are not run against a
    count, and at a cap >= j `resid` is rounding noise and only held below the tolerance.  No stop that does reach them
    meets the condition under which a step count may be compared (module docstring)."""
    deck = lc.SMALLEST()
    K, M, mask, keys = pencil_of(deck, lc.RHO)
    free = np.nonzero(~mask)[0]
    assert len(deck.nodes) == 12 and len(free) == 24
    Kf, Mf = K[np.ix_(free, free)], M[np.ix_(free, free)]
    ref = scipy.linalg.eigh(0.5 * (Kf + Kf.T), Mf, eigvals_only=True)[:8]
    X0, tol = lr.hash_block(keys, mask), 1e-8
    j = restated(K, M, mask, X0, 8, tol, 1000)[1].steps
    assert j >= 1
    s = solver(deck, lc.RHO)
    for cap in (1000, j, j - 1):
        lo, hi = restated(K, M, mask, X0, 8, tol, cap)
        lam, res, it, rc = s.solve_modes(8, tol, cap, check=False)
        phi = s.modes()
        print(f"n_free == 24, cap {cap}: steps {it} rc {rc}, restatement {hi.steps} {hi.code}, resid {res}")
        assert it == hi.steps == min(cap, j)
        assert (hi.code == lr.CONVERGED) == (cap >= j) and rc == (0 if cap >= j else feahip.ENOTCONVERGED)
        assert np.abs(phi @ M @ phi.T - np.eye(8)).max() <= 1e-10 and not phi[:, mask].any()
        if cap >= j:
            assert np.all(res <= tol) and np.all(np.abs(lam - ref) <= 1e-6 * ref)
            assert lr.rel(lam, hi.theta) <= lr.tolerances(lo, hi, M)[0]
            assert lr.subspace_gap(phi.T, hi.X, M) <= lr.FLOOR             # both span the eight lowest eigenvectors
            lam_w, res_w, it_w, rc_w = s.solve_modes(8, tol, cap, warm=True, check=False)
            assert it_w == 0 and rc_w == 0
            assert np.array_equal(lam_w, lam) and np.array_equal(res_w, res) and np.array_equal(s.modes(), phi)
        else:
            assert not np.all(res <= tol)
            compare(f"n_free == 24 cap={cap}", lam, res, phi, lo, hi, M)
    s.close()


@functools.lru_cache(maxsize=None)
def multigrid():
    """the 208-node bar with preconditioner 1: the pencil and the float64 W-cycle of amg_reference.py on the exported
    hierarchy, applied per column"""
    deck = lc.MULTIGRID[0]()
    s = solver(deck, lc.RHO, kind=1)
    Ks = masked_stiffness(s)
    info = s.amg_info()
    levels = [s.amg_level(l) for l in range(info["levels"])]
    mask = lc.prescribed_mask(deck)
    nodes = np.arange(s.N)
    keys = s.node_numbering().astype(np.int64)
    cyc, _ = ar.from_export(Ks, mask, info, levels, nodes, keys[nodes], restate=False)
    s.close()
    return deck, Ks.toarray(), dense_mass(deck, lc.RHO), mask, keys, cyc


@pytest.mark.parametrize("k", lc.MULTIGRID[1])
def test_iterates_with_the_multigrid_preconditioner(k, monkeypatch):
    """W of every step is the reference W-cycle of the masked residual, column by column, masked: the block after 1 and
    3 steps under the same tolerance rule."""
    for e in AMG_ENV:
        monkeypatch.delenv(e, raising=False)
    deck, K, M, mask, keys, cyc = multigrid()
    lo, hi = restated(K, M, mask, lr.hash_block(keys, mask), lr.COLS, NEVER, k, precond=cyc.apply)
    s = solver(deck, lc.RHO, kind=1)
    lam, res, it, rc = s.solve_modes(8, NEVER, k, check=False)
    phi = s.modes()
    s.close()
    assert rc == feahip.ENOTCONVERGED and it == k == hi.steps
    compare(f"multigrid k={k}", lam, res, phi, lo, hi, M)


SHARDS = [(name, n, rc) for name, (_, ranks) in lc.SHARDED.items() for n in ranks for rc in (False, True)
          if not (rc and name == "bar_54_one_super")]               # (rank contexts cut by node planes: another partition)


@functools.lru_cache(maxsize=None)
def sharded_pencil(name):
    return pencil(name) if name in lc.CASES else pencil_of(lc.SHARDED[name][0](), lc.RHO)


@pytest.mark.parametrize("name,n,rank_contexts", SHARDS)
def test_iterates_sharded(name, n, rank_contexts):
    """The same restatement for n in-process ranks after 1, 3 and 8 steps: the start block is keyed by the library id of a
    node on row shards and by the caller's id in the whole mesh on rank contexts (ensure_modal_dist), the sums are
    all-reduced, nothing else differs.  The stitched modes() span the restatement's subspace, and a rank's own modes()
    are zero off its rows.  With three ranks rank 0 of the tet4 bar owns no row, and two ranks of the 54-node bar own
    none."""
    deck = lc.SHARDED[name][0]()
    K, M, mask, keys = sharded_pencil(name)
    X0 = lr.hash_block(np.arange(len(keys)) if rank_contexts else keys, mask)
    g = feahip.FeaGroup(deck, n, rank_contexts=rank_contexts)
    g.set_mass(lc.RHO)
    if name == "bar_54_one_super":
        assert sorted(len(nd) for nd in g.nodes) == [0, 0, len(deck.nodes)]
    if name == "tet4" and n == 3 and not rank_contexts:
        assert len(g.nodes[0]) == 0
    for k in lc.SHARDED_K:
        lo, hi = restated(K, M, mask, X0, lr.COLS, NEVER, k)
        lam, res, it, rc = g.solve_modes(8, NEVER, k, check=False)
        phi = g.modes()
        assert rc == feahip.ENOTCONVERGED and it == k == hi.steps
        compare(f"{name} n={n} rank_contexts={rank_contexts} k={k}", lam, res, phi, lo, hi, M)
        for r, nd in zip(g.ranks, g.nodes):
            own = np.arange(r.n_own) if rank_contexts else nd
            off = np.ones(r.N, dtype=bool)
            off[own] = False
            p = r.modes().reshape(8, -1, 3)
            assert not p[:, off].any() and (p[:, own].any() or len(own) == 0)
    g.close()


def test_grid_stride_loops_on_a_bar_of_41_cubed_nodes():
    """68921 nodes, 206763 dofs: 6462 Gram tiles over 2048 workgroups and 2154 residual blocks over 2048 -- the loops
    `tile += gridDim.x` of k_modal_gram (with its __syncthreads inside) and `a += gridDim.x * 32` of k_modal_residual run
    more than once, which no smaller test reaches.  Three steps; K is the library's own Yale matrix as CSR, M the sparse
    mass of lobpcg_reference.py, both restatements with every product and sum in their precision.  The host side takes
    the time of this one test -- measured 24 s in all: 0.8 s to set up, under 0.1 s for the device's solve, 23 s for the two
    restatements, under the 60 s at which the long-double products would have to go -- so they stay."""
    t0 = time.time()
    nx, ny, nz = lc.GRID_STRIDE_DIMS
    deck = mesh.bar_deck(dims=lc.GRID_STRIDE_DIMS)
    assert len(deck.nodes) == (nx + 1) * (ny + 1) * (nz + 1) > 65536
    s = solver(deck, lc.RHO)
    Ks = masked_stiffness(s)
    keys = s.node_numbering().astype(np.int64)
    K = (Ks.indptr.astype(np.int64), Ks.indices.astype(np.int64), Ks.data)
    M = lr.sparse_mass(deck, lc.RHO)
    mask = lc.prescribed_mask(deck)
    k = lc.GRID_STRIDE_K
    t1 = time.time()
    lam, res, it, rc = s.solve_modes(8, NEVER, k, check=False)
    phi = s.modes()
    s.close()
    t2 = time.time()
    assert rc == feahip.ENOTCONVERGED and it == k
    lo, hi = restated(K, M, mask, lr.hash_block(keys, mask), lr.COLS, NEVER, k)
    t3 = time.time()
    print(f"LOBPCG grid stride: setup {t1 - t0:.1f} s, device solve {t2 - t1:.1f} s, restatements {t3 - t2:.1f} s")
    assert hi.steps == k and not phi[:, mask].any()
    compare(f"41^3 nodes k={k}", lam, res, phi, lo, hi, M)


def invariant_count(lam, n_modes, shift):
    """the largest m <= n_modes at which the spectrum has a gap (lam[m] - lam[m-1] at least 1e-3 of lam[m-1] + shift): the
    span of the first m eigenvectors is defined, that of a block cut through a degenerate group is not"""
    for m in range(n_modes, 0, -1):
        if lam[m] - lam[m - 1] >= 1e-3 * (abs(lam[m - 1]) + shift):
            return m
    return 0


@pytest.mark.parametrize("name", list(lc.LOCKED))
def test_locked_sweeps(name):
    """feahip_solve_modes_locked for 12 modes, on the supported tet4 bar and on the free tet4 block with the two-digit
    shift, against run_locked in long double and scipy.linalg.eigh on the same pencil.  The counts (steps, sweeps, locks)
    are printed next to the restatement's and not asserted: 11 to 21 of the ratios that decide them lie within [1/3, 3]
    of the tolerance, for every tolerance of the set.  Asserted: lambda within 1e-6 (|ref| + shift) of eigh (the bound
    of test_gpu_modal_locked.py) and so within 2e-6 of the restatement's; resid <= tol; locked_modes() M-orthonormal to
    1e-10 and zero on the supports; and they span the restatement's locked subspace up to the last gap of the spectrum
    at or below mode 12 (the free block's modes 12 and 13 are a degenerate pair): each side is within an angle of
    sqrt(m) 2 tol sqrt(cond M) / relative gap of the invariant subspace, and |1 - sigma_min| <= angle^2 / 2 + 1e-10
    for the two angles added.  Then a cap one step short of the end, inside the last sweep: ENOTCONVERGED, and what the
    earlier sweeps locked -- count, lambda, resid, modes -- is there to the bit, the rest NaN."""
    make, n_modes, shifted = lc.LOCKED[name]
    deck = make()
    K, M, mask, keys = pencil_of(deck, lc.RHO)
    free = np.nonzero(~mask)[0]
    Kf, Mf = K[np.ix_(free, free)], M[np.ix_(free, free)]
    ref = scipy.linalg.eigh(0.5 * (Kf + Kf.T), Mf, eigvals_only=True)
    shift, tol = (lc.two_digits(ref[6]) if shifted else 0.0), 1e-8
    hi = lr.run_locked(lr.shifted_pencil(K, M, mask, shift), M, mask, keys, n_modes, shift, tol, 4000, np.longdouble)
    assert hi.code == lr.CONVERGED
    s = solver(deck, lc.RHO)
    lam, res, steps, sweeps = s.solve_modes_locked(n_modes, shift, tol, 4000)
    Q = s.locked_modes()
    print(f"locked {name}: shift {shift}, device steps {steps} sweeps {sweeps}, restatement steps {hi.steps} sweeps {hi.sweeps} "
          f"locks {hi.locks}")
    scale = np.abs(ref[:n_modes]) + shift
    assert np.all(np.abs(lam - ref[:n_modes]) <= 1e-6 * scale) and np.all(np.abs(lam - hi.lam) <= 2e-6 * scale)
    assert np.all(res <= tol) and np.all(np.diff(lam) >= 0) and sweeps >= 2
    assert Q.shape == (n_modes, len(mask)) and not Q[:, mask].any()
    assert np.abs(Q @ M @ Q.T - np.eye(n_modes)).max() <= 1e-10
    m = invariant_count(ref, n_modes, shift)
    assert m >= 6
    angle = 2.0 * np.sqrt(m) * 2.0 * tol * np.sqrt(np.linalg.cond(Mf)) * (abs(ref[m - 1]) + shift) / (ref[m] - ref[m - 1])
    gap = lr.subspace_gap(Q[:m].T, hi.Q[:, :m], M)
    print(f"locked {name}: the first {m} modes span the restatement's to {gap:.2e} (bound {angle ** 2 / 2 + 1e-10:.1e})")
    assert gap <= angle ** 2 / 2 + 1e-10
    lam_c, res_c, steps_c, sweeps_c, rc = s.solve_modes_locked(n_modes, shift, tol, steps - 1, check=False)
    n = s.locked_count()
    print(f"locked {name}: cap {steps - 1}: rc {rc}, sweep {sweeps_c}, {n} modes locked")
    assert rc == feahip.ENOTCONVERGED and steps_c == steps - 1 and sweeps_c == sweeps and 0 < n < n_modes
    assert np.all(np.isnan(lam_c[n:])) and np.all(np.isnan(res_c[n:]))
    at = [int(np.flatnonzero(lam == v)[0]) for v in lam_c[:n]]         # (the full solve sorts all twelve once more)
    assert np.array_equal(lam[at], lam_c[:n]) and np.array_equal(res[at], res_c[:n])
    assert np.array_equal(s.locked_modes(), Q[at])
    s.close()

"""The PCG loops of kernels_solve.hip against their restatement (pcg_reference.py), iterate by iterate, on an MI355X.

A solve capped at k with tolerance 0 returns x_k.  The converged solution cannot tell a wrong p.q, beta, partial-sum slot
or preconditioned residual from a right one -- CG corrects itself and arrives a few iterations later; x_k can.  So x_k
of both loops (two reductions, one reduction) is compared with x_k of the long-double restatement, on one context and
sharded, with plain CG, block-Jacobi and the multigrid, on the smallest meshes that reach each branch of the vector
kernels and of the fused dot (pcg_cases.py), at the k where the restatement is sure of itself
(pcg_reference.iterate_checks; test_pcg_reference_cpu.py shows every mesh keeps three such k).  Then the mechanics around
the recurrence: a stop inside the first batch, a stop after several batches with the cap above, at and below it, what
`iters` and `resid` say each time, two right-hand sides, and the breakdown return.  About 1 s per test.

K and f are read back from the context: the assembly is pinned elsewhere (test_gpu_parity.py)."""
import numpy as np
import pytest
import scipy.sparse as sp

import amg_reference as ar
import feahip
import mesh
import pcg_cases as pc
import pcg_reference as pr

pytestmark = pytest.mark.gpu

SOLVERS = {"cg": feahip.CG, "block_jacobi": feahip.PCG_ILU}
RESID_TOL = 1e-10        # `resid` against the restatement's recurrence residual, relative
MG_FLOOR = 1e-11         # the multigrid loop: the cycle itself is held to 1e-12 (test_gpu_multigrid.Z_TOL)
TOL_BATCH = 1e-6
AMG_ENV = pc.AMG_ENV

_SYSTEMS = {}            # what a test computes once: K, f of a mesh and the restatement's runs on them
_CHECKS = {}


def yale(s):
    off, idx, val = s.matrix_yale()
    return sp.csr_matrix((val, idx, off), shape=(s.ndof, s.ndof))


def one_context(deck, x=None, variant=0, kind=0):
    s = feahip.FeaSolver(deck)
    s.set_pcg_variant(variant)
    pc.masked_system(s, x)
    if kind:
        s.set_preconditioner(kind)
    return s


def group(deck, n, variant, rank_contexts=False):
    g = feahip.FeaGroup(deck, n, rank_contexts=rank_contexts)
    g.each("set_pcg_variant", variant)
    g.each("update_nodes_with_bc", 1.0); g.each("create_stiffness_and_residual"); g.each("apply_prescribed_bc", 0.0)
    return g


def system(key, s):
    """K, f of context s, kept unchanged for every test of the mesh `key`"""
    if key not in _SYSTEMS:
        _SYSTEMS[key] = (yale(s), s.forces().copy())
    return _SYSTEMS[key]


def reference_system(key, deck, x=None):
    """the same from a context of its own, for the tests that run a group"""
    if key not in _SYSTEMS:
        one = one_context(deck, x)
        system(key, one)
        one.close()
    return _SYSTEMS[key]


def precond(K, pname):
    return pr.block_jacobi(K) if pname == "block_jacobi" else None


def checks(key, K, f, pname, variant):
    k = (key, pname, variant)
    if k not in _CHECKS:
        _CHECKS[k] = pr.iterate_checks(K, f, precond(K, pname), variant)
        assert len(_CHECKS[k]) >= 3, (k, sorted(_CHECKS[k]))
    return _CHECKS[k]


def free_run(key, K, f, pname, variant, cap=8):
    k = (key, pname, variant, "free", cap)
    if k not in _CHECKS:
        _CHECKS[k] = pr.FORMS[variant](K, f, precond(K, pname), 0.0, cap, np.longdouble)
    return _CHECKS[k]


def compare_iterates(solve, solution, chk, res, what):
    """solve(tol, cap) -> (iters, resid); every usable x_k against the restatement's, and what the capped solve reports"""
    for k, (xk, tol, gap, step) in sorted(chk.items()):
        it, resid = solve(0.0, k)
        err = pr.linf(solution(), xk, xk)
        print(f"{what} k={k}: |x_k - ref| = {err:.2e} (tolerance {tol:.1e}, gap {gap:.1e}, step {step:.1e}), "
              f"resid {resid:.15e} ref {float(res[k]):.15e}")
        assert it == k, (what, k, it)
        assert err <= tol, (what, k, err, tol)
        assert abs(resid - float(res[k])) <= RESID_TOL * float(res[k]), (what, k, resid, float(res[k]))


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("name", list(pc.MESHES))
def test_iterates_on_one_context(name, variant):
    """x_k and resid_k of a solve capped at k, plain CG and block-Jacobi, against the long-double restatement.
    Tolerance: 100 times the restatement's own float64-to-long-double gap at that k, at least 1e-13, at most 1e-10."""
    deck, x = pc.case(name)
    s = one_context(deck, x, variant)
    K, f = system(name, s)
    if name == "fan_hub_143_blocks":
        assert np.diff(K.indptr).max() == 3 * 143                    # the long-row branch runs
    for pname, solver in SOLVERS.items():
        chk = checks(name, K, f, pname, variant)
        res = free_run(name, K, f, pname, variant).res
        compare_iterates(lambda tol, cap: s.solve_slae(solver, tol, cap), s.solution, chk, res, f"{name} {pname} v{variant}")
    s.close()


SHARDS = [(name, n, rc) for name, (_, ranks) in pc.SHARDED.items() for n in ranks for rc in (False, True)
          if not (rc and name == "bar_54_one_super")]               # (rank contexts cut by node planes: another partition)


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("name,n,rank_contexts", SHARDS)
def test_iterates_sharded(name, n, rank_contexts, variant):
    """The same comparison for n in-process ranks, whole-mesh contexts with a row shard and rank contexts: the same
    recurrence, so the same tolerance rule.  What each mesh reaches is said at pcg_cases.SHARDED and asserted on the host
    (test_shards_reach_the_branches_they_are_there_for): a rank whose interior range is empty, ranks with nothing in front
    of or behind it, ranks without rows."""
    deck = pc.SHARDED[name][0]()
    key = "sharded_" + name
    K, f = reference_system(key, deck)
    g = group(deck, n, variant, rank_contexts)
    for pname, solver in SOLVERS.items():
        chk = checks(key, K, f, pname, variant)
        res = free_run(key, K, f, pname, variant).res
        compare_iterates(lambda tol, cap: g.solve_slae(solver, tol, cap), lambda: g.gather("solution"), chk, res,
                         f"{name} n={n} rc={rank_contexts} {pname} v{variant}")
    g.close()


@pytest.mark.parametrize("sharded", [False, True])
@pytest.mark.parametrize("variant", [0, 1])
def test_stop_inside_the_first_batch(variant, sharded):
    """A tolerance between the residual of iteration j <= 8 and everything before it (a factor >= 1.22 each way): the
    flag fires at j, in the middle of the 32 iterations enqueued, and the rest must be no-ops: iters == j, resid the
    restatement's, x == x_j.  (x0 = f leaves these residuals above 1: it is the mechanics that are under test.)"""
    deck, _ = pc.case("tet4_144")
    K, f = reference_system("tet4_144", deck)
    s = group(deck, 2, variant) if sharded else one_context(deck, None, variant)
    for pname, solver in SOLVERS.items():
        free = free_run("tet4_144", K, f, pname, variant)
        j, tol = pr.stop_in_first_batch(free.res)
        ref = pr.FORMS[variant](K, f, precond(K, pname), tol, 100, np.longdouble)
        assert ref.stopped and ref.iters == j
        it, resid = s.solve_slae(solver, tol, 20000)
        u = s.gather("solution") if sharded else s.solution()
        at_j = pr.iterate_checks(K, f, precond(K, pname), variant, ks=(j,))
        assert j in at_j                                             # the restatement is sure of x_j, and x_j is not x_{j-1}
        xj, xtol = at_j[j][:2]
        print(f"{pname} v{variant} sharded={sharded}: j={j} tol={tol:.3e} it={it} resid={resid:.15e} ref={float(ref.resid):.15e}")
        assert it == j
        assert abs(resid - float(ref.resid)) <= RESID_TOL * float(ref.resid)
        assert pr.linf(u, xj, xj) <= xtol
    s.close()


def batch_checks(s, K, f, M, solver, what):
    """A stop after several batches, then the cap above, at and below the stopping iteration."""
    counts = pr.iteration_counts(K, f, M, TOL_BATCH, 2000)
    margin = max(counts) - min(counts) + 2
    it, resid = s.solve_slae(solver, TOL_BATCH, 20000)
    u = s.solution()
    print(f"{what}: restatement {counts}, library {it}, resid {resid:.6e}")
    assert min(counts) - margin <= it <= max(counts) + margin
    drift = {k: pr.residual_drift(K, f, M, k) for k in (it - 1, it)}

    def resid_is_true(u, resid, k):
        true = pr.true_residual(K, f, u)
        bound = min(100.0 * drift[k], 1e-3)
        print(f"{what}: at {k} resid {resid:.9e}, |f - K u| / |f| = {true:.9e}, relative difference {abs(resid - true) / true:.2e} "
              f"(bound {bound:.1e}, restatement's drift {drift[k]:.1e})")
        assert abs(resid - true) <= bound * true, (what, k, resid, true)

    assert resid <= TOL_BATCH
    resid_is_true(u, resid, it)
    it2, resid2 = s.solve_slae(solver, TOL_BATCH, 10 * it)           # iterations enqueued after the flag change nothing
    assert it2 == it and resid2 == resid and np.array_equal(s.solution(), u)
    it3, resid3 = s.solve_slae(solver, TOL_BATCH, it)                # the cap at the stopping iteration: the same iterate,
    assert np.array_equal(s.solution(), u)                           # and it is reported as what it is
    assert it3 == it and resid3 <= TOL_BATCH
    resid_is_true(s.solution(), resid3, it)
    it4, resid4 = s.solve_slae(solver, TOL_BATCH, it - 1)            # one short: another iterate, not converged
    u4 = s.solution()
    assert it4 == it - 1 and resid4 > TOL_BATCH and not np.array_equal(u4, u)
    resid_is_true(u4, resid4, it - 1)
    x = np.random.default_rng(8).standard_normal(s.ndof)             # the flag is left clear: a stand-alone product runs
    y = s.spmv(x)
    assert np.abs(y - K @ x).max() <= 1e-13 * np.abs(K @ x).max()
    return it


@pytest.mark.parametrize("variant", [0, 1])
def test_stop_across_batches_block_jacobi(variant):
    """tol = 1e-6 on the 144-node bar with block-Jacobi: 80 iterations, two batches of 32 and half of a third.  The three
    variants of the restatement (float64 two-reduction, float64 single-reduction, long double) all need 80 -- spread 0,
    so the library's count must be within 2 of that.  `resid` is the true |f - K u| / |f| of the u returned to 100 times
    the restatement's drift between its recurrence and its true residual (2e-9 at iteration 80, 5e-9 at 79; the library's
    own is 2e-9 .. 1.3e-8), whether the solve ended by its flag or by its cap."""
    deck = mesh.bar_deck(dims=pc.BATCH_DIMS)
    s = one_context(deck, None, variant)
    K, f = system("batch", s)
    it = batch_checks(s, K, f, pr.block_jacobi(K), feahip.PCG_ILU, f"block-Jacobi v{variant}")
    assert it > 64
    s.close()


def multigrid_context(monkeypatch, variant):
    for k in AMG_ENV:
        monkeypatch.delenv(k, raising=False)
    deck = mesh.bar_deck(dims=pc.MULTIGRID_DIMS)
    s = one_context(deck, None, variant, kind=1)
    K, f = system("multigrid", s)
    info = s.amg_info()
    levels = [s.amg_level(l) for l in range(info["levels"])]
    mask = np.zeros(s.ndof, dtype=bool)
    mask[pc.prescribed_dofs(deck)] = True
    nodes = np.arange(s.N)
    cyc, _ = ar.from_export(K, mask, info, levels, nodes, s.node_numbering()[nodes], restate=False)
    return s, K, f, cyc


@pytest.mark.parametrize("variant", [0, 1])
def test_multigrid_loop_iterates(variant, monkeypatch):
    """Preconditioner 1 on the 208-node bar: x_k, k in {1, 2, 4}, against pcg(..., M = the reference cycle built from the
    exported hierarchy).  Tolerance: 100 times the float64-to-long-double gap of that restatement (measured: 2e-15 at
    k = 1, 2e-14 at k = 4; the library is 3e-14 from it at k = 4), at least 1e-11 -- the cycle itself is held to 1e-12 of its reference."""
    s, K, f, cyc = multigrid_context(monkeypatch, variant)
    chk = pr.iterate_checks(K, f, cyc.apply, variant, ks=(1, 2, 4), floor=MG_FLOOR)
    assert sorted(chk) == [1, 2, 4]
    res = pr.FORMS[variant](K, f, cyc.apply, 0.0, 4, np.longdouble).res
    compare_iterates(lambda tol, cap: s.solve_slae(feahip.PCG_ILU, tol, cap), s.solution, chk, res, f"multigrid v{variant}")
    s.close()


@pytest.mark.parametrize("variant", [0, 1])
def test_stop_across_batches_multigrid(variant, monkeypatch):
    """The same as with block-Jacobi with batches of 8 iterations: the restatement's three variants agree on the count
    (44 each, spread 0 measured), the library is within 2 (44 measured)."""
    s, K, f, cyc = multigrid_context(monkeypatch, variant)
    it = batch_checks(s, K, f, cyc.apply, feahip.PCG_ILU, f"multigrid v{variant}")
    assert it > 8
    s.close()


@pytest.mark.parametrize("name", ["tet4_144", "tet4_64_tail_node"])
def test_two_right_hand_sides_iterate_by_iterate(name):
    """feahip_solve_slae2 capped at k: each column is x_k of the single-column restatement of its own right-hand side."""
    deck, x = pc.case(name)
    s = one_context(deck, x, 0)
    K, f = system(name, s)
    f2 = np.random.default_rng(5).standard_normal(s.ndof)
    f2[pc.prescribed_dofs(deck)] = 0.0
    for pname, solver in SOLVERS.items():
        M = precond(K, pname)
        c1, c2 = checks(name, K, f, pname, 0), pr.iterate_checks(K, f2, M, 0)
        ks = sorted(set(c1) & set(c2))
        assert len(ks) >= 3
        r1, r2 = free_run(name, K, f, pname, 0).res, pr.pcg(K, f2, M, 0.0, 8, np.longdouble).res
        for k in ks:
            it, resid = s.solve_slae2(f2, solver, 0.0, k)
            assert list(it) == [k, k]
            for u, (xk, tol, _, _), rk, rs in ((s.solution(), c1[k], r1[k], resid[0]), (s.solution2(), c2[k], r2[k], resid[1])):
                err = pr.linf(u, xk, xk)
                print(f"{name} {pname} k={k}: {err:.2e} (tolerance {tol:.1e})")
                assert err <= tol
                assert abs(rs - float(rk)) <= RESID_TOL * float(rk)
    s.close()


@pytest.mark.parametrize("sharded", [False, True])
@pytest.mark.parametrize("variant", [0, 1])
def test_breakdown_is_reported_and_leaves_nothing_behind(variant, sharded):
    """A NaN in one free entry of f: the kernels do their arithmetic on it, the first iteration's sums are NaN, and the
    solve returns ENOTCONVERGED with "CG breakdown".  The next solve on the same context with the good f gives the bits
    of a context that never saw the NaN."""
    deck, _ = pc.case("tet4_144")

    def make():
        return group(deck, 2, variant) if sharded else one_context(deck, None, variant)

    def solve(s, solver):
        it, resid = s.solve_slae(solver, 1e-12, 20000)
        return it, resid, (s.gather("solution") if sharded else s.solution())

    fresh = make()
    want = {pname: solve(fresh, solver) for pname, solver in SOLVERS.items()}
    fresh.close()
    s = make()
    contexts = s.ranks if sharded else [s]
    good = [c.forces() for c in contexts]
    free = np.setdiff1d(np.arange(len(good[0])), pc.prescribed_dofs(deck))
    for pname, solver in SOLVERS.items():
        for c, f in zip(contexts, good):
            bad = f.copy()
            bad[free[len(free) // 2]] = np.nan
            c.set_forces(bad)
        with pytest.raises(feahip.FeaHipError) as e:
            s.solve_slae(solver, 1e-12, 20000)
        assert f"error {feahip.ENOTCONVERGED}" in str(e.value) and "CG breakdown" in str(e.value)
        for c, f in zip(contexts, good):
            c.set_forces(f)
        it, resid, u = solve(s, solver)
        assert (it, resid) == want[pname][:2] and np.array_equal(u, want[pname][2])
    s.close()

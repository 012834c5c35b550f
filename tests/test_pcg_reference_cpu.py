"""The float64 / long-double restatement of the PCG loops (pcg_reference.py), validated on the CPU oracle's K before the
GPU is held to it iterate by iterate (test_gpu_pcg.py): it reaches the dense solve, its two forms and two precisions
agree at the iterates the GPU test uses -- on every mesh of that test, which is what lets it use them -- its stop, count
and breakdown semantics are the kernels' on a hand-made 6x6 system, and its 3x3 inverse is the library's formula.  The
last tests break the recurrence on purpose and show that the iterate comparison sees what a converged solve cannot."""
import numpy as np
import pytest
import scipy.sparse as sp

import feahip
import mesh
import pcg_cases as pc
import pcg_reference as pr
from oracle_binding import OracleSolver

_SYSTEMS = {}


def system(key, deck, x=None):
    if key not in _SYSTEMS:
        o = OracleSolver(deck)
        pc.masked_system(o, x)
        K = sp.csr_matrix((o.values().copy(), o.indexes().copy(), o.offsets().copy()), shape=(o.ndof, o.ndof))
        f = o.forces().copy()
        o.solve_slae(feahip.CHOLESKY)
        u = o.solution().copy()
        o.close()
        _SYSTEMS[key] = (K, f, u)
    return _SYSTEMS[key]


def all_cases():
    out = {name: (lambda n=name: pc.case(n)) for name in pc.MESHES}
    for name, (make, _) in pc.SHARDED.items():
        out.setdefault("sharded_" + name, lambda m=make: (m(), None))
    out["multigrid_bar"] = lambda: (mesh.bar_deck(dims=pc.MULTIGRID_DIMS), None)
    return out


CASES = all_cases()


def preconditioners(K):
    return {"cg": None, "block_jacobi": pr.block_jacobi(K)}


@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("precond", ["cg", "block_jacobi"])
def test_restatement_reaches_the_dense_solve(form, precond):
    K, f, u = system("tet4_144", *pc.case("tet4_144"))
    dense = np.linalg.solve(K.toarray(), f)
    assert pr.linf(dense, u, u) < 1e-10                              # the oracle's Cholesky, for the record
    r = pr.FORMS[form](K, f, preconditioners(K)[precond], 1e-13, 5000, np.float64)
    assert r.stopped and not r.broke and 0 < r.iters < 5000 and r.resid <= 1e-13
    assert len(r.x) == r.iters + 1 and len(r.res) == r.iters + 1
    assert pr.linf(r.x[r.iters], dense, dense) < 1e-10
    assert abs(pr.true_residual(K, f, r.x[r.iters]) - r.resid) < 1e-12


@pytest.mark.parametrize("name", list(CASES))
def test_forms_and_precisions_agree_where_the_gpu_test_compares(name):
    """For every mesh of test_gpu_pcg.py, plain CG and block-Jacobi, both forms: at least three k of {1, 2, 3, 5, 8}
    pass iterate_checks' conditions (float64 and long double agree to 1e-12, the iterate moved by more than 1e-3), the
    two forms give the same x_k to 1e-12 there, and the tolerance the GPU test will use is between its floor and its
    ceiling.  Measured on these meshes: the gap is at most 3e-14 except on the hex8 bar with plain CG at k = 8 (8e-13,
    tolerance 8e-11); the step is at least 3e-2."""
    deck, x = CASES[name]()
    K, f, _ = system(name, deck, x)
    for pname, M in preconditioners(K).items():
        checks = [pr.iterate_checks(K, f, M, v) for v in (0, 1)]
        for v in (0, 1):
            assert len(checks[v]) >= 3, (name, pname, v, sorted(checks[v]))
            for k, (xk, tol, gap, step) in checks[v].items():
                assert gap <= pr.GAP_MAX and step > pr.STEP_MIN
                assert pr.TOL_FLOOR <= tol <= pr.TOL_CEIL and tol >= min(100 * gap, pr.TOL_CEIL)
        for k in set(checks[0]) & set(checks[1]):
            assert pr.linf(checks[0][k][0], checks[1][k][0], checks[0][k][0]) <= 1e-12, (name, pname, k)


def small_system():
    """6x6: two 3x3 blocks, K = diag(1..6) plus a weak coupling, f = ones.  Plain CG ends in at most 6 steps."""
    K = np.diag(np.arange(1.0, 7.0))
    K[0, 3] = K[3, 0] = 0.25
    K[2, 5] = K[5, 2] = -0.5
    return sp.csr_matrix(K), np.ones(6)


@pytest.mark.parametrize("form", [0, 1])
def test_stop_and_count_semantics(form):
    K, f = small_system()
    run = pr.FORMS[form]
    free = run(K, f, None, 0.0, 4, np.float64)                       # tolerance 0: the cap ends it
    assert free.iters == 4 and not free.stopped and not free.broke
    assert len(free.x) == 5 and np.array_equal(free.x[0], f)         # x0 = f
    assert free.resid == free.res[4]
    assert free.res[0] == pytest.approx(np.linalg.norm(f - K @ f) / np.linalg.norm(f), rel=1e-15)
    for k in range(1, 5):                                            # every recurrence residual is its iterate's
        assert free.res[k] == pytest.approx(pr.true_residual(K, f, free.x[k]), rel=1e-12)
    assert all(free.res[k] < free.res[k - 1] for k in (1, 2, 3))     # (so the tolerances below single out one iteration)
    for j in (1, 2, 3):
        tol = float(np.sqrt(free.res[j] * free.res[j - 1]))
        for cap in (j, j + 1, 50):                                   # the test fires at j, whatever was allowed beyond it
            r = run(K, f, None, tol, cap, np.float64)
            assert r.stopped and r.iters == j and r.resid == free.res[j] and len(r.x) == j + 1
            assert np.array_equal(r.x[j], free.x[j])
        if j > 1:
            r = run(K, f, None, tol, j - 1, np.float64)              # the cap comes first: not a stop
            assert not r.stopped and r.iters == j - 1 and r.resid == free.res[j - 1] > tol
    # `<=`, not `<`: an exact start vector has r.r = 0 = tol^2 b.b at tolerance 0, and is solved before the first iteration
    e = np.zeros(6); e[1] = 1.0                                      # K e = 2 e ... with f = 2 e the start x0 = f is not exact,
    Kone = sp.identity(6, format="csr")                              # with K = 1 it is
    r = run(Kone, e, None, 0.0, 10, np.float64)
    assert r.stopped and r.iters == 0 and r.resid == 0.0 and len(r.x) == 1
    r = run(K, np.zeros(6), None, 1e-6, 10, np.float64)              # a zero right-hand side too (resid = sqrt(r.r))
    assert r.stopped and r.iters == 0 and r.resid == 0.0
    r = run(K, f, None, 1e3, 10, np.float64)                         # and a tolerance the start already meets
    assert r.stopped and r.iters == 0 and r.resid == free.res[0]
    # r.z == 0 with r != 0 (a preconditioner that annihilates r) counts as solved at the start, as in the kernels
    r = run(K, f, np.zeros((2, 3, 3)), 0.0, 10, np.float64)
    assert r.stopped and r.iters == 0 and r.resid == free.res[0] > 0
    bad = f.copy(); bad[4] = np.nan                                  # NaN data: breakdown in the first iteration
    r = run(K, bad, None, 1e-6, 10, np.float64)
    assert r.broke and not r.stopped and r.iters == 1


def test_two_forms_are_one_recurrence_on_the_small_system():
    K, f = small_system()
    M = pr.block_jacobi(K)
    for dtype in (np.float64, np.longdouble):
        a = pr.pcg(K, f, M, 0.0, 5, dtype)
        b = pr.pcg_single_reduction(K, f, M, 0.0, 5, dtype)
        for k in range(6):
            assert pr.linf(a.x[k], b.x[k], a.x[k]) < 1e-13
            assert abs(a.res[k] - b.res[k]) <= 1e-12 * a.res[0]
    exact = np.linalg.solve(K.toarray(), f)
    r = pr.pcg(K, f, None, 0.0, 6, np.longdouble)                    # plain CG: exact after 6 steps
    assert pr.linf(r.x[6], exact, exact) < 1e-12


def test_block_inverse_is_the_library_formula():
    """adjugate / determinant of every diagonal block; the identity where the determinant is 0 or NaN (k_precond_build)"""
    rng = np.random.default_rng(2)
    blocks = []
    for _ in range(5):
        a = rng.standard_normal((3, 3))
        blocks.append(a @ a.T + 0.1 * np.eye(3))
    blocks.append(np.zeros((3, 3)))                                  # a node no element uses
    blocks.append(np.array([[1.0, 2.0, 3.0], [2.0, 4.0, 6.0], [0.0, 0.0, 1.0]]))   # singular, exactly
    nan = np.eye(3); nan[1, 1] = np.nan
    blocks.append(nan)
    n = len(blocks)
    K = sp.lil_matrix((3 * n, 3 * n))
    for a, b in enumerate(blocks):
        K[3 * a:3 * a + 3, 3 * a:3 * a + 3] = b
    K[0, 5] = K[5, 0] = 7.0                                          # off the diagonal blocks: not the preconditioner's business
    M = pr.block_jacobi(K.tocsr())
    for a in range(5):
        assert np.abs(M[a] @ blocks[a] - np.eye(3)).max() < 1e-12
        assert np.abs(M[a] - np.linalg.inv(blocks[a])).max() <= 1e-12 * np.abs(M[a]).max()
    for a in (5, 6, 7):
        assert np.array_equal(M[a], np.eye(3))
    d = blocks[0].ravel()                                            # one entry spelled out: m[1] = (d2 d7 - d1 d8) / det
    det = d[0] * (d[4] * d[8] - d[5] * d[7]) - d[1] * (d[3] * d[8] - d[5] * d[6]) + d[2] * (d[3] * d[7] - d[4] * d[6])
    assert M[0][0, 1] == (d[2] * d[7] - d[1] * d[8]) * (1.0 / det)


def test_first_batch_stops_exist_for_the_gpu_test():
    """stop_in_first_batch finds, on the mesh the GPU test stops on, an iteration j <= 8 whose residual is 1.5 times under
    everything before it; the restatement run at the tolerance it returns stops there, in both forms and precisions."""
    K, f, _ = system("tet4_144", *pc.case("tet4_144"))
    for pname, M in preconditioners(K).items():
        for v in (0, 1):
            free = pr.FORMS[v](K, f, M, 0.0, 8, np.longdouble)
            j, tol = pr.stop_in_first_batch(free.res)
            assert 1 < j <= 8 and tol > 1.0                          # (x0 = f: the residuals are still above |f|)
            for dtype in (np.float64, np.longdouble):
                r = pr.FORMS[v](K, f, M, tol, 100, dtype)
                assert r.stopped and r.iters == j
                assert float(r.resid) == pytest.approx(float(free.res[j]), rel=1e-12)


def test_counts_at_1e_6_agree_among_the_variants():
    """The three variants the GPU test's margin is made of, on its mesh: 80 iterations each, spread 0 (measured)."""
    K, f, _ = system("batch", mesh.bar_deck(dims=pc.BATCH_DIMS))
    M = pr.block_jacobi(K)
    counts = pr.iteration_counts(K, f, M, 1e-6, 2000)
    assert max(counts) - min(counts) <= 3 and min(counts) > 64      # two full batches of 32 and part of a third
    r = pr.pcg(K, f, M, 1e-6, 2000, np.float64)
    assert pr.residual_drift(K, f, M, r.iters) < 1e-7                # 6e-9 measured


def test_shards_reach_the_branches_they_are_there_for():
    """The row ranges restated by shard_chunks are the library's (feahip_shard_plan), and the sharded meshes do what
    pcg_cases.SHARDED says of them."""
    for name, (make, ranks) in pc.SHARDED.items():
        deck = make()
        for n in ranks:
            sc = pc.shard_chunks(deck, n)
            for r, s in enumerate(sc):
                plan = feahip.shard_plan(deck, r, n)
                assert (plan["row0"], plan["row1"]) == (s["row0"], s["row1"])
    two = pc.shard_chunks(pc.SHARDED["tet4_144"][0](), 2)
    assert all(s["hi"] > s["lo"] for s in two)
    assert two[0]["lo"] == 0 and two[0]["hi"] < two[0]["chunks"]       # nothing in front, a back range
    assert two[1]["lo"] > 0 and two[1]["hi"] == two[1]["chunks"]       # a front range, nothing behind
    three = pc.shard_chunks(pc.SHARDED["tet4_144"][0](), 3)
    assert three[0]["chunks"] == 0 and three[0]["row0"] == three[0]["row1"]
    cube = pc.shard_chunks(pc.SHARDED["cube_216_no_interior"][0](), 3)
    assert all(s["chunks"] > 0 for s in cube)
    assert cube[1]["chunks"] == 8 and cube[1]["hi"] == cube[1]["lo"]   # the middle rank: no chunk without a halo column
    assert cube[0]["lo"] == 0 and cube[0]["hi"] > 0
    bar = pc.shard_chunks(pc.SHARDED["bar_54_one_super"][0](), 3)
    assert [s["chunks"] > 0 for s in bar] == [False, False, True]


# ---- the recurrence broken on purpose ---------------------------------------------------------------------------------
def broken_pcg(K, f, M, cap, fault, tol=0.0):
    """pcg() with one of the faults a converged-solution test lets through: "drop_row" leaves one row out of p.q,
    "stale_beta" uses the beta of the previous iteration."""
    Mz = pr._apply(M, np.float64)
    x = f.copy(); r = f - K @ x; z = Mz(r); p = z.copy()
    rz, bb = r @ z, f @ f
    row = int(np.argmax(np.abs(f)))                                    # a loaded, free dof
    xs, beta_prev = [x.copy()], 0.0
    for it in range(cap):
        q = K @ p
        pq = p @ q - (p[row] * q[row] if fault == "drop_row" else 0.0)
        alpha = rz / pq
        x = x + alpha * p; r = r - alpha * q; z = Mz(r)
        xs.append(x.copy())
        if r @ r <= tol * tol * bb:
            break
        rz_new = r @ z
        beta = rz_new / rz
        p = z + (beta_prev if fault == "stale_beta" else beta) * p
        beta_prev, rz = beta, rz_new
    return xs


@pytest.mark.parametrize("fault", ["drop_row", "stale_beta"])
def test_a_broken_recurrence_fails_the_iterate_comparison(fault):
    K, f, u = system("tet4_144", *pc.case("tet4_144"))
    M = pr.block_jacobi(K)
    checks = pr.iterate_checks(K, f, M, 0)
    xs = broken_pcg(K, f, M, 8, fault)
    first = 1 if fault == "drop_row" else 3                            # beta enters p_1; a stale one first differs in p_2, x_3
    seen = [k for k in checks if k >= first]
    assert len(seen) >= 3
    for k in seen:
        xk, tol, _, _ = checks[k]
        assert pr.linf(xs[k], xk, xk) > 1e3 * tol, (fault, k)          # the GPU test's assertion would fail, by far
    if fault == "stale_beta":
        # ... while the solve the rest of the suite looks at is as good as ever: r stays f - K x, so it ends at the solution.
        # (With the loaded row missing from p.q every alpha is too long and this system's run does not converge: that
        # fault the converged-solution tests would see here, where the row carries much of p.q.)
        xs = broken_pcg(K, f, M, 20000, fault, tol=1e-13)
        assert len(xs) - 1 < 20000
        assert pr.linf(xs[-1], u, u) < 1e-10

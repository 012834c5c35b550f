"""A numpy restatement of the PCG loops of fea-large_amd/csrc/kernels_solve.hip, iterate by iterate.

pcg() is the two-reduction recurrence (k_cg_init, k_cg_init_scalars, k_cg_update, k_cg_direction), pcg_single_reduction()
the Chronopoulos / Gear form (k_cgcg_update, k_cgcg_scalars0): the same start x0 = f, the same scalars, the same stop and
breakdown tests in the same order, in float64 or long double.  Nothing of the library is used: K is a scipy CSR matrix
of the masked system, the products and sums are numpy's.  Both return every iterate and every recurrence residual, so a
test can ask the library for x_k (a solve capped at k) and compare.
"""
from collections import namedtuple

import numpy as np

Result = namedtuple("Result", "x res iters resid stopped broke")
"""x[k]: the iterate after k updates (x[0] = f); res[k] = sqrt(r_k.r_k / b.b) of the recurrence residual; iters: the
iteration the stop test fired at (0: solved before the first), the cap if it never fired, the failing iteration on a
breakdown; resid = res[iters] of the iterate returned, x[iters]; stopped / broke: how the loop ended."""


def matvec(K, v):
    """K v in v's precision (scipy's own product does not take long double everywhere): one fixed-order sum per row."""
    K = K.tocsr()
    prod = K.data.astype(v.dtype) * v[K.indices]
    y = np.zeros(K.shape[0], dtype=v.dtype)
    rows = np.diff(K.indptr) > 0
    if prod.size:
        y[rows] = np.add.reduceat(prod, K.indptr[:-1][rows])
    return y


def block_jacobi(K):
    """k_precond_build: the inverse of every diagonal 3x3 block as adjugate / determinant, with the determinant expanded
    along the first row; the identity where the determinant is 0 or NaN.  Returns [N][3][3]."""
    K = K.tocsr()
    N = K.shape[0] // 3
    a, i, j = np.meshgrid(np.arange(N), np.arange(3), np.arange(3), indexing="ij")
    d = np.asarray(K[(3 * a + i).ravel(), (3 * a + j).ravel()], dtype=np.float64).reshape(N, 9).T
    det = d[0] * (d[4] * d[8] - d[5] * d[7]) - d[1] * (d[3] * d[8] - d[5] * d[6]) + d[2] * (d[3] * d[7] - d[4] * d[6])
    ok = (det != 0.0) & (det == det)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / det
        m = np.stack([(d[4] * d[8] - d[5] * d[7]) * inv, (d[2] * d[7] - d[1] * d[8]) * inv, (d[1] * d[5] - d[2] * d[4]) * inv,
                      (d[5] * d[6] - d[3] * d[8]) * inv, (d[0] * d[8] - d[2] * d[6]) * inv, (d[2] * d[3] - d[0] * d[5]) * inv,
                      (d[3] * d[7] - d[4] * d[6]) * inv, (d[1] * d[6] - d[0] * d[7]) * inv, (d[0] * d[4] - d[1] * d[3]) * inv],
                     axis=1)
    m[~ok] = np.eye(3).ravel()
    return m.reshape(N, 3, 3)


def _apply(M, dtype):
    """z = M r: M None (identity), [N][3][3] inverse blocks, or a callable on float64 vectors (the reference cycle)."""
    if M is None:
        return lambda r: r.copy()
    if callable(M):
        return lambda r: np.asarray(M(np.asarray(r, dtype=np.float64)), dtype=dtype)
    blocks = np.asarray(M).astype(dtype)
    return lambda r: np.einsum("aij,aj->ai", blocks, r.reshape(-1, 3)).ravel()


def _nan(*v):
    return any(not (t == t) for t in v)


def _result(xs, rrs, bb, iters, stopped, broke):
    # pcg_outcome: resid = sqrt(r.r / b.b), sqrt(r.r) for a zero right-hand side
    with np.errstate(invalid="ignore"):
        res = [np.sqrt(rr / bb) if bb > 0 else np.sqrt(rr) for rr in rrs]
    k = min(iters, len(res) - 1)
    return Result(xs, res, iters, res[k], stopped, broke)


def pcg(K, f, M=None, tol=0.0, cap=8, dtype=np.float64):
    """The two-reduction loop.  k_cg_init: x0 = f, r = f - K x0, p = z = M r.  Iteration `it` (from 0): k_spmv q = K p with
    p.q; k_cg_update alpha = r.z / p.q, x += alpha p, r -= alpha q, z = M r, r.z, r.r; k_cg_direction: breakdown if
    r.z or r.r is NaN or the old r.z is 0, else stop if r.r <= tol^2 b.b -- either ends the loop at it + 1 -- else
    beta = r.z_new / r.z_old, p = z + beta p."""
    f = np.asarray(f).astype(dtype)
    Mz = _apply(M, dtype)
    tol2 = dtype(tol) * dtype(tol)
    x = f.copy()
    r = f - matvec(K, x)
    z = Mz(r)
    p = z.copy()
    rz, rr, bb = r @ z, r @ r, f @ f
    xs, rrs = [x.copy()], [rr]
    if rr <= tol2 * bb or rz == 0.0:                    # k_cg_init_scalars: solved before the first iteration
        return _result(xs, rrs, bb, 0, True, False)
    for it in range(cap):
        q = matvec(K, p)
        with np.errstate(all="ignore"):
            alpha = rz / (p @ q)
            x = x + alpha * p
            r = r - alpha * q
            z = Mz(r)
            rz_new, rr = r @ z, r @ r
        xs.append(x.copy()); rrs.append(rr)
        if _nan(rz_new, rr) or rz == 0.0:
            return _result(xs, rrs, bb, it + 1, False, True)
        if rr <= tol2 * bb:
            return _result(xs, rrs, bb, it + 1, True, False)
        beta = rz_new / rz
        p = z + beta * p
        rz = rz_new
    return _result(xs, rrs, bb, cap, False, False)


def pcg_single_reduction(K, f, M=None, tol=0.0, cap=8, dtype=np.float64):
    """The single-reduction loop.  Start: x0 = f, r = f - K x0, z = M r, w = K z, p = s = 0, gamma = r.z, delta = w.z.
    k_cgcg_update of iteration `it` tests the state it starts from (stop if r.r <= tol^2 b.b: `it` updates were made;
    breakdown if gamma, delta or r.r is NaN), then alpha = gamma / delta (it = 0) or beta = gamma / gamma_old,
    alpha = gamma / (delta - beta gamma / alpha_old) -- breakdown if either is NaN or alpha is 0 -- then p = z + beta p,
    s = w + beta s, x += alpha p, r -= alpha s, z = M r; w = K z and the three sums follow.  What is returned is the
    contract of pcg(): the iterate the cap leaves is tested too."""
    f = np.asarray(f).astype(dtype)
    Mz = _apply(M, dtype)
    tol2 = dtype(tol) * dtype(tol)
    x = f.copy()
    r = f - matvec(K, x)
    z = Mz(r)
    w = matvec(K, z)
    p, s = np.zeros_like(f), np.zeros_like(f)
    gamma, delta, rr, bb = r @ z, w @ z, r @ r, f @ f
    xs, rrs = [x.copy()], [rr]
    if rr <= tol2 * bb or gamma == 0.0:                 # k_cgcg_scalars0
        return _result(xs, rrs, bb, 0, True, False)
    gamma_old = alpha_old = dtype(0)
    for it in range(cap):
        if it > 0 and rr <= tol2 * bb:
            return _result(xs, rrs, bb, it, True, False)
        broke = _nan(gamma, delta, rr)
        beta = dtype(0)
        if not broke:
            with np.errstate(all="ignore"):
                if it == 0:
                    alpha = gamma / delta
                else:
                    beta = gamma / gamma_old
                    alpha = gamma / (delta - beta * gamma / alpha_old)
            broke = _nan(alpha, beta) or alpha == 0.0
        if broke:
            xs.append(x.copy()); rrs.append(rr)         # nothing moved: the state the iteration found
            return _result(xs, rrs, bb, it + 1, False, True)
        p = z + beta * p
        s = w + beta * s
        x = x + alpha * p
        r = r - alpha * s
        z = Mz(r)
        w = matvec(K, z)
        gamma_old, alpha_old = gamma, alpha
        gamma, delta, rr = r @ z, w @ z, r @ r
        xs.append(x.copy()); rrs.append(rr)
    return _result(xs, rrs, bb, cap, bool(rr <= tol2 * bb), False)


FORMS = {0: pcg, 1: pcg_single_reduction}                # keyed as feahip_set_pcg_variant

ITERATES = (1, 2, 3, 5, 8)
GAP_MAX, STEP_MIN = 1e-12, 1e-3
TOL_FLOOR, TOL_CEIL = 1e-13, 1e-10


def linf(a, b, scale):
    return float(np.abs(np.asarray(a, dtype=np.longdouble) - np.asarray(b, dtype=np.longdouble)).max() / np.abs(scale).max())


def iterate_checks(K, f, M, variant, ks=ITERATES, floor=TOL_FLOOR):
    """The iterates a GPU test may hold the library to: {k: (x_k of the long-double restatement as float64, tolerance,
    gap, step)} for the k of `ks` at which the float64 and long-double restatements agree to GAP_MAX and x_k moved by more
    than STEP_MIN from x_{k-1} (both relative to max|x_k|): where the restatement itself is sure of x_k, and where a
    solve that had stopped early would be seen.  The tolerance is 100 times the gap (another summation order), at least
    `floor`, at most TOL_CEIL."""
    form = FORMS[variant]
    lo = form(K, f, M, 0.0, max(ks), np.float64)
    hi = form(K, f, M, 0.0, max(ks), np.longdouble)
    out = {}
    for k in ks:
        if k >= len(lo.x) or k >= len(hi.x) or not np.isfinite(hi.x[k].astype(np.float64)).all():
            continue
        gap = linf(lo.x[k], hi.x[k], hi.x[k])
        step = linf(hi.x[k], hi.x[k - 1], hi.x[k])
        if gap <= GAP_MAX and step > STEP_MIN:
            out[k] = (hi.x[k].astype(np.float64), min(max(100.0 * gap, floor), TOL_CEIL), gap, step)
    return out


def stop_in_first_batch(res, last=8):
    """A stop iteration j <= last with a clear margin on both sides, and its tolerance: res[j] 1.5 <= min(res[0..j-1]),
    tol = sqrt(res[j] min(res[0..j-1])), so the stop test is false at every k < j and true at j by a factor >= 1.22 each
    way.  The largest such j (the stop furthest into the batch); None if there is none."""
    for j in range(min(last, len(res) - 1), 0, -1):
        before = min(res[:j])
        if res[j] * 1.5 <= before:
            return j, float(np.sqrt(res[j] * before))
    return None


def true_residual(K, f, u):
    """|f - K u| / |f| in float64"""
    f = np.asarray(f, dtype=np.float64)
    return float(np.linalg.norm(f - K @ np.asarray(u, dtype=np.float64)) / np.linalg.norm(f))


def iteration_counts(K, f, M, tol, cap):
    """iterations to `tol` of the three variants: float64 two-reduction, float64 single-reduction, long double"""
    runs = (pcg(K, f, M, tol, cap, np.float64), pcg_single_reduction(K, f, M, tol, cap, np.float64),
            pcg(K, f, M, tol, cap, np.longdouble))
    assert all(r.stopped for r in runs)
    return [r.iters for r in runs]


def residual_drift(K, f, M, k):
    """How far the recurrence residual of x_k has drifted from the true one, relative: the larger of the two float64
    forms.  (The recurrence updates r by -alpha K p; f - K x_k is formed afresh.)"""
    out = 0.0
    for form in (pcg, pcg_single_reduction):
        r = form(K, f, M, 0.0, k, np.float64)
        out = max(out, abs(true_residual(K, f, r.x[k]) - float(r.res[k])) / float(r.res[k]))
    return out

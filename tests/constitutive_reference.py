"""The material law of fem_device.h restated in numpy, in float64 or long double (64-bit mantissa, eps 1.1e-19).

Element stiffness, residual and Gauss-point state of the linear tetrahedron (1 point), the 10-node tetrahedron (4, 5 and
27 points) and the 8-node brick (8 points), both models, written from the formulas of the header of fem_device.h:

    g_a    = J^-T dN_a,  J_ij = sum_k dN_k/dxi_i x_k,j
    F^-1   = sum_k X_k (x) g_k
    NH     sigma = (mu (B - I) + lambda ln J I)/J,             l1 = lambda/J, m1 = (mu - lambda ln J)/J
    A5     sigma = F (lambda tr(E) I + 2 mu E) F'/J, E = (F'F - I)/2,    l1 = lambda/J, m1 = mu/J
    K_ab   = vol [l1 g_a (x) g_b + m1 g_b (x) g_a + (m1 g_a.g_b + g_a.sigma.g_b) I]
    f_a    = -vol sigma g_a        (the residual the library assembles is minus the internal force)
    vol    = w |det J|

Nothing here calls the library under test or the oracle.  The shape-function derivatives are written out; the Gauss
points and weights are the host library's own (oracle_binding.gauss_rule); every 3x3 inverse is adjugate over
determinant in the working dtype, every sum an elementwise numpy product-and-add (no BLAS, no LAPACK: neither exists in
long double).  Inputs are taken as given: float64 coordinates convert to long double exactly, so the float64 and the
long-double run evaluate the same state and their difference is the float64 rounding of this restatement -- the `gap`
every comparison with a kernel derives its tolerance from (tolerance()).

Besides K and f the restatement returns what measures them: for every residual entry the sum of the absolute values
of the terms whose difference it is (`fscale`), the same for the stress of a Gauss point (`sscale`) and for the strain
energy (`wscale`).  Near F = I the stress is a difference of O(mu) terms, and an error of one unit in the last place of
those terms is the honest yardstick -- max|sigma| is not, it goes to zero there."""
import numpy as np

import oracle_binding as ob

NH, A5 = 1, 0                                   # feahip.MODEL_COMPRESSIBLE_NEOHOOKEAN, feahip.MODEL_A5
HEX_CORNER = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0, 0, 1], [1, 0, 1], [1, 1, 1], [0, 1, 1]])
TOL_FLOOR, TOL_CEIL = 1e-13, 1e-10              # the bounds of tests/test_gpu_pcg.py's rule


def tolerance(gap):
    """100 times the restatement's float64-to-long-double gap, at least 1e-13, at most 1e-10."""
    return min(max(100.0 * float(gap), TOL_FLOOR), TOL_CEIL)


def shape_derivatives(kind, pts, dtype):
    """dN[G][3][npe]: derivative of shape function a with respect to parent coordinate d at the points pts[G][3]."""
    p = np.asarray(pts, dtype=dtype)
    r, s, t = p[:, 0], p[:, 1], p[:, 2]
    G = len(p)
    one, zero = np.ones(G, dtype=dtype), np.zeros(G, dtype=dtype)
    if kind == "tet4":
        rows = [[-one, one, zero, zero], [-one, zero, one, zero], [-one, zero, zero, one]]
    elif kind == "tet10":
        c0 = 4 * t + 4 * s + 4 * r - 3
        rows = [[c0, 4 * r - 1, zero, zero, -4 * t - 4 * s - 8 * r + 4, 4 * s, -4 * s, -4 * t, 4 * t, zero],
                [c0, zero, 4 * s - 1, zero, -4 * r, 4 * r, -4 * t - 8 * s - 4 * r + 4, -4 * t, zero, 4 * t],
                [c0, zero, zero, 4 * t - 1, -4 * r, zero, -4 * s, -8 * t - 4 * s - 4 * r + 4, 4 * r, 4 * s]]
    elif kind == "hex8":
        c = (r, s, t)
        rows = []
        for dd in range(3):
            row = []
            for i in range(8):
                v = one
                for d in range(3):
                    hi = HEX_CORNER[i][d]
                    v = v * ((one if hi else -one) if d == dd else (c[d] if hi else 1 - c[d]))
                row.append(v)
            rows.append(row)
    else:
        raise ValueError(kind)
    return np.stack([np.stack(row, axis=-1) for row in rows], axis=1)


def det3(m):
    return (m[..., 0, 0] * (m[..., 1, 1] * m[..., 2, 2] - m[..., 1, 2] * m[..., 2, 1])
            - m[..., 0, 1] * (m[..., 1, 0] * m[..., 2, 2] - m[..., 1, 2] * m[..., 2, 0])
            + m[..., 0, 2] * (m[..., 1, 0] * m[..., 2, 1] - m[..., 1, 1] * m[..., 2, 0]))


def inv3(m):
    """(adjugate / det, det) in m's dtype."""
    det = det3(m)
    a = np.empty_like(m)
    a[..., 0, 0] = m[..., 1, 1] * m[..., 2, 2] - m[..., 1, 2] * m[..., 2, 1]
    a[..., 0, 1] = m[..., 0, 2] * m[..., 2, 1] - m[..., 0, 1] * m[..., 2, 2]
    a[..., 0, 2] = m[..., 0, 1] * m[..., 1, 2] - m[..., 0, 2] * m[..., 1, 1]
    a[..., 1, 0] = m[..., 1, 2] * m[..., 2, 0] - m[..., 1, 0] * m[..., 2, 2]
    a[..., 1, 1] = m[..., 0, 0] * m[..., 2, 2] - m[..., 0, 2] * m[..., 2, 0]
    a[..., 1, 2] = m[..., 0, 2] * m[..., 1, 0] - m[..., 0, 0] * m[..., 1, 2]
    a[..., 2, 0] = m[..., 1, 0] * m[..., 2, 1] - m[..., 1, 1] * m[..., 2, 0]
    a[..., 2, 1] = m[..., 0, 1] * m[..., 2, 0] - m[..., 0, 0] * m[..., 2, 1]
    a[..., 2, 2] = m[..., 0, 0] * m[..., 1, 1] - m[..., 0, 1] * m[..., 1, 0]
    return a / det[..., None, None], det


def mm(a, b):
    """a b of stacks of small matrices by broadcasting (numpy's matmul has no long-double kernel worth trusting to be
    plain sums; this is one)."""
    return (a[..., :, :, None] * b[..., None, :, :]).sum(axis=-2)


def T(a):
    return np.swapaxes(a, -1, -2)


class Element:
    """What one evaluation of all elements gives: per element Ke[E][npe][3][npe][3], fe[E][npe][3], Kse[E][npe][npe],
    fse[E][npe][3] (cancellation scale of fe); per Gauss point F, sig, sscale [E][G][3][3], detJ, vol, vol0, psi,
    psiscale [E][G], g[E][G][npe][3]."""


def evaluate(kind, G, Xe, xe, lam, mu, model, dtype, need_k=True, local=None):
    """Xe, xe [E][npe][3] initial and current element coordinates; lam, mu [E] per element.  local: take both on
    element-local coordinates (every node minus the element's first; sum_k dN_k = 0, so the same J and F^-1) -- by
    default for the linear tetrahedron, whose kernels subtract first, and not for the 10- and 8-node elements, whose
    kernels and the oracle sum sum_k dN_k x_k as it stands.  The subtraction is done in the working dtype: under a
    translation the undifferenced sums lose |x| / cell digits, the differenced ones none."""
    if local is None:
        local = kind == "tet4"
    w, pts = ob.gauss_rule(kind, G)
    dN = shape_derivatives(kind, pts, dtype)                                     # [G][3][npe]
    w = np.asarray(w, dtype=dtype)
    Xe, xe = np.asarray(Xe, dtype=dtype), np.asarray(xe, dtype=dtype)
    if local:
        Xe, xe = Xe - Xe[:, :1, :], xe - xe[:, :1, :]
    lam = np.asarray(lam, dtype=dtype)[:, None, None, None]
    mu = np.asarray(mu, dtype=dtype)[:, None, None, None]
    I = np.eye(3, dtype=dtype)
    J = (dN[None, :, :, :, None] * xe[:, None, None, :, :]).sum(axis=3)          # [E][G][i][j] = sum_k dN[g][i][k] x[k][j]
    Ji, detJ = inv3(J)
    g = (Ji[:, :, None, :, :] * T(dN)[None, :, :, None, :]).sum(axis=-1)         # g[e][g][a][i] = sum_k Ji[i][k] dN[g][k][a]
    Fi = (Xe[:, None, :, :, None] * g[:, :, :, None, :]).sum(axis=2)             # Fi[i][j] = sum_k X[k][i] g[k][j]
    F, _ = inv3(Fi)
    Jd = det3(F)[..., None, None]
    o = Element()
    if model == NH:
        lnJ = np.log(Jd)
        B = mm(F, T(F))
        o.sig = (mu * (B - I) + lam * lnJ * I) / Jd
        o.sscale = (mu * np.abs(B) + mu * I + np.abs(lam * lnJ) * I) / Jd
        l1, m1 = lam / Jd, (mu - lam * lnJ) / Jd
        trb = np.trace(B, axis1=-2, axis2=-1)[..., None, None]
        terms = (mu / 2 * trb, -3 * mu / 2 - mu * lnJ, lam / 2 * lnJ * lnJ)
    else:
        C = mm(T(F), F)
        E = (C - I) / 2
        trE = np.trace(E, axis1=-2, axis2=-1)[..., None, None]
        o.sig = mm(mm(F, (lam * trE * I + 2 * mu * E) / Jd), T(F))
        trC = np.trace(C, axis1=-2, axis2=-1)[..., None, None]
        o.sscale = mm(mm(np.abs(F), (np.abs(lam) * (trC + 3) / 2 * I + mu * (np.abs(C) + I)) / Jd), np.abs(T(F)))
        l1, m1 = lam / Jd, mu / Jd
        EE = (E * E).sum(axis=(-2, -1))[..., None, None]
        terms = (lam / 2 * trE * trE, mu * EE)
        sterms = (np.abs(lam) / 2 * ((trC + 3) / 2) ** 2, mu * (((np.abs(C) + I) / 2) ** 2).sum(axis=(-2, -1))[..., None, None])
    o.F, o.detJ, o.g = F, detJ, g
    o.vol = w[None, :] * np.abs(detJ)
    o.vol0 = w[None, :] * detJ / Jd[..., 0, 0]
    o.psi = sum(terms)[..., 0, 0]
    if model == NH:
        o.psiscale = (mu / 2 * trb + 3 * mu / 2 + np.abs(mu * lnJ) + np.abs(lam) / 2 * lnJ * lnJ)[..., 0, 0]
    else:
        o.psiscale = sum(sterms)[..., 0, 0]
    vol = o.vol[..., None, None]
    sg = (o.sig[:, :, None, :, :] * g[:, :, :, None, :]).sum(axis=-1)            # (sigma g_a)[i]
    o.fe = -(vol * sg).sum(axis=1)
    o.fse = (vol * (o.sscale[:, :, None, :, :] * np.abs(g)[:, :, :, None, :]).sum(axis=-1)).sum(axis=1)
    if need_k:
        gsg = (g[:, :, :, None, :] * sg[:, :, None, :, :]).sum(axis=-1)          # [a][b] = g_a . sigma g_b
        gg = (g[:, :, :, None, :] * g[:, :, None, :, :]).sum(axis=-1)
        o.Kse = (vol * gsg).sum(axis=1)
        ssg = (o.sscale[:, :, None, :, :] * np.abs(g)[:, :, :, None, :]).sum(axis=-1)
        o.Ksse = (vol * (np.abs(g)[:, :, :, None, :] * ssg[:, :, None, :, :]).sum(axis=-1)).sum(axis=1)   # |g_a| . s . |g_b|
        vl, vm = (vol * l1)[..., None, None], (vol * m1)[..., None, None]
        ga = g[:, :, :, :, None, None]                                           # [e][g][a][i][b][j]
        gb = g[:, :, None, None, :, :]
        gai = g[:, :, :, None, None, :]                                          # g_a[j] at [a][.][.][j]
        gbi = np.moveaxis(g, -1, -2)[:, :, None, :, :, None]                     # g_b[i] at [.][i][b][.]
        d = (vol * m1 * gg + vol * gsg)[:, :, :, None, :, None] * I[None, None, None, :, None, :]
        o.Ke = (vl * ga * gb + vm * gbi * gai + d).sum(axis=1)
    return o


class Result:
    """K[3N][3N], f[3N], fscale[3N], Ksigma[3N][3N], Ksscale[3N][3N] (K_sigma with every term's absolute value and the
    stress scale for the stress), W, Wscale (dense, per mesh and state) and the element data `el`."""


def dofs_of(conn):
    return (3 * np.asarray(conn)[:, :, None] + np.arange(3)[None, None, :]).reshape(len(conn), -1)


def run(kind, G, conn, X0, x, materials, ids, model, dtype, need_k=True, local=None):
    """materials [n][2] = (lambda, mu), ids [E] (a single pair: one row and zeros); local: see evaluate()."""
    conn = np.asarray(conn)
    mats = np.asarray(materials, dtype=dtype).reshape(-1, 2)
    ids = np.asarray(ids, dtype=np.int64)
    X0, x = np.asarray(X0, dtype=dtype), np.asarray(x, dtype=dtype)
    el = evaluate(kind, G, X0[conn], x[conn], mats[ids, 0], mats[ids, 1], model, dtype, need_k, local)
    N, E, npe = len(X0), len(conn), conn.shape[1]
    n3 = 3 * npe
    r = Result()
    r.el, r.N = el, N
    d = dofs_of(conn)
    r.f, r.fscale = np.zeros(3 * N, dtype=dtype), np.zeros(3 * N, dtype=dtype)
    np.add.at(r.f, d.ravel(), el.fe.reshape(-1))
    np.add.at(r.fscale, d.ravel(), el.fse.reshape(-1))
    r.W = (el.vol0 * el.psi).sum()
    r.Wscale = (np.abs(el.vol0) * el.psiscale).sum()
    if need_k:
        r.K, r.Ksigma, r.Ksscale = (np.zeros((3 * N, 3 * N), dtype=dtype) for _ in range(3))
        rows, cols = np.repeat(d, n3, axis=1).ravel(), np.tile(d, (1, n3)).ravel()
        np.add.at(r.K, (rows, cols), el.Ke.reshape(-1))
        ks = el.Kse[:, :, None, :, None] * np.eye(3, dtype=dtype)[None, None, :, None, :]
        np.add.at(r.Ksigma, (rows, cols), ks.reshape(-1))
        kc = el.Ksse[:, :, None, :, None] * np.eye(3, dtype=dtype)[None, None, :, None, :]
        np.add.at(r.Ksscale, (rows, cols), kc.reshape(-1))
    return r


def nodal_stress(res, conn, select=None):
    """(sig[N][3][3], weight[N]): the volume-weighted average of the Gauss-point stresses at every node, over the
    elements select[E] (all by default), and its scale (the same average of sscale)."""
    el = res.el
    conn = np.asarray(conn)
    sel = np.ones(len(conn), dtype=bool) if select is None else np.asarray(select, dtype=bool)
    dt = el.sig.dtype
    se = (el.vol[..., None, None] * el.sig).sum(axis=1)[sel]
    sc = (el.vol[..., None, None] * el.sscale).sum(axis=1)[sel]
    ve = el.vol.sum(axis=1)[sel]
    num, scl, den = np.zeros((res.N, 3, 3), dtype=dt), np.zeros((res.N, 3, 3), dtype=dt), np.zeros(res.N, dtype=dt)
    for k in range(conn.shape[1]):
        np.add.at(num, conn[sel][:, k], se)
        np.add.at(scl, conn[sel][:, k], sc)
        np.add.at(den, conn[sel][:, k], ve)
    safe = np.where(den > 0, den, 1)[:, None, None]
    return num / safe, scl / safe, den


# ---- yardsticks ----------------------------------------------------------------------------------------------------
def f64(a):
    return np.asarray(a, dtype=np.float64)


def err_block_rows(K, ref):
    """max over the entries of |K - ref| relative to the largest entry of ref's block row (the three scalar rows of a
    node)."""
    ref = np.asarray(ref)
    scale = np.abs(ref).reshape(len(ref) // 3, -1).max(axis=1)
    d = np.abs(np.asarray(K, dtype=ref.dtype) - ref).reshape(len(ref) // 3, -1).max(axis=1)
    return float((d / scale).max())


def err_scaled(a, ref, scale):
    """max |a - ref| / scale, entry by entry."""
    ref, scale = np.asarray(ref), np.asarray(scale)
    return float((np.abs(np.asarray(a, dtype=ref.dtype) - ref) / scale).max())


def err_own_max(a, ref, axes):
    """max |a - ref| relative to the largest |ref| over the trailing `axes` axes (a tensor against its own scale)."""
    ref = np.asarray(ref)
    ax = tuple(range(-axes, 0))
    scale = np.abs(ref).max(axis=ax, keepdims=True)
    return float((np.abs(np.asarray(a, dtype=ref.dtype) - ref) / scale).max())

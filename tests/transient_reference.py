"""Transient response by mode superposition restated in numpy (include/fea_hip.h, "transient response by mode
superposition, base excitation"): the exact propagator of a mode under a piecewise-linear load from a scaled-and-squared
Taylor series of the augmented 4x4 matrix, in numpy.longdouble (or float64, to measure the gap between the two), the
recurrence, the three coefficient tables, the sum over the modes, its rounding bound, and the dense base load.  Nothing
here calls the library under test."""
import numpy as np

from response_reference import modal_damping

EPS = np.finfo(np.float64).eps
LD = np.longdouble


def propagator(lam, d, dt, dtype=LD):
    """exp(dt Z) of the state (q, q', p, p'), Z = [[0, 1, 0, 0], [-lam, -d, 1, 0], [0, 0, 0, 1], [0, 0, 0, 0]]: its upper
    left block is A, its upper right block L holds the responses to p = 1 and to p = t.  Returns (A[2][2], b0[2], b1[2]) of
    y_{n+1} = A y_n + b0 p_n + b1 p_{n+1}: b1 = L[:, 1] / dt, b0 = L[:, 0] - b1."""
    lam, d, dt = dtype(lam), dtype(d), dtype(dt)
    Z = np.zeros((4, 4), dtype=dtype)
    Z[0, 1], Z[1, 0], Z[1, 1], Z[1, 2], Z[2, 3] = 1, -lam, -d, 1, 1
    Z *= dt
    norm = float(np.abs(Z).sum(axis=1).max())
    s = max(0, int(np.ceil(np.log2(max(norm, 1e-300)))) + 2)            # ||Z / 2^s|| <= 1 / 4
    Zs = Z / dtype(2.0) ** s
    E, term = np.eye(4, dtype=dtype), np.eye(4, dtype=dtype)
    for k in range(1, 30):
        term = term @ Zs / dtype(k)
        E = E + term
    for _ in range(s):
        E = E @ E
    A, L = E[:2, :2], E[:2, 2:]
    b1 = L[:, 1] / dt
    return A, L[:, 0] - b1, b1


def modal_states(lam, q, g, dt, alpha=0.0, beta=0.0, zeta=None, dtype=LD):
    """y[n_steps + 1][n][2] = (q_k(t_n), q_k'(t_n)) from rest under p_k = q_k g, and the damping d[n], in dtype."""
    lam, q, g = np.asarray(lam, dtype=np.float64), np.asarray(q, dtype=np.float64), np.asarray(g, dtype=np.float64)
    d = modal_damping(lam.astype(dtype), dtype(alpha), dtype(beta), None if zeta is None else np.asarray(zeta, dtype=np.float64).astype(dtype))
    y = np.zeros((len(g), len(lam), 2), dtype=dtype)
    parts = [propagator(lam[k], d[k], dt, dtype) for k in range(len(lam))]
    A = np.array([a for a, _, _ in parts], dtype=dtype).reshape(len(lam), 2, 2)
    b0 = np.array([b for _, b, _ in parts], dtype=dtype).reshape(len(lam), 2)
    b1 = np.array([b for _, _, b in parts], dtype=dtype).reshape(len(lam), 2)
    p = g.astype(dtype)[:, None] * q.astype(dtype)
    for n in range(len(g) - 1):                                          # every mode at once, a step after the other
        y[n + 1, :, 0] = A[:, 0, 0] * y[n, :, 0] + A[:, 0, 1] * y[n, :, 1] + b0[:, 0] * p[n] + b1[:, 0] * p[n + 1]
        y[n + 1, :, 1] = A[:, 1, 0] * y[n, :, 0] + A[:, 1, 1] * y[n, :, 1] + b0[:, 1] * p[n] + b1[:, 1] * p[n + 1]
    return y, d


def table(y, d, lam, q, g, correction=True, quantity=0):
    """The coefficient table of one quantity from the states of modal_states, in their dtype."""
    dtype = y.dtype
    lam_t = np.asarray(lam, dtype=np.float64).astype(dtype)
    p = np.asarray(g, dtype=np.float64).astype(dtype)[:, None] * np.asarray(q, dtype=np.float64).astype(dtype)
    if quantity == 0:
        return y[:, :, 0] - p / lam_t if correction else y[:, :, 0]
    if quantity == 1:
        return y[:, :, 1]
    return p - d * y[:, :, 1] - lam_t * y[:, :, 0]


def coefficients(lam, q, g, dt, alpha=0.0, beta=0.0, zeta=None, correction=True, quantity=0, dtype=LD):
    """a[n_steps + 1][n] in dtype: 0 q(t_n), or with the correction q(t_n) - q_k g_n / lam_k; 1 q'(t_n); 2 q_k g_n -
    d_k q' - lam_k q."""
    y, d = modal_states(lam, q, g, dt, alpha, beta, zeta, dtype)
    return table(y, d, lam, q, g, correction, quantity)


def response(Phi, coef, u_s=None, g=None):
    """u[n_steps + 1][3N] = u_s g_n + sum_k phi_k a_k(n): Phi[3N][n], coef[n_steps + 1][n] (float64)."""
    u = np.asarray(coef, dtype=np.float64) @ Phi.T
    return u if u_s is None else u + np.asarray(g, dtype=np.float64)[:, None] * u_s


def rounding_bound(Phi, coef, u_s=None, g=None):
    """4 (m + 5) eps (|u_s,i| |g_n| + sum_k |phi_ik| |a_k(n)|) per dof and step: the sweep's bound with one more term, the
    product u_s g_n."""
    m = Phi.shape[1]
    mag = np.abs(np.asarray(coef, dtype=np.float64)) @ np.abs(Phi).T
    return 4 * (m + 5) * EPS * (mag if u_s is None else mag + np.abs(np.asarray(g, dtype=np.float64))[:, None] * np.abs(u_s))


def base_load(M, mask, direction):
    """(F = -mask(M r), r, r' M r) of the rigid translation `direction` on all dofs, dense M over all dofs."""
    r = np.tile(np.asarray(direction, dtype=np.float64), len(mask) // 3)
    Mr = M @ r
    return np.where(mask, 0.0, -Mr), r, float(r @ Mr)


def shape(kind, t, rise=0.0):
    """g(t) of the deck's (transient :shape ...)."""
    t = np.asarray(t, dtype=np.float64)
    if kind == "step":
        return np.ones_like(t)
    if kind == "ramp":
        return np.minimum(t / rise, 1.0)
    return np.where(t < rise, np.sin(np.pi * t / rise), 0.0)

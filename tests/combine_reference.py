"""Response spectrum and random vibration restated in numpy (include/fea_hip.h, "response spectrum and random vibration on
the locked modes"): the trapezoid weights, the form of a PSD, the grid that resolves the peaks, Der Kiureghian's
correlation coefficient, the form of a response spectrum with its three rules and the missing mass, the interpolation in a
table, the quadratic form per dof with its rounding bound, and the closed forms of white noise.  Every builder runs in the
dtype asked for, float64 or numpy.longdouble.  Nothing here calls the library under test."""
import numpy as np

from response_reference import EPS, modal_damping

LD = np.longdouble
SRSS, CQC, ABS = 0, 1, 2


def _complex(dtype):
    return np.clongdouble if dtype is LD else np.complex128


def coefficients(lam, q, omega, alpha, beta, zeta, correction, dtype=np.float64):
    """a[n_freq][n] = q_k H_k, or q_k (H_k - 1 / lam_k) taken as H_k (w^2 - i w d_k) / lam_k, in the complex type of dtype."""
    lam, q = np.asarray(lam, dtype=dtype), np.asarray(q, dtype=dtype)
    w = np.asarray(omega, dtype=dtype)[:, None]
    d = modal_damping(lam, dtype(alpha), dtype(beta), None if zeta is None else np.asarray(zeta, dtype=dtype))
    one_i = _complex(dtype)(1j)
    H = 1 / ((lam - w * w) + one_i * (w * d))
    return q * (H * ((w * w - one_i * (w * d)) / lam)) if correction else q * H


def trapezoid_weights(omega, dtype=np.float64):
    w = np.asarray(omega, dtype=dtype)
    wt = np.zeros_like(w)
    wt[1:] += (w[1:] - w[:-1]) / 2
    wt[:-1] += (w[1:] - w[:-1]) / 2
    return wt


def form_of_rows(a, omega, S, correction, quantity, dtype=np.float64):
    """(C, b, s) = sum_j wt_j S_j w_j^(2p) (Re(a a^H), Re(a), 1) over the rows a[n_freq][n] given; b = 0, s = 0 without the
    correction."""
    w = np.asarray(omega, dtype=dtype)
    g = trapezoid_weights(omega, dtype) * np.asarray(S, dtype=dtype) * w ** (2 * quantity)
    re, im = a.real.astype(dtype), a.imag.astype(dtype)
    C = (re * g[:, None]).T @ re + (im * g[:, None]).T @ im
    if not correction:
        return C, np.zeros(a.shape[1], dtype=dtype), dtype(0)
    return C, (re * g[:, None]).sum(axis=0), g.sum()


def random_form(lam, q, omega, S, alpha=0.0, beta=0.0, zeta=None, correction=True, quantity=0, dtype=np.float64):
    return form_of_rows(coefficients(lam, q, omega, alpha, beta, zeta, correction, dtype), omega, S, correction, quantity, dtype)


def random_grid(lam, alpha, beta, zeta, w_lo, w_hi, n_background, n_per_mode, breakpoints=()):
    """In long double, rounded to float64 once per point: linspace(w_lo, w_hi) with the end point exact, w_k + (d_k / 2)
    tan(theta_i) per mode with lam_k > 0 and d_k > 0, the breakpoints; clipped, sorted, without duplicates."""
    lam = np.asarray(lam, dtype=LD)
    d = modal_damping(lam, LD(alpha), LD(beta), None if zeta is None else np.asarray(zeta, dtype=LD))
    lo, hi = LD(w_lo), LD(w_hi)
    back = (lo + (hi - lo) * np.arange(n_background, dtype=LD) / LD(n_background - 1)).astype(np.float64)
    back[-1] = w_hi
    parts = [np.asarray(breakpoints, dtype=np.float64).reshape(-1), back]
    pi = 4 * np.arctan(LD(1))
    theta = ((np.arange(n_per_mode, dtype=LD) + LD(0.5)) / LD(n_per_mode)) * pi - pi / LD(2)
    for k in range(len(lam)):
        if lam[k] > 0 and d[k] > 0:
            parts.append((np.sqrt(lam[k]) + LD(0.5) * d[k] * np.tan(theta)).astype(np.float64))
    g = np.concatenate(parts)
    return np.unique(g[(g >= w_lo) & (g <= w_hi)])


def correlation(w, z):
    """rho[n][n] of Der Kiureghian for unequal damping, r = w_k / w_j; the upper triangle evaluated and mirrored, rho_kk = 1,
    a zero denominator off the diagonal gives 1."""
    n = len(w)
    rho = np.ones((n, n), dtype=w.dtype)
    for j in range(n):
        for k in range(j + 1, n):
            r = w[k] / w[j]
            zz = z[j] * z[k]
            num = 8 * np.sqrt(zz) * (z[j] + r * z[k]) * r * np.sqrt(r)
            den = (1 - r * r) ** 2 + 4 * zz * r * (1 + r * r) + 4 * (z[j] * z[j] + z[k] * z[k]) * r * r
            rho[j, k] = rho[k, j] = 1 if den == 0 else num / den
    return rho


def modal_peaks(lam, q, sa, quantity, dtype=np.float64):
    lam, q, sa = np.asarray(lam, dtype=dtype), np.asarray(q, dtype=dtype), np.asarray(sa, dtype=dtype)
    a = q * sa / lam
    return a * np.sqrt(lam) if quantity == 1 else a * lam if quantity == 2 else a


def spectrum_form(lam, q, sa, rule, alpha=0.0, beta=0.0, zeta=None, correction=False, zpa=0.0, quantity=0, dtype=np.float64):
    lam_t, q_t = np.asarray(lam, dtype=dtype), np.asarray(q, dtype=dtype)
    a = modal_peaks(lam, q, sa, quantity, dtype)
    if rule == SRSS:
        C = np.diag(a * a)
    elif rule == ABS:
        C = np.outer(np.abs(a), np.abs(a))
    else:
        d = modal_damping(lam_t, dtype(alpha), dtype(beta), None if zeta is None else np.asarray(zeta, dtype=dtype))
        w = np.sqrt(lam_t)
        C = correlation(w, d / (2 * w)) * np.outer(a, a)
        C[np.diag_indices(len(a))] = a * a
    if not (correction and zpa > 0 and quantity == 0):
        return C, np.zeros(len(a), dtype=dtype), dtype(0)
    c, z2 = -q_t / lam_t, dtype(zpa) * dtype(zpa)
    return C + z2 * np.outer(c, c), z2 * c, z2


def table_value(w, v, at, loglog, clamp):
    """The table at `at`: a point's own value at a point, linear or log-log in between (a segment with a value or an
    abscissa that is not positive is linear), outside zero or (clamp) the end values."""
    w, v = np.asarray(w, dtype=np.float64), np.asarray(v, dtype=np.float64)
    if at < w[0]:
        return v[0] if clamp else 0.0
    if at > w[-1]:
        return v[-1] if clamp else 0.0
    hi = int(np.searchsorted(w, at, side="left"))
    if w[hi] == at:
        return float(v[hi])
    lo = hi - 1
    if loglog and w[lo] > 0 and v[lo] > 0 and v[hi] > 0:
        t = (np.log(LD(at)) - np.log(LD(w[lo]))) / (np.log(LD(w[hi])) - np.log(LD(w[lo])))
        return float(np.exp(np.log(LD(v[lo])) + t * (np.log(LD(v[hi])) - np.log(LD(v[lo])))))
    t = (LD(at) - LD(w[lo])) / (LD(w[hi]) - LD(w[lo]))
    return float(LD(v[lo]) + t * (LD(v[hi]) - LD(v[lo])))


def combine(Phi, u_s, C, b=None, s=0.0, absolute=False):
    """(v, A) per dof in float64: v = x' C x + 2 u_s (b' x) + s u_s^2 over the rows x of Phi (|Phi| with absolute), A the
    same sum of the magnitudes of its terms.  The output of the device is sqrt(max(0, v))."""
    X = np.abs(Phi) if absolute else np.asarray(Phi, dtype=np.float64)
    n = X.shape[1]
    C = np.asarray(C, dtype=np.float64)
    b = np.zeros(n) if b is None else np.asarray(b, dtype=np.float64)
    u = np.zeros(len(X)) if u_s is None else np.asarray(u_s, dtype=np.float64)
    v = ((X @ C) * X).sum(axis=1) + 2 * u * (X @ b) + s * u * u
    A = ((np.abs(X) @ np.abs(C)) * np.abs(X)).sum(axis=1) + 2 * np.abs(u) * (np.abs(X) @ np.abs(b)) + abs(s) * u * u
    return v, A


def combine_bound(m, v, A):
    """4 (m + 5) eps A + 4 eps |v| on out^2: FMA chains of at most m + 3 terms on the device and as many roundings in the
    restatement, and the square of a correctly rounded root."""
    return 4 * (m + 5) * EPS * A + 4 * EPS * np.abs(v)


def white_noise_covariance(lam, q, d, S0):
    """The modal covariance under a one-sided white PSD S0 on [0, inf): C_kk = pi q_k^2 S0 / (2 d_k lam_k), C_jk = pi q_j q_k
    S0 (d_j + d_k) / ((lam_j - lam_k)^2 + (d_j + d_k)(d_j lam_k + d_k lam_j))."""
    lam, q, d = (np.asarray(x, dtype=np.float64) for x in (lam, q, d))
    dj, dk, lj, lk = d[:, None], d[None, :], lam[:, None], lam[None, :]
    return np.pi * np.outer(q, q) * S0 * (dj + dk) / ((lj - lk) ** 2 + (dj + dk) * (dj * lk + dk * lj))

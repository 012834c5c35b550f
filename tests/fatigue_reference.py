"""Random-vibration fatigue restated in numpy (include/fea_hip.h, "random-vibration fatigue"): the form of a spectral moment
by order, the seven moments of a node from the nine forms, the rates, the three damage estimators with their status bits,
and Dirlik's density for quadrature.  Everything runs in the dtype asked for, float64 or numpy.longdouble.  Nothing here
calls the library under test."""
import math

import numpy as np

import combine_reference as cr
import stress_reference as sr

LD = np.longdouble
ORDERS = (0, 1, 2, 4)
NO_STRESS, NARROW, NO_DIRLIK = 1, 2, 4
NARROW_LIMIT = "1e-6"                                   # 1 - alpha2 <= this: the narrow-band limit
EXCUSE = 1e-9                                           # a threshold this near (long double) excuses a pair


def _c(text, dtype):
    """A decimal constant in the dtype: the long-double one is not the float64 one widened."""
    return LD(text) if dtype is LD else np.float64(text)


def moment_form(lam, q, omega, S, alpha=0.0, beta=0.0, zeta=None, correction=True, order=0, dtype=np.float64):
    """(C, b, s) = sum_j wt_j S_j w_j^order (Re(a a^H), Re(a), 1), a the rows of combine_reference.coefficients: the form
    of combine_reference.random_form with the weight w^order in place of w^(2 p)."""
    a = cr.coefficients(lam, q, omega, alpha, beta, zeta, correction, dtype)
    w = np.asarray(omega, dtype=dtype)
    g = cr.trapezoid_weights(omega, dtype) * np.asarray(S, dtype=dtype) * w ** order
    re, im = a.real.astype(dtype), a.imag.astype(dtype)
    C = (re * g[:, None]).T @ re + (im * g[:, None]).T @ im
    if not correction:
        return C, np.zeros(a.shape[1], dtype=dtype), dtype(0)
    return C, (re * g[:, None]).sum(axis=0), g.sum()


def seven_moments(T, Ts, forms):
    """(mom[N][7][len(forms)], bound): max(0, form) on the six components and on the von Mises combination of the nine
    forms, with the bounds of stress_reference.stress_combine; and the raw values v[N][7][len(forms)] before the clamp."""
    mom, bound, raw = [], [], []
    for C, b, s in forms:
        v6, b6, vvm, bvm = sr.stress_combine(T, Ts, np.asarray(C, dtype=np.float64), None if b is None else np.asarray(b, dtype=np.float64), float(s))
        v = np.concatenate([v6, vvm[:, None]], axis=1)
        raw.append(v)
        mom.append(np.maximum(v, 0.0))
        bound.append(np.concatenate([b6, bvm[:, None]], axis=1))
    return np.stack(mom, axis=2), np.stack(bound, axis=2), np.stack(raw, axis=2)


def _gamma(x, dtype):
    """Gamma(x) for x >= 1 in the dtype: math.gamma on [1, 2) and the recurrence up from there in the dtype.  The base value
    has float64 accuracy in either dtype: Gamma enters every damage as ONE factor, so that bounds the relative difference
    to the library (tgammal) at 2e-16, far inside the floor of 1e-13 of every comparison."""
    x = float(x)
    k = 0
    while x - k >= 2.0:
        k += 1
    base = dtype(math.gamma(x - k))
    for j in range(k):
        base = base * (dtype(x) - dtype(k - j))
    return base


def sn_constants(b, A, dtype=np.float64):
    """Gamma(1 + b), Gamma(1 + b / 2), 2^(b / 2), 1 / A."""
    b = dtype(b)
    return _gamma(1 + float(b), dtype), _gamma(1 + float(b) / 2, dtype), dtype(2) ** (b / 2), 1 / dtype(A)


def dirlik_parameters(m, dtype=np.float64):
    """(D1, D2, D3, R, Q, xm, g) of the moments m[...][4]; whatever comes out where a divisor is zero."""
    m = np.asarray(m, dtype=dtype)
    m0, m1, m2, m4 = (m[..., k] for k in range(4))
    with np.errstate(all="ignore"):
        g = m2 / np.sqrt(m0 * m4)
        xm = (m1 / m0) * np.sqrt(m2 / m4)
        D1 = 2 * (xm - g * g) / (1 + g * g)
        den = 1 - g - D1 + D1 * D1
        R = (g - xm - D1 * D1) / den
        D2 = den / (1 - R)
        D3 = 1 - D1 - D2
        Q = _c("1.25", dtype) * (g - D3 - D2 * R) / D1
    return D1, D2, D3, R, Q, xm, g


def dirlik_density(Z, D1, D2, D3, R, Q):
    """Dirlik's density of the normalised amplitude Z = s / sqrt(m0)."""
    return D1 / Q * np.exp(-Z / Q) + D2 * Z / (R * R) * np.exp(-Z * Z / (2 * R * R)) + D3 * Z * np.exp(-Z * Z / 2)


def dirlik_expectation(b, D1, D2, D3, R, Q, dtype=np.float64):
    """E[Z^b] under dirlik_density in closed form."""
    gb, ghb, two_hb, _ = sn_constants(b, 1.0, dtype)
    return D1 * Q ** dtype(b) * gb + two_hb * ghb * (D2 * np.abs(R) ** dtype(b) + D3)


def fatigue(m, b, A, dtype=np.float64):
    """(rates[...][2], damage[...][3], status[...], near[...]) of the moments m[...][4] on N s^b = A: the definitions of
    include/fea_hip.h, elementwise in the dtype.  near: alpha2 or a Dirlik parameter lies within EXCUSE of its threshold."""
    m = np.asarray(m, dtype=dtype)
    m0, m1, m2, m4 = (m[..., k] for k in range(4))
    two_pi = 8 * np.arctan(dtype(1))
    gb, ghb, two_hb, inv_a = sn_constants(b, A, dtype)
    b = dtype(b)
    live = (m0 > 0) & (m2 > 0)
    with np.errstate(all="ignore"):
        nu0 = np.where(live, np.sqrt(m2 / m0) / two_pi, 0)
        nup = np.where(live & (m4 > 0), np.sqrt(m4 / m2) / two_pi, 0)
        d_nb = (nu0 * inv_a) * (2 * m0) ** (b / 2) * ghb
        clamp = lambda v: np.where(v > 0, np.minimum(v, 1), 0)
        D1, D2, D3, R, Q, xm, g = dirlik_parameters(m, dtype)
        a1, a2 = clamp(m1 / np.sqrt(m0 * m2)), clamp(g)
        narrow = live & (1 - a2 <= _c(NARROW_LIMIT, dtype))
        da = a1 - a2
        bw = da * (_c("1.112", dtype) * (1 + a1 * a2 - a1 - a2) * np.exp(_c("2.11", dtype) * a2) + da) / ((a2 - 1) * (a2 - 1))
        d_tb = (bw + (1 - bw) * a2 ** (b - 1)) * d_nb
        fin = np.isfinite(D1) & np.isfinite(D2) & np.isfinite(D3) & np.isfinite(R) & np.isfinite(Q)
        valid = fin & (D1 >= 0) & (D2 >= 0) & (D3 >= 0) & (~(D1 > 0) | (Q > 0))
        d_dk = (nup * inv_a) * m0 ** (b / 2) * (D1 * Q ** b * gb + two_hb * ghb * (D2 * np.abs(R) ** b + D3))
        near = live & (np.abs(a2 - (1 - _c(NARROW_LIMIT, dtype))) <= EXCUSE)
        for p in (D1, D2, D3, Q):
            near = near | (live & ~narrow & (np.abs(p) <= EXCUSE))
    other = live & ~narrow
    d_tb = np.where(narrow, d_nb, d_tb)
    d_dk = np.where(narrow, d_nb, np.where(valid, d_dk, d_tb))
    zero = dtype(0)
    damage = np.stack([np.where(live, d, zero) for d in (d_nb, d_dk, d_tb)], axis=-1)
    status = np.where(~live, NO_STRESS, np.where(narrow, NARROW, np.where(other & ~valid, NO_DIRLIK, 0))).astype(np.int32)
    return np.stack([nu0, nup], axis=-1).astype(dtype), damage.astype(dtype), status, near


def moments_of_psd(w, G, dtype=np.float64):
    """(m0, m1, m2, m4) of the PSD G on the grid w by the trapezoid rule."""
    w = np.asarray(w, dtype=dtype)
    g = cr.trapezoid_weights(w, dtype) * np.asarray(G, dtype=dtype)
    return np.array([(g * w ** n).sum() for n in ORDERS], dtype=dtype)


def shapes():
    """Three PSDs on [0, 400] rad per unit time, 40001 points: two Lorentzian peaks, a flat band, one peak."""
    w = np.linspace(0.0, 400.0, 40001)
    lor = lambda w0, d: 1.0 / ((w - w0) ** 2 + (d / 2) ** 2)
    return {"two peaks": (w, lor(60.0, 4.0) + lor(150.0, 6.0)),
            "flat band": (w, ((w >= 20.0) & (w <= 200.0)).astype(np.float64)),
            "one peak": (w, lor(100.0, 4.0))}

"""Frequency response by mode superposition restated in numpy complex128 (include/fea_hip.h, "frequency response by mode
superposition"): the modal damping, the transfer functions, the coefficient table with and without the static
correction, the sum over the modes, its rounding bound, and the dense direct solve of (K - w^2 M + i w (alpha M + beta K))
u = F on the free dofs that the sum converges to with all modes.  Nothing here calls the library under test."""
import numpy as np

EPS = np.finfo(np.float64).eps


def modal_damping(lam, alpha=0.0, beta=0.0, zeta=None):
    """d_k = alpha + beta lam_k + 2 zeta_k sqrt(max(lam_k, 0)): the three parts are additive, zeta None means zero."""
    lam = np.asarray(lam)
    z = np.zeros_like(lam) if zeta is None else np.broadcast_to(np.asarray(zeta, dtype=lam.dtype), lam.shape)
    return alpha + beta * lam + 2 * z * np.sqrt(np.maximum(lam, 0))


def coefficients(lam, q, omega, alpha=0.0, beta=0.0, zeta=None, correction=True):
    """a[n_freq][n] in complex128: a_k = q_k H_k, or with the correction q_k (H_k - 1 / lam_k), H_k = 1 / (lam_k - w^2 +
    i w d_k).  The difference is taken as H_k (w^2 - i w d_k) / lam_k, the same number without the cancellation of two
    nearly equal terms where w^2 << lam_k (coefficients_exact evaluates it as written)."""
    lam, q = np.asarray(lam, dtype=np.float64), np.asarray(q, dtype=np.float64)
    w = np.atleast_1d(np.asarray(omega, dtype=np.float64))[:, None]
    d = modal_damping(lam, alpha, beta, zeta)
    H = 1 / ((lam - w * w) + 1j * (w * d))
    return q * (H * ((w * w - 1j * (w * d)) / lam)) if correction else q * H


def coefficients_exact(lam, q, omega, alpha=0.0, beta=0.0, zeta=None, correction=True, digits=60):
    """The same formulas as written, in decimal arithmetic of `digits` digits on the float64 inputs, rounded once to
    complex128: the yardstick of the host test.  (H_k - 1 / lam_k as written loses log10(lam_k / |w^2 - i w d_k|) digits,
    more than extended precision has to spare at low frequencies.)"""
    import decimal
    with decimal.localcontext() as ctx:
        ctx.prec = digits
        D = decimal.Decimal
        out = np.zeros((len(omega), len(lam)), dtype=np.complex128)
        for k, (l, qk) in enumerate(zip(lam, q)):
            l, qk = D(float(l)), D(float(qk))
            z = D(0) if zeta is None else D(float(np.broadcast_to(zeta, np.shape(lam))[k]))
            d = D(float(alpha)) + D(float(beta)) * l + 2 * z * max(l, D(0)).sqrt()
            for j, w in enumerate(omega):
                w = D(float(w))
                a, b = l - w * w, w * d
                den = a * a + b * b
                re, im = a / den, -b / den
                if correction:
                    re -= 1 / l
                out[j, k] = complex(float(qk * re), float(qk * im))
        return out


def response(Phi, coef, u_s=None):
    """u[n_freq][3N] = u_s + sum_k phi_k a_k(w): Phi[3N][n], coef[n_freq][n]."""
    u = coef @ Phi.T.astype(np.complex128)
    return u if u_s is None else u + u_s


def rounding_bound(Phi, coef, u_s=None):
    """4 (m + 4) eps (|u_s,i| + sum_k |phi_ik| |a_k|) per dof and frequency: the rounding of an (m + 1)-term sum on both
    sides."""
    m = Phi.shape[1]
    mag = np.abs(coef) @ np.abs(Phi).T
    return 4 * (m + 4) * EPS * (mag if u_s is None else mag + np.abs(u_s))


def static_solve(K, mask, F):
    """K u_s = F on the free dofs (K masked as feahip_apply_prescribed_bc(0.0) masks it), zero on the prescribed ones."""
    free = np.nonzero(~mask)[0]
    u = np.zeros(len(mask))
    u[free] = np.linalg.solve(K[np.ix_(free, free)], np.asarray(F, dtype=np.float64)[free])
    return u


def direct(K, M, mask, F, omega, alpha=0.0, beta=0.0):
    """u[3N] complex of (K - w^2 M + i w (alpha M + beta K)) u = F on the free dofs: Rayleigh damping, every mode."""
    free = np.nonzero(~mask)[0]
    Kf, Mf = K[np.ix_(free, free)], M[np.ix_(free, free)]
    u = np.zeros(len(mask), dtype=np.complex128)
    u[free] = np.linalg.solve(Kf - omega * omega * Mf + 1j * omega * (alpha * Mf + beta * Kf), np.asarray(F, dtype=np.float64)[free])
    return u

"""Stress from mode superposition restated in float64 numpy on the oracle: the linearised Cauchy stress of a displacement
increment at a Gauss point, the fixed-weight nodal average of it (the weights of ResultsRestatement.nodal_stresses), and
the nine-form von Mises combination.  F, sigma and det J of every Gauss point come from the oracle through
ResultsRestatement.state; the spatial shape gradients from the element tables.  Nothing here calls the library under test.

Rounding bounds.  Every sum below is evaluated twice, once on the values and once on the magnitudes of its terms: A is the
same expression with every product and every sum taken on absolute values.  `chain(deck)` counts the roundings on the
longest path from the nodes to a nodal stress component on the device:
    J = dN x                 npe        F^-1 = g' X              npe       l = du g            npe
    two 3x3 inversions       2 x 11     g = J^-1 dN              3         sigma(F)            12
    b, b:d, b d b, c:d       22         l sigma, the sum, d, tr  10        vol, the division   2
    the Gauss points         G          the visits of a node     the longest visit list
and the restatement makes as many, so |device - restatement| <= 2 chain eps A."""
import numpy as np

import combine_reference as cr
import feahip
from results_reference import SIG6, ResultsRestatement, von_mises

EPS = np.finfo(np.float64).eps
NINE = ((0, None), (1, None), (2, None), (3, None), (4, None), (5, None), (0, 1), (1, 2), (2, 0))


def gp_increment(model, lam, mu, F, sig, l):
    """dsigma = c : d + l sigma + sigma l' - tr(d) sigma for l[..., 3, 3] at the states F, sig[..., 3, 3]; lam, mu
    broadcast against the leading axes."""
    lam, mu = np.asarray(lam, dtype=np.float64)[..., None, None], np.asarray(mu, dtype=np.float64)[..., None, None]
    I = np.eye(3)
    d = 0.5 * (l + np.swapaxes(l, -1, -2))
    tr = np.einsum("...ii->...", d)[..., None, None]
    J = np.linalg.det(F)[..., None, None]
    if model == feahip.MODEL_COMPRESSIBLE_NEOHOOKEAN:
        cd = (lam / J) * tr * I + 2.0 * ((mu - lam * np.log(J)) / J) * d
    else:
        b = F @ np.swapaxes(F, -1, -2)
        bd = np.einsum("...ij,...ij->...", b, d)[..., None, None]
        cd = (lam * bd * b + 2.0 * mu * (b @ d @ b)) / J
    return cd + l @ sig + sig @ np.swapaxes(l, -1, -2) - tr * sig


def gp_increment_magnitudes(model, lam, mu, F, sig, labs):
    """The same sum on the magnitudes of its terms, labs = sum_a |du_a| |g_a|."""
    lam, mu = np.asarray(lam, dtype=np.float64)[..., None, None], np.asarray(mu, dtype=np.float64)[..., None, None]
    I = np.eye(3)
    d = 0.5 * (labs + np.swapaxes(labs, -1, -2))
    tr = np.einsum("...ii->...", d)[..., None, None]
    Jd = np.linalg.det(F)
    J = np.abs(Jd)[..., None, None]
    sa = np.abs(sig)
    if model == feahip.MODEL_COMPRESSIBLE_NEOHOOKEAN:
        cd = (lam / J) * tr * I + 2.0 * ((mu + lam * np.abs(np.log(Jd))[..., None, None]) / J) * d
    else:
        b = np.abs(F) @ np.abs(np.swapaxes(F, -1, -2))
        bd = np.einsum("...ij,...ij->...", b, d)[..., None, None]
        cd = (lam * bd * b + 2.0 * mu * (b @ d @ b)) / J
    return cd + labs @ sa + sa @ np.swapaxes(labs, -1, -2) + tr * sa


class StressRestatement:
    def __init__(self, deck):
        self.deck = deck
        self.r = ResultsRestatement(deck)
        self.w, _, self.dN = feahip.element_tables(deck.ele_type, deck.gauss_nodes_count)
        self.N, self.E, self.npe = self.r.N, self.r.E, self.r.npe

    def close(self):
        self.r.close()

    def chain(self):
        visits = np.bincount(np.asarray(self.deck.elements).ravel(), minlength=self.N).max()
        return 3 * self.npe + 22 + 3 + 12 + 22 + 10 + 2 + len(self.w) + int(visits)

    def gradients(self, x):
        """g[E][G][npe][3] = dN_a/dx_j at the nodes x."""
        xe = np.asarray(x, dtype=np.float64)[self.deck.elements]                       # [E][npe][3]
        J = np.einsum("gik,ekj->egij", self.dN, xe)
        return np.einsum("egik,gka->egai", np.linalg.inv(J), self.dN)

    def gauss_points(self, x, dU):
        """(dsigma[m][E][G][3][3], its magnitude sums, vol[E][G]) of the columns of dU[m][3N] at the nodes x."""
        r = self.r
        F, S, dj = r.state(x)
        g = self.gradients(x)
        du = np.asarray(dU, dtype=np.float64).reshape(len(dU), self.N, 3)[:, self.deck.elements]   # [m][E][npe][3]
        l = np.einsum("meai,egaj->megij", du, g)
        labs = np.einsum("meai,egaj->megij", np.abs(du), np.abs(g))
        lam, mu = r.mats[r.ids, 0][:, None], r.mats[r.ids, 1][:, None]
        ds = gp_increment(self.deck.model, lam, mu, F, S, l)
        da = gp_increment_magnitudes(self.deck.model, lam, mu, F, S, labs)
        return ds, da, self.w[None, :] * np.abs(dj)

    def nodal(self, x, dU, material=-1):
        """(T[m][N][6], A[m][N][6]): the fixed-weight nodal average of dsigma for the columns of dU[m][3N], over all
        elements or those of one material, and the same average of the magnitude sums."""
        ds, da, vol = self.gauss_points(x, dU)
        sel = np.ones(self.E, dtype=bool) if material < 0 else self.r.ids == material
        conn = self.deck.elements[sel]
        ve = vol.sum(axis=1)[sel]
        den = np.zeros(self.N)
        for k in range(self.npe):
            np.add.at(den, conn[:, k], ve)
        out = []
        for field in (ds, da):
            se = np.einsum("eg,megij->emij", vol, field)[sel]
            num = np.zeros((self.N,) + se.shape[1:])
            for k in range(self.npe):
                np.add.at(num, conn[:, k], se)
            t = np.where(den[:, None, None, None] > 0, num / np.where(den > 0, den, 1.0)[:, None, None, None], 0.0)
            out.append(np.stack([t[:, :, i, j] for i, j in SIG6], axis=2).transpose(1, 0, 2))
        return out[0], out[1]

    def bound(self, A):
        return 2 * self.chain() * EPS * A


def nine_forms(T, Ts, C, b=None, s=0.0, absolute=False):
    """The forms of combine_reference.combine on the nine combinations of T[m][N][6] and Ts[N][6]: the six components, then
    xx - yy, yy - zz, zz - xx.  Returns (v[N][9], A[N][9]); the magnitude sums of a difference take |T_0| + |T_1|."""
    T = np.asarray(T, dtype=np.float64)
    Ts = np.zeros(T.shape[1:]) if Ts is None else np.asarray(Ts, dtype=np.float64)
    v, A = [], []
    for c0, c1 in NINE:
        if c1 is None:
            y, ys, ya, ysa = T[:, :, c0].T, Ts[:, c0], np.abs(T[:, :, c0].T), np.abs(Ts[:, c0])
        else:
            y, ys = (T[:, :, c0] - T[:, :, c1]).T, Ts[:, c0] - Ts[:, c1]
            ya, ysa = (np.abs(T[:, :, c0]) + np.abs(T[:, :, c1])).T, np.abs(Ts[:, c0]) + np.abs(Ts[:, c1])
        if absolute:
            y = np.abs(y)
        vi, _ = cr.combine(y, ys, C, b, s)
        _, Ai = cr.combine(ya, ysa, C, b, s)
        v.append(vi)
        A.append(Ai)
    return np.stack(v, axis=1), np.stack(A, axis=1)


def stress_combine(T, Ts, C, b=None, s=0.0, absolute=False):
    """(v6[N][6], bound6, vvm[N], boundvm) in float64: the device returns sqrt(max(0, v6)) and sqrt(max(0, vvm)),
        vvm = (q(xx-yy) + q(yy-zz) + q(zz-xx)) / 2 + 3 (q(xy) + q(yz) + q(xz)).
    Bounds as combine_bound builds them: a component is a chain of at most m + 3 terms (m + 5 with the margin of
    combine_bound); a difference adds the rounding of the subtraction (m + 6); the von Mises sum adds the five additions
    and two products of its six forms (m + 13)."""
    m = len(T)
    v, A = nine_forms(T, Ts, C, b, s, absolute)
    vvm = 0.5 * (v[:, 6] + v[:, 7] + v[:, 8]) + 3.0 * (v[:, 3] + v[:, 4] + v[:, 5])
    Avm = 0.5 * (A[:, 6] + A[:, 7] + A[:, 8]) + 3.0 * (A[:, 3] + A[:, 4] + A[:, 5])
    return v[:, :6], cr.combine_bound(m, v[:, :6], A[:, :6]), vvm, cr.combine_bound(m + 8, vvm, Avm)


def field(T, Ts, coef, cs=0.0):
    """(sig6[N][6], its von Mises stress) of cs Ts + sum_k coef_k T_k."""
    sig6 = np.einsum("k,kac->ac", np.asarray(coef, dtype=np.float64), np.asarray(T, dtype=np.float64))
    if Ts is not None:
        sig6 = sig6 + cs * np.asarray(Ts, dtype=np.float64)
    return sig6, von_mises(sig6)

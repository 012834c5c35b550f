"""Stress peaks over a frequency sweep or a transient restated in float64 numpy (include/fea_hip.h, "stress peaks over a
frequency sweep or a transient"): the stress components of every table row from a stress store T[m][N][6], T_s[N][6] and a
coefficient table, the von Mises stress of a real state, the largest von Mises stress over the cycle of a harmonic state
by its closed form and by brute force over 4096 phases, the rounding bounds, and which peak indices the bounds decide.
Nothing here calls the entries under test.

The harmonic peak.  sigma(t) = re cos wt - im sin wt, and with V the (positive semidefinite) von Mises form, A = re' V re,
B = im' V im, C = re' V im,
    vm^2(t) = A cos^2 + B sin^2 - 2 C sin cos = (A + B) / 2 + ((A - B) / 2) cos 2wt - C sin 2wt,
whose largest value is (A + B) / 2 + sqrt(((A - B) / 2)^2 + C^2).  V acts on the deviators: 1.5 d_a d_b on the three normal
components, 3 s_a s_b on the three shears.

Bounds (EPS is float64 epsilon, m the number of modes).
  e_c = 4 (m + 5) EPS (|T_s,c| |g| + sum_k |T_k,c| |a_k|) bounds the error of the real and of the imaginary part of a
      component each, device against restatement: rounding_bound of tests/transient_reference.py on stress rows (|g| = 1
      for a sweep, |a_k| the complex magnitude there).
  peak6   transient: e_c (fabs is exact).  Sweep: the complex error is at most sqrt(2) e_c, and |s|^2 = fma(re, re, im im)
      with its root is three roundings on either side: sqrt(2) e_c + K_MAG EPS |s_c|, K_MAG = 6.
  vm      the cycle peak of the von Mises stress is a seminorm on C^6, bounded by sqrt(3) |.|_2: moving the six components
      by (sqrt(2) e_c each) moves it by at most sqrt(3 sum_c 2 e_c^2) = sqrt(6 sum_c e_c^2); a real state by at most
      sqrt(3 sum_c e_c^2).  The arithmetic of the combination adds k EPS sqrt(3 sum_c |s_c|^2), k twice the roundings on
      its longest path.  Sweep: the mean (2 sums, 1 product), the deviator (1), the share w d d (2), the tree of the six
      shares (3), A + B (1), the product C C and the fma (2), the inner root (1), the outer sum (1), the last root (1):
      15, K_SWEEP = 30.  Transient: mean (3), deviator (1), share (2), tree (3), root (1): 10, K_TRANSIENT = 20.
      Every one of these roundings is relative to a quantity no larger than sqrt(3) |s|_2 -- the mean included, which is
      why the bound is stated on |s| and holds at a nearly hydrostatic state only for the deviator form."""
import numpy as np

from results_reference import von_mises

EPS = np.finfo(np.float64).eps
PHASES = 4096
K_MAG, K_SWEEP, K_TRANSIENT = 6, 30, 20


def deviator(s):
    """s[..., 6] with the mean of the three normal components taken off them."""
    s = np.asarray(s)
    out = s.copy()
    out[..., :3] -= (s[..., :3].sum(axis=-1) / 3.0)[..., None]
    return out


def vm_form(a, b):
    """a' V b on deviators a, b[..., 6] (real)."""
    return 1.5 * (a[..., :3] * b[..., :3]).sum(axis=-1) + 3.0 * (a[..., 3:] * b[..., 3:]).sum(axis=-1)


def harmonic_peak(s):
    """The closed form: the largest von Mises stress over the cycle of Re(s exp(i w t)), s complex [..., 6]."""
    s = np.asarray(s, dtype=np.complex128)
    re, im = deviator(s.real), deviator(s.imag)
    A, B, C = vm_form(re, re), vm_form(im, im), vm_form(re, im)
    return np.sqrt(0.5 * (A + B) + np.sqrt((0.5 * (A - B)) ** 2 + C * C))


def harmonic_sampled(s, phases=PHASES):
    """The same by brute force: the largest von Mises stress of re cos - im sin over `phases` equally spaced phases."""
    s = np.asarray(s, dtype=np.complex128)
    best = np.zeros(s.shape[:-1])
    for th in 2 * np.pi * np.arange(phases) / phases:
        best = np.maximum(best, von_mises(s.real * np.cos(th) - s.imag * np.sin(th)))
    return best


def harmonic_peak_expanded(s):
    """The form the entries must NOT use: sum p^2 - (sum p)^2 / 3 on the normal components.  For the hydrostatic test."""
    s = np.asarray(s, dtype=np.complex128)

    def form(a, b):
        n = (a[..., :3] * b[..., :3]).sum(axis=-1) - a[..., :3].sum(axis=-1) * b[..., :3].sum(axis=-1) / 3.0
        return 1.5 * n + 3.0 * (a[..., 3:] * b[..., 3:]).sum(axis=-1)
    A, B, C = form(s.real, s.real), form(s.imag, s.imag), form(s.real, s.imag)
    return np.sqrt(np.maximum(0.5 * (A + B) + np.sqrt((0.5 * (A - B)) ** 2 + C * C), 0.0))


def harmonic_peak_longdouble(s):
    """The closed form in numpy.longdouble on the float64 inputs, rounded once."""
    LD = np.longdouble
    s = np.asarray(s, dtype=np.complex128)
    re, im = deviator(s.real.astype(LD)), deviator(s.imag.astype(LD))
    A, B, C = vm_form(re, re), vm_form(im, im), vm_form(re, im)
    return np.sqrt(LD(0.5) * (A + B) + np.sqrt((LD(0.5) * (A - B)) ** 2 + C * C)).astype(np.float64)


def components(T, Ts, coef, g=None):
    """s[rows][N][6] = T_s g + sum_k T_k a_k: T[m][N][6], Ts[N][6] or None, coef[rows][m] complex (a sweep: g is 1) or
    real (a transient: g[rows])."""
    T = np.asarray(T, dtype=np.float64)
    coef = np.asarray(coef)
    s = np.einsum("jk,kac->jac", coef, T.astype(coef.dtype))
    if Ts is not None:
        s = s + (np.ones(len(coef)) if g is None else np.asarray(g, dtype=np.float64))[:, None, None] * np.asarray(Ts, dtype=np.float64)
    return s


def component_bound(T, Ts, coef, g=None):
    """e[rows][N][6] = 4 (m + 5) EPS (|T_s| |g| + sum_k |T_k| |a_k|)."""
    T = np.asarray(T, dtype=np.float64)
    mag = np.einsum("jk,kac->jac", np.abs(np.asarray(coef)), np.abs(T))
    if Ts is not None:
        mag = mag + np.abs(np.ones(len(coef)) if g is None else np.asarray(g, dtype=np.float64))[:, None, None] * np.abs(np.asarray(Ts, dtype=np.float64))
    return 4 * (len(T) + 5) * EPS * mag


def sweep_values(T, Ts, coef):
    """(|s|[j][N][6], its bound, vm_peak[j][N], its bound) of a frequency sweep."""
    s, e = components(T, Ts, coef), component_bound(T, Ts, coef)
    mag = np.abs(s)
    norm = np.sqrt(3.0 * (mag ** 2).sum(axis=-1))
    return mag, np.sqrt(2.0) * e + K_MAG * EPS * mag, harmonic_peak(s), np.sqrt(6.0 * (e ** 2).sum(axis=-1)) + K_SWEEP * EPS * norm


def transient_values(T, Ts, coef, g):
    """(|sigma|[n][N][6], its bound, vm[n][N], its bound) of a transient."""
    s, e = components(T, Ts, coef, g), component_bound(T, Ts, coef, g)
    mag = np.abs(s)
    norm = np.sqrt(3.0 * (mag ** 2).sum(axis=-1))
    return mag, e, von_mises(s), np.sqrt(3.0 * (e ** 2).sum(axis=-1)) + K_TRANSIENT * EPS * norm


def decided(V, B):
    """(the argmax of V[rows][...] over the rows, where it is decided): the largest value exceeds the runner-up by more
    than both their bounds B.  A single row decides everything."""
    best = V.argmax(axis=0)
    if len(V) == 1:
        return best, np.ones(V.shape[1:], dtype=bool)
    order = np.argsort(V, axis=0, kind="stable")
    top, second = order[-1], order[-2]
    take = lambda a, idx: np.take_along_axis(a, idx[None], axis=0)[0]
    gap = take(V, top) - take(V, second)
    return best, gap > take(B, top) + take(B, second)


def decided_share(V, B, keep=None):
    """The decided share of the entries `keep` (all of them by default)."""
    _, sure = decided(V, B)
    keep = np.ones(sure.shape, dtype=bool) if keep is None else np.broadcast_to(keep, sure.shape)
    return (sure & keep).sum() / max(keep.sum(), 1)


def check_peaks(what, V, B, peak, at, keep=None, share=0.95):
    """peak within the bound of the restatement's largest value (the largest bound over the rows, as check_peaks of
    tests/test_gpu_transient.py takes it); at the restatement's argmax wherever decided, at least `share` of the entries
    `keep` decided, elsewhere the value at the returned index within twice the bound of the largest."""
    assert peak.shape == V.shape[1:] and at.shape == V.shape[1:], (peak.shape, at.shape, V.shape)
    worst = B.max(axis=0)
    err = np.abs(peak - V.max(axis=0))
    print(what, "largest error / bound", (err / np.where(worst > 0, worst, 1.0)).max())
    assert np.all(err <= worst)
    best, sure = decided(V, B)
    keep = np.ones(sure.shape, dtype=bool) if keep is None else np.broadcast_to(keep, sure.shape)
    print(what, "_at: decided", (sure & keep).sum(), "of", keep.sum(), "; rows", at.min(), "..", at.max())
    assert (sure & keep).sum() >= share * keep.sum()
    assert np.array_equal(at[sure & keep], best[sure & keep])
    assert at.min() >= 0 and at.max() < len(V)
    got = np.take_along_axis(V, at[None].astype(np.int64), axis=0)[0]
    assert np.all(got >= V.max(axis=0) - 2 * worst)

"""Response spectrum and random vibration on the host side: the three builders of csrc/combine_table.cpp against the
restatement of tests/combine_reference.py in float64 and in long double, the form of a PSD against the library's own sweep
coefficients and against the closed forms of white noise, the grid helper to the bit, the CQC coefficient, the
interpolation, every refusal, the deck grammar of (spectrum ...) and (random ...), the struct fields and the exported
symbols.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import combine_reference as cr
import feahip
import mesh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps
LD = cr.LD
NEW = ("feahip_response_combine", "feahip_response_random", "feahip_response_spectrum", "feahip_host_random_form",
       "feahip_host_random_grid", "feahip_host_psd_value", "feahip_host_spectrum_value", "feahip_host_spectrum_form")
_dp = C.POINTER(C.c_double)


def _within(name, got, want, exact, plain):
    """got within the project's tolerance of want: 100 times the gap between the restatement in float64 (plain) and in
    long double (exact), with a floor of 64 eps times the largest entry (the rule of tests/test_gpu_pcg.py)."""
    exact = np.asarray(exact, dtype=LD)
    gap = float(np.abs(np.asarray(plain, dtype=LD) - exact).max())
    tol = max(100.0 * gap, 64 * EPS * float(np.abs(exact).max()))
    err = float(np.abs(np.asarray(got, dtype=LD) - np.asarray(want, dtype=LD)).max())
    print(f"{name}: error {err:.3e}, float64 gap {gap:.3e}, tolerance {tol:.3e}")
    assert err <= tol


def _modes(n):
    """Frequencies over a decade and a half, two of them 1 % apart where there are that many; q of either sign."""
    w = np.array([3.0]) if n == 1 else np.geomspace(1.0, 30.0, n)
    if n >= 3:
        w[2] = 1.01 * w[1]
    w = np.sort(w)
    return w * w, np.random.default_rng(n).standard_normal(n)


PSD_W, PSD_S = np.array([0.2, 1.0, 10.0, 45.0]), np.array([0.5, 2.0, 2.0, 0.1])


@pytest.mark.parametrize("n_modes", [1, 8, 9, 64])
@pytest.mark.parametrize("ratio", [0.005, 0.02, 1.0])
@pytest.mark.parametrize("correction", [False, True])
def test_builders_against_the_restatement(n_modes, ratio, correction):
    """Modal damping ratio 0.005, 0.02 or 1 on every mode beside a little Rayleigh damping; the PSD a table read log-log on
    the helper's own grid; the three quantities; the three rules, and the missing mass where it applies."""
    lam, q = _modes(n_modes)
    zeta = np.full(n_modes, ratio)
    alpha, beta = 0.01, 1e-5
    omega = feahip.host_random_grid(lam, alpha, beta, zeta, 0.0, 40.0, 65, 8, breakpoints=PSD_W)
    assert np.array_equal(omega, cr.random_grid(lam, alpha, beta, zeta, 0.0, 40.0, 65, 8, PSD_W))
    S = feahip.host_psd_value(PSD_W, PSD_S, omega, loglog=True)
    assert S.min() == 0.0 and S.max() == 2.0                            # zero outside the table, the plateau inside
    sa = feahip.host_spectrum_value(PSD_W, PSD_S, np.sqrt(lam), loglog=False)
    for quantity in (0, 1, 2):
        got = feahip.host_random_form(lam, q, omega, S, alpha, beta, zeta, correction, quantity)
        exact = cr.random_form(lam, q, omega, S, alpha, beta, zeta, correction, quantity, LD)
        plain = cr.random_form(lam, q, omega, S, alpha, beta, zeta, correction, quantity, np.float64)
        assert got[0].shape == (n_modes, n_modes) and np.array_equal(got[0], got[0].T)
        assert correction or (not got[1].any() and got[2] == 0.0)
        # the same sum over the rows the sweep itself uses
        rows = feahip.host_response_coefficients(lam, q, omega, alpha, beta, zeta, correction)[:, :n_modes]
        of_rows = cr.form_of_rows(rows, omega, S, correction, quantity, LD)
        for name, g, r, e, p in zip("Cbs", got, of_rows, exact, plain):
            _within(f"random {name}, quantity {quantity}", g, e, e, p)
            _within(f"random {name} from the sweep's rows, quantity {quantity}", g, r, e, p)
        for rule in (cr.SRSS, cr.CQC, cr.ABS):
            zpa = 0.75 if correction and quantity == 0 and rule != cr.ABS else 0.0
            got = feahip.host_spectrum_form(lam, q, sa, rule, alpha, beta, zeta, correction, zpa, quantity)
            exact = cr.spectrum_form(lam, q, sa, rule, alpha, beta, zeta, correction, zpa, quantity, LD)
            plain = cr.spectrum_form(lam, q, sa, rule, alpha, beta, zeta, correction, zpa, quantity, np.float64)
            assert np.array_equal(got[0], got[0].T) and (zpa > 0) == bool(got[1].any()) and got[2] == zpa * zpa
            for name, g, e, p in zip("Cbs", got, exact, plain):
                _within(f"spectrum rule {rule} {name}, quantity {quantity}", g, e, e, p)


def test_white_noise_against_the_closed_forms():
    """lam = (4, 9, 9.5), zeta = (0.02, 0.01, 0.05), S0 = 1 on [0, 200 sqrt(9.5)], 2049 background points and 1024 per mode.
    Numpy on exactly this grid is off by 5.6e-5, 1.3e-5, 3.8e-5 on the diagonal and 2.9e-5 on C_23 (relative): the bound
    is 2e-4, three times the worst, and covers the band's cut-off."""
    lam, zeta, q = np.array([4.0, 9.0, 9.5]), np.array([0.02, 0.01, 0.05]), np.array([1.0, -0.7, 1.3])
    w_hi = 200 * np.sqrt(9.5)
    omega = feahip.host_random_grid(lam, 0.0, 0.0, zeta, 0.0, w_hi, 2049, 1024)
    assert np.array_equal(omega, cr.random_grid(lam, 0.0, 0.0, zeta, 0.0, w_hi, 2049, 1024))
    assert omega[0] == 0.0 and omega[-1] == w_hi and np.all(np.diff(omega) > 0) and len(omega) <= 2049 + 3 * 1024
    Cm, b, s = feahip.host_random_form(lam, q, omega, np.ones_like(omega), zeta=zeta, static_correction=False)
    want = cr.white_noise_covariance(lam, q, 2 * zeta * np.sqrt(lam), 1.0)
    rel = np.abs(Cm - want) / np.abs(want)
    print("grid points", len(omega), "relative errors: diagonal", np.diag(rel), "C_23", rel[1, 2], "C_12", rel[0, 1], "C_13", rel[0, 2])
    assert np.all(np.diag(rel) <= 2e-4) and rel[1, 2] <= 2e-4
    # with the correction s is the mean square of the load factor itself
    _, _, s = feahip.host_random_form(lam, q, omega, np.ones_like(omega), zeta=zeta, static_correction=True)
    assert abs(s - w_hi) <= 1e-12 * w_hi


def test_grid_helper():
    lam, zeta = np.array([0.0, -1.0, 4.0, 9.0, 1e4]), np.array([0.1, 0.1, 0.0, 0.05, 0.05])
    # a zero, a negative and an undamped mode add nothing; a mode outside the band adds what falls inside
    g = feahip.host_random_grid(lam, 0.0, 0.0, zeta, 1.0, 5.0, 5, 16)
    assert np.array_equal(g, cr.random_grid(lam, 0.0, 0.0, zeta, 1.0, 5.0, 5, 16))
    assert set(np.linspace(1.0, 5.0, 5)) <= set(g) and 5 < len(g) <= 5 + 2 * 16 and g.min() == 1.0 and g.max() == 5.0
    # breakpoints are kept inside the band, dropped outside, and a duplicate of a background point is one point
    g2 = feahip.host_random_grid(lam, 0.0, 0.0, zeta, 1.0, 5.0, 5, 16, breakpoints=[2.5, 0.5, 3.0, 7.0, 2.5])
    assert np.array_equal(g2, np.unique(np.concatenate([g, [2.5]])))
    # the size query: a NULL output, no breakpoints
    lib = feahip.load_library()
    n = C.c_int(0)
    l, z = np.ascontiguousarray(lam), np.ascontiguousarray(zeta)
    args = (len(l), l.ctypes.data_as(_dp), 0.0, 0.0, z.ctypes.data_as(_dp), 1.0, 5.0, 5, 16)
    assert lib.feahip_host_random_grid(*args, None, C.byref(n)) == 0 and n.value == len(g)
    # Rayleigh damping alone gives every positive mode its points
    assert len(feahip.host_random_grid([4.0, 9.0], 0.1, 0.0, None, 0.0, 10.0, 3, 4)) == 3 + 8
    for kw in (dict(w_lo=-1.0), dict(w_hi=1.0), dict(w_hi=0.5), dict(w_hi=np.inf), dict(w_lo=np.nan), dict(n_background=1),
               dict(n_per_mode=-1), dict(alpha=-0.1), dict(beta=np.nan), dict(zeta=[0.1, -0.1, 0, 0, 0]),
               dict(lam=[np.nan, 1, 1, 1, 1]), dict(breakpoints=[np.nan]), dict(breakpoints=[np.inf]),
               dict(n_background=feahip.RANDOM_MAX_FREQ + 1)):
        a = dict(lam=lam, alpha=0.0, beta=0.0, zeta=zeta, w_lo=1.0, w_hi=5.0, n_background=5, n_per_mode=16)
        a.update(kw)
        with pytest.raises(feahip.FeaHipError):
            feahip.host_random_grid(**a)
    assert lib.feahip_host_random_grid(*args, None, None) == feahip.EINVAL
    assert lib.feahip_host_random_grid(65, *args[1:], None, C.byref(n)) == feahip.EINVAL


def test_cqc():
    rng = np.random.default_rng(24)
    w = np.sort(rng.uniform(1.0, 50.0, 24))
    w[11] = 1.001 * w[10]                                               # two of them 0.1 % apart
    w = np.sort(w)
    lam, q, zeta = w * w, rng.standard_normal(24), rng.uniform(0.01, 0.1, 24)
    sa = np.ones(24)
    Cm, b, s = feahip.host_spectrum_form(lam, q, sa, feahip.CQC, zeta=zeta)
    a = q / lam
    assert np.array_equal(Cm, Cm.T) and not b.any() and s == 0.0
    rho = Cm / np.outer(a, a)
    assert np.all(np.abs(np.diag(rho) - 1.0) <= 4 * EPS)
    assert np.all(np.abs(np.diag(Cm) - a * a) <= 2 * EPS * a * a)       # rho_kk = 1 exactly: the diagonal is a_k^2
    ref = cr.correlation(w.astype(LD), zeta.astype(LD))
    assert np.abs(rho - ref.astype(np.float64)).max() <= 64 * EPS
    low = np.linalg.eigvalsh(rho).min()
    print("smallest eigenvalue of rho", low, "largest off-diagonal", np.abs(rho - np.eye(24)).max())
    assert low > 0 and np.abs(rho - np.eye(24)).max() > 0.9 and np.all(rho > 0) and np.all(rho <= 1 + 4 * EPS)
    # zero damping: the SRSS table entry for entry
    srss = feahip.host_spectrum_form(lam, q, sa, feahip.SRSS)
    cqc0 = feahip.host_spectrum_form(lam, q, sa, feahip.CQC)
    assert np.array_equal(srss[0], cqc0[0]) and np.array_equal(srss[0], np.diag(np.diag(srss[0])))
    # equal undamped frequencies: a zero denominator off the diagonal gives 1
    same = feahip.host_spectrum_form([4.0, 4.0], [1.0, -2.0], [1.0, 1.0], feahip.CQC)[0]
    assert np.array_equal(same, np.outer([0.25, -0.5], [0.25, -0.5]))
    # ABS: |a||a|'; SRSS its diagonal; pseudo-velocity and pseudo-acceleration scale a by w and w^2
    for quantity, scale in ((0, np.ones(24)), (1, w), (2, lam)):
        ak = np.abs(a) * scale
        ab = feahip.host_spectrum_form(lam, q, sa, feahip.ABS, quantity=quantity)[0]
        assert np.abs(ab - np.outer(ak, ak)).max() <= 8 * EPS * ak.max() ** 2


def test_interpolation():
    w, v = [1.0, 2.0, 4.0, 8.0], [1.0, 4.0, 4.0, 0.0]
    for loglog in (False, True):
        for fn, outside in ((feahip.host_psd_value, (0.0, 0.0)), (feahip.host_spectrum_value, (1.0, 0.0))):
            assert [fn(w, v, x, loglog) for x in w] == v                # at the points: their own values, to the bit
            assert fn(w, v, 0.5, loglog) == outside[0] and fn(w, v, 9.0, loglog) == outside[1]
            assert fn(w, v, 3.0, loglog) == 4.0                         # a plateau either way
            for x in (1.5, 5.0, 7.999):
                assert fn(w, v, x, loglog) == cr.table_value(w, v, x, loglog, fn is feahip.host_spectrum_value)
    assert abs(feahip.host_psd_value(w, v, 1.5) - 2.5) <= 4 * EPS and abs(feahip.host_psd_value(w, v, 6.0) - 2.0) <= 4 * EPS
    assert abs(feahip.host_psd_value(w, v, np.sqrt(2.0), True) - 2.0) <= 8 * EPS       # a power law: v = w^2 on [1, 2]
    assert abs(feahip.host_psd_value(w, v, 6.0, True) - 2.0) <= 4 * EPS                # a segment ending at zero is linear
    assert feahip.host_psd_value([0.0, 2.0], [1.0, 3.0], 1.0, True) == 2.0             # and so is one starting at w = 0
    assert feahip.host_spectrum_value([3.0], [7.0], 1.0) == 7.0 and feahip.host_psd_value([3.0], [7.0], 3.0) == 7.0
    assert np.array_equal(feahip.host_psd_value(w, v, np.array([0.5, 1.0, 3.0])), [0.0, 1.0, 4.0])
    for bad in (dict(w=[1.0, 1.0]), dict(w=[2.0, 1.0]), dict(w=[1.0, np.nan]), dict(v=[1.0, np.inf]), dict(at=np.nan), dict(w=[], v=[])):
        a = dict(w=[1.0, 2.0], v=[1.0, 2.0], at=1.5)
        a.update(bad)
        for fn in (feahip.host_psd_value, feahip.host_spectrum_value):
            with pytest.raises(feahip.FeaHipError):
                fn(a["w"], a["v"], a["at"])
    lib = feahip.load_library()
    assert np.isnan(lib.feahip_host_psd_value(2, None, None, 0, 1.0))


def test_refusals():
    lam, q = np.array([4.0, 9.0]), np.array([1.0, -1.0])
    omega, S = np.array([0.0, 1.0, 2.5]), np.array([1.0, 0.0, 2.0])
    ok = feahip.host_random_form(lam, q, omega, S, 0.1)
    assert np.isfinite(ok[0]).all() and ok[2] > 0
    for kw in (dict(omega=[0.0, 1.0, 1.0]), dict(omega=[0.0, 2.0, 1.0]), dict(omega=[-1.0, 1.0, 2.0]), dict(omega=[0.0, 1.0, np.inf]),
               dict(omega=[0.0, np.nan, 2.0]), dict(S=[1.0, -1e-300, 1.0]), dict(S=[1.0, np.inf, 1.0]), dict(S=[np.nan, 1.0, 1.0]),
               dict(omega=[1.0], S=[1.0]), dict(quantity=-1), dict(quantity=3), dict(alpha=-0.1), dict(alpha=np.nan),
               dict(beta=-1e-3), dict(beta=np.inf), dict(zeta=[0.1, -0.1]), dict(zeta=[np.inf, 0.0]), dict(lam=[4.0, np.nan]),
               dict(q=[np.inf, 1.0]), dict(lam=[0.0, 4.0]), dict(lam=[-1.0, 4.0]),
               dict(omega=[0.0, 2.0, 2.5], alpha=0.0)):                   # the last: w^2 = lam_k without damping
        a = dict(lam=lam, q=q, omega=omega, S=S, alpha=0.1, beta=0.0, zeta=None, static_correction=True, quantity=0)
        a.update(kw)
        with pytest.raises(feahip.FeaHipError):
            feahip.host_random_form(**a)
    feahip.host_random_form([0.0, 4.0], q, [0.5, 1.0], [1.0, 1.0], 0.1, static_correction=False)   # a zero mode without the correction, w > 0
    with pytest.raises(feahip.FeaHipError):
        feahip.host_random_form([0.0, 4.0], q, [0.0, 1.0], [1.0, 1.0], 0.1, static_correction=False)    # ... refused at w = 0
    lib = feahip.load_library()
    one = (C.c_double * 2)(1.0, 2.0)
    out = (C.c_double * 4096)()
    s = C.c_double(0)
    tail = (0.1, 0.0, None, 0, 0, out, out, C.byref(s))
    assert lib.feahip_host_random_form(1, one, one, 2, one, one, *tail) == 0
    for n in (0, 65):
        assert lib.feahip_host_random_form(n, one, one, 2, one, one, *tail) == feahip.EINVAL
    for n in (1, 0, -1, feahip.RANDOM_MAX_FREQ + 1):
        assert lib.feahip_host_random_form(1, one, one, n, one, one, *tail) == feahip.EINVAL
    for k in range(6):
        args = [one] * 6
        args[k] = None
        assert lib.feahip_host_random_form(1, args[0], args[1], 2, args[2], args[3], 0.1, 0.0, None, 0, 0, args[4], args[5],
                                           C.byref(s)) == feahip.EINVAL
    assert lib.feahip_host_random_form(1, one, one, 2, one, one, 0.1, 0.0, None, 0, 0, out, out, None) == feahip.EINVAL
    # the cap itself is accepted
    w = np.linspace(0.0, 10.0, feahip.RANDOM_MAX_FREQ)
    big = feahip.host_random_form([4.0], [1.0], w, np.ones_like(w), 0.1, static_correction=False)
    assert abs(big[0][0, 0] - np.pi / (2 * 0.1 * 4.0)) <= 2e-3 * big[0][0, 0]
    # the spectrum
    sa = np.array([1.0, 2.0])
    feahip.host_spectrum_form(lam, q, sa, feahip.CQC, zeta=0.05, static_correction=True, zpa=0.5)
    for kw in (dict(lam=[0.0, 4.0]), dict(lam=[-1.0, 4.0]), dict(lam=[np.nan, 4.0]), dict(rule=-1), dict(rule=3), dict(quantity=-1),
               dict(quantity=3), dict(zpa=0.5, quantity=1), dict(zpa=0.5, quantity=2), dict(zpa=-0.5), dict(zpa=np.inf),
               dict(zpa=0.5, static_correction=False), dict(zpa=0.5, rule=feahip.ABS), dict(sa=[1.0, -1.0]),
               dict(sa=[np.nan, 1.0]), dict(q=[np.inf, 1.0]), dict(alpha=-0.1), dict(beta=np.nan), dict(zeta=[0.1, -0.1])):
        a = dict(lam=lam, q=q, sa=sa, rule=feahip.CQC, alpha=0.0, beta=0.0, zeta=None, static_correction=True, zpa=0.0, quantity=0)
        a.update(kw)
        with pytest.raises(feahip.FeaHipError):
            feahip.host_spectrum_form(**a)
    for n in (0, 65):
        assert lib.feahip_host_spectrum_form(n, one, one, one, 0.0, 0.0, None, 0, 0, 0.0, 0, out, out, C.byref(s)) == feahip.EINVAL
    assert lib.feahip_host_spectrum_form(1, one, one, one, 0.0, 0.0, None, 0, 0, 0.0, 0, out, out, C.byref(s)) == 0
    assert lib.feahip_host_spectrum_form(1, one, one, None, 0.0, 0.0, None, 0, 0, 0.0, 0, out, out, C.byref(s)) == feahip.EINVAL
    assert lib.feahip_host_spectrum_form(1, one, one, one, 0.0, 0.0, None, 0, 0, 0.0, 0, None, out, C.byref(s)) == feahip.EINVAL
    # the device entries refuse a null context before anything else
    assert lib.feahip_response_combine(None, out, None, 0.0, 0, out) == feahip.EINVAL
    assert lib.feahip_response_random(None, 2, one, one, 0.1, 0.0, None, 0, out, None) == feahip.EINVAL
    assert lib.feahip_response_spectrum(None, 2, one, one, 0, 0, 0.0, 0.0, None, 0.0, 0, out, None) == feahip.EINVAL


def test_symbols_and_constants():
    lib = feahip.load_library()
    top = open(os.path.join(ROOT, "include", "fea_hip.h")).read()
    out = os.popen(f"nm -D --defined-only {feahip.LIB_PATH}").read()
    for name in NEW:
        assert name in feahip.ABI and hasattr(lib, name), name
        assert re.search(r"\b(int|double)\s+%s\(" % name, top) and re.search(rf"\bT {name}\b", out), name
    assert re.search(r"#define\s+FEA_RANDOM_MAX_FREQ\s+262144\b", top) and feahip.RANDOM_MAX_FREQ == 262144
    assert re.search(r"FEAHIP_SRSS = 0, FEAHIP_CQC = 1, FEAHIP_ABS = 2", top)
    assert (feahip.SRSS, feahip.CQC, feahip.ABS) == (0, 1, 2)
    for name in ("response_combine", "response_random", "response_spectrum"):
        assert callable(getattr(feahip.FeaSolver, name))
        assert not hasattr(feahip.FeaGroup, name)                      # the locked solve is unsharded, and so is this
    for name in ("host_random_form", "host_random_grid", "host_spectrum_form", "host_psd_value", "host_spectrum_value"):
        assert callable(getattr(feahip, name))
    src = open(os.path.join(ROOT, "fea-large_amd", "csrc", "Makefile")).read()
    assert "kernels_combine.o" in src and "combine_table.o" in src


def _deck(**kw):
    d = mesh.bar_deck(dims=(1, 2, 1))
    keys = ("model", "parameters", "ele_type", "gauss_nodes_count", "nodes", "elements", "presc_node", "presc_type", "presc_values")
    return feahip.Deck(**{k: getattr(d, k) for k in keys}, **kw)


BASE = dict(density=1.5, dynamics=dict(steps=0, dt=1.0), modal_count=12)
FIELDS = ["has_spectrum", "spectrum_count", "spectrum_points", "spectrum_rule", "spectrum_static", "spectrum_loglog",
          "spectrum_has_base", "spectrum_zeta", "spectrum_zpa", "spectrum_base", "has_random", "random_count", "random_points",
          "random_static", "random_loglog", "random_per_mode", "random_background", "random_has_base", "random_zeta",
          "random_base"]
SPECTRUM = dict(spectrum_points=[(0.5, 1.0 / 3.0), (5.0, 2.0), (50.0, 2.0)], spectrum_rule="cqc", spectrum_zeta=0.05,
                spectrum_zpa=0.7, spectrum_interp="loglog", spectrum_base=(1.0, 0.0, -1.0 / 3.0))
RANDOM = dict(random_points=[(0.0, 1.0), (1.0 / 3.0, 2.5), (40.0, 0.0)], random_zeta=1.0 / 30.0, random_per_mode=16,
              random_background=65, random_static=False)


def test_deck_round_trip(tmp_path):
    d = _deck(**BASE, damping=(0.25, 1e-4), **SPECTRUM, **RANDOM)
    p = tmp_path / "both.sexp"
    d.save(str(p))
    text = p.read_text()
    assert re.search(r"\(spectrum :rule cqc :zeta \S+ :static-correction t :zpa \S+ :interp loglog :base \(1 0 \S+\)\n"
                     r"    \(points \(0.5 \S+\) \(5 2\) \(50 2\)\)\)", text)
    assert re.search(r"\(random :zeta \S+ :static-correction nil :interp linear :per-mode 16 :background 65\n"
                     r"    \(psd \(0 1\) \(\S+ 2.5\) \(40 0\)\)\)", text)
    back = feahip.Deck.load(str(p))
    assert np.array_equal(back.spectrum_points, SPECTRUM["spectrum_points"]) and np.array_equal(back.random_points, RANDOM["random_points"])
    assert (back.spectrum_rule, back.spectrum_zeta, back.spectrum_zpa, back.spectrum_interp, back.spectrum_static,
            back.spectrum_base) == ("cqc", 0.05, 0.7, "loglog", True, (1.0, 0.0, -1.0 / 3.0))
    assert (back.random_zeta, back.random_per_mode, back.random_background, back.random_static, back.random_interp,
            back.random_base) == (1.0 / 30.0, 16, 65, False, "linear", None)
    assert back.damping == (0.25, 1e-4) and back.modal_count == 12
    q = tmp_path / "again.sexp"
    back.save(str(q))
    assert q.read_bytes() == p.read_bytes()
    # the defaults
    p.write_text(re.sub(r"\(spectrum [^\n]*\n", "(spectrum\n", re.sub(r"\(random [^\n]*\n", "(random\n", text)))
    back = feahip.Deck.load(str(p))
    assert (back.spectrum_rule, back.spectrum_zeta, back.spectrum_zpa, back.spectrum_interp, back.spectrum_static,
            back.spectrum_base) == ("srss", 0.0, 0.0, "linear", True, None)
    assert (back.random_zeta, back.random_per_mode, back.random_background, back.random_static, back.random_interp,
            back.random_base) == (0.0, 32, 257, True, "linear", None)
    fd = back.to_struct()
    assert (fd.has_spectrum, fd.spectrum_count, fd.spectrum_rule, fd.spectrum_static, fd.spectrum_has_base) == (1, 3, 0, 1, 0)
    assert (fd.has_random, fd.random_count, fd.random_per_mode, fd.random_background, fd.random_has_base) == (1, 3, 32, 257, 0)
    # each alone, beside a transient and a harmonic section
    for kw in (SPECTRUM, RANDOM):
        _deck(**BASE, harmonic_count=3, harmonic_from=1.0, harmonic_to=2.0, transient_steps=3, transient_dt=0.5, **kw).save(str(p))
        back = feahip.Deck.load(str(p))
        assert bool(len(back.spectrum_points)) == (kw is SPECTRUM) and bool(len(back.random_points)) == (kw is RANDOM)
        assert back.harmonic_count == 3 and back.transient_steps == 3
        assert ("(spectrum" in p.read_text()) == (kw is SPECTRUM) and ("(random" in p.read_text()) == (kw is RANDOM)


def test_a_deck_without_the_sections_saves_as_before(tmp_path):
    """Byte for byte the golden file written before the sections existed, and none of their fields set on the way."""
    want = open(os.path.join(ROOT, "tests", "golden", "decks", "undamped_dynamics.sexp"), "rb").read()
    assert b"spectrum" not in want and b"random" not in want
    kw = dict(density=1.5, body_force=[0.0, 0.0, -2.0], dynamics=dict(steps=3, dt=0.0625, dlambda=1.0))
    for extra in ({}, dict(spectrum_points=[], random_points=None)):
        p = tmp_path / "plain.sexp"
        _deck(**kw, **extra).save(str(p))
        assert p.read_bytes() == want
        back = feahip.Deck.load(str(p))
        fd = back.to_struct()
        assert not len(back.spectrum_points) and not len(back.random_points) and not fd.has_spectrum and not fd.has_random
        back.save(str(p))
        assert p.read_bytes() == want
    p = tmp_path / "modal.sexp"
    _deck(**BASE, harmonic_count=3, harmonic_to=1.0, transient_steps=3, transient_dt=0.5).save(str(p))
    assert "spectrum" not in p.read_text() and "random" not in p.read_text()


def test_deck_load_errors(tmp_path):
    p = tmp_path / "bad.sexp"
    _deck(**BASE, spectrum_points=[(1.0, 2.0), (3.0, 4.0)], spectrum_rule="cqc", spectrum_zeta=0.02, spectrum_zpa=0.5,
          spectrum_base=(1.0, 0.0, 0.0), random_points=[(1.0, 2.0), (3.0, 4.0)], random_zeta=0.02, random_base=(1.0, 0.0, 0.0)).save(str(p))
    text = p.read_text()
    feahip.Deck.load(str(p))
    for old, new in ((":rule cqc", ":rule max"), (":rule cqc", ":rule abs"), (":zpa 0.5", ":zpa -1"), (":zpa 0.5", ":zpa inf"),
                     (":static-correction t :zpa", ":static-correction nil :zpa"), (":static-correction t :zpa", ":static-correction maybe :zpa"),
                     (":interp linear :base", ":interp cubic :base"), (":interp linear :per-mode", ":interp cubic :per-mode"),
                     (":static-correction t :interp", ":static-correction maybe :interp"),
                     ("(spectrum :rule cqc :zeta 0.02", "(spectrum :rule cqc :zeta -0.02"), ("(random :zeta 0.02", "(random :zeta inf"),
                     (":per-mode 32", ":per-mode -1"), (":per-mode 32", ":per-mode 2.5"), (":per-mode 32", ":per-mode 4097"),
                     (":background 257", ":background 1"), (":background 257", ":background 131073"),
                     (":base (1 0 0)\n    (points", ":base (0 0 0)\n    (points"), (":base (1 0 0)\n    (psd", ":base (1 0)\n    (psd"),
                     (":base (1 0 0)\n    (points", ":base (1 x 0)\n    (points"), (":base (1 0 0)\n    (psd", ":base (1 inf 0)\n    (psd"),
                     ("(points (1 2) (3 4))", "(points (3 2) (1 4))"), ("(points (1 2) (3 4))", "(points (1 2) (1 4))"),
                     ("(points (1 2) (3 4))", "(points (1 -2) (3 4))"), ("(points (1 2) (3 4))", "(points (1 2 3) (3 4))"),
                     ("(points (1 2) (3 4))", "(points (1) (3 4))"), ("(points (1 2) (3 4))", "(points (1 nan) (3 4))"),
                     ("(points (1 2) (3 4))", "(points 1 2)"), ("\n    (points (1 2) (3 4))", ""),
                     ("(psd (1 2) (3 4))", "(psd (1 2))"), ("(psd (1 2) (3 4))", "(psd (-1 2) (3 4))"), ("\n    (psd (1 2) (3 4))", "")):
        bad = text.replace(old, new)
        assert bad != text, old
        p.write_text(bad)
        with pytest.raises(feahip.FeaHipError):
            feahip.Deck.load(str(p))
    many = " ".join(f"({k} 1)" for k in range(feahip.DECK_MAX_POINTS + 1))
    p.write_text(text.replace("(psd (1 2) (3 4))", f"(psd {many})"))
    with pytest.raises(feahip.FeaHipError, match="more than 4096"):
        feahip.Deck.load(str(p))
    p.write_text(text.replace("(psd (1 2) (3 4))", "(psd " + " ".join(f"({k} 1)" for k in range(feahip.DECK_MAX_POINTS)) + ")"))
    assert len(feahip.Deck.load(str(p)).random_points) == feahip.DECK_MAX_POINTS
    # they need the locked store, and the correction excludes a shift
    p.write_text(text.replace(":count 12", ":modes 4"))
    with pytest.raises(feahip.FeaHipError, match="no locked modes"):
        feahip.Deck.load(str(p))
    p.write_text(text.replace(":max 1000", ":max 1000 :shift 3"))
    with pytest.raises(feahip.FeaHipError, match="exclude each other"):
        feahip.Deck.load(str(p))
    p.write_text(text.replace(":max 1000", ":max 1000 :shift 3").replace(":static-correction t", ":static-correction nil").replace(":zpa 0.5", ":zpa 0"))
    back = feahip.Deck.load(str(p))
    assert len(back.spectrum_points) == 2 and len(back.random_points) == 2 and back.modal_shift == 3.0
    # the same refusals of feahip.Deck
    pts = [(1.0, 2.0), (3.0, 4.0)]
    for kw in (dict(spectrum_points=[(3.0, 2.0), (1.0, 4.0)]), dict(spectrum_points=[(1.0, -2.0)]), dict(spectrum_points=[(np.nan, 2.0)]),
               dict(spectrum_points=pts, spectrum_rule="max"), dict(spectrum_points=pts, spectrum_zeta=-0.1),
               dict(spectrum_points=pts, spectrum_zpa=-1.0), dict(spectrum_points=pts, spectrum_zpa=0.5, spectrum_static=False),
               dict(spectrum_points=pts, spectrum_zpa=0.5, spectrum_rule="abs"), dict(spectrum_points=pts, spectrum_interp="cubic"),
               dict(spectrum_points=pts, spectrum_base=(0.0, 0.0, 0.0)), dict(random_points=[(1.0, 2.0)]),
               dict(random_points=[(1.0, 2.0), (1.0, 3.0)]), dict(random_points=pts, random_zeta=np.inf),
               dict(random_points=pts, random_per_mode=-1), dict(random_points=pts, random_background=1),
               dict(random_points=pts, random_base=(1.0, np.nan, 0.0)), dict(random_points=pts, random_interp="cubic")):
        with pytest.raises(ValueError, match="spectrum|random"):
            _deck(**BASE, **kw)
    with pytest.raises(ValueError, match="needs the locked modes"):
        _deck(density=1.5, modal_modes=4, spectrum_points=pts)
    with pytest.raises(ValueError, match="exclude each other"):
        _deck(**BASE, modal_shift=3.0, random_points=pts)
    _deck(**BASE, modal_shift=3.0, random_points=pts, random_static=False)


def test_struct_fields():
    hdr = open(os.path.join(ROOT, "fea-large_amd", "host", "fea_host.h")).read()
    fields = [n for n, _ in feahip.FeaDeck._fields_]
    at = fields.index("transient_steps")
    assert fields[at - len(FIELDS):at] == FIELDS                        # immediately in front of transient_steps
    types = dict(feahip.FeaDeck._fields_)
    assert [types[n] for n in FIELDS] == [C.c_int, C.c_int, _dp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double,
                                          C.c_double * 3, C.c_int, C.c_int, _dp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                          C.c_double, C.c_double * 3]
    m = re.search(r"#define\s+FEA_DECK_MAX_POINTS\s+(\d+)\b", hdr)
    assert m and int(m.group(1)) == feahip.DECK_MAX_POINTS
    host = feahip.load_host_library()
    assert hasattr(host, "fea_spectrum_run") and hasattr(host, "fea_random_run")
    # what stays out is said where the rest of it is
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "zero-crossing rates" in design

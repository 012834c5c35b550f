"""Random-vibration fatigue on the host side: feahip_host_moment_form against feahip_host_random_form (to the bit at the even
orders) and against the long-double restatement of tests/fatigue_reference.py at order 1, feahip_host_fatigue against the
restatement on the three PSD shapes and at the corners, every refusal, the three deck keys through reader and writer, the
struct fields and the exported symbols.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fatigue_reference as fr
import feahip
from test_combine_host import BASE, PSD_S, PSD_W, RANDOM, _deck, _modes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = fr.LD
NEW = ("feahip_host_moment_form", "feahip_host_fatigue", "feahip_response_stress_moments", "feahip_response_stress_fatigue")


def relative_tolerance(plain, exact):
    """100 times the largest relative gap between the restatement in float64 and in long double, at least 1e-13 and at
    most 1e-10."""
    exact = np.asarray(exact, dtype=LD)
    scale = np.where(exact != 0, np.abs(exact), 1)
    gap = float((np.abs(np.asarray(plain, dtype=LD) - exact) / scale).max()) if exact.size else 0.0
    return min(max(100.0 * gap, 1e-13), 1e-10), gap


def within(name, got, exact, plain):
    """Every entry of got within relative_tolerance of the long-double value, relative to that value."""
    tol, gap = relative_tolerance(plain, exact)
    exact = np.asarray(exact, dtype=LD)
    err = np.abs(np.asarray(got, dtype=LD) - exact)
    worst = float((err / np.where(exact != 0, np.abs(exact), 1)).max()) if exact.size else 0.0
    print(f"{name}: relative error {worst:.3e}, float64 gap {gap:.3e}, tolerance {tol:.3e}")
    assert np.all(err <= tol * np.abs(exact))


@pytest.mark.parametrize("n_modes", [1, 9, 64])
@pytest.mark.parametrize("correction", [False, True])
def test_moment_form_by_order(n_modes, correction):
    """9000 frequencies are more than two chunks of 4096.  The even orders to the bit of host_random_form; order 1 against
    the long-double restatement, relative to the largest entry of each of C, b, s (a form has entries that cancel to
    nothing: the rule of tests/test_combine_host.py, with the tolerance clamped as DESIGN.md section 5 does)."""
    lam, q = _modes(n_modes)
    zeta = np.full(n_modes, 0.02)
    alpha, beta = 0.01, 1e-5
    omega = np.linspace(0.0, 40.0, 9000)
    S = feahip.host_psd_value(PSD_W, PSD_S, omega, loglog=True)
    for order, quantity in ((0, 0), (2, 1), (4, 2)):
        got = feahip.host_moment_form(lam, q, omega, S, alpha, beta, zeta, correction, order)
        want = feahip.host_random_form(lam, q, omega, S, alpha, beta, zeta, correction, quantity)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]
    got = feahip.host_moment_form(lam, q, omega, S, alpha, beta, zeta, correction, 1)
    exact = fr.moment_form(lam, q, omega, S, alpha, beta, zeta, correction, 1, LD)
    plain = fr.moment_form(lam, q, omega, S, alpha, beta, zeta, correction, 1, np.float64)
    assert np.array_equal(got[0], got[0].T) and (correction or (not got[1].any() and got[2] == 0.0))
    for name, g, e, p in zip("Cbs", got, exact, plain):
        e, p = np.asarray(e, dtype=LD), np.asarray(p, dtype=LD)
        top = float(np.abs(e).max())
        if top == 0.0:
            assert not np.any(g)
            continue
        gap = float(np.abs(p - e).max()) / top
        tol = min(max(100.0 * gap, 1e-13), 1e-10)
        err = float(np.abs(np.asarray(g, dtype=LD) - e).max()) / top
        print(f"order 1 {name}: error {err:.3e}, float64 gap {gap:.3e}, tolerance {tol:.3e}")
        assert err <= tol
    # the first moment lies between its neighbours: m1^2 <= m0 m2 on every diagonal entry (Cauchy-Schwarz on the weights)
    m0, m2 = (np.diag(feahip.host_moment_form(lam, q, omega, S, alpha, beta, zeta, correction, o)[0]) for o in (0, 2))
    assert np.all(np.diag(got[0]) ** 2 <= m0 * m2 * (1 + 1e-12))


def test_moment_form_refusals():
    lam, q = _modes(3)
    omega, S = np.array([0.5, 1.0, 1.5]), np.ones(3)
    assert feahip.host_moment_form(lam, q, omega, S, 0.1, order=1)[0].shape == (3, 3)
    for order in (3, -1, 5, 6, 8):
        with pytest.raises(feahip.FeaHipError):
            feahip.host_moment_form(lam, q, omega, S, 0.1, order=order)
    # what host_random_form refuses
    for kw in (dict(omega=[0.5, 0.5, 1.0]), dict(omega=[-0.5, 1.0, 1.5]), dict(S=[1.0, -1.0, 1.0]), dict(S=[1.0, np.nan, 1.0]),
               dict(omega=[0.5, 1.0, np.inf]), dict(alpha=-1.0), dict(zeta=-0.1), dict(omega=[1.0], S=[1.0]),
               dict(alpha=0.0)):                                       # (undamped, and omega = 1 is the first mode's own)
        a = dict(lam=lam, q=q, omega=omega, S=S, alpha=0.1, beta=0.0, zeta=None)
        a.update(kw)
        for fn, extra in ((feahip.host_moment_form, dict(order=1)), (feahip.host_random_form, dict(quantity=0))):
            with pytest.raises(feahip.FeaHipError):
                fn(**a, **extra)
    lib = feahip.load_library()
    assert lib.feahip_host_moment_form(3, None, None, 3, None, None, 0.0, 0.0, None, 1, 1, None, None, None) == feahip.EINVAL


def _corner_moments():
    w1 = 37.0
    return np.array([[0.0, 0.0, 0.0, 0.0],                                # nothing
                     [2.5, 1.0, 0.0, 0.0],                                # m2 = 0
                     [0.0, 0.0, 3.0, 4.0],                                # m0 = 0
                     [2.5, 2.5 * w1, 2.5 * w1 ** 2, 2.5 * w1 ** 4]])       # one live frequency: m_n = w^n m0


@pytest.mark.parametrize("b,A", [(3.0, 1e3), (5.5, 2.5e7), (1.0, 1.0), (64.0, 1e40)])
def test_host_fatigue_against_the_restatement(b, A):
    shapes = fr.shapes()
    m = np.array([fr.moments_of_psd(*shapes[k]) for k in sorted(shapes)])
    # the same shapes at a stress scale of 1e3 and 1e-3 (m_n scale with the square), and with the frequency axis stretched
    m = np.concatenate([m, 1e6 * m, 1e-6 * m, m * np.array([1.0, 7.0, 49.0, 2401.0])])
    rates, damage, status = feahip.host_fatigue(m, b, A)
    er, ed, es, near = fr.fatigue(m, b, A, LD)
    pr, pd, ps, _ = fr.fatigue(m, b, A, np.float64)
    assert not near.any() and np.array_equal(status, es) and np.array_equal(ps, es) and not status.any()
    for k, name in enumerate(("nu0", "nup")):
        within(f"b {b} {name}", rates[:, k], er[:, k], pr[:, k])
    for k, name in enumerate(feahip.FATIGUE_DAMAGE):
        within(f"b {b} {name}", damage[:, k], ed[:, k], pd[:, k])
    assert np.all(damage[:, 2] <= damage[:, 0]) and np.all(damage > 0)
    # the corners
    c = _corner_moments()
    rates, damage, status = feahip.host_fatigue(c, b, A)
    er, ed, es, _ = fr.fatigue(c, b, A, LD)
    assert list(status) == [feahip.FATIGUE_NO_STRESS] * 3 + [feahip.FATIGUE_NARROW] and np.array_equal(status, es)
    assert not rates[:3].any() and not damage[:3].any() and np.all(np.isfinite(rates)) and np.all(np.isfinite(damage))
    assert damage[3, 0] == damage[3, 1] == damage[3, 2] > 0
    assert abs(rates[3, 0] - 37.0 / (2 * np.pi)) <= 1e-15 * 37.0 and rates[3, 0] == rates[3, 1]
    within(f"b {b} one frequency", damage[3], ed[3], fr.fatigue(c, b, A, np.float64)[1][3])


def test_host_fatigue_where_dirlik_is_no_density():
    """Moments no PSD gives (m1 far too small for m0 and m2): xm < g^2 makes D1 and D3 negative.  D_DK takes D_TB and bit
    2 is set; nothing is NaN."""
    m = np.array([[1.0, 0.1, 1.0, 2.0], [1.0, 0.05, 4.0, 40.0]])
    for b, A in ((3.0, 1e3), (5.5, 2.5e7)):
        rates, damage, status = feahip.host_fatigue(m, b, A)
        er, ed, es, near = fr.fatigue(m, b, A, LD)
        pd = fr.fatigue(m, b, A, np.float64)[1]
        D1, D2, D3, R, Q, _, _ = fr.dirlik_parameters(m)
        print("D1", D1, "D2", D2, "D3", D3, "Q", Q, "status", status)
        assert np.all(D1 < 0) and not near.any()
        assert np.all(status == feahip.FATIGUE_NO_DIRLIK) and np.array_equal(status, es)
        assert np.all(np.isfinite(damage)) and np.array_equal(damage[:, 1], damage[:, 2]) and np.all(rates > 0)
        for k, name in enumerate(feahip.FATIGUE_DAMAGE):
            within(f"b {b} {name}", damage[:, k], ed[:, k], pd[:, k])


def test_host_fatigue_shapes_and_refusals():
    m = np.ones((2, 3, 4)) * np.array([1.0, 1.5, 4.0, 40.0])
    rates, damage, status = feahip.host_fatigue(m, 3.0, 1e3)
    assert rates.shape == (2, 3, 2) and damage.shape == (2, 3, 3) and status.shape == (2, 3) and status.dtype == np.int32
    assert np.all(rates == rates[0, 0]) and np.all(damage == damage[0, 0])
    for b, A in ((0.999, 1.0), (64.001, 1.0), (np.nan, 1.0), (np.inf, 1.0), (3.0, 0.0), (3.0, -1.0), (3.0, np.inf), (3.0, np.nan)):
        with pytest.raises(feahip.FeaHipError):
            feahip.host_fatigue(m, b, A)
    for bad in (-1.0, np.nan, np.inf):
        mm = m.copy()
        mm[1, 2, 3] = bad
        with pytest.raises(feahip.FeaHipError):
            feahip.host_fatigue(mm, 3.0, 1e3)
    # any output may be left out
    lib = feahip.load_library()
    flat = np.ascontiguousarray(m.reshape(-1, 4))
    assert lib.feahip_host_fatigue(len(flat), flat.ctypes.data_as(C.POINTER(C.c_double)), 3.0, 1e3, None, None, None) == 0
    assert lib.feahip_host_fatigue(0, None, 3.0, 1e3, None, None, None) == 0
    assert lib.feahip_host_fatigue(1, None, 3.0, 1e3, None, None, None) == feahip.EINVAL


FATIGUE = dict(random_sn_exponent=5.5, random_sn_coefficient=1.0 / 3.0 * 1e12, random_duration=3600.0)


def test_deck_keys_round_trip(tmp_path):
    d = _deck(**BASE, **RANDOM, **FATIGUE)
    p = tmp_path / "fatigue.sexp"
    d.save(str(p))
    text = p.read_text()
    assert re.search(r"\(random :zeta \S+ :static-correction nil :interp linear :per-mode 16 :background 65 :sn-exponent 5.5 "
                     r":sn-coefficient \S+ :duration 3600\n    \(psd", text)
    back = feahip.Deck.load(str(p))
    assert (back.random_sn_exponent, back.random_sn_coefficient, back.random_duration) == (5.5, FATIGUE["random_sn_coefficient"], 3600.0)
    fd = back.to_struct()
    assert (fd.random_sn_exponent, fd.random_sn_coefficient, fd.random_duration) == (5.5, FATIGUE["random_sn_coefficient"], 3600.0)
    q = tmp_path / "again.sexp"
    back.save(str(q))
    assert q.read_bytes() == p.read_bytes()
    # beside :stress t, and the default of :duration
    _deck(**BASE, **RANDOM, random_stress=True, random_sn_exponent=3.0, random_sn_coefficient=2.0).save(str(p))
    assert ":stress t :sn-exponent 3 :sn-coefficient 2 :duration 1\n" in p.read_text()
    p.write_text(p.read_text().replace(" :duration 1\n", "\n"))
    back = feahip.Deck.load(str(p))
    assert back.random_stress and (back.random_sn_exponent, back.random_sn_coefficient, back.random_duration) == (3.0, 2.0, 1.0)
    # without the keys: written as before, and none of the fields set
    _deck(**BASE, **RANDOM).save(str(p))
    plain = p.read_bytes()
    assert b"sn-" not in plain and b"duration" not in plain
    back = feahip.Deck.load(str(p))
    fd = back.to_struct()
    assert (back.random_sn_exponent, back.random_duration) == (0.0, 1.0) and fd.random_sn_exponent == 0.0
    back.save(str(q))
    assert q.read_bytes() == plain
    assert q.read_text() == text.replace(" :sn-exponent 5.5 :sn-coefficient %.17g :duration 3600" % FATIGUE["random_sn_coefficient"], "")
    want = open(os.path.join(ROOT, "tests", "golden", "decks", "undamped_dynamics.sexp"), "rb").read()
    _deck(density=1.5, body_force=[0.0, 0.0, -2.0], dynamics=dict(steps=3, dt=0.0625, dlambda=1.0)).save(str(p))
    assert p.read_bytes() == want


def test_deck_key_errors(tmp_path):
    p = tmp_path / "bad.sexp"
    _deck(**BASE, **RANDOM, random_sn_exponent=3.0, random_sn_coefficient=2.0, random_duration=10.0).save(str(p))
    text = p.read_text()
    feahip.Deck.load(str(p))
    for old, new in ((":sn-exponent 3", ":sn-exponent 0.5"), (":sn-exponent 3", ":sn-exponent 65"), (":sn-exponent 3", ":sn-exponent nan"),
                     (":sn-exponent 3", ":sn-exponent x"), (":sn-coefficient 2", ":sn-coefficient 0"), (":sn-coefficient 2", ":sn-coefficient -2"),
                     (":sn-coefficient 2", ":sn-coefficient inf"), (" :sn-coefficient 2", ""), (":duration 10", ":duration 0"),
                     (":duration 10", ":duration -1"), (":duration 10", ":duration inf"), (":sn-exponent 3 ", ""),
                     (":sn-exponent 3 :sn-coefficient 2 ", "")):
        bad = text.replace(old, new)
        assert bad != text, old
        p.write_text(bad)
        with pytest.raises(feahip.FeaHipError):
            feahip.Deck.load(str(p))
    pts = RANDOM["random_points"]
    for kw in (dict(random_points=pts, random_sn_exponent=0.5, random_sn_coefficient=1.0),
               dict(random_points=pts, random_sn_exponent=65.0, random_sn_coefficient=1.0),
               dict(random_points=pts, random_sn_exponent=3.0), dict(random_points=pts, random_sn_exponent=3.0, random_sn_coefficient=-1.0),
               dict(random_points=pts, random_sn_exponent=3.0, random_sn_coefficient=1.0, random_duration=0.0),
               dict(random_points=pts, random_sn_coefficient=1.0), dict(random_points=pts, random_duration=5.0),
               dict(random_sn_exponent=3.0, random_sn_coefficient=1.0)):
        with pytest.raises(ValueError, match="random"):
            _deck(**BASE, **kw)


def test_struct_fields_and_symbols():
    fields = [n for n, _ in feahip.FeaDeck._fields_]
    new = ["random_sn_exponent", "random_sn_coefficient", "random_duration"]
    at = fields.index("harmonic_stress")
    assert fields[at - 3:at] == new and all(dict(feahip.FeaDeck._fields_)[n] is C.c_double for n in new)
    hdr = open(os.path.join(ROOT, "fea-large_amd", "host", "fea_host.h")).read()
    assert re.search(r"double random_sn_exponent, random_sn_coefficient, random_duration;\s*/\*[^;]*?\*/\s*int harmonic_stress, transient_stress;", hdr, re.S)
    lib = feahip.load_library()
    for name in NEW:
        assert name in feahip.ABI and hasattr(lib, name)
    for name in ("host_moment_form", "host_fatigue"):
        assert callable(getattr(feahip, name))
    for name in ("response_stress_moments", "response_stress_fatigue"):
        assert callable(getattr(feahip.FeaSolver, name))
    src = open(os.path.join(ROOT, "fea-large_amd", "csrc", "Makefile")).read()
    assert "kernels_stress_fatigue.o" in src and "fatigue_table.o" in src

"""Transient response on the host side: feahip_host_transient_coefficients against the long-double restatement of
tests/transient_reference.py and against closed forms at the step points, its refusals, the deck grammar of
(transient ...), the struct fields and the exported symbols.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import feahip
import mesh
import transient_reference as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps
NEW = ("feahip_response_base_load", "feahip_response_transient", "feahip_host_transient_coefficients")
FIELDS = ["transient_steps", "transient_dt", "transient_zeta", "transient_static", "transient_shape", "transient_rise",
          "transient_has_base", "transient_base"]
_dp = C.POINTER(C.c_double)


def _history(n_steps, seed):
    """A pulse, a ramp and noise: nothing in it is smooth on the grid."""
    t = np.arange(n_steps + 1, dtype=np.float64)
    rng = np.random.default_rng(seed)
    return np.sin(0.37 * t) + np.minimum(t / 7.0, 1.0) + 0.1 * rng.standard_normal(n_steps + 1)


def _against_the_restatement(lam, q, g, dt, alpha, beta, zeta, correction):
    """The library's table within 100 times the gap between the restatement in float64 and in long double, with a floor of
    64 eps times the largest entry (the rule of tests/test_gpu_pcg.py), for the three quantities.  Returns the largest
    error / tolerance."""
    n = len(lam)
    exact = tr.modal_states(lam, q, g, dt, alpha, beta, zeta, tr.LD)
    plain = tr.modal_states(lam, q, g, dt, alpha, beta, zeta, np.float64)
    worst = 0.0
    for quantity in (0, 1, 2):
        got = feahip.host_transient_coefficients(lam, q, g, dt, alpha, beta, zeta, correction, quantity)
        assert got.shape == (len(g), 64) and not got[:, n:].any()
        ref = tr.table(*exact, lam, q, g, correction, quantity)
        gap = float(np.abs(tr.table(*plain, lam, q, g, correction, quantity).astype(tr.LD) - ref).max())
        tol = max(100.0 * gap, 64 * EPS * float(np.abs(ref).max()))
        err = float(np.abs(got[:, :n].astype(tr.LD) - ref).max())
        print(f"quantity {quantity}: error {err:.3e}, float64 gap {gap:.3e}, error / tolerance {err / tol:.3e}")
        assert err <= tol
        worst = max(worst, err / tol)
    return worst


DAMPING = {"undamped": 0.0, "under": 0.02, "critical": 1.0, "over": 3.0}


@pytest.mark.parametrize("n_modes", [1, 8, 9, 64])
@pytest.mark.parametrize("n_steps", [1, 2, 1000])
@pytest.mark.parametrize("damping", sorted(DAMPING))
@pytest.mark.parametrize("correction", [False, True])
def test_table_against_the_long_double_restatement(n_modes, n_steps, damping, correction):
    """omega dt spread from 1e-3 to 50 over the modes (a single mode sits at 50), modal damping ratio 0, 0.02, 1 or 3 on
    every mode: undamped, under-damped, critically damped and over-damped."""
    dt = 0.25
    wdt = np.array([50.0]) if n_modes == 1 else np.geomspace(1e-3, 50.0, n_modes)
    lam = (wdt / dt) ** 2
    q = np.random.default_rng(n_modes).standard_normal(n_modes)
    zeta = np.full(n_modes, DAMPING[damping])
    worst = _against_the_restatement(lam, q, _history(n_steps, n_steps), dt, 0.0, 0.0, zeta, correction)
    print(n_modes, n_steps, damping, correction, "largest error / tolerance", worst)


@pytest.mark.parametrize("alpha", [0.0, 0.7])
@pytest.mark.parametrize("n_steps", [1, 2, 1000])
def test_zero_and_nearly_zero_modes(alpha, n_steps):
    """lam = 0 and +-1e-12 (the rigid-body modes of a solve with a shift), with d = 0 and with d = alpha > 0, beside an
    elastic mode and Rayleigh and modal damping together; the correction is refused for them."""
    lam = np.array([0.0, 1e-12, -1e-12, 0.0, 4.0e2])
    q = np.array([1.0, -0.5, 2.0, 0.25, 1.5])
    zeta = np.array([0.0, 0.3, 0.3, 0.0, 0.05])
    worst = _against_the_restatement(lam, q, _history(n_steps, 5), 0.5, alpha, 1e-4 if alpha else 0.0, zeta, False)
    print(alpha, n_steps, "largest error / tolerance", worst)
    with pytest.raises(feahip.FeaHipError):
        feahip.host_transient_coefficients(lam, q, np.ones(3), 0.5, static_correction=True)


def test_closed_forms_at_the_step_points():
    """An undamped mode under a step, (q / lam)(1 - cos(w t)); under a ramp of length T, (q / lam)(t - sin(w t) / w) / T
    while t <= T; the rigid mode under a step, q t^2 / 2.  1e-11 of the largest value for n <= 1000 and w t <= 1e3, about
    fifty times n eps (1 + w t)."""
    n, dt = 1000, 0.01
    t = np.arange(n + 1) * dt
    for w in (1.0, 37.0, 100.0):                                        # w t up to 1e3
        lam, q = np.array([w * w]), np.array([1.7])
        got = feahip.host_transient_coefficients(lam, q, np.ones(n + 1), dt, static_correction=False)[:, 0]
        want = q[0] / lam[0] * (1.0 - np.cos(w * t))
        print("step, w =", w, "error / largest", np.abs(got - want).max() / np.abs(want).max())
        assert np.abs(got - want).max() <= 1e-11 * np.abs(want).max()
        T = t[-1]
        got = feahip.host_transient_coefficients(lam, q, t / T, dt, static_correction=False)[:, 0]
        want = q[0] / lam[0] * (t - np.sin(w * t) / w) / T
        print("ramp, w =", w, "error / largest", np.abs(got - want).max() / np.abs(want).max())
        assert np.abs(got - want).max() <= 1e-11 * np.abs(want).max()
        vel = feahip.host_transient_coefficients(lam, q, np.ones(n + 1), dt, static_correction=False, quantity=1)[:, 0]
        want = q[0] / w * np.sin(w * t)
        assert np.abs(vel - want).max() <= 1e-11 * np.abs(want).max()
    got = feahip.host_transient_coefficients([0.0], [1.7], np.ones(n + 1), dt, static_correction=False)[:, 0]
    want = 1.7 * t * t / 2
    assert np.abs(got - want).max() <= 1e-11 * want.max()
    acc = feahip.host_transient_coefficients([0.0], [1.7], np.ones(n + 1), dt, static_correction=False, quantity=2)[:, 0]
    assert np.array_equal(acc, np.full(n + 1, 1.7))
    # the mode-acceleration coefficient is the dynamic part alone: zero under a load that never moves the mode
    assert not feahip.host_transient_coefficients([4.0], [1.0], np.zeros(5), 0.1, static_correction=True).any()


def test_refusals():
    lam, q, g = np.array([4.0, 9.0]), np.ones(2), np.ones(4)
    ok = feahip.host_transient_coefficients(lam, q, g, 0.1)
    assert ok.shape == (4, 64) and np.isfinite(ok).all()
    bad_g = g.copy()
    bad_g[2] = np.nan
    for kw in (dict(dt=0.0), dict(dt=-1.0), dict(dt=np.inf), dict(dt=np.nan), dict(g=bad_g), dict(g=[1.0, np.inf]),
               dict(g=[1.0]), dict(quantity=-1), dict(quantity=3), dict(alpha=-0.1), dict(alpha=np.nan), dict(beta=-1e-3),
               dict(beta=np.inf), dict(zeta=[0.1, -0.1]), dict(zeta=[np.inf, 0.0]), dict(lam=[4.0, np.nan]),
               dict(q=[np.inf, 1.0]), dict(lam=[0.0, 4.0]), dict(lam=[-1.0, 4.0])):
        a = dict(lam=lam, q=q, g=g, dt=0.1, alpha=0.0, beta=0.0, zeta=None, static_correction=True, quantity=0)
        a.update(kw)
        with pytest.raises(feahip.FeaHipError):
            feahip.host_transient_coefficients(**a)
    feahip.host_transient_coefficients([0.0, 4.0], q, g, 0.1, static_correction=False)     # a zero mode without the correction
    with pytest.raises(feahip.FeaHipError):                                                  # a coefficient that is not finite
        feahip.host_transient_coefficients([-1e6], [1.0], np.ones(1001), 1.0, static_correction=False)
    lib = feahip.load_library()
    one = (C.c_double * 2)(4.0, 4.0)
    out = (C.c_double * (2 * 64))()
    args = (0.0, 0.0, None, 0, 0, out)
    assert lib.feahip_host_transient_coefficients(1, one, one, 1, 0.1, one, *args) == 0
    assert lib.feahip_host_transient_coefficients(0, one, one, 1, 0.1, one, *args) == feahip.EINVAL
    assert lib.feahip_host_transient_coefficients(65, one, one, 1, 0.1, one, *args) == feahip.EINVAL
    assert lib.feahip_host_transient_coefficients(1, one, one, 0, 0.1, one, *args) == feahip.EINVAL
    assert lib.feahip_host_transient_coefficients(1, one, one, feahip.TRANSIENT_MAX_STEPS + 1, 0.1, one, *args) == feahip.EINVAL
    assert lib.feahip_host_transient_coefficients(1, None, one, 1, 0.1, one, *args) == feahip.EINVAL
    assert lib.feahip_host_transient_coefficients(1, one, None, 1, 0.1, one, *args) == feahip.EINVAL
    assert lib.feahip_host_transient_coefficients(1, one, one, 1, 0.1, None, *args) == feahip.EINVAL
    assert lib.feahip_host_transient_coefficients(1, one, one, 1, 0.1, one, 0.0, 0.0, None, 0, 0, None) == feahip.EINVAL
    # the device entries refuse a null context before anything else
    assert lib.feahip_response_transient(None, 1, 0.1, one, 0.0, 0.0, None, 0, None, None, 0, None, None, 0, None, None) == feahip.EINVAL
    assert lib.feahip_response_base_load(None, one, 0, 0, 1e-12, 10, None, None, None, None, None, None) == feahip.EINVAL


def _deck(**kw):
    d = mesh.bar_deck(dims=(1, 2, 1))
    keys = ("model", "parameters", "ele_type", "gauss_nodes_count", "nodes", "elements", "presc_node", "presc_type", "presc_values")
    return feahip.Deck(**{k: getattr(d, k) for k in keys}, **kw)


BASE = dict(density=1.5, dynamics=dict(steps=0, dt=1.0), modal_count=12)


def test_deck_round_trip(tmp_path):
    dt, rise, z = 0.1 / 3.0, 1.0 / 7.0, 1.0 / 30.0                      # none has a short decimal form
    d = _deck(**BASE, damping=(0.25, 1e-4), transient_steps=257, transient_dt=dt, transient_shape="half-sine",
              transient_rise=rise, transient_zeta=z, transient_static=False, transient_base=(1.0, 0.0, -1.0 / 3.0))
    p = tmp_path / "transient.sexp"
    d.save(str(p))
    assert re.search(r"\(transient :steps 257 :dt \S+ :shape half-sine :rise \S+ :zeta \S+ :static-correction nil "
                     r":base \(1 0 \S+\)\)", p.read_text())
    back = feahip.Deck.load(str(p))
    assert (back.transient_steps, back.transient_dt, back.transient_shape, back.transient_rise, back.transient_zeta,
            back.transient_static, back.transient_base) == (257, dt, "half-sine", rise, z, False, (1.0, 0.0, -1.0 / 3.0))
    assert back.damping == (0.25, 1e-4) and back.modal_count == 12
    q = tmp_path / "again.sexp"
    back.save(str(q))
    assert q.read_bytes() == p.read_bytes()
    # the defaults: a step, zeta 0, the correction on, no base
    p.write_text(re.sub(r"\(transient [^\n]*\)\)\)", "(transient :steps 257 :dt 0.5))", p.read_text()))
    back = feahip.Deck.load(str(p))
    assert (back.transient_steps, back.transient_dt, back.transient_shape, back.transient_zeta, back.transient_static,
            back.transient_base) == (257, 0.5, "step", 0.0, True, None)
    fd = back.to_struct()
    assert (fd.transient_steps, fd.transient_dt, fd.transient_shape, fd.transient_static, fd.transient_has_base) == (257, 0.5, 0, 1, 0)
    # beside a harmonic section, with a shift and without the correction
    _deck(**BASE, modal_shift=50.0, harmonic_count=3, harmonic_from=1.0, harmonic_to=2.0, harmonic_static=False,
          transient_steps=3, transient_dt=0.5, transient_shape="ramp", transient_rise=1.0, transient_static=False).save(str(p))
    back = feahip.Deck.load(str(p))
    assert back.modal_shift == 50.0 and back.harmonic_count == 3 and back.transient_shape == "ramp"


def test_a_deck_without_the_section_saves_as_before(tmp_path):
    """Byte for byte the golden file written before the section existed, and no transient field set on the way."""
    want = open(os.path.join(ROOT, "tests", "golden", "decks", "undamped_dynamics.sexp"), "rb").read()
    assert b"transient" not in want
    kw = dict(density=1.5, body_force=[0.0, 0.0, -2.0], dynamics=dict(steps=3, dt=0.0625, dlambda=1.0))
    for extra in ({}, dict(transient_steps=0)):
        p = tmp_path / "plain.sexp"
        _deck(**kw, **extra).save(str(p))
        assert p.read_bytes() == want
        back = feahip.Deck.load(str(p))
        assert back.transient_steps == 0 and back.to_struct().transient_steps == 0
        back.save(str(p))
        assert p.read_bytes() == want
    p = tmp_path / "modal.sexp"
    _deck(**BASE, harmonic_count=3, harmonic_to=1.0).save(str(p))
    assert "transient" not in p.read_text()


def test_load_errors(tmp_path):
    p = tmp_path / "bad.sexp"
    _deck(**BASE, transient_steps=5, transient_dt=0.5, transient_shape="ramp", transient_rise=2.0, transient_zeta=0.02,
          transient_base=(1.0, 0.0, 0.0)).save(str(p))
    text = p.read_text()
    feahip.Deck.load(str(p))
    for old, new in ((":steps 5 ", ":steps 0 "), (":steps 5 ", ":steps 1048577 "), (":steps 5 ", ":steps 2.5 "),
                     (":dt 0.5 ", ":dt 0 "), (":dt 0.5 ", ":dt -1 "), (":dt 0.5 ", ":dt inf "),
                     (":dt 0.5 ", ""), (":zeta 0.02", ":zeta -0.02"), (":zeta 0.02", ":zeta inf"), (":rise 2 ", ":rise 0 "),
                     (":rise 2 ", ":rise -1 "), (":rise 2 ", ""), (":shape ramp", ":shape sawtooth"),
                     (":static-correction t", ":static-correction maybe"), (":base (1 0 0)", ":base (0 0 0)"),
                     (":base (1 0 0)", ":base (1 0)"), (":base (1 0 0)", ":base (1 0 0 0)"), (":base (1 0 0)", ":base (1 inf 0)"),
                     (":base (1 0 0)", ":base (1 x 0)")):
        bad = text.replace(old, new)
        assert bad != text, old
        p.write_text(bad)
        with pytest.raises(feahip.FeaHipError):
            feahip.Deck.load(str(p))
    # a step needs no :rise
    p.write_text(text.replace(":shape ramp :rise 2 ", ":shape step "))
    assert feahip.Deck.load(str(p)).transient_shape == "step"
    # it needs the locked store: (modal :count ...) or a :shift
    p.write_text(text.replace(":count 12", ":modes 4"))
    with pytest.raises(feahip.FeaHipError, match="no locked modes"):
        feahip.Deck.load(str(p))
    p.write_text(re.sub(r"\n   \(modal [^)]*\)", "", text))
    with pytest.raises(feahip.FeaHipError, match="no locked modes"):
        feahip.Deck.load(str(p))
    p.write_text(text.replace(":count 12", ":modes 4").replace(":max 1000", ":max 1000 :shift 3").replace(":static-correction t", ":static-correction nil"))
    assert feahip.Deck.load(str(p)).transient_steps == 5
    # the correction and a shift exclude each other
    p.write_text(text.replace(":max 1000", ":max 1000 :shift 3"))
    with pytest.raises(feahip.FeaHipError, match="exclude each other"):
        feahip.Deck.load(str(p))
    # the same refusals of feahip.Deck
    for kw in (dict(transient_steps=1048577), dict(transient_steps=-1), dict(transient_steps=3, transient_dt=0.0),
               dict(transient_steps=3, transient_dt=np.inf), dict(transient_steps=3, transient_dt=1.0, transient_zeta=-0.1),
               dict(transient_steps=3, transient_dt=1.0, transient_shape="sawtooth"),
               dict(transient_steps=3, transient_dt=1.0, transient_shape="ramp"),
               dict(transient_steps=3, transient_dt=1.0, transient_shape="half-sine", transient_rise=-1.0),
               dict(transient_steps=3, transient_dt=1.0, transient_base=(0.0, 0.0, 0.0)),
               dict(transient_steps=3, transient_dt=1.0, transient_base=(1.0, np.nan, 0.0))):
        with pytest.raises(ValueError, match="transient"):
            _deck(**BASE, **kw)
    with pytest.raises(ValueError, match="needs the locked modes"):
        _deck(density=1.5, modal_modes=4, transient_steps=3, transient_dt=1.0)
    with pytest.raises(ValueError, match="exclude each other"):
        _deck(**BASE, modal_shift=3.0, transient_steps=3, transient_dt=1.0)
    _deck(**BASE, modal_shift=3.0, transient_steps=3, transient_dt=1.0, transient_static=False)


def test_struct_fields_and_symbols():
    hdr = open(os.path.join(ROOT, "fea-large_amd", "host", "fea_host.h")).read()
    body = re.sub(r"/\*.*?\*/", "", hdr[hdr.index("typedef struct fea_deck {"):hdr.index("} fea_deck;")], flags=re.S)
    names = []
    for stmt in body.split(";"):
        stmt = stmt.replace("typedef struct fea_deck {", "").strip()
        if stmt:
            names += [re.sub(r"\[.*\]", "", n).strip(" *") for n in re.sub(r"^\s*(int|double)\s", "", stmt).split(",")]
    fields = [n for n, _ in feahip.FeaDeck._fields_]
    assert names == fields
    at = fields.index("harmonic_count")
    assert fields[at - len(FIELDS):at] == FIELDS                        # immediately in front of harmonic_count
    types = dict(feahip.FeaDeck._fields_)
    assert [types[n] for n in FIELDS] == [C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, C.c_double, C.c_int, C.c_double * 3]
    lib = feahip.load_library()
    top = open(os.path.join(ROOT, "include", "fea_hip.h")).read()
    out = os.popen(f"nm -D --defined-only {feahip.LIB_PATH}").read()
    for name in NEW:
        assert name in feahip.ABI and hasattr(lib, name), name
        assert re.search(r"\bint\s+%s\(" % name, top) and re.search(rf"\bT {name}\b", out), name
    assert re.search(r"#define\s+FEA_TRANSIENT_MAX_STEPS\s+1048576\b", top) and feahip.TRANSIENT_MAX_STEPS == 1048576
    chunk = re.search(r"#define\s+FEA_TRANSIENT_CHUNK\s+(\d+)\b", top)
    assert chunk and int(chunk.group(1)) == feahip.TRANSIENT_CHUNK
    assert feahip.TRANSIENT_CHUNK * 65 <= feahip.RESPONSE_MAX_FREQ * 2 * 64     # a chunk and its g fit the sweep's table
    assert hasattr(feahip.load_host_library(), "fea_transient_run")
    for name in ("response_base_load", "response_transient"):
        assert callable(getattr(feahip.FeaSolver, name))
        assert not hasattr(feahip.FeaGroup, name)                      # the locked solve is unsharded, and so is this
    assert callable(feahip.host_transient_coefficients)
    # the lists of what is not offered no longer name the two
    readme = open(os.path.join(ROOT, "README.md")).read()
    for text in (top, readme):
        assert "transient modal superposition, base" not in re.sub(r"\s+\*?\s*", " ", text)

"""Frequency response on the host side: feahip_host_response_coefficients against the formulas of
tests/response_reference.py, its refusals, the deck grammar of (harmonic ...), the struct fields and the exported
symbols.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import feahip
import mesh
from response_reference import coefficients_exact

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps
NEW = ("feahip_response_set_basis", "feahip_response_load", "feahip_get_response_static", "feahip_response_sweep",
       "feahip_response_field", "feahip_host_response_coefficients")
DAMPING = {"alpha": dict(alpha=0.7), "beta": dict(beta=3e-4), "zeta": dict(zeta=0.02),
           "all": dict(alpha=0.7, beta=3e-4, zeta=0.02)}


def _pairs(n, seed=3):
    """n eigenvalues spread over four decades, participations of both signs."""
    rng = np.random.default_rng(seed)
    lam = np.sort(10.0 ** rng.uniform(2.0, 6.0, n))
    return lam, rng.standard_normal(n)


def _omegas(lam):
    w1 = np.sqrt(lam[0])
    between = np.sqrt(0.5 * (lam[min(3, len(lam) - 1)] + lam[min(4, len(lam) - 1)]) * 1.01)
    return np.array([0.0, 1e-3 * w1, 0.5 * w1, 0.98 * w1, w1, between, 10.9 * w1])


@pytest.mark.parametrize("n", [1, 20, 64])
@pytest.mark.parametrize("damping", sorted(DAMPING))
@pytest.mark.parametrize("correction", [False, True])
def test_coefficients_match_the_formulas(n, damping, correction):
    """|a - ref| <= 4 eps |ref| per complex entry, ref the formulas as the header writes them evaluated in 60-digit
    decimal arithmetic and rounded once (the float64 evaluation of H - 1 / lam as written is itself wrong by
    eps |H| / |H - 1 / lam|, millions of eps at w = 1e-3 w1); the columns past n are zero."""
    lam, q = _pairs(n)
    om = _omegas(lam)
    kw = dict(DAMPING[damping])
    zeta = None if "zeta" not in kw else np.full(n, kw.pop("zeta")) * np.linspace(1.0, 2.0, n)
    got = feahip.host_response_coefficients(lam, q, om, zeta=zeta, static_correction=correction, **kw)
    assert got.shape == (len(om), 64) and not got[:, n:].any()
    ref = coefficients_exact(lam, q, om, zeta=zeta, correction=correction, **kw)
    scale = np.abs(ref)
    err = np.abs(got[:, :n] - ref)
    own = 1e-50 * np.abs(q / lam)                                      # the yardstick's own rounding: 60 digits of 1 / lam
    big = scale > 1e6 * own
    print("largest error / (eps |ref|):", (err[big] / (EPS * scale[big])).max())
    assert np.all(err <= 4 * EPS * scale + own)
    if correction:
        assert not got[0].any()                                        # w = 0: H = 1 / lam exactly


def test_refusals():
    lam, q = np.array([0.0, 4.0, 9.0]), np.ones(3)
    ok = feahip.host_response_coefficients(lam, q, [1.0, 5.0], static_correction=False)      # a zero mode sweeps at w > 0
    assert np.isfinite(ok).all() and ok[0, 0] == -1.0
    with pytest.raises(feahip.FeaHipError):                                                  # w = 0 on a zero mode
        feahip.host_response_coefficients(lam, q, [0.0], static_correction=False)
    with pytest.raises(feahip.FeaHipError):                                                  # the correction on a zero mode
        feahip.host_response_coefficients(lam, q, [1.0], static_correction=True)
    with pytest.raises(feahip.FeaHipError):                                                  # undamped exact resonance
        feahip.host_response_coefficients(lam[1:], q[1:], [3.0], static_correction=False)
    assert np.isfinite(feahip.host_response_coefficients(lam[1:], q[1:], [3.0], alpha=0.1, static_correction=False)).all()
    for bad in (dict(omega=[-1.0]), dict(omega=[np.inf]), dict(alpha=-0.1), dict(beta=-1e-3), dict(beta=np.nan),
                dict(zeta=[0.1, -0.1]), dict(zeta=[np.inf, 0.0])):
        kw = dict(omega=[1.0], static_correction=True)
        kw.update(bad)
        with pytest.raises(feahip.FeaHipError):
            feahip.host_response_coefficients(lam[1:], q[1:], kw.pop("omega"), **kw)
    lib = feahip.load_library()
    one = (C.c_double * 1)(4.0)
    out = (C.c_double * (2 * 64 * 2))()
    assert lib.feahip_host_response_coefficients(0, one, one, 1, one, 0.0, 0.0, None, 0, out) == feahip.EINVAL
    assert lib.feahip_host_response_coefficients(65, one, one, 1, one, 0.0, 0.0, None, 0, out) == feahip.EINVAL
    assert lib.feahip_host_response_coefficients(1, one, one, 0, one, 0.0, 0.0, None, 0, out) == feahip.EINVAL
    assert lib.feahip_host_response_coefficients(1, one, one, 4097, one, 0.0, 0.0, None, 0, out) == feahip.EINVAL
    assert lib.feahip_host_response_coefficients(1, None, one, 1, one, 0.0, 0.0, None, 0, out) == feahip.EINVAL


def _deck(**kw):
    d = mesh.bar_deck(dims=(1, 2, 1))
    keys = ("model", "parameters", "ele_type", "gauss_nodes_count", "nodes", "elements", "presc_node", "presc_type", "presc_values")
    return feahip.Deck(**{k: getattr(d, k) for k in keys}, **kw)


BASE = dict(density=1.5, dynamics=dict(steps=0, dt=1.0), modal_count=12)


def test_deck_round_trip(tmp_path):
    f0, f1, z = 0.1 + 0.2, 1.0e3 / 3.0, 1.0 / 30.0                      # none has a short decimal form
    d = _deck(**BASE, damping=(0.25, 1e-4), harmonic_count=257, harmonic_from=f0, harmonic_to=f1, harmonic_zeta=z,
              harmonic_static=False)
    p = tmp_path / "harmonic.sexp"
    d.save(str(p))
    assert re.search(r"\(harmonic :from \S+ :to \S+ :count 257 :zeta \S+ :static-correction nil\)", p.read_text())
    back = feahip.Deck.load(str(p))
    assert (back.harmonic_count, back.harmonic_from, back.harmonic_to, back.harmonic_zeta, back.harmonic_static) == (257, f0, f1, z, False)
    assert back.damping == (0.25, 1e-4) and back.modal_count == 12
    q = tmp_path / "again.sexp"
    back.save(str(q))
    assert q.read_bytes() == p.read_bytes()
    # the defaults: zeta 0, the correction on
    text = re.sub(r" :zeta \S+ :static-correction nil", "", p.read_text())
    p.write_text(text)
    back = feahip.Deck.load(str(p))
    assert back.harmonic_count == 257 and back.harmonic_zeta == 0.0 and back.harmonic_static is True
    fd = back.to_struct()
    assert (fd.harmonic_count, fd.harmonic_from, fd.harmonic_to, fd.harmonic_zeta, fd.harmonic_static) == (257, f0, f1, 0.0, 1)
    # with a shift and without the correction
    _deck(**BASE, modal_shift=50.0, harmonic_count=3, harmonic_from=1.0, harmonic_to=2.0, harmonic_static=False).save(str(p))
    assert feahip.Deck.load(str(p)).modal_shift == 50.0


def test_a_deck_without_the_section_saves_as_before(tmp_path):
    """Byte for byte the golden file written before the section existed, and no harmonic field set on the way."""
    want = open(os.path.join(ROOT, "tests", "golden", "decks", "undamped_dynamics.sexp"), "rb").read()
    assert b"harmonic" not in want
    kw = dict(density=1.5, body_force=[0.0, 0.0, -2.0], dynamics=dict(steps=3, dt=0.0625, dlambda=1.0))
    for extra in ({}, dict(harmonic_count=0)):
        p = tmp_path / "plain.sexp"
        _deck(**kw, **extra).save(str(p))
        assert p.read_bytes() == want
        back = feahip.Deck.load(str(p))
        assert back.harmonic_count == 0 and back.to_struct().harmonic_count == 0
        back.save(str(p))
        assert p.read_bytes() == want
    p = tmp_path / "modal.sexp"
    _deck(**BASE).save(str(p))
    assert "harmonic" not in p.read_text()


def test_load_errors(tmp_path):
    p = tmp_path / "bad.sexp"
    _deck(**BASE, harmonic_count=5, harmonic_from=1.0, harmonic_to=9.0, harmonic_zeta=0.02).save(str(p))
    text = p.read_text()
    feahip.Deck.load(str(p))
    for old, new in ((":count 5 ", ":count 0 "), (":count 5 ", ":count 4097 "), (":count 5 ", ":count 2.5 "),
                     (":from 1 ", ":from -1 "), (":from 1 ", ":from 10 "), (":to 9 ", ":to inf "), (":zeta 0.02", ":zeta -0.02"),
                     (":static-correction t", ":static-correction maybe"), (":from 1 ", "")):
        bad = text.replace(old, new)
        assert bad != text, old
        p.write_text(bad)
        with pytest.raises(feahip.FeaHipError):
            feahip.Deck.load(str(p))
    # it needs the locked store: (modal :count ...) or a :shift
    p.write_text(text.replace(":count 12", ":modes 4"))
    with pytest.raises(feahip.FeaHipError, match="no locked modes"):
        feahip.Deck.load(str(p))
    p.write_text(re.sub(r"\n   \(modal [^)]*\)", "", text))
    with pytest.raises(feahip.FeaHipError, match="no locked modes"):
        feahip.Deck.load(str(p))
    p.write_text(text.replace(":count 12", ":modes 4").replace(":max 1000", ":max 1000 :shift 3").replace(":static-correction t", ":static-correction nil"))
    assert feahip.Deck.load(str(p)).harmonic_count == 5
    # the correction and a shift exclude each other
    p.write_text(text.replace(":max 1000", ":max 1000 :shift 3"))
    with pytest.raises(feahip.FeaHipError, match="exclude each other"):
        feahip.Deck.load(str(p))
    # the same refusals of feahip.Deck
    for kw in (dict(harmonic_count=4097), dict(harmonic_count=-1), dict(harmonic_count=3, harmonic_from=2.0, harmonic_to=1.0),
               dict(harmonic_count=3, harmonic_from=-1.0, harmonic_to=1.0), dict(harmonic_count=3, harmonic_to=np.inf),
               dict(harmonic_count=3, harmonic_to=1.0, harmonic_zeta=-0.1)):
        with pytest.raises(ValueError, match="harmonic"):
            _deck(**BASE, **kw)
    with pytest.raises(ValueError, match="needs the locked modes"):
        _deck(density=1.5, modal_modes=4, harmonic_count=3, harmonic_to=1.0)
    with pytest.raises(ValueError, match="exclude each other"):
        _deck(**BASE, modal_shift=3.0, harmonic_count=3, harmonic_to=1.0)
    _deck(**BASE, modal_shift=3.0, harmonic_count=3, harmonic_to=1.0, harmonic_static=False)


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
    new = ["harmonic_count", "harmonic_from", "harmonic_to", "harmonic_zeta", "harmonic_static"]
    at = fields.index("damping_alpha")
    assert fields[at - 5:at] == new                                     # immediately in front of damping_alpha
    types = dict(feahip.FeaDeck._fields_)
    assert [types[n] for n in new] == [C.c_int, C.c_double, C.c_double, C.c_double, C.c_int]
    lib = feahip.load_library()
    top = open(os.path.join(ROOT, "include", "fea_hip.h")).read()
    out = os.popen(f"nm -D --defined-only {feahip.LIB_PATH}").read()
    for name in NEW:
        assert name in feahip.ABI and hasattr(lib, name), name
        assert re.search(r"\bint\s+%s\(" % name, top) and re.search(rf"\bT {name}\b", out), name
    assert re.search(r"#define\s+FEA_RESPONSE_MAX_FREQ\s+4096\b", top) and feahip.RESPONSE_MAX_FREQ == 4096
    assert hasattr(feahip.load_host_library(), "fea_harmonic_run")
    for name in ("response_set_basis", "response_load", "response_static", "response_sweep", "response_field"):
        assert callable(getattr(feahip.FeaSolver, name))
        assert not hasattr(feahip.FeaGroup, name)                      # the locked solve is unsharded, and so is this
    assert callable(feahip.host_response_coefficients)

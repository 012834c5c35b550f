"""Rayleigh damping on the host side: feahip_host_rayleigh, the deck grammar (:damping-alpha / :damping-beta inside
(dynamics ...)), the struct fields and the exported symbols.  No GPU."""
import os
import re

import numpy as np
import pytest

import feahip
import mesh
from damping_reference import rayleigh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("feahip_set_damping", "feahip_get_damping", "feahip_damping_spmv", "feahip_host_rayleigh")


def _deck(**kw):
    d = mesh.bar_deck(dims=(1, 2, 1))
    keys = ("model", "parameters", "ele_type", "gauss_nodes_count", "nodes", "elements", "presc_node", "presc_type", "presc_values")
    return feahip.Deck(**{k: getattr(d, k) for k in keys}, **kw)


def test_host_rayleigh_returns_the_ratios_it_was_given():
    for w1, z1, w2, z2 in ((3.0, 0.02, 40.0, 0.05), (1.0, 0.1, 2.0, 0.1), (250.0, 0.01, 7.0, 0.3)):
        a, b = feahip.host_rayleigh(w1, z1, w2, z2)
        for w, z in ((w1, z1), (w2, z2)):
            assert abs(0.5 * (a / w + b * w) - z) <= 1e-14
        ar, br = rayleigh(w1, z1, w2, z2)
        assert abs(a - ar) <= 1e-12 * max(abs(ar), 1.0) and abs(b - br) <= 1e-12 * max(abs(br), 1.0)
    # z1 w1 = z2 w2: the mass-proportional part alone
    a, b = feahip.host_rayleigh(2.0, 0.25, 4.0, 0.125)              # (both products are 0.5 exactly)
    assert b == 0.0 and a == 2 * 0.25 * 2.0
    # two ratios no C >= 0 meets: the negative coefficient comes back as it is
    a, b = feahip.host_rayleigh(1.0, 0.01, 10.0, 0.5)
    assert a < 0.0 < b
    for bad in ((3.0, 0.1, 3.0, 0.2), (0.0, 0.1, 3.0, 0.1), (3.0, 0.1, -1.0, 0.1), (np.nan, 0.1, 3.0, 0.1)):
        with pytest.raises(feahip.FeaHipError, match="feahip_host_rayleigh"):
            feahip.host_rayleigh(*bad)
    lib = feahip.load_library()
    assert lib.feahip_host_rayleigh(1.0, 0.1, 2.0, 0.1, None, None) == feahip.EINVAL


def test_deck_round_trip_keeps_the_coefficients_to_the_bit(tmp_path):
    a, b = 0.1 + 0.2, 1.0 / 3.0e3                              # neither has a short decimal form
    d = _deck(density=1.5, dynamics=dict(steps=2, dt=0.01), damping=(a, b))
    p = tmp_path / "damped.sexp"
    d.save(str(p))
    text = p.read_text()
    assert re.search(r":damping-alpha \S+ :damping-beta \S+\)", text)
    back = feahip.Deck.load(str(p))
    assert back.damping == (a, b)
    q = tmp_path / "again.sexp"
    back.save(str(q))
    assert q.read_bytes() == p.read_bytes()
    # one coefficient alone is written alone
    _deck(density=1.5, dynamics=dict(steps=2, dt=0.01), damping=(a, 0.0)).save(str(p))
    assert ":damping-alpha" in p.read_text() and ":damping-beta" not in p.read_text()
    assert feahip.Deck.load(str(p)).damping == (a, 0.0)
    # the explicit scheme takes alpha
    _deck(density=1.5, dynamics=dict(steps=2, dt=0.0, scheme="explicit"), damping=(a, 0.0)).save(str(p))
    back = feahip.Deck.load(str(p))
    assert back.damping == (a, 0.0) and back.dynamics["scheme"] == "explicit"


def test_load_errors(tmp_path):
    p = tmp_path / "bad.sexp"
    _deck(density=1.5, dynamics=dict(steps=2, dt=0.0, scheme="explicit"), damping=(0.5, 0.0)).save(str(p))
    text = p.read_text()
    p.write_text(text.replace(":scheme explicit", ":damping-beta 0.01 :scheme explicit"))
    with pytest.raises(feahip.FeaHipError, match=r":scheme explicit takes mass-proportional damping only"):
        feahip.Deck.load(str(p))
    for bad in (":damping-alpha -1", ":damping-alpha nan", ":damping-alpha x"):
        p.write_text(re.sub(r":damping-alpha \S+", bad, text))
        with pytest.raises(feahip.FeaHipError):
            feahip.Deck.load(str(p))
    with pytest.raises(ValueError, match="damping"):
        _deck(density=1.5, damping=(-0.1, 0.0))
    with pytest.raises(ValueError, match="needs a density"):
        _deck(damping=(0.1, 0.0)).save(str(p))


def test_a_deck_without_the_keys_saves_as_before(tmp_path):
    """Byte for byte the file the code before the damping wrote (tests/golden/decks/undamped_dynamics.sexp was written by
    it), with the keys absent, zero, or None."""
    want = open(os.path.join(ROOT, "tests", "golden", "decks", "undamped_dynamics.sexp"), "rb").read()
    assert b"damping" not in want
    kw = dict(density=1.5, body_force=[0.0, 0.0, -2.0], dynamics=dict(steps=3, dt=0.0625, dlambda=1.0))
    for extra in ({}, dict(damping=None), dict(damping=(0.0, 0.0))):
        p = tmp_path / "plain.sexp"
        _deck(**kw, **extra).save(str(p))
        assert p.read_bytes() == want
        back = feahip.Deck.load(str(p))
        assert back.damping is None
        back.save(str(p))
        assert p.read_bytes() == want


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
    at = fields.index("damping_alpha")
    assert fields[at:at + 3] == ["damping_alpha", "damping_beta", "contact_faces_count"]   # in front of the pinned fields
    lib = feahip.load_library()
    top = open(os.path.join(ROOT, "include", "fea_hip.h")).read()
    for name in NEW:
        assert name in feahip.ABI and hasattr(lib, name) and re.search(r"\bint\s+%s\(" % name, top)

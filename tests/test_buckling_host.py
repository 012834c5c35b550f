"""Linear buckling, the parts that need no GPU: feahip_host_buckling_factor, the (buckling ...) section of the deck
reader / writer, the struct the Python side shares with the C side, and the exported symbols."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import feahip
from buckling_reference import column_deck

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("feahip_solve_buckling", "feahip_get_buckling_modes", "feahip_geometric_spmv", "feahip_host_buckling_factor")


def _deck(**kw):
    d = column_deck("tet4", dims=(1, 2, 1), size=(1.0, 2.0, 1.0))
    return feahip.Deck(nodes=d.nodes, elements=d.elements, ele_type=d.ele_type, gauss_nodes_count=d.gauss_nodes_count,
                       presc_node=d.presc_node, presc_type=d.presc_type, presc_values=d.presc_values, **kw)


def test_host_buckling_factor():
    nu = np.array([-0.5, -0.025, -1e-300, 0.0, -0.0, 0.3, np.inf])
    f = feahip.host_buckling_factor(nu)
    assert f[0] == 3.0 and f[1] == 1.0 - 1.0 / -0.025 and f[2] == 1.0 - 1.0 / -1e-300
    assert np.all(np.isposinf(f[3:]))
    assert feahip.host_buckling_factor([-0.25])[0] == 5.0
    lib = feahip.load_library()
    assert lib.feahip_host_buckling_factor(0, None, None) == 0
    assert lib.feahip_host_buckling_factor(2, None, None) == feahip.EINVAL
    assert lib.feahip_host_buckling_factor(-1, None, None) == feahip.EINVAL


def test_buckling_section_round_trip(tmp_path):
    deck = _deck(buckling_modes=5, buckling_tolerance=2.5e-9, buckling_max=321)
    path = str(tmp_path / "b.sexp")
    deck.save(path)
    text = open(path).read()
    assert re.search(r"\(buckling :modes 5 :tolerance 2\.5\d*e-09 :max 321\)", text), text
    assert "(dynamics" not in text                          # no density is needed
    back = feahip.Deck.load(path)
    assert (back.buckling_modes, back.buckling_tolerance, back.buckling_max) == (5, 2.5e-9, 321)
    back.save(str(tmp_path / "again.sexp"))
    assert open(str(tmp_path / "again.sexp")).read() == text


def test_buckling_section_defaults_and_absence(tmp_path):
    path = str(tmp_path / "b.sexp")
    _deck(buckling_modes=2).save(path)
    text = open(path).read()
    open(path, "w").write(re.sub(r"\(buckling [^)]*\)", "(buckling :modes 3)", text))
    back = feahip.Deck.load(path)
    assert (back.buckling_modes, back.buckling_tolerance, back.buckling_max) == (3, 1e-8, 2000)
    plain = str(tmp_path / "plain.sexp")
    _deck().save(plain)
    assert "buckling" not in open(plain).read()
    assert feahip.Deck.load(plain).buckling_modes == 0
    # the text of a deck without the section is the text of the same deck with the section taken out
    assert re.sub(r"\n\s*\(buckling [^)]*\)", "", text) == open(plain).read()


def test_a_deck_may_hold_modal_and_buckling_sections(tmp_path):
    path = str(tmp_path / "both.sexp")
    _deck(density=1.5, modal_modes=2, buckling_modes=3).save(path)
    back = feahip.Deck.load(path)
    assert (back.modal_modes, back.buckling_modes) == (2, 3)


def test_bad_buckling_sections_are_refused(tmp_path):
    for kw in (dict(buckling_modes=9), dict(buckling_modes=-1), dict(buckling_modes=2, buckling_tolerance=0.0)):
        with pytest.raises(ValueError, match="buckling"):
            _deck(**kw)
    path = str(tmp_path / "b.sexp")
    _deck(buckling_modes=2).save(path)
    text = open(path).read()
    for bad in ("(buckling :modes 0)", "(buckling :modes 9)", "(buckling :modes 2.5)", "(buckling :modes 2 :tolerance 0)",
                "(buckling :modes 2 :tolerance -1e-8)", "(buckling :modes 2 :max -1)", "(buckling :tolerance 1e-8)"):
        open(path, "w").write(re.sub(r"\(buckling [^)]*\)", bad, text))
        with pytest.raises(feahip.FeaHipError, match="buckling|modes"):
            feahip.Deck.load(path)


def test_deck_struct_holds_the_buckling_fields():
    """The three fields are in struct fea_deck and in FeaDeck at the same place: the newest of the struct, in front of
    the five modal fields whose place at the end the modal tests pin."""
    hdr = open(os.path.join(ROOT, "fea-large_amd", "host", "fea_host.h")).read()
    body = re.sub(r"/\*.*?\*/", "", hdr[hdr.index("typedef struct fea_deck {"):hdr.index("} fea_deck;")], flags=re.S)
    names = []
    for stmt in body.split(";"):
        stmt = stmt.replace("typedef struct fea_deck {", "").strip()
        if stmt:
            names += [re.sub(r"\[.*\]", "", n).strip(" *") for n in re.sub(r"^\s*(int|double)\s", "", stmt).split(",")]
    fields = [n for n, _ in feahip.FeaDeck._fields_]
    assert names == fields
    assert fields[-8:-5] == ["buckling_modes", "buckling_tolerance", "buckling_max"]
    types = dict(feahip.FeaDeck._fields_)
    assert (types["buckling_modes"], types["buckling_tolerance"], types["buckling_max"]) == (C.c_int, C.c_double, C.c_int)


def test_new_symbols_are_exported_and_declared():
    lib = feahip.load_library()
    top = open(os.path.join(ROOT, "include", "fea_hip.h")).read()
    for name in NEW:
        assert name in feahip.ABI and hasattr(lib, name)
        assert re.search(r"\bint\s+%s\(" % name, top)
    host = feahip.load_host_library()
    assert hasattr(host, "fea_buckling_run")
    for name in ("solve_buckling", "buckling_modes", "geometric_spmv"):
        assert callable(getattr(feahip.FeaSolver, name))
    assert callable(feahip.host_buckling_factor)
    assert "18 k_geom_elements" in top and "19 k_geom_blocks" in top

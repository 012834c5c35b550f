"""The locked modal solve, the parts that need no GPU: the :count and :shift keys of the (modal ...) section through the C
reader and writer and through feahip.Deck, and the two struct fields they add in front of the three pinned ones."""
import os
import re

import pytest

import feahip
from dynamics_reference import loaded_bar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _deck(**kw):
    d = loaded_bar("tet4", (1, 2, 1), end_motion=0.01)
    return feahip.Deck(nodes=d.nodes, elements=d.elements, ele_type=d.ele_type, gauss_nodes_count=d.gauss_nodes_count,
                       presc_node=d.presc_node, presc_type=d.presc_type, presc_values=d.presc_values, **kw)


def test_count_and_shift_round_trip(tmp_path):
    deck = _deck(density=1.5, modal_count=24, modal_shift=12.5, modal_tolerance=2.5e-9, modal_max=321)
    path = str(tmp_path / "locked.sexp")
    deck.save(path)
    text = open(path).read()
    assert re.search(r"\(modal :count 24 :tolerance 2\.5\d*e-09 :max 321 :shift 12\.5\)", text), text
    back = feahip.Deck.load(path)
    assert (back.modal_count, back.modal_shift, back.modal_modes) == (24, 12.5, 0)
    assert (back.modal_tolerance, back.modal_max) == (2.5e-9, 321)
    back.save(str(tmp_path / "again.sexp"))
    assert open(str(tmp_path / "again.sexp")).read() == text


def test_shift_is_written_only_when_not_zero_and_goes_with_modes_too(tmp_path):
    path = str(tmp_path / "m.sexp")
    _deck(density=1.5, modal_count=64).save(path)
    text = open(path).read()
    assert re.search(r"\(modal :count 64 :tolerance \S+ :max 1000\)", text), text
    back = feahip.Deck.load(path)
    assert (back.modal_count, back.modal_shift) == (64, 0.0)
    _deck(density=1.5, modal_modes=6, modal_shift=3.0).save(path)
    text = open(path).read()
    assert re.search(r"\(modal :modes 6 :tolerance \S+ :max 1000 :shift 3\)", text), text
    back = feahip.Deck.load(path)
    assert (back.modal_modes, back.modal_count, back.modal_shift) == (6, 0, 3.0)


def test_without_the_new_keys_the_text_is_the_old_one(tmp_path):
    path = str(tmp_path / "old.sexp")
    _deck(density=1.5, modal_modes=5, modal_tolerance=1e-8, modal_max=1000).save(path)
    text = open(path).read()
    assert "\n   (modal :modes 5 :tolerance 1e-08 :max 1000)" in text
    assert ":count" not in text and ":shift" not in text
    back = feahip.Deck.load(path)
    assert (back.modal_modes, back.modal_count, back.modal_shift) == (5, 0, 0.0)
    _deck(density=1.5).save(path)
    assert "(modal" not in open(path).read()


def test_refusals_of_the_reader_and_of_the_deck(tmp_path):
    path = str(tmp_path / "m.sexp")
    _deck(density=1.5, modal_count=10).save(path)
    text = open(path).read()
    for bad, why in (("(modal :count 10 :modes 4)", "not both"), ("(modal :count 65)", r"\[1, 64\]"), ("(modal :count 0)", r"\[1, 64\]"),
                     ("(modal :count 2.5)", r"\[1, 64\]"), ("(modal :count 10 :shift -1)", "not negative"),
                     ("(modal :modes 4 :shift -1)", "not negative"), ("(modal :shift 1)", "modes"), ("(modal :modes 9)", r"\[0, 8\]")):
        open(path, "w").write(re.sub(r"\(modal [^)]*\)", bad, text))
        with pytest.raises(feahip.FeaHipError, match=why):
            feahip.Deck.load(path)
    open(path, "w").write(re.sub(r"\n\s*\(dynamics [^)]*\)", "", text))
    with pytest.raises(feahip.FeaHipError, match=r"\(modal \.\.\.\) but no density"):
        feahip.Deck.load(path)
    for kw, why in ((dict(modal_count=10, modal_modes=4), "not both"), (dict(modal_count=65), "modal_count"),
                    (dict(modal_count=-1), "modal_count"), (dict(modal_count=10, modal_shift=-1.0), "modal_shift"),
                    (dict(modal_count=10, modal_shift=float("nan")), "modal_shift"), (dict(modal_shift=1.0), "modal_shift needs"),
                    (dict(modal_modes=9), "modal_modes")):
        with pytest.raises(ValueError, match=why):
            _deck(density=1.5, **kw)
    with pytest.raises(ValueError, match="density"):
        _deck(modal_count=10)


def test_the_new_struct_fields_sit_before_the_pinned_three():
    hdr = open(os.path.join(ROOT, "fea-large_amd", "host", "fea_host.h")).read()
    body = re.sub(r"/\*.*?\*/", "", hdr[hdr.index("typedef struct fea_deck {"):hdr.index("} fea_deck;")], flags=re.S)
    names = []
    for stmt in body.split(";"):
        stmt = stmt.replace("typedef struct fea_deck {", "").strip()
        if stmt:
            names += [re.sub(r"\[.*\]", "", n).strip(" *") for n in re.sub(r"^\s*(int|double)\s", "", stmt).split(",")]
    fields = [n for n, _ in feahip.FeaDeck._fields_]
    assert names == fields
    assert fields[-5:] == ["modal_count", "modal_shift", "modal_modes", "modal_tolerance", "modal_max"]
    assert feahip.MODAL_MAX_LOCKED == 64
    top = open(os.path.join(ROOT, "include", "fea_hip.h")).read()
    assert re.search(r"#define\s+FEA_MODAL_MAX_LOCKED\s+64\b", top)
    for name in ("feahip_solve_modes_locked", "feahip_get_locked_modes", "feahip_get_locked_count", "feahip_modal_deflate"):
        assert name in feahip.ABI and re.search(r"\bint\s+%s\(" % name, top)

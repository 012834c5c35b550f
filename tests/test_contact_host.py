"""The host side of the contact feature, without a device: the (contact ...) section through the C reader and writer,
the refusals of malformed sections, the place of the new struct fields, the exported symbols, and the text of a deck
without the section."""
import os
import re

import numpy as np
import pytest

import feahip
import mesh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "contact")
NEW = ["feahip_set_contact", "feahip_get_contact_nodes", "feahip_get_contact_obstacles", "feahip_get_contact_multipliers", "feahip_set_contact_multipliers",
       "feahip_get_contact_forces", "feahip_get_contact_status", "feahip_contact_info", "feahip_contact_augment"]


def plain_deck():
    """The deck of tests/golden/contact/plain_deck.sexp, which the writer of the commit before contact wrote."""
    deck = mesh.bar_deck(dims=(1, 2, 1), recipe="uniaxial", modified_newton=False, load_increments_count=3)
    faces = mesh.block_side_faces(deck.nodes, deck.elements, 0, True)
    deck.surface_faces, deck.surface_kind = faces, np.zeros(len(faces), np.int32)
    deck.surface_values = np.tile([0.25, 0.0, 0.0], (len(faces), 1))
    return deck


OBSTACLES = [(feahip.OBSTACLE_PLANE, (0.0, 7.0, 0.0), (0.0, -2.0, 0.0), 0.0, (0.0, -0.1, 0.0)),
             (feahip.OBSTACLE_SPHERE, (0.5, 7.5, 0.5), (0.0, 0.0, 0.0), 0.625, (0.0, -0.05, 0.0)),
             (feahip.OBSTACLE_SPHERE_INSIDE, (0.5, 4.0, 0.5), (0.0, 0.0, 0.0), 4.0, (0.0, 0.0, 0.0)),
             (feahip.OBSTACLE_CYLINDER, (2.0, 0.0, 0.5), (0.0, 1.0, 0.25), 0.75, (-0.125, 0.0, 0.0)),
             (feahip.OBSTACLE_CYLINDER_INSIDE, (0.5, 0.0, 0.5), (0.0, 1.0, 0.0), 1.5, (0.0, 0.0, 0.0))]


def contact_deck():
    deck = plain_deck()
    deck.contact_faces = mesh.block_side_faces(deck.nodes, deck.elements, 1, True)
    deck.contact_obstacles = OBSTACLES
    deck.contact_penalty, deck.contact_augment, deck.contact_gap_tolerance = 1.5e3, 4, 2.5e-7
    return deck


def test_a_deck_without_the_section_is_written_as_before(tmp_path):
    path = str(tmp_path / "plain.sexp")
    plain_deck().save(path)
    assert open(path, "rb").read() == open(os.path.join(GOLDEN, "plain_deck.sexp"), "rb").read()
    back = feahip.Deck.load(os.path.join(GOLDEN, "plain_deck.sexp"))
    assert len(back.contact_faces) == 0 and back.contact_obstacles == []
    back.save(path)
    assert open(path, "rb").read() == open(os.path.join(GOLDEN, "plain_deck.sexp"), "rb").read()


def test_contact_section_round_trip(tmp_path):
    deck = contact_deck()
    path = str(tmp_path / "c.sexp")
    deck.save(path)
    text = open(path).read()
    assert re.search(r"\(contact :penalty 1500 :augment 4 :gap-tolerance 2\.\d+e-07\s+\(faces", text), text
    assert "(plane :point (0 7 0) :normal (0 -2 0) :travel (0 -0.1" in text
    assert "(sphere :center (0.5 7.5 0.5) :radius 0.625 :travel (0 -0.05" in text and ":inside nil)" in text
    assert "(cylinder :point (0.5 0 0.5) :axis (0 1 0) :radius 1.5 :travel (0 0 0) :inside t)" in text
    assert text.index("(surface-loads") < text.index("(contact") < text.rindex(")))")
    back = feahip.Deck.load(path)
    assert np.array_equal(back.contact_faces, deck.contact_faces)
    assert (back.contact_penalty, back.contact_augment, back.contact_gap_tolerance) == (1.5e3, 4, 2.5e-7)
    k0, g0 = feahip.obstacle_arrays(OBSTACLES)
    k1, g1 = feahip.obstacle_arrays(back.contact_obstacles)
    assert np.array_equal(k0, k1) and np.array_equal(g0, g1)
    back.save(str(tmp_path / "again.sexp"))
    assert open(str(tmp_path / "again.sexp")).read() == text
    # the rest of the deck is the plain deck's text
    plain = open(os.path.join(GOLDEN, "plain_deck.sexp")).read()
    cut = text[:text.index("\n   (contact")] + text[text.index(")))\n", text.index("(contact")):]
    assert cut == plain


BAD = [("(contact :augment 1 (faces (0 1 2)) (plane :point (0 0 0) :normal (0 1 0)))", "needs :penalty"),
       ("(contact :penalty 0 (faces (0 1 2)) (plane :point (0 0 0) :normal (0 1 0)))", ":penalty must be positive"),
       ("(contact :penalty 1 :augment -1 (faces (0 1 2)) (plane :point (0 0 0) :normal (0 1 0)))", ":augment"),
       ("(contact :penalty 1 :gap-tolerance -1 (faces (0 1 2)) (plane :point (0 0 0) :normal (0 1 0)))", ":gap-tolerance"),
       ("(contact :penalty 1 (plane :point (0 0 0) :normal (0 1 0)))", "without (faces"),
       ("(contact :penalty 1 (faces (0 1 2)))", "without an obstacle"),
       ("(contact :penalty 1 (faces (0 1 2) (0 1)) (plane :point (0 0 0) :normal (0 1 0)))", "same number of nodes"),
       ("(contact :penalty 1 (faces (0 1 2)) (plane :point (0 0 0)))", "plane needs :normal"),
       ("(contact :penalty 1 (faces (0 1 2)) (plane :point (0 0 0) :normal (0 0 0)))", ":normal is zero"),
       ("(contact :penalty 1 (faces (0 1 2)) (sphere :center (0 0 0)))", "sphere needs :radius"),
       ("(contact :penalty 1 (faces (0 1 2)) (sphere :center (0 0 0) :radius -1))", ":radius must be positive"),
       ("(contact :penalty 1 (faces (0 1 2)) (cylinder :point (0 0 0) :radius 1))", "cylinder needs :axis"),
       ("(contact :penalty 1 (faces (0 1 2)) (sphere :center (0 0) :radius 1))", "three numbers"),
       ("(contact :penalty 1 (faces (0 1 2)) (sphere :center (0 0 0) :radius 1 :inside yes))", ":inside must be t or nil"),
       ("(contact :penalty 1 (faces (0 1 2)) (torus :point (0 0 0)))", "expected (faces"),
       ("(contact :penalty 1 (faces (0 1 2))" + " (plane :point (0 0 0) :normal (0 1 0))" * 9 + ")", "more than 8 obstacles")]


@pytest.mark.parametrize("section,why", BAD)
def test_malformed_sections_are_refused(tmp_path, section, why):
    plain = open(os.path.join(GOLDEN, "plain_deck.sexp")).read()
    at = plain.rindex(")))")
    path = str(tmp_path / "bad.sexp")
    open(path, "w").write(plain[:at] + "\n   " + section + plain[at:])
    with pytest.raises(feahip.FeaHipError) as e:
        feahip.Deck.load(path)
    assert why in str(e.value) and "line " in str(e.value), str(e.value)


def test_the_new_struct_fields_sit_in_front_of_buckling_modes():
    hdr = open(os.path.join(ROOT, "fea-large_amd", "host", "fea_host.h")).read()
    body = re.sub(r"/\*.*?\*/", "", hdr[hdr.index("typedef struct fea_deck {"):hdr.index("} fea_deck;")], flags=re.S)
    names = []
    for stmt in body.split(";"):
        stmt = stmt.replace("typedef struct fea_deck {", "").strip()
        if stmt:
            assert re.match(r"^(int|double)\s", stmt), stmt      # plain int, double or pointer members
            names += [re.sub(r"\[.*\]", "", n).strip(" *") for n in re.sub(r"^\s*(int|double)\s", "", stmt).split(",")]
    fields = [n for n, _ in feahip.FeaDeck._fields_]
    assert names == fields
    new = ["contact_faces_count", "contact_nodes_per_face", "contact_nodes", "contact_obstacles_count", "contact_kind",
           "contact_geom", "contact_penalty", "contact_augment", "contact_gap_tolerance"]
    at = fields.index("buckling_modes")
    assert fields[at - len(new):at] == new and len(fields) - at == 8


def test_new_symbols_are_exported_and_declared():
    lib = feahip.load_library()
    top = open(os.path.join(ROOT, "include", "fea_hip.h")).read()
    out = os.popen(f"nm -D --defined-only {feahip.LIB_PATH}").read()
    for name in NEW:
        assert name in feahip.ABI and hasattr(lib, name)
        assert re.search(r"\bint\s+%s\(" % name, top) and re.search(rf"\bT {name}\b", out), name
    assert re.search(r"#define\s+FEAHIP_MAX_OBSTACLES\s+8\b", top) and feahip.MAX_OBSTACLES == 8
    for k, name in enumerate(("PLANE", "SPHERE", "SPHERE_INSIDE", "CYLINDER", "CYLINDER_INSIDE")):
        assert re.search(r"FEAHIP_OBSTACLE_%s = %d\b" % (name, k), top) and getattr(feahip, "OBSTACLE_" + name) == k
    assert "20 k_contact alone" in top and "rho = |x - c| or |q|" in top
    for name in ("set_contact", "contact_nodes", "contact_multipliers", "set_contact_multipliers", "contact_forces",
                 "contact_status", "contact_info", "contact_augment"):
        assert callable(getattr(feahip.FeaSolver, name))
    assert callable(feahip.FeaGroup.contact_info)

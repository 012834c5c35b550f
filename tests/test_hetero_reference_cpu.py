"""tests/hetero_reference.py against the oracle it is built on, without a device: with every element of one material
the restatement is the single oracle's assembled K and f; the Python deck and slab carry the table."""
import numpy as np
import pytest

import feahip
import mesh
from hetero_reference import MATERIALS, HeteroRestatement, layered_ids, perturbed, scattered_ids, with_materials
from oracle_binding import OracleSolver


@pytest.mark.parametrize("kind", ["tet4", "tet10", "hex8"])
@pytest.mark.parametrize("model", [feahip.MODEL_COMPRESSIBLE_NEOHOOKEAN, feahip.MODEL_A5])
def test_one_material_is_the_single_oracle(kind, model):
    deck = {"tet4": lambda: mesh.bar_deck(dims=(2, 3, 2), model=model),
            "tet10": lambda: mesh.bar_deck(dims=(1, 2, 1), quadratic=True, gauss=5, model=model),
            "hex8": lambda: mesh.bar_deck(dims=(2, 3, 2), hexa=True, model=model)}[kind]()
    x = perturbed(deck.nodes)
    pair = np.array([[400.0, 250.0]])
    r = HeteroRestatement(deck, np.tile(pair, (3, 1)), scattered_ids(deck))
    K, f, F, S = r.assemble(x)
    import copy
    d = copy.copy(deck); d.parameters = pair[0].copy()
    o = OracleSolver(d)
    o.set_nodes(x); o.update_state(); o.create_stiffness(); o.create_residual_forces()
    val = r.yale_values(K, o.offsets(), o.indexes())
    assert np.abs(val - o.values()).max() <= 1e-13 * np.abs(o.values()).max()
    assert np.abs(f - o.forces()).max() <= 1e-13 * np.abs(o.forces()).max()
    assert np.count_nonzero(K) <= o.nnz()                     # nothing outside the pattern
    assert np.array_equal(F, o.graddefs()) and np.array_equal(S, o.stresses())
    r.close(); o.close()


def test_two_materials_differ_and_layers_are_layers():
    deck = mesh.bar_deck(dims=(2, 6, 2))
    ids = layered_ids(deck)
    assert sorted(set(ids.tolist())) == [0, 1, 2]
    y = deck.nodes[deck.elements].mean(axis=1)[:, 1]
    assert y[ids == 0].max() < y[ids == 1].min() and y[ids == 1].max() < y[ids == 2].min()
    assert sorted(set(scattered_ids(deck)[:3].tolist())) == [0, 1, 2]
    x = perturbed(deck.nodes)
    a = HeteroRestatement(deck, MATERIALS, ids)
    b = HeteroRestatement(deck, MATERIALS[[0, 0, 0]], ids)
    Ka, Kb = a.assemble(x)[0], b.assemble(x)[0]
    assert np.abs(Ka - Ka.T).max() <= 1e-12 * np.abs(Ka).max()
    assert np.abs(Ka - Kb).max() > 0.1 * np.abs(Kb).max()
    a.close(); b.close()


def test_deck_and_slab_carry_the_table():
    deck = mesh.bar_deck(dims=(2, 8, 2))
    ids = scattered_ids(deck)
    d = with_materials(deck, MATERIALS, ids)
    for n in (2, 3):
        seen = np.zeros(len(deck.elements), dtype=int)
        for r in range(n):
            sl = feahip.slab_of(d, r, n)
            assert np.array_equal(sl.materials, MATERIALS)
            assert np.array_equal(sl.element_material, ids[sl.elem_global])
            seen[sl.elem_global] += 1
        assert np.all(seen >= 1)
    assert len(feahip.slab_of(deck, 0, 2).materials) == 0     # no table: nothing to carry
    with pytest.raises(ValueError):
        feahip.Deck(nodes=deck.nodes, elements=deck.elements, materials=MATERIALS)
    with pytest.raises(ValueError):
        feahip.Deck(nodes=deck.nodes, elements=deck.elements, materials=MATERIALS, element_material=ids[:-1])


def hetero_deck():
    deck = mesh.bar_deck(dims=(2, 3, 2))
    return with_materials(deck, np.array([[100.0, 100.0], [1.0 / 3.0, 250.125], [29.999999999999996, 80.0]]), scattered_ids(deck))


def test_deck_file_round_trip_keeps_table_and_ids_to_the_bit(tmp_path):
    d = hetero_deck()
    p = tmp_path / "het.sexp"
    d.save(str(p))
    text = p.read_text()
    assert "(materials" in text and "(element-materials" in text
    back = feahip.Deck.load(str(p))
    assert np.array_equal(back.materials, d.materials) and back.materials.dtype == np.float64
    assert np.array_equal(back.element_material, d.element_material)
    assert np.array_equal(back.nodes, d.nodes) and np.array_equal(back.elements, d.elements)
    assert np.array_equal(back.parameters, d.parameters)
    back.save(str(tmp_path / "again.sexp"))                   # and the file itself is a fixed point
    assert (tmp_path / "again.sexp").read_text() == text


def test_deck_without_the_sections_round_trips_as_before(tmp_path):
    d = mesh.bar_deck(dims=(2, 3, 2))
    p = tmp_path / "plain.sexp"
    d.save(str(p))
    text = p.read_text()
    assert "materials" not in text
    back = feahip.Deck.load(str(p))
    assert len(back.materials) == 0 and len(back.element_material) == 0
    assert np.array_equal(back.nodes, d.nodes) and np.array_equal(back.elements, d.elements)
    assert np.array_equal(back.presc_node, d.presc_node) and np.array_equal(back.presc_values, d.presc_values)
    back.save(str(tmp_path / "again.sexp"))
    assert (tmp_path / "again.sexp").read_text() == text
    # what a deck without a table writes has not changed: the model and geometry lists close where they closed
    assert "(model-parameters :mu 100 :lambda 100))\n (solution" in text
    assert "))\n  (boundary-conditions" in text


def test_loader_refuses_inconsistent_material_sections(tmp_path):
    import re
    d = hetero_deck()
    p = tmp_path / "het.sexp"
    d.save(str(p))
    text = p.read_text()
    mats = re.search(r"\n\s*\(materials.*?\)\)", text, re.S).group(0)
    ids = re.search(r"\n\s*\(element-materials.*?\)", text, re.S).group(0)
    assert mats.count("(material ") == 3

    def refused(new, what):
        q = tmp_path / "bad.sexp"
        q.write_text(new)
        with pytest.raises(feahip.FeaHipError, match=what):
            feahip.Deck.load(str(q))

    refused(text.replace(ids, ""), r"\(materials \.\.\.\) but no \(element-materials")
    refused(text.replace(mats, ""), r"\(element-materials \.\.\.\) but no \(materials")
    E = len(d.elements)
    refused(text.replace(ids, ids[:-1] + " 0)"), f"element-materials has {E + 1} ids for {E} elements")
    short = ids[:ids.rstrip(")").rstrip().rfind(" ")] + ")"
    refused(text.replace(ids, short), f"element-materials has {E - 1} ids for {E} elements")
    first = re.search(r"\(element-materials\s+(\d+)", ids)
    bad = ids[:first.start(1)] + "3" + ids[first.end(1):]
    refused(text.replace(ids, bad), r"element 0 has material 3 outside \[0,3\)")
    many = mats[:-1] + "\n (material :lambda 1 :mu 1)" * 254 + ")"      # 3 + 254 = 257 entries
    refused(text.replace(mats, many), "more than 256 materials")
    neg = ids[:first.start(1)] + "-1" + ids[first.end(1):]
    refused(text.replace(ids, neg), r"element 0 has material -1 outside \[0,3\)")


def test_gmsh_export_tags_elements_with_their_material(tmp_path):
    d = hetero_deck()
    E = len(d.elements)
    zero = [np.zeros((E, 3, 3))]

    def tags(deck):
        p = tmp_path / "o.msh"
        feahip.export_gmsh(str(p), deck, [deck.nodes], zero)
        lines = p.read_text().splitlines()
        k = lines.index("$Elements")
        return np.array([[int(v) for v in ln.split()[2:6]] for ln in lines[k + 2:k + 2 + E]])

    t = tags(d)
    assert np.all(t[:, 0] == 3) and np.array_equal(t[:, 1], d.element_material + 1) and np.all(t[:, 2:] == 1)
    assert np.all(tags(mesh.bar_deck(dims=(2, 3, 2)))[:, 1:] == 1)      # no table: what it wrote before

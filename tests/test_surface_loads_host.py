"""Surface loads, host side (no GPU): the ABI symbols, the resolution of loaded faces to (element, local face) that
feahip_set_surface_loads makes, and the (surface-loads ...) section of the deck through libfeahost.so."""
import ctypes as C
import math

import numpy as np
import pytest

import feahip
import mesh

NEW_SYMBOLS = ["feahip_set_surface_loads", "feahip_get_surface_forces", "feahip_set_load_factor",
               "feahip_get_load_factor", "feahip_host_surface_faces"]


def test_library_exports_the_surface_load_entries():
    lib = C.CDLL(feahip.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name


def _blocks():
    n4, e4 = mesh.kuhn_block(2, 3, 2)
    n10, e10 = mesh.kuhn_block(2, 2, 2, quadratic=True)
    n8, e8 = mesh.hex_block(2, 3, 2)
    return {"tet4": (n4, e4), "tet10": (n10, e10), "hex8": (n8, e8)}


def _faces_of(elements, e, lf):
    return elements[e][mesh.element_faces(elements.shape[1])[lf]]


@pytest.mark.parametrize("kind", ["tet4", "tet10", "hex8"])
def test_every_boundary_face_resolves_in_any_node_order(kind):
    nodes, el = _blocks()[kind]
    # the boundary: faces of one element, counted over ALL element faces here (independent of mesh.boundary_faces)
    table = mesh.element_faces(el.shape[1])
    keys = {}
    for e in range(len(el)):
        for lf in range(len(table)):
            keys.setdefault(tuple(sorted(el[e][table[lf]])), []).append((e, lf))
    bnd = [(k, v[0]) for k, v in keys.items() if len(v) == 1]
    # block of nx*ny*nz cubes: 2 (xy + yz + zx) squares, 2 triangles each for tetrahedra
    nx, ny, nz = (2, 3, 2) if kind != "tet10" else (2, 2, 2)
    squares = 2 * (nx * ny + ny * nz + nz * nx)
    assert len(bnd) == (squares if kind == "hex8" else 2 * squares)
    rng = np.random.default_rng(7)
    faces = np.array([rng.permutation(k) for k, _ in bnd], dtype=np.int32)
    fe, fl, bad = feahip.host_surface_faces(el, len(nodes), faces)
    assert bad == -1
    assert [(int(a), int(b)) for a, b in zip(fe, fl)] == [v for _, v in bnd]
    # outward: the face's normal in the element's order points away from the element's centroid
    for f in range(len(faces)):
        x = nodes[_faces_of(el, fe[f], fl[f])]
        n = np.cross(x[1] - x[0], x[2] - x[0])
        assert n @ (x[:3].mean(axis=0) - nodes[el[fe[f]]].mean(axis=0)) > 0


@pytest.mark.parametrize("kind", ["tet4", "tet10", "hex8"])
def test_interior_unknown_and_wrong_size_faces_are_refused(kind):
    nodes, el = _blocks()[kind]
    bnd, _, _ = mesh.boundary_faces(el)
    table = mesh.element_faces(el.shape[1])
    bset = {tuple(sorted(f)) for f in bnd}
    interior = next(el[e][table[lf]] for e in range(len(el)) for lf in range(len(table))
                    if tuple(sorted(el[e][table[lf]])) not in bset)
    faces = np.array(bnd[:5].tolist() + [interior.tolist()] + bnd[5:8].tolist(), dtype=np.int32)
    fe, fl, bad = feahip.host_surface_faces(el, len(nodes), faces)
    assert bad == 5
    # a node set that is no face at all: the first face with one node replaced by a far one
    odd = bnd[:3].copy()
    odd[2, 0] = int(np.argmax(np.linalg.norm(nodes - nodes[odd[2, 1]], axis=1)))
    assert feahip.host_surface_faces(el, len(nodes), odd)[2] == 2
    # the corner nodes only of a 10-node face, or one node short of any face
    short = bnd[:, :-1] if kind != "tet10" else bnd[:, :3]
    assert feahip.host_surface_faces(el, len(nodes), short)[2] == 0
    # a repeated node
    rep = bnd[:4].copy()
    rep[3, 1] = rep[3, 0]
    assert feahip.host_surface_faces(el, len(nodes), rep)[2] == 3


def test_side_faces_of_the_blocks():
    for kind, (nodes, el) in _blocks().items():
        nx, ny, nz = (2, 3, 2) if kind != "tet10" else (2, 2, 2)
        f = mesh.block_side_faces(nodes, el, 1, True)
        assert len(f) == nx * nz * (1 if kind == "hex8" else 2)
        assert np.allclose(nodes[f][:, :, 1], nodes[:, 1].max())
        assert f.shape[1] == {"tet4": 3, "tet10": 6, "hex8": 4}[kind]


def test_six_point_triangle_rule_is_degree_four():
    """The closed form of the tri6 rule the kernel uses (kernels_surface.hip): exact for x^a y^b, a + b <= 4."""
    s10, r = math.sqrt(10.0), math.sqrt(38.0 - 44.0 * math.sqrt(0.4))
    a = [(8.0 - s10 + r) / 18.0, (8.0 - s10 - r) / 18.0]
    d = math.sqrt(213125.0 - 53320.0 * s10)
    w = [(620.0 + d) / 3720.0, (620.0 - d) / 3720.0]
    pts = [(ak, ak, wk) for ak, wk in zip(a, w)] + [(1 - 2 * ak, ak, wk) for ak, wk in zip(a, w)] + \
          [(ak, 1 - 2 * ak, wk) for ak, wk in zip(a, w)]
    for p in range(5):
        for q in range(5 - p):
            exact = math.factorial(p) * math.factorial(q) / math.factorial(p + q + 2)
            got = 0.5 * sum(wk * x ** p * y ** q for x, y, wk in pts)
            assert abs(got - exact) < 1e-15, (p, q)


DECK_WITH_LOADS = """(task (model :name COMPRESSIBLE_NEOHOOKEAN (model-parameters :mu 100 :lambda 100))
 (solution :desired-tolerance 1e-8 :task-type CARTESIAN3D :load-increments-count 2 :modified-newton no :max-newton-count 9
   (element-type :gauss-nodes-count 1 :name TETRAHEDRA4 :nodes-count 4))
 (input-data (geometry (nodes (0 0 0) (1 0 0) (0 1 0) (0 0 1)) (elements (0 1 2 3)))
  (boundary-conditions (prescribed-displacements (presc-node :x 0 :y 0.5 :z 0 :type 7 :node-id 3))
   (surface-loads
     (pressure :value 0.5 :nodes (0 1 2))
     (traction :x 0 :y 1.5 :z -0.25 :nodes (1 2 3))))))
"""

# what fea_deck_save wrote for the deck above without its surface-loads section before the section existed
SAVED_WITHOUT_LOADS = """;; -*- Mode: lisp; -*-
(task
 (model :name COMPRESSIBLE_NEOHOOKEAN
        (model-parameters :mu 100 :lambda 100))
 (solution :desired-tolerance 1e-08 :task-type CARTESIAN3D :load-increments-count 2 :modified-newton no :max-newton-count 9
   (element-type :gauss-nodes-count 1 :name TETRAHEDRA4 :nodes-count 4)
   (slae-solver :type CG :tolerance 1e-14 :max-iterations 20000)
   (line-search :max 0)
   (arc-length :max 0))
 (input-data
  (geometry
   (nodes
    (0 0 0)
    (1 0 0)
    (0 1 0)
    (0 0 1))
   (elements
    (0 1 2 3)))
  (boundary-conditions
   (prescribed-displacements
    (presc-node :y 0.5 :x 0 :z 0 :type 7 :node-id 3)))))
"""


def test_deck_surface_loads_round_trip(tmp_path):
    src = tmp_path / "loads.sexp"
    src.write_text(DECK_WITH_LOADS)
    d = feahip.Deck.load(str(src))
    assert d.surface_faces.tolist() == [[0, 1, 2], [1, 2, 3]]
    assert d.surface_kind.tolist() == [feahip.LOAD_PRESSURE, feahip.LOAD_TRACTION]
    assert d.surface_values.tolist() == [[0.5, 0.0, 0.0], [0.0, 1.5, -0.25]]
    out = tmp_path / "saved.sexp"
    d.save(str(out))
    assert "(surface-loads" in out.read_text()
    d2 = feahip.Deck.load(str(out))
    for name in ("surface_faces", "surface_kind", "surface_values", "nodes", "elements", "presc_node", "presc_values"):
        assert np.array_equal(getattr(d, name), getattr(d2, name)), name
    out2 = tmp_path / "saved2.sexp"
    d2.save(str(out2))
    assert out2.read_bytes() == out.read_bytes()


def test_deck_without_loads_saves_as_before(tmp_path):
    src = tmp_path / "plain.sexp"
    src.write_text(DECK_WITH_LOADS.replace("""
   (surface-loads
     (pressure :value 0.5 :nodes (0 1 2))
     (traction :x 0 :y 1.5 :z -0.25 :nodes (1 2 3)))""", ""))
    d = feahip.Deck.load(str(src))
    assert len(d.surface_kind) == 0 and d.surface_faces.shape[0] == 0
    out = tmp_path / "saved.sexp"
    d.save(str(out))
    assert out.read_text() == SAVED_WITHOUT_LOADS
    # a Python deck with its loads cleared writes the same bytes
    d.surface_faces, d.surface_kind, d.surface_values = np.zeros((0, 0), np.int32), np.zeros(0, np.int32), np.zeros((0, 3))
    d.save(str(out))
    assert out.read_text() == SAVED_WITHOUT_LOADS


@pytest.mark.parametrize("bad,msg", [("(pressure :nodes (0 1 2))", "pressure needs :value"),
                                     ("(traction :x 1 :nodes (0 1 2))", "traction needs"),
                                     ("(pressure :value 1 :nodes (0 1 2)) (pressure :value 1 :nodes (0 1 2 3))", "same number"),
                                     ("(gravity :value 1)", "expected (pressure")])
def test_bad_surface_load_sections_are_refused(tmp_path, bad, msg):
    src = tmp_path / "bad.sexp"
    src.write_text(DECK_WITH_LOADS.replace("(pressure :value 0.5 :nodes (0 1 2))\n     (traction :x 0 :y 1.5 :z -0.25 :nodes (1 2 3))", bad))
    with pytest.raises(feahip.FeaHipError, match=msg.replace("(", r"\(")):
        feahip.Deck.load(str(src))

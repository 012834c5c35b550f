"""Crafted meshes that drive the GATHER maps of 10-node tetrahedra and 8-node bricks (csrc/gather10.cpp) and of
4-node tetrahedra (csrc/gather.cpp) to their edges: fans around one axis edge, hubs around one node, fans welded into
a lattice.  Shared by the host-side checks (test_gather10_maps_host.py) and the GPU ones (test_gpu_gather10_limits.py),
so that both speak of the same meshes.  Every element has a positive volume."""
import numpy as np

import feahip
import mesh


def quadratic(corners, tets):
    """10-node tetrahedra on 4-node ones: one mid-side node per edge, shared between the elements that share the edge
    (local order of mesh.py)."""
    nodes = [tuple(c) for c in corners]
    mid, out = {}, []
    for e in tets:
        row = list(e)
        for (i, j) in mesh._EDGES:
            key = (min(e[i], e[j]), max(e[i], e[j]))
            if key not in mid:
                mid[key] = len(nodes)
                nodes.append(tuple(0.5 * (np.asarray(corners[key[0]]) + np.asarray(corners[key[1]]))))
            row.append(mid[key])
        out.append(row)
    return np.array(nodes, dtype=np.float64), np.array(out, dtype=np.int32)


def _arc(m, span):
    ang = span * np.arange(m) / (m if span >= 2 * np.pi else m - 1)
    return np.stack([np.cos(ang), np.sin(ang)], axis=1)


def edge_fan_tets(k, origin=(0.0, 0.0, 0.0), radius=1.0, height=1.0):
    """(corners, tets): k linear tetrahedra around the axis edge A = origin, B = origin + height e_z (nodes 0 and 1);
    ring node i at mid height.  A closed ring for k >= 3."""
    o = np.asarray(origin, dtype=np.float64)
    ring = _arc(k, 2 * np.pi) if k >= 3 else _arc(k + 1, 0.9 * np.pi)
    nring = len(ring)
    corners = [o, o + [0.0, 0.0, height]] + [o + [radius * c, radius * s, 0.5 * height] for c, s in ring]
    tets = [[0, 2 + i, 2 + (i + 1) % nring, 1] for i in range(k)]
    return np.array(corners), np.array(tets, dtype=np.int64)


def node_hub_tets(k):
    """(corners, tets): k linear tetrahedra around node 0, grown one at a time over an open ring (so that every count
    is reachable): element 2i above the ring, 2i + 1 below it."""
    m = (k + 1) // 2 + 1
    ring = _arc(m, 1.9 * np.pi)
    corners = [np.zeros(3)] + [np.array([c, s, 0.0]) for c, s in ring] + [np.array([0.0, 0.0, 0.7]), np.array([0.0, 0.0, -0.7])]
    top, bot = m + 1, m + 2
    tets = []
    for i in range(m - 1):
        a, b = 1 + i, 2 + i
        tets.append([0, a, b, top])
        tets.append([0, b, a, bot])
    return np.array(corners), np.array(tets[:k], dtype=np.int64)


def hex_fan(k, closed=True, layers=1):
    """(nodes, bricks): k 8-node bricks around the axis edge x = y = 0, each a prism of the convex quadrilateral
    (axis, ring i, outer i, ring i + 1) -- every brick of a layer holds both axis nodes of that layer.  Open fans
    (closed=False) span 1.9 pi so that every count is reachable; `layers` stacks the fan along z."""
    nr = k if closed else k + 1
    span = 2 * np.pi if closed else 1.9 * np.pi
    step = span / k
    th = step * np.arange(nr)
    ring = np.stack([np.cos(th), np.sin(th)], axis=1)
    outer = 1.5 * np.stack([np.cos(th[:k] + 0.5 * step), np.sin(th[:k] + 0.5 * step)], axis=1)
    per = 1 + nr + k                       # nodes per z level: axis, ring, outer
    nodes = []
    for z in range(layers + 1):
        nodes.append([0.0, 0.0, float(z)])
        nodes += [[x, y, float(z)] for x, y in ring]
        nodes += [[x, y, float(z)] for x, y in outer]
    el = []
    for z in range(layers):
        b0, b1 = z * per, (z + 1) * per
        for i in range(k):
            j = (i + 1) % nr
            q = [0, 1 + i, 1 + nr + i, 1 + j]
            el.append([b0 + v for v in q] + [b1 + v for v in q])
    return np.array(nodes), np.array(el, dtype=np.int32)


def tet10_face_pair(gauss=5):
    """Two 10-node tetrahedra sharing a face (14 nodes): rows of 14 blocks (the shared face) and of 10.  With the
    K tile cut down to a few elements, whole rows of nearly half a tile each take one write-out pass or two."""
    corners = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 1.0, 1.0]])
    return deck_of(*quadratic(corners, np.array([[0, 1, 2, 3], [1, 2, 3, 4]])), 10, gauss)


def hex8_row_of_three(gauss=8):
    """Three bricks in a row (16 nodes): rows of 12 blocks (the two shared faces) and of 8."""
    nodes, el = mesh.hex_block(3, 1, 1, origin=(0.0, 0.0, 0.0), size=(3.0, 1.0, 1.0))
    return deck_of(nodes, el, 8, gauss)


def deck_of(nodes, elements, npe, gauss=None, clamp=None, model=feahip.MODEL_COMPRESSIBLE_NEOHOOKEAN):
    """A deck of the mesh with its lowest-z nodes clamped (K and f do not depend on it; the solve tests do)."""
    ele = {10: feahip.TETRAHEDRA10, 8: feahip.HEXAHEDRA8, 4: feahip.TETRAHEDRA4}[npe]
    g = gauss if gauss is not None else {10: 5, 8: 8, 4: 1}[npe]
    if clamp is None:
        clamp = np.nonzero(nodes[:, 2] <= nodes[:, 2].min() + 1e-12)[0]
    return feahip.Deck(model=model, parameters=[100.0, 100.0], nodes=np.ascontiguousarray(nodes, dtype=np.float64), elements=np.ascontiguousarray(elements, dtype=np.int32),
                       ele_type=ele, gauss_nodes_count=g, presc_node=np.asarray(clamp, dtype=np.int32),
                       presc_type=np.full(len(clamp), 7, dtype=np.int32), presc_values=np.zeros((len(clamp), 3)))


def tet10_edge_fan(k, gauss=5):
    c, t = edge_fan_tets(k)
    return deck_of(*quadratic(c, t), 10, gauss)


def tet10_node_hub(k, gauss=5):
    c, t = node_hub_tets(k)
    return deck_of(*quadratic(c, t), 10, gauss)


def hex8_edge_fan(k, closed=True, layers=1, gauss=8):
    return deck_of(*hex_fan(k, closed, layers), 8, gauss)


def weld(nodes, elements, fan_nodes, fan_elements, fan_axis, edge, scale=0.3):
    """A fan appended to a mesh: the fan's axis nodes fan_axis = (lower, upper) become the mesh's nodes edge = (a, b),
    the rest is scaled (by `scale` times the edge's length across the axis) and turned onto that edge.  The fan's
    elements overlap the mesh's: K and f do not mind, and every volume stays positive.  The two meshes must have the
    same element type.  Returns (nodes, elements)."""
    a, b = nodes[edge[0]], nodes[edge[1]]
    h = np.linalg.norm(b - a)
    ez = (b - a) / h
    ex = np.cross(ez, [1.0, 0.0, 0.0] if abs(ez[0]) < 0.9 else [0.0, 1.0, 0.0])
    ex /= np.linalg.norm(ex)
    R = np.stack([ex, np.cross(ez, ex), ez], axis=1)     # fan frame -> mesh frame, right-handed
    lo = fan_nodes[fan_axis[0]]
    length = np.linalg.norm(fan_nodes[fan_axis[1]] - lo)
    local = (fan_nodes - lo) / length * [scale, scale, 1.0]
    ids = np.full(len(fan_nodes), -1, dtype=np.int64)
    ids[list(fan_axis)] = edge
    rest = np.nonzero(ids < 0)[0]
    ids[rest] = len(nodes) + np.arange(len(rest))
    new_nodes = a + (local[rest] * h) @ R.T
    return np.vstack([nodes, new_nodes]), np.vstack([elements, ids[fan_elements]]).astype(np.int32)


def lattice_edge(nodes, elements, axis=2):
    """An edge of the mesh along `axis`, nearest the middle of the mesh."""
    npe = elements.shape[1]
    pairs = [(0, 3), (1, 2), (0, 1), (0, 2), (1, 3), (2, 3)] if npe in (4, 10) else [(0, 4), (1, 5), (2, 6), (3, 7)]
    centre = nodes.mean(axis=0)
    best, bd = None, None
    for (i, j) in pairs:
        a, b = elements[:, i], elements[:, j]
        d = nodes[b] - nodes[a]
        along = (np.abs(d[:, axis]) > 0) & (np.abs(d).sum(axis=1) - np.abs(d[:, axis]) < 1e-12)
        for e in np.nonzero(along)[0]:
            lo, hi = (a[e], b[e]) if d[e, axis] > 0 else (b[e], a[e])
            dist = np.linalg.norm(0.5 * (nodes[lo] + nodes[hi]) - centre)
            if bd is None or dist < bd:
                best, bd = (int(lo), int(hi)), dist
    return best


def tet_lattice_with_fan(dims, k, quadratic_=True, gauss=5):
    """A Kuhn block of dims cubes with a k-tetrahedron fan welded onto an edge near its middle (along z): the edge's
    block gets the lattice's contributions and k more."""
    nodes, tets = mesh.kuhn_block(*dims, quadratic=False)
    edge = lattice_edge(nodes, tets)
    fc, ft = edge_fan_tets(k)
    nodes, tets = weld(nodes, tets, fc, ft, (0, 1), edge)
    if quadratic_:
        return deck_of(*quadratic(nodes, tets), 10, gauss)
    return deck_of(nodes, tets, 4, 1)


def hex_lattice_with_fan(dims, k, gauss=8):
    """A brick block of dims cubes with a k-brick fan welded onto an edge near its middle (along z)."""
    nodes, el = mesh.hex_block(*dims)
    edge = lattice_edge(nodes, el)
    fn, fe = hex_fan(k)
    per = 1 + 2 * k
    nodes, el = weld(nodes, el, fn, fe, (0, per), edge)
    return deck_of(nodes, el, 8, gauss)


def library_elements(deck):
    """The deck's elements in the node ids a context works in (what the maps are built for)."""
    ids, _ = feahip.host_numbering(deck.elements, deck.nodes)
    return ids[deck.elements]


def shape(deck):
    """host_gather10_shape of the deck as a context numbers it."""
    return feahip.host_gather10_shape(library_elements(deck), len(deck.nodes))

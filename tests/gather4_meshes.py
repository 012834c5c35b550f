"""Crafted meshes of 4-node tetrahedra that drive the GATHER maps of csrc/gather.cpp to the limits of a chunk record
(feahip_internal.h): 256 node slots, 720 element slots, 768 block threads, more than two visits per residual thread,
block and diagonal lists longer than the registers hold, and runs of chunks that are all unlike.  Shared by the host
checks (test_gather4_maps_host.py) and the GPU ones (test_gpu_gather4_limits.py); the fans, hubs and weld() they are
put together from are those of gather10_meshes.py.  Every element has a positive volume."""
import numpy as np

import feahip
import mesh
from gather10_meshes import deck_of, edge_fan_tets, library_elements, node_hub_tets

FLIPS = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)]
HEADER_FIELDS = ("r0", "r1", "b0", "nb", "nnode", "nelem", "noffd", "depth", "nvthr", "vdepth", "ddepth", "wdepth0", "wdepth1",
                 "wdepth2", "flags", "pad")
HEADER = np.dtype([(n, np.uint32 if n.startswith("wdepth") else np.int32) for n in HEADER_FIELDS])
G_MAX_NODES, G_MAX_SLOTS_USED, G_TASK_THREADS, G_REGW, G_MAX_ROWS = 256, 720, 768, 6, 64     # feahip_internal.h
KNOBS = ("FEAHIP_GATHER_ROWS", "FEAHIP_GATHER_ELEMS", "FEAHIP_GATHER_ALPHA")
KNOB_SETTINGS = {"rows1": {"FEAHIP_GATHER_ROWS": 1}, "rows3": {"FEAHIP_GATHER_ROWS": 3}, "elems8": {"FEAHIP_GATHER_ELEMS": 8},
                 "rows64_alpha0": {"FEAHIP_GATHER_ROWS": 64, "FEAHIP_GATHER_ALPHA": 0}}


def positive(nodes, tets):
    """The tetrahedra with the last two nodes swapped wherever the volume comes out negative."""
    p = nodes[tets]
    vol = np.einsum("ei,ei->e", np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), p[:, 3] - p[:, 0])
    assert np.all(np.abs(vol) > 0)
    out = tets.copy()
    out[vol < 0] = tets[vol < 0][:, [0, 1, 3, 2]]
    return out


def multi_kuhn(nx, ny, nz, flips=FLIPS[:1]):
    """(nodes, tets): the unit lattice of (nx+1)(ny+1)(nz+1) points, every cube cut into six Kuhn tetrahedra once per
    entry of `flips`.  A flip mirrors the cube's axes, so that the cut runs along another body diagonal; the
    decompositions overlap (K and f do not mind: gather10_meshes.weld).  len(flips) times the elements around every node
    and edge of a plain Kuhn block."""
    off = mesh._kuhn_corner_offsets()                                   # [6][4][3]
    gx, gz = nx + 1, nz + 1
    j, k, i = np.meshgrid(np.arange(ny + 1), np.arange(nz + 1), np.arange(nx + 1), indexing="ij")
    nodes = np.stack([i.ravel(), j.ravel(), k.ravel()], axis=1).astype(np.float64)      # x fastest, then z, y slowest
    ci, cj, ck = np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij")
    order = np.lexsort((ci.ravel(), ck.ravel(), cj.ravel()))
    cubes = np.stack([ci.ravel()[order], cj.ravel()[order], ck.ravel()[order]], axis=1)
    tets = []
    for flip in flips:
        assert tuple(flip) in FLIPS
        fl = np.asarray(flip)
        o = np.where(fl[None, None, :] == 1, 1 - off, off)
        c = (cubes[:, None, None, :] + o[None]).reshape(-1, 4, 3)
        tets.append((c[:, :, 1] * gz + c[:, :, 2]) * gx + c[:, :, 0])
    return nodes, positive(nodes, np.concatenate(tets).astype(np.int64))


def hub_cluster(H, k):
    """(nodes, tets): H copies of node_hub_tets(k), each with its own nodes, copy h shifted by h (0.013, 0.007, 0.003):
    disconnected bodies that lie in each other, so that a chunk of consecutive rows meets the elements of several hubs
    and runs out of node slots before it runs out of rows."""
    c, t = node_hub_tets(k)
    nodes = np.vstack([c + h * np.array([0.013, 0.007, 0.003]) for h in range(H)])
    tets = np.vstack([t + h * len(c) for h in range(H)])
    return nodes, tets


def join(parts, gap=10.0):
    """(nodes, tets) of the parts side by side along x, `gap` apart, not connected."""
    nodes, tets, x0, n0 = [], [], 0.0, 0
    for c, t in parts:
        c = np.asarray(c, dtype=np.float64)
        nodes.append(c + [x0 - c[:, 0].min(), 0.0, 0.0])
        tets.append(np.asarray(t, dtype=np.int64) + n0)
        x0 = nodes[-1][:, 0].max() + gap
        n0 += len(c)
    return np.vstack(nodes), np.vstack(tets)


def kuhn(nx, ny, nz):
    """A plain Kuhn block of unit cubes."""
    return multi_kuhn(nx, ny, nz)


def chunk_headers(walk):
    """The GatherHeader of every record of a feahip.host_gather_walk result, in walk order, as a record array with the
    fields r0 r1 b0 nb nnode nelem noffd depth nvthr vdepth ddepth wdepth0..2 flags."""
    rec = walk["blob"].reshape(walk["chunks"], walk["stride"])[:, :64]
    return np.ascontiguousarray(rec).view(HEADER).reshape(-1)


def headers(deck, rows=None):
    """chunk_headers of the deck's maps as a context numbers it, under the environment's knobs."""
    return chunk_headers(feahip.host_gather_walk(library_elements(deck), len(deck.nodes), rows=rows))


def wave_depths(h):
    """[chunks][12]: the contribution words the block threads of each wave slot walk."""
    w = np.stack([h["wdepth0"], h["wdepth1"], h["wdepth2"]], axis=1)
    return np.stack([(w[:, s >> 2] >> (8 * (s & 3))) & 255 for s in range(12)], axis=1)


def tet4(part):
    return deck_of(part[0], part[1], 4, 1)


# ---- the meshes, by the edge each is named for (test_gather4_maps_host.py shows that it reaches it)

def composite_parts():
    return [kuhn(5, 5, 5), hub_cluster(6, 90), multi_kuhn(3, 3, 3, FLIPS), edge_fan_tets(50), multi_kuhn(4, 4, 3, FLIPS),
            hub_cluster(4, 120), kuhn(43, 3, 3)]


def small_composite_parts():
    lone = (np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]), np.array([[0, 1, 2, 3]]))
    return [kuhn(3, 3, 3), hub_cluster(6, 90), multi_kuhn(3, 3, 3, FLIPS), edge_fan_tets(50), lone]


CRAFTED = {
    "kuhn333_x3_vdepth3": lambda: tet4(multi_kuhn(3, 3, 3, FLIPS[:3])),
    "kuhn333_x4_vdepth4": lambda: tet4(multi_kuhn(3, 3, 3, FLIPS)),
    "kuhn433_x3_threads": lambda: tet4(multi_kuhn(4, 3, 3, FLIPS[:3])),
    "kuhn443_x4_element_limit": lambda: tet4(multi_kuhn(4, 4, 3, FLIPS)),
    "hubs6x90_node_limit": lambda: tet4(hub_cluster(6, 90)),
    "hubs4x120_nodes_and_threads": lambda: tet4(hub_cluster(4, 120)),
    "composite": lambda: tet4(join(composite_parts())),
}


def small_composite(lone_node=False):
    """The composite of the knob tests: a lattice, hubs, the four-flip block, a fan and one tetrahedron far away; with
    lone_node, one more node that no element refers to, last and clamped."""
    nodes, tets = join(small_composite_parts())
    clamp = np.nonzero(nodes[:, 2] <= nodes[:, 2].min() + 1e-12)[0]
    if lone_node:
        nodes = np.vstack([nodes, [[nodes[:, 0].max() + 10.0, 0.5, 0.5]]])
        clamp = np.append(clamp, len(nodes) - 1)
    return deck_of(nodes, tets, 4, 1, clamp=clamp)


def graded_lattice():
    """A Kuhn block of 4 x 12 x 4 cubes whose y-coordinates are a geometric progression of ratio 2: cell sizes 1 : 2048
    along the bar, 0.25 across it, so that the rows of K at the fine end are about 1e-3 of the largest entry of the matrix."""
    nodes, tets = mesh.kuhn_block(4, 12, 4, origin=(0.0, 0.0, 0.0), size=(1.0, 12.0, 1.0))
    j = np.rint(nodes[:, 1]).astype(np.int64)
    nodes = nodes.copy()
    nodes[:, 1] = 2.0 ** j
    return deck_of(nodes, tets, 4, 1)


def set_chunk_knobs(monkeypatch, settings):
    """The chunk knobs of gather.cpp set to `settings`, the others unset (a context reads them when it builds its maps)."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in settings.items():
        monkeypatch.setenv(k, str(v))

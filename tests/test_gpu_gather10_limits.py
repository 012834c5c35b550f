"""The 10-node / 8-node GATHER assembly (k_state10 + k_assemble_gather10) held to the oracle at the edges of its maps,
on an MI355X.  The meshes are the crafted ones of gather10_meshes.py; test_gather10_maps_host.py shows on the host
that each reaches the edge it is named for.

Bars.  The pattern is bit-exact.  K is checked block row by block row, each against the largest |entry| of the
oracle's row, so that a small row cannot hide under a large one.  f is checked node by node against two scales: the
sum of |element residual| over the node's elements, and the size of the terms summed there, sum over the node's
elements and Gauss points of w |det J| |sigma| |g_a|.  The K-only and f-only launches must give the fused launch's
bits, and the context must report the chunks the host entry describes.

The bars were measured, not guessed, with the row-owner kernel (a plain per-row sum; the atomic scatter where rows
are too long for it) against the oracle on these meshes:
  - K per row: at worst 2.8e-12 (TET10 at 27 points, jittered).  ROW_TOL = 1e-11.
  - f per node against the terms summed: at worst 3.6e-12 (brick_fine).  TERM_TOL = 1e-11.  The gather kernel stayed
    within 2.4x of the row-owner kernel on every case; the differences are those of two codes forming J^-1, the stress
    and the gradients in their own order, largest on the worst-shaped elements.
  - f per node against sum |f_e|: at worst 3.5e-10 (brick_fine).  This scale is small at the corner nodes of 10-node
    tetrahedra: a corner's shape function integrates to zero over every face, so a constant stress puts no force on a
    corner, and f_e there is only the stress's variation across the element -- on brick_fine 6e-4 to 3e-3 of the
    terms summed (mid-side nodes 0.2 to 0.6).  NODE_TOL = 2e-9.
Since those worst cases sit far above most cases' own level, the gather kernel must also stay within NEAR = 10x of
the row-owner kernel's error on the same case and model, or below FLOOR: a missing or
doubled contribution moves a row or a node by O(1) of its scale."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import feahip
import mesh
import gather10_meshes as gm
import oracle_binding
from oracle_binding import OracleSolver

pytestmark = pytest.mark.gpu

ROW_TOL = 1e-11         # K per block row, relative to the row's max |entry| (the oracle's)
NODE_TOL = 2e-9         # f per node, relative to sum_e |f_e| at the node
NEAR, FLOOR = 10.0, 1e-13   # and within 10x of the yardstick kernel's own error on the same case, or below FLOOR
TERM_TOL = 1e-11        # f per node, relative to the sum of |w det J| |sigma| |g_a| over the node's elements and points
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = [feahip.MODEL_COMPRESSIBLE_NEOHOOKEAN, feahip.MODEL_A5]


def deform(nodes):
    """A non-affine deformation at the scale of the mesh: f is not zero, K not that of the reference state."""
    ext = np.ptp(nodes, axis=0)
    ext[ext == 0] = 1.0
    u = np.sin(2.1 * nodes[:, [1, 2, 0]] / ext[[1, 2, 0]]) * np.cos(1.3 * nodes / ext)
    return nodes * np.array([1.02, 0.99, 1.03]) + 0.002 * ext * u


class Want:
    """The oracle's K and f of a deck at nodes x, and the scales every row and node is held to."""

    def __init__(self, deck, x):
        o = OracleSolver(deck)
        o.set_nodes(x)
        o.update_state()
        o.create_stiffness()
        o.create_residual_forces()
        self.off, self.idx = o.offsets().copy(), o.indexes().copy()
        self.K, self.f = o.values().copy(), o.forces().copy()
        self.starts = self.off[0:-1:3]
        self.kscale = np.maximum.reduceat(np.abs(self.K), self.starts)
        fs = np.zeros((len(deck.nodes), 3))
        npe = deck.elements.shape[1]
        for e in range(len(deck.elements)):
            fs[deck.elements[e]] += np.abs(o.element_residual(e)).reshape(npe, 3)
        self.fscale = fs.sum(axis=1)
        # the size of the terms f sums at a node: w |det J| |sigma| |g_a| over its elements' Gauss points
        w, _, _ = oracle_binding.elem_table({10: oracle_binding.TET10, 8: oracle_binding.HEX8, 4: oracle_binding.TET4}[npe],
                                            deck.gauss_nodes_count)
        sn = np.sqrt((o.stresses() ** 2).sum(axis=(2, 3)))
        gn = np.sqrt((o.grads() ** 2).sum(axis=2))
        term = (w[None, :, None] * np.abs(o.detj())[:, :, None] * sn[:, :, None] * gn).sum(axis=1)
        self.tscale = np.zeros(len(deck.nodes))
        np.add.at(self.tscale, deck.elements, term)
        o.close()

    def row_err(self, val):
        d = np.maximum.reduceat(np.abs(val - self.K), self.starts)
        return float((d / np.where(self.kscale > 0, self.kscale, 1.0)).max())

    def node_err(self, f):
        d = np.abs(f - self.f).reshape(-1, 3).max(axis=1)
        return float((d / np.where(self.fscale > 0, self.fscale, 1.0)).max())

    def term_err(self, f):
        d = np.abs(f - self.f).reshape(-1, 3).max(axis=1)
        return float((d / np.where(self.tscale > 0, self.tscale, 1.0)).max())


def assemble(s, strategy, want, label):
    s.set_assembly(strategy)
    s.create_stiffness_and_residual()
    assert s.assembly_in_use() == strategy, label
    off, idx, val = s.matrix_yale()
    assert np.array_equal(off, want.off) and np.array_equal(idx, want.idx), label
    return val.copy(), s.forces().copy()


def yardstick(s):
    """The kernel the gather kernel is measured beside: the row owner (a plain per-row sum), or the atomic scatter
    where a block row is longer than the row owner's 128-block tile."""
    try:
        s.set_assembly(feahip.ASM_ROWOWNER)
        s.create_stiffness_and_residual()
        return feahip.ASM_ROWOWNER
    except feahip.FeaHipError:
        return feahip.ASM_ATOMIC


def check_case(label, deck, x=None, shared=True):
    """Every model: GATHER against the oracle (fused, K-only, f-only), ROW_OWNER measured, SHARED where it builds."""
    x = deform(deck.nodes) if x is None else x
    for model in MODELS:
        deck.model = model
        want = Want(deck, x)
        s = feahip.FeaSolver(deck)
        s.set_nodes(x)
        try:
            K, f = assemble(s, feahip.ASM_GATHER, want, label)
            ek, ef, et = want.row_err(K), want.node_err(f), want.term_err(f)
            assert s.assembly_stats()["chunks"] == gm.shape(deck)["chunks"], label   # the maps the host entry describes
            Kr, fr = assemble(s, yardstick(s), want, label)
            rk, rf, rt = want.row_err(Kr), want.node_err(fr), want.term_err(fr)
            print(f"\n{label} model {model}: gather K row {ek:.2e} f node {ef:.2e} term {et:.2e} | "
                  f"yardstick K row {rk:.2e} f node {rf:.2e} term {rt:.2e}")
            assert et < TERM_TOL and rt < TERM_TOL, f"{label} model {model}: f term error {et:.2e} ({rt:.2e})"
            assert ek < ROW_TOL and ek <= max(NEAR * rk, FLOOR), f"{label} model {model}: K row error {ek:.2e} ({rk:.2e})"
            assert ef < NODE_TOL and ef <= max(NEAR * rf, FLOOR), f"{label} model {model}: f node error {ef:.2e} ({rf:.2e})"
            assert rk < ROW_TOL and rf < NODE_TOL, label
            s.set_assembly(feahip.ASM_GATHER)
            s.create_stiffness()                                     # K only
            assert s.assembly_in_use() == feahip.ASM_GATHER
            assert np.array_equal(s.matrix_yale()[2], K), label
            s.create_residual_forces()                               # f only
            assert s.assembly_in_use() == feahip.ASM_GATHER
            assert np.array_equal(s.forces(), f), label
            assert np.array_equal(s.matrix_yale()[2], K), label       # the f-only launch leaves K alone
            if shared and deck.elements.shape[1] == 10:
                try:
                    s.set_assembly(feahip.ASM_SHARED)
                    s.create_stiffness_and_residual()
                except feahip.FeaHipError:
                    shared = False                                    # its maps do not build for this mesh
                else:
                    assert s.assembly_in_use() == feahip.ASM_SHARED
                    off, idx, val = s.matrix_yale()
                    assert np.array_equal(off, want.off) and np.array_equal(idx, want.idx)
                    assert want.row_err(val) < ROW_TOL and want.node_err(s.forces()) < NODE_TOL, label
                    s.set_assembly(feahip.ASM_GATHER)
        finally:
            s.close()


# ---- the crafted meshes of test_gather10_maps_host.py

CRAFTED = {
    "tet10_fan9": lambda: gm.tet10_edge_fan(9),
    "tet10_fan12": lambda: gm.tet10_edge_fan(12),
    "tet10_hub127_element_limit": lambda: gm.tet10_node_hub(127),
    "tet10_lattice_with_fan": lambda: gm.tet_lattice_with_fan((3, 8, 3), 12),
    "tet10_lattice_fdw2": lambda: mesh.bar_deck(dims=(3, 8, 3), quadratic=True),
    "hex8_fan12": lambda: gm.hex8_edge_fan(12),
    "hex8_fan87_row_length_limit": lambda: gm.hex8_edge_fan(87, closed=False),
    "hex8_lattice_with_fan": lambda: gm.hex_lattice_with_fan((4, 12, 4), 12),
    "hex8_lattice_fdw2": lambda: gm.deck_of(*mesh.hex_block(6, 12, 6), 8),
}


@pytest.mark.parametrize("name", list(CRAFTED))
def test_crafted_mesh(name):
    deck = CRAFTED[name]()
    assert gm.shape(deck)["ok"]
    check_case(name, deck)


@pytest.mark.parametrize("case", ["tet10", "hex8"])
def test_seven_write_out_passes(case, monkeypatch):
    """FEAHIP_GATHER10_ELEMS=5: whole rows of nearly half a 33-block (26 for bricks) tile, seven passes through it per
    chunk -- the last one decoded from the header's second pass word."""
    deck = gm.tet10_face_pair() if case == "tet10" else gm.hex8_row_of_three()
    monkeypatch.setenv("FEAHIP_GATHER10_ELEMS", "5")
    assert gm.shape(deck)["max_passes"] == 7
    check_case(f"{case}_seven_passes", deck, shared=False)


@pytest.mark.parametrize("gauss", [4, 5, 27])
def test_tet10_gauss_rules(gauss):
    """4 and 5 points keep the shape-gradient table in LDS, 27 reads it through the cache (the other variant)."""
    deck = mesh.jitter_permute(mesh.bar_deck(dims=(2, 6, 2), quadratic=True, gauss=gauss))
    check_case(f"tet10_g{gauss}", deck)


def test_hex8_jittered_permuted_block():
    deck = mesh.jitter_permute(mesh.bar_deck(dims=(4, 10, 4), hexa=True))
    check_case("hex8_jittered", deck)


def _brick_fine(tmp_path):
    import shutil
    p = tmp_path / "brick_fine.sexp"
    with gzip.open(os.path.join(ROOT, "tests", "golden", "decks", "brick_fine.sexp.gz"), "rb") as src, open(p, "wb") as dst:
        shutil.copyfileobj(src, dst)
    deck = feahip.Deck.load(str(p))
    deck.presc_node = (deck.presc_node - 1).astype(np.int32)
    return deck


def test_brick_fine_every_row(tmp_path):
    """The unstructured TetGen deck in full (22 934 TET10, 5 points): every block row, every node."""
    deck = _brick_fine(tmp_path)
    check_case("brick_fine", deck, shared=False)


def test_brick_fine_piece_at_27_points(tmp_path):
    """A piece of brick_fine (the elements of the first ninth along the bar) at 27 points: the oracle takes 25 s for
    the full deck at that rule, the piece keeps the file's time budget."""
    deck = _brick_fine(tmp_path)
    c = deck.nodes[deck.elements[:, :4]].mean(axis=1)
    y0, y1 = deck.nodes[:, 1].min(), deck.nodes[:, 1].max()
    keep = c[:, 1] < y0 + (y1 - y0) / 9.0
    used = np.unique(deck.elements[keep])
    new = np.full(len(deck.nodes), -1, dtype=np.int64)
    new[used] = np.arange(len(used))
    piece = gm.deck_of(deck.nodes[used], new[deck.elements[keep]], 10, gauss=27)
    assert len(piece.elements) > 2000
    check_case("brick_fine_piece_g27", piece, shared=False)


# ---- run length: tuning only, the bits must not move

CHILD = r"""
import sys, numpy as np
sys.path[:0] = [{pkg!r}, {tests!r}]
import feahip, mesh, gather10_meshes as gm
from test_gpu_gather10_limits import MESHES_FOR_RUNS, deform
deck, strategy = MESHES_FOR_RUNS[{name!r}]()
x = deform(deck.nodes)
s = feahip.FeaSolver(deck)
s.set_nodes(x)
s.set_assembly(strategy)
s.create_stiffness_and_residual()
assert s.assembly_in_use() == strategy
np.savez({out!r}, off=s.matrix_yale()[0], K=s.matrix_yale()[2], f=s.forces())
s.close()
"""

MESHES_FOR_RUNS = {
    "tet10": lambda: (gm.tet_lattice_with_fan((3, 8, 3), 12), feahip.ASM_GATHER),
    "hex8": lambda: (gm.hex_lattice_with_fan((4, 12, 4), 12), feahip.ASM_GATHER),
    "tet4": lambda: (gm.tet_lattice_with_fan((3, 60, 3), 50, quadratic_=False), feahip.ASM_GATHER),
    "tet10_shared": lambda: (gm.tet_lattice_with_fan((3, 8, 3), 12), feahip.ASM_SHARED),
}
RUN_KNOB = {"tet10": "FEAHIP_GATHER10_RUN", "hex8": "FEAHIP_GATHER10_RUN", "tet4": "FEAHIP_GATHER_RUN",
            "tet10_shared": "FEAHIP_QUAD_RUN"}


def _child(name, tmp_path, tag, run):
    out = str(tmp_path / f"{name}_{tag}.npz")
    script = tmp_path / f"child_{name}_{tag}.py"
    script.write_text(CHILD.format(pkg=os.path.join(ROOT, "fea-large_amd"), tests=os.path.join(ROOT, "tests"), name=name, out=out))
    env = dict(os.environ)
    for k in set(RUN_KNOB.values()):
        env.pop(k, None)
    if run is not None:
        env[RUN_KNOB[name]] = str(run)
    res = subprocess.run([sys.executable, str(script)], env=env, timeout=120, capture_output=True, text=True)
    assert res.returncode == 0, f"{name} run={run}: exit {res.returncode}\n{res.stderr[-2000:]}"
    return np.load(out)


@pytest.mark.parametrize("name", list(MESHES_FOR_RUNS))
def test_run_length_leaves_the_bits(name, tmp_path):
    """The run length is read once per process (a function-local static): one fresh child per setting, one at a
    time; a child that fails or hangs fails the test before the next one starts."""
    deck, strategy = MESHES_FOR_RUNS[name]()
    if strategy == feahip.ASM_GATHER and name != "tet4":
        nch = gm.shape(deck)["chunks"]
    elif name == "tet4":
        nch = feahip.host_gather_stats(gm.library_elements(deck), len(deck.nodes))[0]["chunks"]
    else:
        nch = 4096                                            # more than the shared-state maps' chunks
    assert nch % 8 != 0 or name == "tet10_shared"
    base = _child(name, tmp_path, "default", None)
    for run in (1, 3, nch + 1):
        got = _child(name, tmp_path, f"run{run}", run)
        if strategy == feahip.ASM_GATHER:
            assert np.array_equal(got["K"], base["K"]), f"{name}: K moved with run length {run}"
            assert np.array_equal(got["f"], base["f"]), f"{name}: f moved with run length {run}"
        else:
            # the shared-state kernel sums a chunk's blocks with LDS atomics: its bits are not those of one fixed
            # order even at one run length, so it is held per block row to the bar of the oracle comparisons
            st = base["off"][0:-1:3]
            d = np.maximum.reduceat(np.abs(got["K"] - base["K"]), st) / np.maximum.reduceat(np.abs(base["K"]), st)
            assert d.max() < ROW_TOL, f"{name}: K moved with run length {run}: {d.max():.2e}"
            assert np.abs(got["f"] - base["f"]).max() <= ROW_TOL * np.abs(base["f"]).max()


def test_tet4_overflow_lists_inside_a_run():
    """4-node gather: a 50-tetrahedron fan welded into a long TET4 lattice -- more than 12 contributions on the axis
    edge's block and more than 48 elements around its nodes -- in a run of chunks where others repeat their
    predecessor's map words (test_gather10_maps_host.py).  Every block row against the oracle."""
    deck = gm.tet_lattice_with_fan((3, 60, 3), 50, quadratic_=False)
    flags = feahip.host_gather_chunks(gm.library_elements(deck), len(deck.nodes))
    over = np.nonzero(flags & 6)[0]
    assert any(p >= 2 and flags[p - 2] & 1 for p in over)       # right after a chunk that repeats its predecessor
    x = deform(deck.nodes)
    for model in MODELS:
        deck.model = model
        want = Want(deck, x)
        s = feahip.FeaSolver(deck)
        s.set_nodes(x)
        try:
            K, f = assemble(s, feahip.ASM_GATHER, want, "tet4_fan")
            Kr, fr = assemble(s, yardstick(s), want, "tet4_fan")
            print(f"\ntet4_fan model {model}: gather K row {want.row_err(K):.2e} f node {want.node_err(f):.2e} | "
                  f"row-owner K row {want.row_err(Kr):.2e} f node {want.node_err(fr):.2e}")
            assert want.row_err(K) < ROW_TOL and want.row_err(K) <= max(NEAR * want.row_err(Kr), FLOOR)
            assert want.node_err(f) < NODE_TOL and want.node_err(f) <= max(NEAR * want.node_err(fr), FLOOR)
            assert want.term_err(f) < TERM_TOL
            s.set_assembly(feahip.ASM_GATHER)
            s.create_stiffness()
            assert np.array_equal(s.matrix_yale()[2], K)
            s.create_residual_forces()                 # the 4-node f-only launch sums in another order: the oracle's bar
            fo = want.node_err(s.forces())
            assert fo < NODE_TOL and fo <= max(NEAR * want.node_err(fr), FLOOR)
        finally:
            s.close()

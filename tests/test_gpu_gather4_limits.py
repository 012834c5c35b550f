"""The linear-tet GATHER assembly (k_assemble_gather, csrc/kernels_gather.hip; maps of csrc/gather.cpp) held to the
oracle at the limits of its maps, on an MI355X.  The meshes are the crafted ones of gather4_meshes.py;
test_gather4_maps_host.py shows on the host that each reaches the limit it is named for: 256 node slots, 720 element
slots, 768 block threads, three and four visits per residual thread (the visit loop of the f-only kernel), lists longer
than the registers, chunks of one row and of no element, and one run that walks through all of them.

Bars: those of test_gpu_gather10_limits.py, and its helpers.  The pattern is bit-exact.  K is checked block row by
block row against the largest |entry| of the oracle's row; f node by node against the sum of |element residual| at the
node and against the size of the terms summed there.  No scale is capped: on every mesh here each row's and node's
scale is positive (asserted).  The K-only launch gives the fused launch's bits; the f-only launch sums the visits in
another order and is held to the oracle's bar.  Beside ROW_TOL, NODE_TOL and TERM_TOL the gather kernel must stay
within NEAR = 10x of the yardstick kernel (the row owner, or the atomic scatter where a row exceeds its tile) on the
same case and model, or below FLOOR.

Measured on an MI355X against the oracle, worst of the two models: gather | yardstick (the row owner: the longest block row
here has 64 blocks, half its tile).
                                   K per row            f per node           f per term           f alone, node / term
  kuhn333_x3_vdepth3               9.1e-16 | 1.4e-15    6.9e-15 | 7.3e-15    3.9e-15 | 5.2e-15    6.7e-15 / 3.8e-15
  kuhn333_x4_vdepth4               8.0e-16 | 1.0e-15    7.3e-15 | 6.5e-15    4.5e-15 | 4.0e-15    7.1e-15 / 4.4e-15
  kuhn433_x3_threads               8.8e-16 | 9.1e-16    7.5e-15 | 8.9e-15    5.4e-15 | 6.4e-15    7.8e-15 / 5.6e-15
  kuhn443_x4_element_limit         7.7e-16 | 9.1e-16    8.1e-15 | 1.1e-14    5.0e-15 | 6.4e-15    7.1e-15 / 4.3e-15
  hubs6x90_node_limit              1.9e-15 | 2.4e-15    4.3e-14 | 4.4e-14    2.2e-14 | 2.2e-14    4.3e-14 / 2.2e-14
  hubs4x120_nodes_and_threads      3.9e-15 | 3.3e-15    5.9e-14 | 7.2e-14    3.0e-14 | 2.6e-14    5.8e-14 / 3.0e-14
  composite                        6.1e-14 | 6.1e-14    2.2e-12 | 2.2e-12    1.1e-12 | 1.1e-12    2.2e-12 / 1.1e-12
  composite, two materials         8.2e-14 | 8.3e-14    2.7e-12 | 2.7e-12    1.3e-12 | 1.3e-12    2.7e-12 / 1.3e-12
  composite, either row shard      6.1e-14 | 6.1e-14    2.2e-12 | 2.2e-12    1.1e-12 | 1.1e-12
  small composite, every knob      3.0e-14 | 3.1e-14    1.0e-12 | 1.0e-12    6.8e-13 | 6.9e-13    1.0e-12 / 6.8e-13
  graded lattice                   9.7e-13 | 4.9e-13    3.0e-12 | 3.5e-12    2.6e-13 | 2.1e-13    3.0e-12 / 2.6e-13
The yardstick's worst values (4.9e-13 per row, 3.5e-12 per node, 1.3e-12 per term) stay below a third of ROW_TOL = 1e-11,
NODE_TOL = 2e-9 and TERM_TOL = 1e-11, so every mesh keeps those bars; the gather kernel stayed within 2x of the yardstick
everywhere.  The composites' figures are those of coordinates far from the origin (parts side by side along x, 10 apart:
the edge vectors x_k - x_0 lose the digits the offset takes), the same for both kernels and under every cut of the rows;
the graded lattice's K figure is the A5 model's under a shear of 17.
"""
import functools

import numpy as np
import pytest

import feahip
import gather4_meshes as g4
import oracle_binding
from hetero_reference import MATERIALS, HeteroRestatement, with_materials
from test_gpu_gather10_limits import FLOOR, MODELS, NEAR, NODE_TOL, ROW_TOL, TERM_TOL, Want, assemble, deform, yardstick
from test_gpu_gather_walk import assembled, same_bits

pytestmark = pytest.mark.gpu

CASES = dict(g4.CRAFTED, small=g4.small_composite, graded=g4.graded_lattice)


@pytest.fixture(autouse=True)
def default_knobs(monkeypatch):
    """Every test starts from the defaults of the chunk and walk knobs."""
    g4.set_chunk_knobs(monkeypatch, {})
    for k in ("FEAHIP_GATHER_ORDER", "FEAHIP_GATHER_BALANCE", "FEAHIP_GATHER_RUN", "FEAHIP_GATHER_NRUNS"):
        monkeypatch.delenv(k, raising=False)


def positive_scales(want):
    assert np.all(want.kscale > 0) and np.all(want.fscale > 0) and np.all(want.tscale > 0)


@functools.lru_cache(maxsize=None)
def reference(name, model):
    """(deck, x, the oracle's K, f and scales) -- computed once, shared, never written to."""
    deck = CASES[name]()
    deck.model = model
    x = deform(deck.nodes)
    want = Want(deck, x)
    positive_scales(want)
    for a in (x, want.off, want.idx, want.K, want.f, want.kscale, want.fscale, want.tscale):
        a.setflags(write=False)
    return deck, x, want


class Errors:
    """K per block row and f per node against the oracle's scales; `nodes`: the (caller's) nodes looked at."""

    def __init__(self, want, K, f, nodes=None):
        nnz, ndof = len(want.K), len(want.f)
        rk = np.maximum.reduceat(np.abs(K[:nnz] - want.K), want.starts) / want.kscale
        d = np.abs(f[:ndof] - want.f).reshape(-1, 3).max(axis=1)
        sel = slice(None) if nodes is None else nodes
        self.row, self.node, self.term = float(rk[sel].max()), float((d / want.fscale)[sel].max()), float((d / want.tscale)[sel].max())


def hold(label, model, want, got, yard, f_alone=None, nodes=None):
    """The bars of this file on one assembly: print the figures, then assert."""
    g, y = Errors(want, *got, nodes=nodes), Errors(want, *yard, nodes=nodes)
    a = Errors(want, got[0], f_alone, nodes=nodes) if f_alone is not None else None
    print(f"\n{label} model {model}: gather K row {g.row:.2e} f node {g.node:.2e} term {g.term:.2e} | "
          f"yardstick K row {y.row:.2e} f node {y.node:.2e} term {y.term:.2e}" +
          (f" | f alone node {a.node:.2e} term {a.term:.2e}" if a else ""))
    row_tol, node_tol, term_tol = ROW_TOL, NODE_TOL, TERM_TOL
    assert y.row < row_tol and y.node < node_tol and y.term < term_tol, f"{label} model {model}: the yardstick"
    assert g.row < row_tol and g.row <= max(NEAR * y.row, FLOOR), f"{label} model {model}: K row error {g.row:.2e} ({y.row:.2e})"
    assert g.node < node_tol and g.node <= max(NEAR * y.node, FLOOR), f"{label} model {model}: f node error {g.node:.2e} ({y.node:.2e})"
    assert g.term < term_tol and g.term <= max(NEAR * y.term, FLOOR), f"{label} model {model}: f term error {g.term:.2e} ({y.term:.2e})"
    if a:
        assert a.node < node_tol and a.node <= max(NEAR * y.node, FLOOR), f"{label} model {model}: f alone, node error {a.node:.2e} ({y.node:.2e})"
        assert a.term < term_tol and a.term <= max(NEAR * y.term, FLOOR), f"{label} model {model}: f alone, term error {a.term:.2e} ({y.term:.2e})"


def three_launches(s, want, label):
    """(K, f) of the fused launch, f of the f-only launch; the K-only launch must give the fused launch's bits and the
    f-only launch must leave K alone."""
    K, f = assemble(s, feahip.ASM_GATHER, want, label)
    s.create_stiffness()
    assert s.assembly_in_use() == feahip.ASM_GATHER
    assert np.array_equal(s.matrix_yale()[2], K), f"{label}: K alone"
    s.create_residual_forces()
    assert s.assembly_in_use() == feahip.ASM_GATHER
    f_alone = s.forces().copy()
    assert np.array_equal(s.matrix_yale()[2], K), f"{label}: the f-only launch wrote K"
    return K, f, f_alone


def check_mesh(name, model):
    deck, x, want = reference(name, model)
    chunks = len(g4.headers(deck))
    s = feahip.FeaSolver(deck)
    try:
        s.set_nodes(x)
        assert s.update_state() == 0
        K, f, f_alone = three_launches(s, want, name)
        assert s.assembly_stats()["chunks"] == chunks, name         # the maps the host entry describes
        yard = assemble(s, yardstick(s), want, name)
        hold(name, model, want, (K, f), yard, f_alone)
    finally:
        s.close()


# ---- a. each crafted mesh alone, and the composite

@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("name", list(g4.CRAFTED))
def test_crafted_mesh(name, model):
    check_mesh(name, model)


# ---- b. the composite under the walk

@pytest.mark.parametrize("model", MODELS)
def test_composite_walked_by_one_workgroup(model, monkeypatch):
    """One workgroup walks all chunks in row order -- from a brick to a chunk cut by the node limit to a 720-slot chunk
    and back, each handing the next its coordinates and header -- against every chunk in a run of its own: the same bits."""
    deck, x, want = reference("composite", model)
    each = assembled(monkeypatch, deck, x, {"FEAHIP_GATHER_NRUNS": 64})
    assert each["stats"]["chunks"] == len(g4.headers(deck))
    one = assembled(monkeypatch, deck, x, {"FEAHIP_GATHER_ORDER": 0, "FEAHIP_GATHER_NRUNS": 1})
    assert one["stats"]["chunks"] == each["stats"]["chunks"] and one["stats"]["chunks_with_predecessors_words"] >= 1
    grouped = assembled(monkeypatch, deck, x, {"FEAHIP_GATHER_NRUNS": 1})
    dflt = assembled(monkeypatch, deck, x, {})                   # the defaults: equal chunks adjacent, runs cut by cost for the device
    assert np.array_equal(each["off"], want.off) and np.array_equal(each["idx"], want.idx)
    for label, got in (("one run in row order", one), ("one run, equal chunks adjacent", grouped), ("defaults", dflt)):
        for k in ("K", "f", "K_alone", "f_alone"):
            assert np.array_equal(got[k], each[k]), f"composite model {model}, {label}: {k} moved"
        assert same_bits(got, each)
    e = Errors(want, each["K"], each["f"])
    assert e.row < ROW_TOL and e.node < NODE_TOL and e.term < TERM_TOL


# ---- c. the small composite under the row and element knobs

def with_lone_pattern(want, off, idx):
    """The oracle's pattern of the mesh without the lone node, plus its one block."""
    nnz, ndof = len(want.K), len(want.f)
    return (np.array_equal(off[:ndof + 1], want.off) and np.array_equal(off[ndof + 1:], nnz + np.array([3, 6, 9])) and
            np.array_equal(idx[:nnz], want.idx) and np.array_equal(idx[nnz:], np.tile(ndof + np.arange(3), 3)))


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("lone", [False, True], ids=["plain", "lone_node"])
@pytest.mark.parametrize("knob", list(g4.KNOB_SETTINGS))
def test_small_composite_under_the_chunk_knobs(knob, lone, model, monkeypatch):
    """Another cut of the rows sums a block and its mirror with the roles of a and b exchanged where the two rows fall
    into different chunks: no bits to compare, every setting against the oracle.  lone_node: one more node that no
    element refers to, the last one -- under FEAHIP_GATHER_ROWS=1 a chunk with no element."""
    deck, x, want = reference("small", model)
    nnz, ndof = len(want.K), len(want.f)
    if lone:
        deck = g4.small_composite(lone_node=True)
        deck.model = model
        x = np.vstack([x, deck.nodes[-1:]])
    g4.set_chunk_knobs(monkeypatch, g4.KNOB_SETTINGS[knob])
    chunks = len(g4.headers(deck))
    s = feahip.FeaSolver(deck)
    try:
        s.set_nodes(x)
        assert s.update_state() == 0
        s.set_assembly(feahip.ASM_GATHER)
        s.create_stiffness_and_residual()
        assert s.assembly_in_use() == feahip.ASM_GATHER and s.assembly_stats()["chunks"] == chunks
        off, idx, K = s.matrix_yale()
        f = s.forces().copy()
        if lone:
            assert with_lone_pattern(want, off, idx)
            assert np.all(K[nnz:] == 0) and np.all(f[ndof:] == 0)       # nine zeros, and three
        else:
            assert np.array_equal(off, want.off) and np.array_equal(idx, want.idx)
        s.create_stiffness()
        assert np.array_equal(s.matrix_yale()[2], K)
        s.create_residual_forces()
        f_alone = s.forces().copy()
        assert np.all(f_alone[ndof:] == 0)
        s.set_assembly(yardstick(s))
        s.create_stiffness_and_residual()
        yard = (s.matrix_yale()[2].copy(), s.forces().copy())
        hold(f"small {knob}{' lone node' if lone else ''}", model, want, (K, f), yard, f_alone)
    finally:
        s.close()


# ---- d. two materials at the limits

@functools.lru_cache(maxsize=None)
def hetero_reference_of_composite(model):
    """The composite with two materials alternating by element index (every element slot range carries both ids): the
    oracle's restatement, and the scales of Want from the solver of every element's own material."""
    deck, x, homog = reference("composite", model)
    ids = (np.arange(len(deck.elements)) % 2).astype(np.int32)
    r = HeteroRestatement(deck, MATERIALS[:2], ids)
    K, f, _, _ = r.assemble(x)
    assert r.bad == 0
    want = Want.__new__(Want)
    want.off, want.idx = homog.off, homog.idx
    want.K, want.f = r.yale_values(K, homog.off, homog.idx), f
    del K
    want.starts = homog.starts
    want.kscale = np.maximum.reduceat(np.abs(want.K), want.starts)
    fs = np.zeros((len(deck.nodes), 3))
    for e in range(len(deck.elements)):
        fs[deck.elements[e]] += np.abs(r.solvers[ids[e]].element_residual(e)).reshape(4, 3)
    want.fscale = fs.sum(axis=1)
    w, _, _ = oracle_binding.elem_table(oracle_binding.TET4, deck.gauss_nodes_count)
    terms = []
    for o in r.solvers:
        sn = np.sqrt((o.stresses() ** 2).sum(axis=(2, 3)))
        gn = np.sqrt((o.grads() ** 2).sum(axis=2))
        terms.append((w[None, :, None] * np.abs(o.detj())[:, :, None] * sn[:, :, None] * gn).sum(axis=1))
    term = np.where((ids == 0)[:, None], terms[0], terms[1])
    want.tscale = np.zeros(len(deck.nodes))
    np.add.at(want.tscale, deck.elements, term)
    r.close()
    positive_scales(want)
    for a in (want.K, want.f, want.kscale, want.fscale, want.tscale):
        a.setflags(write=False)
    return with_materials(deck, MATERIALS[:2], ids), x, want, homog


@pytest.mark.parametrize("model", MODELS)
def test_two_materials_at_the_limits(model):
    """The material id of an element slot is one byte of the record's last section, read by thread id: slots up to 719
    carry both ids here.  With a table the K-only request of the A5 model runs the fused kernel with the residual sent
    to a vector nobody reads: K is the fused launch's to the bit, and f stays what it was."""
    deck, x, want, homog = hetero_reference_of_composite(model)
    s = feahip.FeaSolver(deck)
    try:
        s.set_nodes(x)
        K, f = assemble(s, feahip.ASM_GATHER, want, "two materials")
        assert not np.array_equal(K, homog.K)                      # the table is in use
        s.create_stiffness()
        assert s.assembly_in_use() == feahip.ASM_GATHER
        assert np.array_equal(s.matrix_yale()[2], K), "two materials: K alone"
        assert np.array_equal(s.forces(), f), "two materials: the K-only request wrote f"
        s.create_residual_forces()
        f_alone = s.forces().copy()
        assert np.array_equal(s.matrix_yale()[2], K)
        yard = assemble(s, yardstick(s), want, "two materials")
        hold("composite, two materials", model, want, (K, f), yard, f_alone)
    finally:
        s.close()


# ---- e. row shards

@pytest.mark.parametrize("model", MODELS)
def test_composite_in_two_row_shards(model):
    deck, x, want = reference("composite", model)
    el = g4.library_elements(deck)
    s = feahip.FeaSolver(deck)
    try:
        s.set_nodes(x)
        yard = assemble(s, yardstick(s), want, "shards")          # the whole mesh: a row's sum does not depend on the shard
        s.set_assembly(feahip.ASM_GATHER)
        seen = np.zeros(len(deck.nodes), dtype=int)
        for r in (0, 1):
            s.set_row_shard(r, 2)
            s.create_stiffness_and_residual()
            assert s.assembly_in_use() == feahip.ASM_GATHER
            rows = s.owned_rows()
            assert s.assembly_stats()["chunks"] == feahip.host_gather_walk(el, len(deck.nodes), rows=rows)["chunks"]
            off, idx, K = s.matrix_yale()
            assert np.array_equal(off, want.off) and np.array_equal(idx, want.idx)
            own = s.owned_nodes()
            seen[own] += 1
            mine = np.zeros(s.ndof, dtype=bool)
            mine[s.owned_dofs()] = True
            assert np.all(K[~mine[np.repeat(np.arange(s.ndof), np.diff(off))]] == 0)
            hold(f"composite shard {r} of 2", model, want, (K, s.forces().copy()), yard, nodes=own)
        assert np.all(seen == 1)
    finally:
        s.close()


# ---- f. a graded lattice

@pytest.mark.parametrize("model", MODELS)
def test_graded_lattice_every_row(model):
    """Cell sizes 1 : 2048 along the bar: the rows at the fine end are orders of magnitude below the largest entry of
    the matrix, where a comparison in the maximum norm sees nothing of them."""
    deck, x, want = reference("graded", model)
    assert want.kscale.min() < 1e-3 * want.kscale.max()
    check_mesh("graded", model)

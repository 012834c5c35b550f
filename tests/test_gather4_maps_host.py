"""Host side of the 4-node GATHER maps (csrc/gather.cpp), no device: the crafted meshes of gather4_meshes.py reach the
limits of a chunk record they are named for.  test_gpu_gather4_limits.py assembles the same meshes on the GPU; these
checks keep it honest -- a GPU test of a limit the maps never reach proves nothing about that limit.

Limits of a chunk record (feahip_internal.h, gather.cpp):
  - 256 node slots (8-bit chunk-local node ids), 64 rows;
  - 720 element slots: FEA_G_MAX_ELEMS = 719 elements and the all-zero record, in sixteens;
  - 768 block threads (wave slots 0-11, the last four under GatherHeader::wdepth[2]);
  - FEA_G_REGW = 6 contribution words per block thread and per diagonal lane in registers, longer lists read inside
    the gather phase;
  - two visits per residual thread in registers (the f-only kernel), further ones read inside its visit loop.
The maps are built in the node numbering a context uses (library ids), so every mesh is looked at in it, through the
GatherHeader of every record of feahip.host_gather_walk (gather4_meshes.chunk_headers)."""
import functools

import numpy as np
import pytest

import feahip
import mesh
import gather4_meshes as g4
from gather4_meshes import G_MAX_NODES, G_MAX_ROWS, G_MAX_SLOTS_USED, G_REGW, G_TASK_THREADS


@functools.lru_cache(maxsize=None)
def crafted(name):
    deck = g4.CRAFTED[name]()
    h = g4.headers(deck)
    h.setflags(write=False)
    return deck, h


def rows(h):
    return h["r1"] - h["r0"]


@pytest.fixture(autouse=True)
def default_knobs(monkeypatch):
    g4.set_chunk_knobs(monkeypatch, {})
    for k in ("FEAHIP_GATHER_ORDER", "FEAHIP_GATHER_BALANCE", "FEAHIP_GATHER_RUN", "FEAHIP_GATHER_NRUNS"):
        monkeypatch.delenv(k, raising=False)


def test_chunk_headers_are_the_records_headers():
    """The decoded headers cover the rows and the blocks of the matrix once, in walk order, and agree with what the
    other host entries say about the same maps."""
    deck, h = crafted("composite")
    el = g4.library_elements(deck)
    w = feahip.host_gather_walk(el, len(deck.nodes))
    assert len(h) == w["chunks"] == feahip.host_gather_stats(el, len(deck.nodes))[0]["chunks"]
    order = np.argsort(h["r0"])
    assert h["r0"][order][0] == 0 and h["r1"][order][-1] == len(deck.nodes)
    assert np.array_equal(h["r1"][order][:-1], h["r0"][order][1:])
    assert np.array_equal((h["b0"] + h["nb"])[order][:-1], h["b0"][order][1:])
    assert np.array_equal(h["flags"] & 1, feahip.host_gather_chunks(el, len(deck.nodes)) & 1)
    assert int((h["flags"] & 1).sum()) == w["chunks_with_predecessors_words"]
    assert np.all(h["nelem"] % 16 == 0) and np.all(h["nnode"] % 16 == 0) and np.all(h["pad"] == 0)
    assert np.array_equal(g4.wave_depths(h).max(axis=1), h["depth"])


@pytest.mark.parametrize("name,vdepth", [("kuhn333_x3_vdepth3", 3), ("kuhn333_x4_vdepth4", 4)])
def test_overlapping_kuhn_cuts_reach_the_visit_loop(name, vdepth):
    """Three and four Kuhn cuts of one 3 x 3 x 3 block: one chunk whose rows have more visits than 768 residual threads
    take two at a time, and whose block and diagonal lists outgrow the registers."""
    deck, h = crafted(name)
    assert len(h) == 1 and len(deck.nodes) == 64
    assert h["vdepth"][0] >= vdepth and h["vdepth"][0] >= 3
    assert h["depth"][0] > G_REGW and h["ddepth"][0] > G_REGW
    assert h["nvthr"][0] <= G_TASK_THREADS


def test_block_threads_past_wave_slot_ten():
    """4 x 3 x 3 cubes cut three times: a chunk with more than 704 block threads (wave slot 11, the last of
    wdepth[2], holds blocks and walks a list), and a chunk that starts at an odd block."""
    deck, h = crafted("kuhn433_x3_threads")
    big = h[np.argmax(h["noffd"])]
    assert big["noffd"] > 704 and big["noffd"] <= G_TASK_THREADS
    assert g4.wave_depths(h)[np.argmax(h["noffd"])][11] > 0                # (the host deals the waves to the slots SIMD by SIMD: not every slot below is taken)
    assert big["vdepth"] >= 3 and big["nvthr"] > 704
    assert np.any(h["b0"] & 1)


def test_element_limit():
    """4 x 4 x 3 cubes cut four times: a chunk with all 720 element slots, cut short of 64 rows by the element limit."""
    deck, h = crafted("kuhn443_x4_element_limit")
    full = h[h["nelem"] == G_MAX_SLOTS_USED]
    assert len(full) >= 1 and np.all(h["nelem"] <= G_MAX_SLOTS_USED)
    assert np.all(rows(full) < G_MAX_ROWS)
    assert full["vdepth"].max() >= 3 and full["depth"].max() > G_REGW


def test_node_limit_cuts_a_chunk():
    """Six hubs of 90 tetrahedra lying in each other: chunks of a few rows with all 256 node slots."""
    deck, h = crafted("hubs6x90_node_limit")
    cut = h[(h["nnode"] == G_MAX_NODES) & (rows(h) < G_MAX_ROWS)]
    assert len(cut) >= 1 and rows(cut).min() < 16
    assert h["depth"].max() > G_REGW and h["ddepth"].max() > G_REGW
    assert len(h) >= 5


def test_full_chunk_at_the_node_and_thread_limits():
    """Four hubs of 120: a 64-row chunk with 256 node slots and all 768 block threads."""
    deck, h = crafted("hubs4x120_nodes_and_threads")
    full = h[(h["nnode"] == G_MAX_NODES) & (rows(h) == G_MAX_ROWS)]
    assert len(full) >= 1 and full["noffd"].max() == G_TASK_THREADS
    assert h["depth"].max() > 4 * G_REGW and h["ddepth"].max() > 2 * G_REGW
    assert np.any(h["b0"] & 1)


def test_composite_is_a_run_of_unlike_chunks(monkeypatch):
    """All parts side by side: in row order one workgroup goes from lattice bricks to chunks cut by the node limit, to
    the four-cut block at vdepth 4, to chunks at the element limit, to a full chunk of 256 nodes and 768 threads, and
    into a lattice where one chunk repeats its predecessor's words.  The layout asks for the largest LDS the kernel
    takes: 256 node slots and 720 records."""
    deck, h = crafted("composite")
    assert h["nnode"].max() == G_MAX_NODES and h["nelem"].max() == G_MAX_SLOTS_USED and h["noffd"].max() == G_TASK_THREADS
    assert G_MAX_NODES * 48 + G_MAX_SLOTS_USED * 208 == 162048
    assert np.any((h["nnode"] == G_MAX_NODES) & (rows(h) < G_MAX_ROWS))
    assert np.any((h["nnode"] == G_MAX_NODES) & (h["noffd"] == G_TASK_THREADS))
    assert h["vdepth"].max() >= 4 and np.any(h["vdepth"] == 3) and np.any(h["vdepth"] == 2) and np.any(h["vdepth"] == 1)
    assert h["depth"].max() > G_REGW and h["ddepth"].max() > G_REGW
    assert np.any(h["b0"] & 1) and np.any(h["b0"] & 1 == 0)
    assert len(h) >= 24
    monkeypatch.setenv("FEAHIP_GATHER_ORDER", "0")
    monkeypatch.setenv("FEAHIP_GATHER_NRUNS", "1")
    w = feahip.host_gather_walk(g4.library_elements(deck), len(deck.nodes))
    one = g4.chunk_headers(w)
    assert w["runs"] == 1 and np.array_equal(w["walk"], np.arange(w["chunks"]))
    flagged = np.nonzero(one["flags"] & 1)[0]
    assert 1 <= len(flagged) < len(one) // 4                        # nearly every chunk loads words of its own
    # the next chunk has fewer node slots than the current one somewhere in the run, and more somewhere else
    assert np.any(np.diff(one["nnode"]) < 0) and np.any(np.diff(one["nnode"]) > 0)
    p = int(np.argmax(one["nelem"]))
    assert 0 < p < len(one) - 1                                     # the 720-slot chunk has a predecessor and a successor
    monkeypatch.setenv("FEAHIP_GATHER_NRUNS", "64")
    assert feahip.host_gather_walk(g4.library_elements(deck), len(deck.nodes))["runs"] == len(h)


def test_the_lattices_of_the_suite_reach_none_of_this():
    """Why this file exists: the block the walk tests assemble stays far from every limit above."""
    h = g4.headers(mesh.bar_deck(n=5))
    assert h["nnode"].max() <= 144 and h["vdepth"].max() <= 2
    assert h["nelem"].max() < 688 and h["noffd"].max() <= 512
    assert h["depth"].max() <= G_REGW and h["ddepth"].max() <= G_REGW


# ---- the chunk knobs on the small composite

@functools.lru_cache(maxsize=None)
def small():
    deck = g4.small_composite(lone_node=True)
    el = g4.library_elements(deck)
    lone = int(feahip.host_numbering(deck.elements, deck.nodes)[0][-1])
    digest = feahip.host_assembly_digest(el, len(deck.nodes))[0]
    digest.setflags(write=False)
    return deck, el, lone, digest


def test_rows_knob_one_chunk_per_node(monkeypatch):
    deck, el, lone, _ = small()
    assert len(deck.nodes) == 479
    g4.set_chunk_knobs(monkeypatch, g4.KNOB_SETTINGS["rows1"])
    h = g4.headers(deck)
    assert len(h) == len(deck.nodes) and np.all(rows(h) == 1)
    empty = h[h["r0"] == lone]                                   # the node no element refers to: a chunk with no element
    assert len(empty) == 1 and empty["nelem"][0] == 16 and empty["noffd"][0] == 0 and empty["nb"][0] == 1 and empty["nvthr"][0] == 0
    assert h["depth"].max() > G_REGW and h["ddepth"].max() > G_REGW      # the hub and the fan axis, one row each


def test_rows_knob_three(monkeypatch):
    deck, el, lone, _ = small()
    g4.set_chunk_knobs(monkeypatch, g4.KNOB_SETTINGS["rows3"])
    h = g4.headers(deck)
    assert rows(h).max() == 3 and len(h) >= len(deck.nodes) // 3


def test_elems_knob_below_a_single_row_still_builds(monkeypatch):
    """FEAHIP_GATHER_ELEMS=8: nearly every row has more elements around it; a single row may exceed the knob."""
    deck, el, lone, _ = small()
    g4.set_chunk_knobs(monkeypatch, g4.KNOB_SETTINGS["elems8"])
    h = g4.headers(deck)
    assert np.any((rows(h) == 1) & (h["nelem"] > 16)) and np.any(rows(h) > 1)
    assert h["nelem"].max() >= 96                                # the hubs' centres


def test_alpha_zero_mixes_one_row_and_full_chunks(monkeypatch):
    deck, el, lone, _ = small()
    g4.set_chunk_knobs(monkeypatch, g4.KNOB_SETTINGS["rows64_alpha0"])
    h = g4.headers(deck)
    assert np.any(rows(h) == 1) and np.any(rows(h) == G_MAX_ROWS)
    g4.set_chunk_knobs(monkeypatch, {})
    assert len(g4.headers(deck)) < len(h)


@pytest.mark.parametrize("knob", list(g4.KNOB_SETTINGS))
def test_digest_does_not_depend_on_the_cut(knob, monkeypatch):
    """What the maps say about a row -- which elements contribute to which block, with which local nodes -- is the
    same however the rows are cut into chunks."""
    deck, el, lone, digest = small()
    g4.set_chunk_knobs(monkeypatch, g4.KNOB_SETTINGS[knob])
    assert np.array_equal(feahip.host_assembly_digest(el, len(deck.nodes))[0], digest)
    for name in g4.CRAFTED:
        d = g4.CRAFTED[name]()
        e = g4.library_elements(d)
        got = feahip.host_assembly_digest(e, len(d.nodes))[0]
        g4.set_chunk_knobs(monkeypatch, {})
        assert np.array_equal(got, feahip.host_assembly_digest(e, len(d.nodes))[0]), name
        g4.set_chunk_knobs(monkeypatch, g4.KNOB_SETTINGS[knob])


@pytest.mark.parametrize("name", list(g4.CRAFTED) + ["small", "graded"])
def test_no_scale_of_the_bars_is_zero(name):
    """The GPU file divides every row's and node's error by the oracle's scale of that row or node and caps none: under
    the deformation it assembles at no element is inverted and every scale is positive, for both models."""
    from oracle_binding import OracleSolver
    from test_gpu_gather10_limits import MODELS, Want, deform
    for model in MODELS:
        deck = dict(g4.CRAFTED, small=g4.small_composite, graded=g4.graded_lattice)[name]()
        deck.model = model
        x = deform(deck.nodes)
        o = OracleSolver(deck)
        o.set_nodes(x)
        assert o.update_state() == 0
        o.close()
        want = Want(deck, x)
        assert want.kscale.min() > 0 and want.fscale.min() > 0 and want.tscale.min() > 0

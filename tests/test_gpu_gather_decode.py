"""The decoded map words of the linear-tet gather kernel on an MI355X (GDecoded, csrc/gather_device.h; DEC of
k_assemble_gather, csrc/kernels_gather.hip): a chunk's map words are turned into LDS addresses once, where they arrive,
and stay decoded while the following chunks run with the same words.  That moves integer arithmetic out of the gather
phase and touches no sum: with FEAHIP_GATHER_DECODE=0 (the kernel that decodes in every chunk), with the default (the
decoded kernel where more than half of a context's chunks keep their predecessor's words) and with
FEAHIP_GATHER_DECODE=1 (the decoded kernel on any mesh), K and f of the fused launch, K alone and f alone are the same
bits -- on a run that alternates between chunks that keep
their predecessor's words and chunks that request new ones, on a run of one chunk (the prologue's decode only), where
decoded words, words in registers and words read inside the gather phase meet in one list, on a chunk of five rows, on
one with all 720 element slots, and with a material table (whose kernels have no registers for the decoded form and
run as they were: the switch must then change nothing either)."""
import functools

import numpy as np
import pytest

import feahip
import gather4_meshes as g4
import mesh
from gather10_meshes import library_elements
from hetero_reference import MATERIALS, layered_ids, with_materials
from test_gpu_gather10_limits import deform
from test_gpu_gather_walk import A5, NH, assembled, same_bits, set_knobs

pytestmark = pytest.mark.gpu

ONE_RUN = {"FEAHIP_GATHER_NRUNS": 1}


@pytest.fixture(autouse=True)
def default_knobs(monkeypatch):
    g4.set_chunk_knobs(monkeypatch, {})
    monkeypatch.delenv("FEAHIP_GATHER_DECODE", raising=False)


def both(monkeypatch, deck, x, walk):
    """The assembly of a fresh context with the switch off, and of another with the decoded kernel.  By default a context
    runs the decoded kernel where more than half of its chunks keep their predecessor's words; FEAHIP_GATHER_DECODE=1
    runs it on any mesh.  Both are compared with the switch off: the forced context is returned, the default one held
    to it here."""
    monkeypatch.setenv("FEAHIP_GATHER_DECODE", "0")
    off = assembled(monkeypatch, deck, x, walk)
    monkeypatch.delenv("FEAHIP_GATHER_DECODE")
    dflt = assembled(monkeypatch, deck, x, walk)
    monkeypatch.setenv("FEAHIP_GATHER_DECODE", "1")
    on = assembled(monkeypatch, deck, x, walk)
    monkeypatch.delenv("FEAHIP_GATHER_DECODE")
    assert np.any(on["K"] != 0) and np.any(on["f"] != 0)
    assert same_bits(dflt, off), "the default against FEAHIP_GATHER_DECODE=0"
    return off, on


def headers(monkeypatch, deck, walk):
    set_knobs(monkeypatch, walk)
    return g4.chunk_headers(feahip.host_gather_walk(library_elements(deck), len(deck.nodes)))


@functools.lru_cache(maxsize=None)
def bar(model, n):
    deck = mesh.bar_deck(n=n, model=model)
    x = mesh.deformed_state(deck.nodes, k1=1.08, wiggle=5e-3)
    x.setflags(write=False)
    return deck, x


@functools.lru_cache(maxsize=None)
def crafted(name, model):
    deck = g4.CRAFTED[name]()
    deck.model = model
    x = deform(deck.nodes)
    x.setflags(write=False)
    return deck, x


@pytest.mark.parametrize("model", [NH, A5])
def test_words_kept_and_words_requested_alternate(model, monkeypatch):
    """6 x 31 x 6 nodes walked by one workgroup, equal chunks adjacent: 23 chunks, the flags of consecutive chunks go
    1, 0, 1 -- addresses that stay, a decode at the bottom of the loop, addresses that stay again."""
    deck, x = bar(model, 5)
    h = headers(monkeypatch, deck, ONE_RUN)
    flags = "".join(str(f & 1) for f in h["flags"])
    assert "101" in flags and "00" in flags and "11" in flags, flags
    off, on = both(monkeypatch, deck, x, ONE_RUN)
    for got in (off, on):                               # both kinds of transition did occur on the device's maps
        st = got["stats"]
        assert st["chunks"] == len(h) == 23 and st["chunks_with_predecessors_words"] == flags.count("1")
        assert 0 < st["chunks_with_predecessors_words"] < st["chunks"] - 1
        assert 2 * st["chunks_with_predecessors_words"] > st["chunks"]      # the default is the decoded kernel here
    assert same_bits(on, off)


@pytest.mark.parametrize("model", [NH, A5])
def test_default_runs(model, monkeypatch):
    """The same mesh under the default cut: a workgroup per chunk or two, the decode of the prologue in every one."""
    deck, x = bar(model, 5)
    off, on = both(monkeypatch, deck, x, {})
    assert same_bits(on, off)


@pytest.mark.parametrize("model", [NH, A5])
def test_a_run_of_one_chunk(model, monkeypatch):
    deck, x = bar(model, 1)
    assert len(headers(monkeypatch, deck, ONE_RUN)) == 1
    off, on = both(monkeypatch, deck, x, ONE_RUN)
    assert on["stats"]["chunks"] == 1
    assert same_bits(on, off)


@pytest.mark.parametrize("model", [NH, A5])
@pytest.mark.parametrize("name", ["kuhn333_x3_vdepth3", "hubs6x90_node_limit", "kuhn443_x4_element_limit"])
def test_crafted_mesh(name, model, monkeypatch):
    """Lists of nine words (three decoded, three in registers, three read inside the gather phase), for blocks and
    diagonal lanes; chunks of five rows between full ones; a chunk with all 720 element slots."""
    deck, x = crafted(name, model)
    h = headers(monkeypatch, deck, ONE_RUN)
    if name == "kuhn333_x3_vdepth3":
        assert h["depth"].max() > g4.G_REGW and h["ddepth"].max() > g4.G_REGW
    elif name == "hubs6x90_node_limit":
        assert np.any(h["r1"] - h["r0"] == 5) and len(h) > 1
    else:
        assert h["nelem"].max() == g4.G_MAX_SLOTS_USED and len(h) > 1
    off, on = both(monkeypatch, deck, x, ONE_RUN)
    assert on["stats"]["chunks"] == len(h)
    assert same_bits(on, off)


@pytest.mark.parametrize("model", [NH, A5])
def test_with_a_material_table(model, monkeypatch):
    deck, x = bar(model, 5)
    het = with_materials(deck, MATERIALS[:2], layered_ids(deck, 2))
    off, on = both(monkeypatch, het, x, ONE_RUN)
    assert same_bits(on, off)
    assert not np.array_equal(on["K"], assembled(monkeypatch, deck, x, ONE_RUN)["K"])      # the table is in use

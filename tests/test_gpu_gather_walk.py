"""The walk of the linear-tet gather kernel on an MI355X (csrc/gather.cpp, kernels_gather.hip): cutting the runs by
cost and putting equal chunks next to each other changes which workgroup assembles a chunk and when, never what the chunk
computes -- K and f are the same bits with the walk on and off.  Small meshes, runs of several chunks forced."""
import functools
import os

import numpy as np
import pytest

import feahip
import mesh
from gather10_meshes import library_elements
from hetero_reference import MATERIALS, layered_ids, with_materials
from oracle_binding import OracleSolver

pytestmark = pytest.mark.gpu

NH, A5 = feahip.MODEL_COMPRESSIBLE_NEOHOOKEAN, feahip.MODEL_A5
K_TOL = 1e-12                             # the bar tests/test_gpu_parity.py holds the gather kernel to: of max|K|, max|f|
KNOBS = ("FEAHIP_GATHER_ORDER", "FEAHIP_GATHER_BALANCE", "FEAHIP_GATHER_RUN", "FEAHIP_GATHER_NRUNS")
OFF = {"FEAHIP_GATHER_ORDER": "0", "FEAHIP_GATHER_BALANCE": "0"}


def set_knobs(monkeypatch, settings):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in {"FEAHIP_GATHER_ORDER": 1, "FEAHIP_GATHER_BALANCE": 1, **settings}.items():      # both parts on unless a case says otherwise
        monkeypatch.setenv(k, str(v))


def host_walk(monkeypatch, deck, settings, rows=None):
    set_knobs(monkeypatch, settings)
    return feahip.host_gather_walk(library_elements(deck), len(deck.nodes), rows=rows)


def assembled(monkeypatch, deck, x, settings, shard=None):
    """(K of K-and-f, f of K-and-f, K alone, f alone, chunks with their predecessor's words) of a fresh context: the maps
    are built at its first assembly, under the settings."""
    set_knobs(monkeypatch, settings)
    s = feahip.FeaSolver(deck)
    try:
        s.set_nodes(x)
        s.set_assembly(feahip.ASM_GATHER)
        if shard is not None:
            s.set_row_shard(*shard)
        s.create_stiffness_and_residual()
        assert s.assembly_in_use() == feahip.ASM_GATHER
        off, idx, k = s.matrix_yale64()
        f = s.forces()
        s.create_stiffness()
        k_alone = s.matrix_yale64()[2]
        s.create_residual_forces()
        f_alone = s.forces()
        return {"off": off, "idx": idx, "K": k, "f": f, "K_alone": k_alone, "f_alone": f_alone, "stats": s.assembly_stats()}
    finally:
        s.close()


def same_bits(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("off", "idx", "K", "f", "K_alone", "f_alone"))


@functools.lru_cache(maxsize=None)
def base(model):
    deck = mesh.bar_deck(n=5, model=model)            # 6 x 31 x 6 nodes: a partial brick on every axis, 23 chunks
    x = mesh.deformed_state(deck.nodes, k1=1.08, wiggle=5e-3)
    x.setflags(write=False)
    return deck, x


@pytest.mark.parametrize("walk", [{"FEAHIP_GATHER_NRUNS": 4}, {"FEAHIP_GATHER_RUN": 7}, {"FEAHIP_GATHER_NRUNS": 4, "FEAHIP_GATHER_ORDER": 0},
                                  {"FEAHIP_GATHER_RUN": 7, "FEAHIP_GATHER_BALANCE": 0}],
                         ids=["nruns4", "run7", "nruns4-row-order", "run7-unbalanced"])
@pytest.mark.parametrize("model", [NH, A5])
def test_walk_changes_no_bit(model, walk, monkeypatch):
    deck, x = base(model)
    w = host_walk(monkeypatch, deck, walk)
    assert w["runs"] == 4 and np.diff(w["run_start"]).max() >= 6
    if "FEAHIP_GATHER_ORDER" not in walk:
        assert not np.array_equal(w["walk"], np.arange(w["chunks"]))      # chunks do move on this mesh
        flags = np.ascontiguousarray(w["blob"].reshape(w["chunks"], w["stride"])[:, :64]).view(np.int32).reshape(-1, 16)[:, 14] & 1
        rs = w["run_start"]
        assert any(not flags[rs[r + 1] - 2] for r in range(w["runs"]))     # a run whose last group is a single chunk
    ref = assembled(monkeypatch, deck, x, OFF)
    got = assembled(monkeypatch, deck, x, walk)
    assert got["stats"]["chunks"] == w["chunks"] and got["stats"]["chunks_with_predecessors_words"] == w["chunks_with_predecessors_words"]
    assert same_bits(got, ref)


def test_walk_against_the_oracle(monkeypatch):
    deck, x = base(NH)
    got = assembled(monkeypatch, deck, x, {"FEAHIP_GATHER_NRUNS": 4})
    o = OracleSolver(deck)
    o.set_nodes(x)
    o.update_state(); o.create_stiffness(); o.create_residual_forces()
    s = feahip.FeaSolver(deck)                        # (the oracle's Yale arrays are 32-bit: the same K through matrix_yale)
    s.set_nodes(x); s.set_assembly(feahip.ASM_GATHER); s.create_stiffness_and_residual()
    off, idx, val = s.matrix_yale()
    s.close()
    assert np.array_equal(off, o.offsets()) and np.array_equal(idx, o.indexes())
    assert np.array_equal(val, got["K"])
    kerr = np.abs(val - o.values()).max() / np.abs(o.values()).max()
    ferr = np.abs(got["f"] - o.forces()).max() / np.abs(o.forces()).max()
    f1err = np.abs(got["f_alone"] - o.forces()).max() / np.abs(o.forces()).max()
    print(f"K {kerr:.2e} f {ferr:.2e} f alone {f1err:.2e}")
    assert kerr < K_TOL and ferr < K_TOL and f1err < K_TOL


@pytest.mark.parametrize("model", [NH, A5])
def test_walk_changes_no_bit_with_two_materials(model, monkeypatch):
    deck, x = base(model)
    het = with_materials(deck, MATERIALS[:2], layered_ids(deck, 2))
    ref = assembled(monkeypatch, het, x, OFF)
    got = assembled(monkeypatch, het, x, {"FEAHIP_GATHER_NRUNS": 4})
    assert same_bits(got, ref)
    assert not np.array_equal(got["K"], assembled(monkeypatch, deck, x, OFF)["K"])      # the table is in use


@pytest.mark.parametrize("case", ["one_chunk", "fewer_chunks_than_runs", "default_runs"])
def test_few_chunks(case, monkeypatch):
    """One chunk (a single cube: 8 rows); fewer chunks than runs asked for; the default cut for the device's compute
    units, which gives every chunk of a small mesh a run of its own."""
    deck = mesh.bar_deck(n=1) if case == "one_chunk" else mesh.bar_deck(n=3)
    x = mesh.deformed_state(deck.nodes, k1=1.08, wiggle=5e-3)
    walk = {} if case == "default_runs" else {"FEAHIP_GATHER_NRUNS": 64}
    w = host_walk(monkeypatch, deck, walk)
    assert w["runs"] == w["chunks"] and (w["chunks"] == 1) == (case == "one_chunk")
    ref = assembled(monkeypatch, deck, x, OFF)
    got = assembled(monkeypatch, deck, x, walk)
    assert same_bits(got, ref)


def test_a_reshard_rebuilds_the_walk(monkeypatch):
    """One context moved between row shards: the maps of the shard installed are built with their own walk, and the
    rows it owns carry the bits they carry with the walk off."""
    deck, x = base(NH)
    for shard in ((1, 2), (0, 2), (0, 1)):
        ref = assembled(monkeypatch, deck, x, OFF, shard=shard)
        got = assembled(monkeypatch, deck, x, {"FEAHIP_GATHER_NRUNS": 3}, shard=shard)
        assert got["stats"]["chunks"] < 23 or shard == (0, 1)
        assert same_bits(got, ref)
    # and inside one context: shard, other shard, whole mesh
    set_knobs(monkeypatch, {"FEAHIP_GATHER_NRUNS": 3})
    s = feahip.FeaSolver(deck)
    s.set_nodes(x); s.set_assembly(feahip.ASM_GATHER)
    whole = assembled(monkeypatch, deck, x, OFF)
    set_knobs(monkeypatch, {"FEAHIP_GATHER_NRUNS": 3})
    try:
        for shard in ((1, 2), (0, 2), (0, 1)):
            s.set_row_shard(*shard)
            s.create_stiffness_and_residual()
            d = s.owned_dofs()
            own = np.zeros(s.ndof, dtype=bool); own[d] = True
            off, idx, k = s.matrix_yale64()
            mine = own[np.repeat(np.arange(s.ndof), np.diff(off))]
            ref = assembled(monkeypatch, deck, x, OFF, shard=shard)
            set_knobs(monkeypatch, {"FEAHIP_GATHER_NRUNS": 3})
            assert np.array_equal(k, ref["K"]) and np.array_equal(s.forces()[d], ref["f"][d])
            assert np.all(k[~mine] == 0)
        assert np.array_equal(k, whole["K"]) and np.array_equal(s.forces(), whole["f"])
    finally:
        s.close()

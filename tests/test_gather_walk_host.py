"""The walk of the 4-node gather maps (csrc/gather.cpp), host only: which chunk records a workgroup walks and in what
order.  The runs are cut to near-equal modelled cost and, inside a run, chunks with byte-identical map words follow one
another; neither may lose a chunk, a row or a flag.  Everything is recomputed here from the records themselves."""
import contextlib
import functools
import gzip
import hashlib
import json
import os
import shutil
import tempfile

import numpy as np
import pytest

import feahip
import mesh
from gather10_meshes import library_elements

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS = ("FEAHIP_GATHER_ORDER", "FEAHIP_GATHER_BALANCE", "FEAHIP_GATHER_RUN", "FEAHIP_GATHER_NRUNS")
SHAPE = (5, 6, 7, 8, 9, 10)               # header ints that belong to the map words: nelem, noffd, depth, nvthr, vdepth, ddepth


@contextlib.contextmanager
def knobs(**kw):
    old = {k: os.environ.pop(k, None) for k in KNOBS}
    try:
        for k, v in {"order": 1, "balance": 1, **kw}.items():      # both parts on unless a case says otherwise, whatever the library's default
            os.environ["FEAHIP_GATHER_" + k.upper()] = str(v)
        yield
    finally:
        for k in KNOBS:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]


@functools.lru_cache(maxsize=None)
def deck_of(name):
    if name.startswith("bar"):
        return mesh.bar_deck(n=int(name[3:]))
    if name == "jitter5":
        return mesh.jitter_permute(mesh.bar_deck(n=5))
    assert name == "tetgen"
    with tempfile.TemporaryDirectory() as td:
        pth = os.path.join(td, "brick_fine.sexp")
        with gzip.open(os.path.join(ROOT, "tests", "golden", "decks", "brick_fine.sexp.gz"), "rb") as fi, open(pth, "wb") as fo:
            shutil.copyfileobj(fi, fo)
        bf = feahip.Deck.load(pth)
    bf.presc_node = (bf.presc_node - 1).astype(np.int32)
    return mesh.tiled(mesh.corner_tets(bf), (1, 1, 1))


@functools.lru_cache(maxsize=None)
def elements_of(name):
    deck = deck_of(name)
    el = np.ascontiguousarray(library_elements(deck), dtype=np.int32)
    el.setflags(write=False)
    return el, len(deck.nodes)


@functools.lru_cache(maxsize=None)
def walk_of(name, settings=(), rows=None, ncu=0):
    """The walk of a mesh under the settings ((knob, value), ...): computed once, shared, never written to."""
    el, n = elements_of(name)
    with knobs(**dict(settings)):
        w = feahip.host_gather_walk(el, n, rows=rows, ncu=ncu)
    w["header"] = np.ascontiguousarray(w["blob"].reshape(w["chunks"], w["stride"])[:, :64]).view(np.int32).reshape(w["chunks"], 16)
    for v in w.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return w


def word_kinds(w):
    """kind[i] of record i: records share a number exactly when their map words (and the header ints that go with
    them) are the same bytes -- compared as bytes, no hash trusted."""
    rec = w["blob"].reshape(w["chunks"], w["stride"])
    keys = {}
    kind = np.zeros(w["chunks"], dtype=np.int64)
    for i in range(w["chunks"]):
        h = w["header"][i]
        key = (tuple(int(h[j]) for j in SHAPE), int(h[1] - h[0]), rec[i, w["words_begin"]:w["words_end"]].tobytes())
        kind[i] = keys.setdefault(key, len(keys))
    return kind


MESHES = ["bar2", "bar3", "bar5", "bar9", "jitter5", "tetgen"]
SETTINGS = [(), (("nruns", 3),), (("nruns", 7),), (("run", 3),), (("nruns", 5), ("order", 0)), (("balance", 0),),
            (("order", 0), ("balance", 0))]


@pytest.mark.parametrize("settings", SETTINGS, ids=lambda s: "-".join(f"{k}{v}" for k, v in s) or "default")
@pytest.mark.parametrize("name", MESHES)
def test_walk_keeps_every_chunk_row_and_flag(name, settings):
    w = walk_of(name, settings)
    n, hd = w["chunks"], w["header"]
    _, nodes = elements_of(name)
    assert np.array_equal(np.sort(w["walk"]), np.arange(n))                 # a permutation of the chunks
    owned = np.zeros(nodes, dtype=np.int64)
    for i in range(n):
        owned[hd[i, 0]:hd[i, 1]] += 1
    assert np.all(owned == 1)                                               # every row in exactly one record
    assert np.array_equal(np.argsort(np.argsort(hd[:, 0])), w["walk"])      # record i is chunk walk[i] of the row order
    rs = w["run_start"]
    assert rs[0] == 0 and rs[-1] == n and len(rs) == w["runs"] + 1
    assert np.all(np.diff(rs) > 0)                                          # monotone, and no run is empty
    s = dict(settings)
    if "nruns" in s:
        assert w["runs"] == min(s["nruns"], n)
    if "run" in s:
        assert np.all(np.diff(rs)[:-1] == s["run"]) and 0 < rs[-1] - rs[-2] <= s["run"]
    # the flag of record i says that record i + 1 has byte-identical map words, and says so whenever it has
    kind = word_kinds(w)
    flagged = (hd[:, 14] & 1) != 0
    assert not flagged[-1]
    assert np.array_equal(flagged[:-1], kind[:-1] == kind[1:])
    assert w["chunks_with_predecessors_words"] == int(flagged.sum())
    # inside a run: the kinds in order of first appearance (in row order), row order inside a kind
    grouped = s.get("order", 1) != 0
    for r in range(w["runs"]):
        a, b = rs[r], rs[r + 1]
        chunks = w["walk"][a:b]
        assert np.array_equal(np.sort(chunks), np.arange(a, b))            # a run is a contiguous range of the row order too
        if not grouped:
            assert np.array_equal(chunks, np.arange(a, b))
            continue
        k = kind[a:b]
        firsts = [k[0]] + [k[i] for i in range(1, b - a) if k[i] != k[i - 1]]
        assert len(firsts) == len(set(firsts))                              # each kind is one block of the run
        by_row = {}
        for c, kk in sorted(zip(chunks.tolist(), k.tolist())):
            by_row.setdefault(kk, []).append(c)
        assert firsts == list(by_row)                                       # kinds by the first chunk, in row order, that has them
        assert chunks.tolist() == [c for kk in firsts for c in by_row[kk]]


@pytest.mark.parametrize("settings", [(), (("nruns", 3),), (("nruns", 7),), (("nruns", 5), ("order", 0))],
                         ids=lambda s: "-".join(f"{k}{v}" for k, v in s) or "default")
@pytest.mark.parametrize("name", MESHES)
def test_heaviest_run_is_within_one_chunk_of_the_mean(name, settings):
    w = walk_of(name, settings)
    cost = w["cost"].astype(np.int64)
    assert np.all(cost > 0)
    run = np.add.reduceat(cost, w["run_start"][:-1])
    print(f"{name} {settings}: {w['runs']} runs of {w['chunks']} chunks, heaviest {run.max()}, mean {run.mean():.0f}, dearest chunk {cost.max()}")
    assert run.max() <= run.mean() + cost.max()


def test_switches_off_give_the_maps_as_they_were():
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "gather_walk", "bar3_row_order_maps.json")))
    w = walk_of("bar3", (("order", 0), ("balance", 0)))
    assert w["chunks"] == gold["chunks"] and w["stride"] == gold["bytes_per_record"] and len(w["blob"]) == gold["bytes"]
    assert hashlib.sha256(w["blob"].tobytes()).hexdigest() == gold["sha256"]
    assert np.array_equal(w["walk"], np.arange(w["chunks"]))


@pytest.mark.parametrize("name", ["bar9", "tetgen"])
def test_equal_count_runs_when_balancing_is_off(name):
    """Runs of ceil(chunks / (k CUs)) chunks, k = 1 or 2 by the shorter launch counted in chunks (two on a tie)."""
    for ncu in (4, 7, 256):
        w = walk_of(name, (("balance", 0),), ncu=ncu)
        n = w["chunks"]
        best = None
        for k in (2, 1):
            rl = max(1, -(-n // (k * ncu)))
            nr = -(-n // rl)
            c = -(-nr // ncu) * rl
            if best is None or c < best[0]:
                best = (c, rl)
        assert np.array_equal(w["run_start"], np.append(np.arange(0, n, best[1]), n))


def test_a_rank_builds_the_walk_of_its_rows():
    el, n = elements_of("bar9")
    lo, hi = n // 3, 2 * n // 3
    w = walk_of("bar9", (("nruns", 4),), rows=(lo, hi))
    hd = w["header"]
    owned = np.zeros(n, dtype=np.int64)
    for i in range(w["chunks"]):
        owned[hd[i, 0]:hd[i, 1]] += 1
    assert np.all(owned[lo:hi] == 1) and owned[:lo].sum() == 0 and owned[hi:].sum() == 0
    assert w["runs"] == 4 and np.array_equal(np.sort(w["walk"]), np.arange(w["chunks"]))


def test_grouping_moves_chunks_on_a_block_with_equal_bricks():
    """The cases above must not all be walks nothing moved in: on the 9-cube block equal bricks are apart in row order."""
    on, off = walk_of("bar9", (("nruns", 3),)), walk_of("bar9", (("nruns", 3), ("order", 0)))
    assert not np.array_equal(on["walk"], np.arange(on["chunks"]))
    assert on["chunks_with_predecessors_words"] > off["chunks_with_predecessors_words"]

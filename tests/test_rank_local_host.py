"""A rank made from its own slab, host side (feahip_host_rank_local_plan, feahip_host_slab_order, mesh.bar_slab).

The reference is one process with one store of the whole mesh (fea_solver.c:444-448).  feahip_create_rank made a rank
hold only its slab but still took the whole mesh to cut it; feahip_create_rank_local takes the slab.  Here, without a
device: the halo plan derived from a slab names the rows the whole-mesh plan names and its two ends fit each other in
GLOBAL id order; the generated slabs tile the block and never build it; the proposed local order is a function of the
mesh, not of the order it arrives in, and it helps the gather maps; every malformed slab is refused.
"""
import ctypes as C
import gzip
import os
import shutil
import subprocess
import tracemalloc

import numpy as np
import pytest

import feahip
import mesh

BLOCKS = {"tet4": dict(dims=(6, 24, 6)), "tet10": dict(dims=(3, 12, 3), quadratic=True), "hex8": dict(dims=(5, 20, 5), hexa=True)}
_decks = {}


def deck_of(name, decks_dir, tmp_path_factory):
    if name not in _decks:
        if name == "corner":
            p = tmp_path_factory.mktemp("fine") / "brick_fine.sexp"
            with gzip.open(os.path.join(decks_dir, "brick_fine.sexp.gz"), "rb") as src, open(p, "wb") as dst:
                shutil.copyfileobj(src, dst)
            _decks[name] = mesh.corner_tets(feahip.Deck.load(str(p)))
        else:
            _decks[name] = mesh.bar_deck(**BLOCKS[name])
    return _decks[name]


def plans_fit(plans, nranks):
    """rank a's send list to b is rank b's receive list from a, element for element; every list ascends in global id."""
    for a in range(nranks):
        for k, b in enumerate(plans[a]["peers"]):
            assert a in plans[b]["peers"]
            kb = plans[b]["peers"].index(a)
            assert np.array_equal(plans[a]["send"][k], plans[b]["recv"][kb])
            assert np.array_equal(plans[a]["recv"][k], plans[b]["send"][kb])
            for lst in (plans[a]["send"][k], plans[a]["recv"][k]):
                assert np.all(np.diff(lst) > 0)


@pytest.mark.parametrize("nranks", [2, 3, 8])
@pytest.mark.parametrize("name", ["tet4", "tet10", "hex8", "corner"])
def test_plan_of_a_slab_names_the_rows_of_the_whole_mesh_plan(name, nranks, decks_dir, tmp_path_factory):
    deck = deck_of(name, decks_dir, tmp_path_factory)
    local = []
    for r in range(nranks):
        slab = feahip.slab_of(deck, r, nranks)
        lp, wp = feahip.host_rank_local_plan(slab, r, nranks), feahip.host_rank_plan(deck, r, nranks)
        assert lp["peers"] == wp["peers"]
        for k in range(len(lp["peers"])):
            for side in ("send", "recv"):
                assert len(lp[side][k]) == len(wp[side][k]) == len(set(wp[side][k]))
                assert set(lp[side][k]) == set(wp[side][k])             # the same SET of global rows per peer
        local.append(lp)
    plans_fit(local, nranks)


@pytest.mark.parametrize("nranks", [2, 3, 8])
@pytest.mark.parametrize("name", ["tet4", "tet10", "hex8"])
def test_generated_slabs_tile_the_block(name, nranks):
    kw = BLOCKS[name]
    deck = mesh.bar_deck(**kw)
    presc = {int(a): (int(t), tuple(v)) for a, t, v in zip(deck.presc_node, deck.presc_type, deck.presc_values)}
    seen = np.zeros(len(deck.nodes), dtype=int)
    plans = []
    for r in range(nranks):
        s = mesh.bar_slab(r, nranks, **kw)
        assert s.n_global_nodes == len(deck.nodes) and s.ele_type == deck.ele_type and s.gauss_nodes_count == deck.gauss_nodes_count
        assert len(s.halo_owner) == len(s.nodes) - s.n_own
        own = s.node_global[:s.n_own]
        seen[own] += 1
        touches = np.isin(deck.elements, own).any(axis=1)                   # the deck's elements with a node it owns
        want = np.sort(deck.elements[touches], axis=1)
        got = np.sort(s.node_global[s.elements], axis=1)
        assert np.array_equal(want[np.lexsort(want.T[::-1])], got[np.lexsort(got.T[::-1])])
        assert np.array_equal(deck.elements[s.elem_global], s.node_global[s.elements])     # and their ids and node order
        assert np.array_equal(s.nodes, deck.nodes[s.node_global])
        mine = {int(s.node_global[a]): (int(t), tuple(v)) for a, t, v in zip(s.presc_node, s.presc_type, s.presc_values)}
        assert mine == {g: presc[g] for g in s.node_global.tolist() if g in presc}         # halo nodes included
        plans.append(feahip.host_rank_local_plan(s, r, nranks))
    assert np.all(seen == 1)
    plans_fit(plans, nranks)
    u = mesh.bar_slab(1, nranks, recipe="uniaxial", **kw)
    du = mesh.bar_deck(recipe="uniaxial", **kw)
    pu = {int(a): int(t) for a, t in zip(du.presc_node, du.presc_type)}
    assert {int(u.node_global[a]): int(t) for a, t in zip(u.presc_node, u.presc_type)} == \
        {g: pu[g] for g in u.node_global.tolist() if g in pu}


def test_bar_slab_is_sized_by_the_slab():
    """Rank 3 of 8 of a 16 x 512 x 16 TET4 block: its own arrays are 66 of 513 node planes, 13 % of the block's; index
    temporaries may take two to three times that; anything that builds the block peaks above 100 %.  The bound is half
    of the bytes of the block's nodes + elements arrays, from the counts -- the block itself is never built here."""
    nx, ny, nz = 16, 512, 16
    block = (nx + 1) * (ny + 1) * (nz + 1) * 3 * 8 + nx * ny * nz * 6 * 4 * 4
    mesh.bar_slab(0, 2, dims=(2, 4, 2))                                    # imports and caches out of the measurement
    tracemalloc.start()
    s = mesh.bar_slab(3, 8, dims=(nx, ny, nz))
    _, peak = tracemalloc.get_traced_memory()
    tracemalloc.stop()
    print(f"peak {peak} bytes, block {block} bytes, ratio {peak / block:.3f}")
    assert len(s.nodes) == 66 * 17 * 17 and len(s.elements) == 65 * 16 * 16 * 6
    assert peak < 0.5 * block


def shuffled(slab, seed):
    """The same slab with its local ids shuffled within owned and within halo."""
    rng = np.random.default_rng(seed)
    n, no = len(slab.nodes), slab.n_own
    return slab.permuted(np.concatenate([rng.permutation(no), no + rng.permutation(n - no)]).astype(np.int32))


@pytest.mark.parametrize("name", ["tet4", "tet10", "hex8"])
def test_slab_order_is_a_function_of_the_mesh(name):
    s = mesh.bar_slab(1, 3, **BLOCKS[name])
    a, b = shuffled(s, 1), shuffled(s, 2)
    for t in (s, a, b):
        new = np.empty(len(t.nodes), dtype=np.int32)
        rc = feahip.load_library().feahip_host_slab_order(len(t.nodes), t.n_own, len(t.elements), t.nodes_per_element,
                                                          t.elements.ctypes.data_as(C.POINTER(C.c_int)),
                                                          t.nodes.ctypes.data_as(C.POINTER(C.c_double)),
                                                          new.ctypes.data_as(C.POINTER(C.c_int)))
        assert rc in (0, 1)
        assert np.array_equal(np.sort(new), np.arange(len(t.nodes)))       # a bijection
        assert np.all(new[:t.n_own] < t.n_own) and np.all(new[t.n_own:] >= t.n_own)
    ra, rb = a.reordered(), b.reordered()
    assert np.array_equal(ra.node_global, rb.node_global) and np.array_equal(ra.nodes, rb.nodes)
    assert np.array_equal(ra.halo_owner, rb.halo_owner)
    assert np.array_equal(ra.node_global[ra.elements], rb.node_global[rb.elements])
    assert ra.n_own == s.n_own and set(ra.node_global[:ra.n_own]) == set(s.node_global[:s.n_own])


def test_slab_order_helps_the_gather_maps():
    s = shuffled(mesh.bar_slab(1, 3, dims=(8, 48, 8)), 7)
    r = s.reordered()
    before, _ = feahip.host_gather_stats(s.elements, len(s.nodes))
    after, _ = feahip.host_gather_stats(r.elements, len(r.nodes))
    print("before", before, "after", after)
    assert after["elements"] == before["elements"] == len(s.elements)
    assert after["chunks"] < before["chunks"] and after["evals"] < before["evals"]


def _plan_rc(s, rank=1, nranks=3, **over):
    a = dict(n_local=len(s.nodes), n_own=s.n_own, n_elems=len(s.elements), elements=s.elements, node_global=s.node_global,
             halo_owner=s.halo_owner)
    a.update(over)
    ip = C.POINTER(C.c_int)
    arr = {k: np.ascontiguousarray(a[k], dtype=np.int32) for k in ("elements", "node_global", "halo_owner")}
    cnt = np.zeros(3, dtype=np.int32)
    lib = feahip.load_library()
    rc = lib.feahip_host_rank_local_plan(rank, nranks, a["n_local"], a["n_own"], a["n_elems"], s.nodes_per_element,
                                         arr["elements"].ctypes.data_as(ip), arr["node_global"].ctypes.data_as(ip),
                                         arr["halo_owner"].ctypes.data_as(ip), cnt.ctypes.data_as(ip), None, None, None, None, None)
    return rc, lib.feahip_create_error().decode()


def test_malformed_slabs_are_refused():
    s = mesh.bar_slab(1, 3, dims=(2, 12, 2))
    n, no = len(s.nodes), s.n_own
    assert _plan_rc(s)[0] == 0
    for bad in (0, -1, n + 1):
        rc, msg = _plan_rc(s, n_own=bad)
        assert rc == -1 and "n_own" in msg and str(bad) in msg
    for bad in (-1, n):
        el = s.elements.copy(); el[5, 2] = bad
        rc, msg = _plan_rc(s, elements=el)
        assert rc == -1 and "element 5 " in msg and str(bad) in msg
    halo_only = np.nonzero(np.all(s.elements >= no, axis=1))[0]
    assert len(halo_only) == 0
    el = s.elements.copy(); el[7, :] = np.arange(no, no + 4)               # an element of halo nodes only
    rc, msg = _plan_rc(s, elements=el)
    assert rc == -1 and "element 7 " in msg and "no owned node" in msg
    assert 0 not in s.node_global                                          # (rank 0's first plane is far from rank 1's slab)
    rc, msg = _plan_rc(s, n_local=n + 1, node_global=np.append(s.node_global, 0),
                       halo_owner=np.append(s.halo_owner, 0))               # a halo node nothing touches
    assert rc == -1 and f"halo node {n} " in msg
    for bad in (-1, 3, 1):                                                  # outside [0, nranks), or this rank itself
        ho = s.halo_owner.copy(); ho[4] = bad
        rc, msg = _plan_rc(s, halo_owner=ho)
        assert rc == -1 and "halo_owner[4]" in msg and str(bad) in msg
    ng = s.node_global.copy(); ng[9] = ng[3]
    rc, msg = _plan_rc(s, node_global=ng)
    assert rc == -1 and "node_global[" in msg and "repeats" in msg and "[3]" in msg and "[9]" in msg
    ng = s.node_global.copy(); ng[2] = -4
    rc, msg = _plan_rc(s, node_global=ng)
    assert rc == -1 and "node_global[2]" in msg
    assert _plan_rc(s, rank=3)[0] == -1 and _plan_rc(s, rank=0, nranks=0)[0] == -1


def test_rank_local_builders_under_sanitizers(tmp_path):
    """rankmesh.cpp's builders for a caller's slab (plan, validation, slab order) under AddressSanitizer and UBSan."""
    if shutil.which("g++") is None or not os.path.isdir("/opt/rocm/include"):
        pytest.skip("needs g++ and the HIP headers")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = os.path.join(root, "fea-large_amd", "csrc")
    exe = str(tmp_path / "host_asan_rank_local")
    cmd = ["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-std=c++17",
           "-I" + src, "-I" + os.path.join(root, "include"), "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__", "-o", exe,
           os.path.join(root, "tests", "host_asan_rank_local.cpp")] + [os.path.join(src, f) for f in
                                                                       ("pattern.cpp", "visits.cpp", "gather.cpp", "gather10.cpp", "shard.cpp", "renumber.cpp", "rankmesh.cpp", "amg_setup.cpp")] + ["-lpthread"]
    subprocess.run(cmd, check=True, capture_output=True, timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr
    assert r.stdout.count("plans fit: 1") == 2 and r.stdout.count("refused: 7/7") == 2 and r.stdout.count("order: bijection 1") == 2

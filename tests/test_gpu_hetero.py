"""Bodies of several materials (feahip_set_materials) on an MI355X, against tests/hetero_reference.py: the oracle's
element matrices picked per element by material.  Tolerances are those tests/test_gpu_parity.py holds the uniform case
to: K and f 1e-12 of their scale, F 1e-13, sigma 1e-12, displacements 1e-10 relative."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import feahip
import mesh
from hetero_reference import (MATERIALS, HeteroRestatement, arclength_hetero, layered_ids, perturbed, scattered_ids,
                              with_materials)

pytestmark = pytest.mark.gpu

K_TOL, F_TOL, S_TOL, U_TOL = 1e-12, 1e-13, 1e-12, 1e-10
NH, A5 = feahip.MODEL_COMPRESSIBLE_NEOHOOKEAN, feahip.MODEL_A5


def rel(a, b):
    s = np.abs(b).max()
    return np.abs(a - b).max() / (s if s > 0 else 1.0)


def base_deck(kind, model=NH, **kw):
    if kind == "tet4":
        return mesh.bar_deck(dims=(4, 12, 4), model=model, **kw)          # 325 nodes, 1152 tets: six or more 64-row chunks
    if kind == "tet10":
        return mesh.bar_deck(dims=(2, 6, 2), quadratic=True, gauss=5, model=model, **kw)
    return mesh.bar_deck(dims=(3, 8, 3), hexa=True, model=model, **kw)


def ids_of(deck, how):
    return scattered_ids(deck) if how == "scattered" else layered_ids(deck)


@functools.lru_cache(maxsize=None)
def reference(kind, model, how):
    """(deck with the table, x, K dense, f, F, sigma) -- computed once, shared, never written to."""
    deck = base_deck(kind, model)
    ids = ids_of(deck, how)
    x = perturbed(deck.nodes)
    r = HeteroRestatement(deck, MATERIALS, ids)
    K, f, F, S = r.assemble(x)
    r.close()
    for a in (K, f, F, S, x):
        a.setflags(write=False)
    return with_materials(deck, MATERIALS, ids), x, K, f, F, S


def yale_of(K, off, idx):
    rows = np.repeat(np.arange(K.shape[0]), np.diff(off))
    return K[rows, idx]


def assembled(s, strategy=None):
    if strategy is not None:
        s.set_assembly(strategy)
    s.create_stiffness_and_residual()
    return s.matrix_yale()[2], s.forces()


# ---- 1. K, f, F and sigma against the restatement
@pytest.mark.parametrize("how", ["scattered", "layered"])
@pytest.mark.parametrize("model", [NH, A5])
@pytest.mark.parametrize("kind", ["tet4", "tet10", "hex8"])
def test_assembly_and_state_match_the_restatement(kind, model, how):
    deck, x, K, f, F, S = reference(kind, model, how)
    s = feahip.FeaSolver(deck)
    par, ids = s.materials()
    assert np.array_equal(par, MATERIALS) and np.array_equal(ids, deck.element_material)
    s.set_nodes(x)
    for strat in (feahip.ASM_AUTO, feahip.ASM_GATHER, feahip.ASM_ROWOWNER, feahip.ASM_ATOMIC):
        s.set_assembly(strat)
        s.create_stiffness_and_residual()
        off, idx, val = s.matrix_yale()
        ref = yale_of(K, off, idx)
        print(f"{kind} model {model} {how} strategy {strat}: K {rel(val, ref):.2e} f {rel(s.forces(), f):.2e}")
        assert rel(val, ref) < K_TOL, strat
        assert rel(s.forces(), f) < K_TOL, strat
        if strat == feahip.ASM_AUTO and kind == "tet4":
            assert s.assembly_in_use() == feahip.ASM_GATHER
        s.create_stiffness()                                  # the separate entry points: the same K, the same f
        assert rel(s.matrix_yale()[2], ref) < K_TOL
        s.create_residual_forces()
        assert rel(s.forces(), f) < K_TOL
    print(f"F {rel(s.graddefs(), F):.2e} sigma {rel(s.stresses(), S):.2e}")
    assert rel(s.graddefs(), F) < F_TOL
    assert rel(s.stresses(), S) < S_TOL
    s.close()


# ---- 2. a table of the creation pair is the table-less context, to the bit
@pytest.mark.parametrize("strategy", [feahip.ASM_GATHER, feahip.ASM_ROWOWNER])
@pytest.mark.parametrize("kind", ["tet4", "tet10", "hex8"])
def test_a_table_of_the_creation_pair_changes_no_bit(kind, strategy):
    deck = base_deck(kind)
    x = perturbed(deck.nodes)
    s = feahip.FeaSolver(deck)
    s.set_nodes(x)
    v0, f0 = assembled(s, strategy)
    def same(a, b, scale):
        print(f"{kind} strategy {strategy}: largest difference {np.abs(a - b).max() / scale:.2e} of scale")
        return np.array_equal(a, b)
    ks, fs = np.abs(v0).max(), np.abs(f0).max()
    s.set_materials(np.tile(deck.parameters[:2], (3, 1)), scattered_ids(deck))
    v1, f1 = assembled(s)
    assert same(v1, v0, ks) and same(f1, f0, fs)
    s.set_materials(MATERIALS, scattered_ids(deck))
    v2, _ = assembled(s)
    assert not np.array_equal(v2, v0)
    s.set_materials(None)                                     # back to the pair given at creation
    assert s.materials()[0].shape == (0, 2)
    v3, f3 = assembled(s)
    assert same(v3, v0, ks) and same(f3, f0, fs)
    s.close()


# ---- 3. relabelling and repetition; 4. a table set after the maps were built
@pytest.mark.parametrize("kind", ["tet4", "tet10"])
def test_relabelling_repetition_and_set_after_build(kind):
    deck = base_deck(kind)
    x = perturbed(deck.nodes)
    ids = scattered_ids(deck)
    het = feahip.FeaSolver(with_materials(deck, MATERIALS, ids))          # the table from the start
    het.set_nodes(x)
    v0, f0 = assembled(het, feahip.ASM_GATHER)
    v1, f1 = assembled(het)
    assert np.array_equal(v0, v1) and np.array_equal(f0, f1)
    perm = np.array([2, 0, 1])                                # material m becomes entry perm[m] of the new table
    table = np.empty_like(MATERIALS); table[perm] = MATERIALS
    het.set_materials(table, perm[ids])
    v2, f2 = assembled(het)
    assert np.array_equal(v0, v2) and np.array_equal(f0, f2)
    het.close()
    late = feahip.FeaSolver(deck)                             # uniform first: the maps are built without ids
    late.set_nodes(x)
    vu, _ = assembled(late, feahip.ASM_GATHER)
    late.set_materials(MATERIALS, ids)
    v3, f3 = assembled(late)
    assert late.assembly_in_use() == feahip.ASM_GATHER
    assert np.array_equal(v3, v0) and np.array_equal(f3, f0) and not np.array_equal(vu, v0)
    late.close()


# ---- 5. solve
def layer_stretches(deck, x):
    """Mean y-extension of each of the three layers: (top plane - bottom plane) of the displacement."""
    y0 = deck.nodes[:, 1]
    lo, hi = y0.min(), y0.max()
    planes = [np.abs(y0 - (lo + k * (hi - lo) / 3)) < 1e-9 for k in range(4)]
    uy = x[:, 1] - y0
    return [uy[planes[k + 1]].mean() - uy[planes[k]].mean() for k in range(3)]


@functools.lru_cache(maxsize=None)
def solved_reference(kind):
    deck = base_deck(kind, solver_type=feahip.CHOLESKY, modified_newton=False)
    ids = layered_ids(deck)
    r = HeteroRestatement(deck, MATERIALS, ids)
    done, its, x = r.solve(2, deck.max_newton_count, deck.desired_tolerance)
    r.close()
    x.setflags(write=False)
    return with_materials(deck, MATERIALS, ids), done, its, x


@pytest.mark.parametrize("precond", [0, 1])
@pytest.mark.parametrize("kind", ["tet4", "tet10"])
def test_layered_bar_solve(kind, precond):
    deck, rdone, rits, rx = solved_reference(kind)
    s = feahip.FeaSolver(deck)
    s.set_preconditioner(precond)
    done, its, _ = s.solve(load_increments=2, modified_newton=False, solver_type=feahip.CHOLESKY, solver_tolerance=1e-15)
    x = s.nodes()
    err = rel(x - deck.nodes, rx - deck.nodes)
    print(f"{kind} precond {precond}: iterations {list(its)} / {rits}, |du| {err:.2e}")
    assert done == rdone == 2 and list(its) == list(rits)
    assert err < U_TOL
    st = np.abs(layer_stretches(deck, x))
    assert st[1] < st[0] < st[2]                              # E = 654 (stiff), 250, 182 (soft)
    s.close()


# ---- 6. sharded
def slabs_of(deck, n):
    return [feahip.slab_of(deck, r, n) for r in range(n)]


@pytest.mark.parametrize("form", ["row_shard", "rank_contexts", "slabs"])
@pytest.mark.parametrize("n", [2, 3])
def test_sharded_assembly_is_the_unsharded_one(n, form):
    deck = mesh.bar_deck(dims=(3, 40, 3))
    deck = with_materials(deck, MATERIALS, scattered_ids(deck))
    x = perturbed(deck.nodes, amp=0.01)
    one = feahip.FeaSolver(deck)
    one.set_nodes(x)
    val, f = assembled(one)
    off, idx, _ = one.matrix_yale()
    Kd = sp.csr_matrix((val, idx, off), shape=(one.ndof, one.ndof)).toarray()
    assert one.assembly_in_use() == feahip.ASM_GATHER
    kscale = np.abs(val).max()
    row_of_value = np.repeat(np.arange(one.ndof), np.diff(off))
    if form == "row_shard":
        g = feahip.FeaGroup(deck, n)
        g.each("set_nodes", x)
    elif form == "rank_contexts":
        g = feahip.FeaGroup(deck, n, rank_contexts=True)
        for r in g.ranks:
            r.set_nodes(x[r.node_global])
    else:
        slabs = slabs_of(deck, n)
        assert all(np.array_equal(sl.element_material, deck.element_material[sl.elem_global]) for sl in slabs)
        g = feahip.FeaGroup(slabs)
        for r in g.ranks:
            r.set_nodes(x[r.node_global])
    g.each("create_stiffness_and_residual")
    seen = np.zeros(len(deck.nodes), dtype=int)
    for nd, r in zip(g.nodes, g.ranks):
        assert r.assembly_in_use() == feahip.ASM_GATHER
        seen[nd] += 1
        if form == "row_shard":                               # owned rows of the whole mesh's Yale store
            own = np.zeros(len(deck.nodes), dtype=bool); own[nd] = True
            mine = own[row_of_value // 3]
            v = r.matrix_yale()[2]
            assert np.abs(v[mine] - val[mine]).max() < 4e-16 * kscale
            assert np.all(v[~mine] == 0)
            d = r.owned_dofs()
            assert np.array_equal(r.forces()[d], f[d])
        else:                                                 # a rank context: local rows [0, n_own) are the nodes nd
            par, ids = r.materials()
            assert np.array_equal(ids, deck.element_material[r.elem_global])
            fl = r.forces().reshape(-1, 3)[:r.n_own]
            assert np.array_equal(fl, f.reshape(-1, 3)[nd])
            # the owned rows of the rank's local Yale store against the same rows of the unsharded K, column by
            # column through node_global: the same entries, equal to rounding (mirror blocks, as for a row shard)
            lo, li, lv = r.matrix_yale()
            Kl = sp.csr_matrix((lv, li, lo), shape=(r.ndof, r.ndof)).toarray()
            gd = (3 * r.node_global.astype(np.int64)[:, None] + np.arange(3)[None, :]).ravel()
            own = np.arange(3 * r.n_own)
            ref = Kd[gd[own]][:, gd]
            assert np.array_equal(Kl[own] == 0, ref == 0)
            assert np.abs(Kl[own] - ref).max() < 1e-12 * kscale
            assert np.all(Kl[3 * r.n_own:] == 0)              # nothing written to the halo rows
    assert np.all(seen == 1)
    g.close(); one.close()


@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("form", ["row_shard", "rank_contexts", "slabs"])
def test_group_solve_reaches_the_unsharded_displacements(form, n):
    deck = mesh.bar_deck(dims=(3, 24, 3), solver_type=feahip.CHOLESKY, modified_newton=False)
    deck = with_materials(deck, MATERIALS, layered_ids(deck))
    one = feahip.FeaSolver(deck)
    done, its, _ = one.solve(load_increments=1, solver_tolerance=1e-15)
    u = one.nodes() - deck.nodes
    one.close()
    g = (feahip.FeaGroup(deck, n) if form == "row_shard" else
         feahip.FeaGroup(deck, n, rank_contexts=True) if form == "rank_contexts" else feahip.FeaGroup(slabs_of(deck, n)))
    gd, gits, _ = g.solve(1, deck.max_newton_count, False, deck.desired_tolerance, feahip.CHOLESKY, 1e-15)
    assert gd == done == 1 and list(gits) == list(its)
    assert rel(g.gather("nodes") - deck.nodes, u) < U_TOL
    g.close()


# ---- 7. refusals
def test_refusals():
    deck = base_deck("tet4")
    ids = scattered_ids(deck)
    s = feahip.FeaSolver(deck)
    lib = s._lib
    import ctypes as C
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    par = np.ascontiguousarray(MATERIALS)
    def call(n, p, e):
        rc = lib.feahip_set_materials(s._ctx, n, p.ctypes.data_as(dp) if p is not None else None,
                                      e.ctypes.data_as(ip) if e is not None else None)
        return rc, lib.feahip_last_error(s._ctx).decode()
    EINVAL = -1                                               # FEAHIP_EINVAL (include/fea_hip.h)
    rc, msg = call(3, None, ids)
    assert rc != 0 and "null" in msg
    rc, msg = call(3, par, None)
    assert rc != 0 and "null" in msg
    big = np.tile(par, (100, 1))[:257].copy()
    rc, msg = call(257, big, ids)
    assert rc != 0 and "257" in msg
    bad = ids.copy(); bad[17] = 3
    rc, msg = call(3, par, bad)
    assert rc != 0 and "element 17" in msg
    bad[17] = -1
    rc, msg = call(3, par, bad)
    assert rc != 0 and "element 17" in msg
    nan = par.copy(); nan[1, 1] = np.nan
    rc, msg = call(3, nan, ids)
    assert rc != 0 and "material 1" in msg and "mu" in msg
    inf = par.copy(); inf[2, 0] = np.inf
    rc, msg = call(3, inf, ids)
    assert rc != 0 and "material 2" in msg and "lambda" in msg
    assert s.materials()[0].shape == (0, 2)                   # every refusal left the context as it was
    rcs = {call(3, nan, ids)[0], call(257, big, ids)[0], call(3, par, bad)[0], call(3, None, ids)[0]}
    assert rcs == {EINVAL}
    # STAGED and SHARED know one pair: refused with a table, with the way out in the message
    s.set_materials(MATERIALS, ids)
    s.set_assembly(feahip.ASM_STAGED)
    with pytest.raises(feahip.FeaHipError, match="GATHER or ROWOWNER"):
        s.create_stiffness_and_residual()
    s.close()
    q = feahip.FeaSolver(base_deck("tet10"))
    q.set_materials(MATERIALS, scattered_ids(q.deck))
    q.set_assembly(feahip.ASM_SHARED)
    with pytest.raises(feahip.FeaHipError, match="GATHER or ROWOWNER"):
        q.create_stiffness_and_residual()
    q.set_assembly(feahip.ASM_AUTO)                           # AUTO never lands on them
    q.create_stiffness_and_residual()
    assert q.assembly_in_use() in (feahip.ASM_GATHER, feahip.ASM_ROWOWNER)
    q.close()


# ---- 7. arc length and the two-column solve see only K and f
@functools.lru_cache(maxsize=None)
def lame():
    deck = mesh.lame_quarter_deck(2, 4, 1, p=1.0, load_increments_count=3, max_newton_count=30, desired_tolerance=1e-22,
                                  modified_newton=False, solver_type=feahip.CHOLESKY, solver_tolerance=1e-15)
    return with_materials(deck, MATERIALS, scattered_ids(deck))


def test_arclength_on_a_heterogeneous_cylinder():
    deck = lame()
    want = arclength_hetero(deck, 1e9, 3, deck.max_newton_count, deck.desired_tolerance)
    assert want["rc"] == 0 and len(want["lam"]) == 3
    s = feahip.FeaSolver(deck)
    n, lam, its, _, rc = s.solve_arclength(1e9, 3)
    print(f"lambda {lam} / {want['lam']}, iterations {its} / {want['its']}")
    assert rc == 0 and n == 3 and list(its[:3]) == list(want["its"])
    assert rel(np.asarray(lam[:3]), want["lam"]) < U_TOL
    assert rel(s.nodes() - deck.nodes, want["x"][-1] - deck.nodes) < U_TOL
    uniform = feahip.FeaSolver(with_materials(deck, np.zeros((0, 2)), []))       # the table matters on this path
    _, lam_u, _, _, _ = uniform.solve_arclength(1e9, 3)
    assert rel(np.asarray(lam_u[:3]), want["lam"]) > 1e-3
    uniform.close(); s.close()


def test_solve_slae2_on_a_heterogeneous_cylinder():
    deck = lame()
    x = perturbed(deck.nodes, amp=0.005)
    r = HeteroRestatement(deck, MATERIALS, deck.element_material)
    K, f, _, _ = r.assemble(x)
    K, f = r.masked(K, f)
    s = feahip.FeaSolver(deck)
    s.set_nodes(x)
    s.set_load_factor(1.0)
    f2 = s.surface_forces()
    f2[r.mask] = 0.0
    s.set_load_factor(0.0)
    s.create_stiffness_and_residual()
    s.apply_prescribed_bc(0.0)
    s.solve_slae2(f2, feahip.CHOLESKY, 1e-15, 20000)
    u, u2 = np.linalg.solve(K, f), np.linalg.solve(K, f2)
    print(f"u {rel(s.solution(), u):.2e} u2 {rel(s.solution2(), u2):.2e}")
    assert rel(s.solution(), u) < U_TOL and rel(s.solution2(), u2) < U_TOL
    r.close(); s.close()

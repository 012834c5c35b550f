"""A rank's context made from its own slab (feahip_create_rank_local), on the GPU.

The reference holds the whole mesh in one process (fea_solver.c:387-456).  feahip_create_rank made a context that holds
one rank's slab, but from the whole mesh; feahip_create_rank_local makes it from the slab alone.  Same local mesh, same
kernels: against the whole-mesh rank context the results are the same bits; groups of such contexts solve what the
RankSolver groups solve; slabs generated directly (mesh.bar_slab, another cut) give the rows of the unsharded context.
"""
import copy
import os

import numpy as np
import pytest
import scipy.sparse as sp

import feahip
import mesh
from oracle_binding import OracleSolver

pytestmark = pytest.mark.gpu

BLOCKS = {"tet4": dict(dims=(3, 48, 3)), "tet10": dict(dims=(3, 20, 3), quadratic=True), "hex8": dict(dims=(3, 20, 3), hexa=True)}


def rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300)


def dofs(nodes):
    return (3 * np.asarray(nodes, dtype=np.int64)[:, None] + np.arange(3)[None, :]).ravel()


def slabs_of(deck, n):
    return [feahip.slab_of(deck, r, n) for r in range(n)]


def whole_K_f(deck, x=None, lam=None, bc=None):
    one = feahip.FeaSolver(deck)
    if lam is not None:
        one.update_nodes_with_bc(lam)
    if x is not None:
        one.set_nodes(x)
    one.create_stiffness_and_residual()
    if bc is not None:
        one.apply_prescribed_bc(bc)
    off, idx, val = one.matrix_yale()
    K = sp.csr_matrix((val, idx, off), shape=(one.ndof, one.ndof))
    return one, K, one.forces()


def owned_rows_against(r, K, f, ktol, ftol):
    """every owned row of the rank's K and f, taken to global ids through node_global, against the whole K and f"""
    lo, li, lv = r.matrix_yale()
    Kl = sp.csr_matrix((lv, li, lo), shape=(r.ndof, r.ndof))
    gd = dofs(r.node_global)
    own = np.arange(3 * r.n_own)
    ref = K[gd[own]][:, gd]
    dk = abs(Kl[own] - ref).max() / np.abs(K.data).max()
    df = np.abs(r.forces()[own] - f[gd[own]]).max() / np.abs(f).max()
    print(f"owned rows: K {dk:.3e} (bound {ktol:g}), f {df:.3e} (bound {ftol:g}) of scale")
    assert dk < ktol and df < ftol


# ------------------------------------------------------------------ 6: the same bits as the whole-mesh rank context
@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("name", ["tet4", "tet10", "hex8"])
def test_same_bits_as_the_whole_mesh_rank_context(name, n):
    """Same local mesh, same kernels: any difference is a bug, so the tolerance is zero."""
    deck = mesh.bar_deck(**BLOCKS[name])
    x = mesh.deformed_state(deck.nodes, k1=1.03)
    for r in range(n):
        a = feahip.LocalRankSolver(feahip.slab_of(deck, r, n), r, n)
        b = feahip.RankSolver(deck, r, n)
        for k in ("N", "n_own", "E", "N_global", "nnzb_local", "nnzb_owned", "rows_sent", "rows_received"):
            assert getattr(a, k) == getattr(b, k), k                       # feahip_rank_counts
        assert np.array_equal(a.node_global, b.node_global) and np.array_equal(a.elem_global, b.elem_global)
        assert a.owned_rows() == b.owned_rows() == (0, a.n_own)
        for state in ("bc", "deformed"):
            for s in (a, b):
                if state == "bc":
                    s.update_nodes_with_bc(1.0)
                else:
                    s.set_nodes(x[s.node_global])
                s.create_stiffness_and_residual()
            if name == "tet4":
                assert a.assembly_in_use() == b.assembly_in_use() == feahip.ASM_GATHER
            else:
                assert a.assembly_in_use() == b.assembly_in_use()
            (ao, ai, av), (bo, bi, bv) = a.matrix_yale(), b.matrix_yale()
            assert np.array_equal(ao, bo) and np.array_equal(ai, bi)
            assert np.isfinite(av).all() and np.abs(av).max() > 0
            assert np.array_equal(av, bv)
            own = np.arange(3 * a.n_own)
            assert np.isfinite(a.forces()[own]).all() and np.array_equal(a.forces()[own], b.forces()[own])
            assert np.array_equal(a.nodes(), b.nodes())
        a.close(); b.close()


# ------------------------------------------------------------------ 7: groups of such contexts
@pytest.mark.parametrize("n,dims,precond", [(2, (3, 48, 3), 0), (3, (3, 48, 3), 0), (2, (6, 96, 6), 1)])
def test_groups_of_slabs_solve_like_groups_of_rank_contexts(n, dims, precond):
    """Block-Jacobi and multigrid PCG and one Newton iteration: 1e-11 of scale, the bound tests/test_rankmesh.py uses
    for rank contexts against the unsharded run."""
    deck = mesh.bar_deck(dims=dims)
    out = []
    for g in (feahip.FeaGroup(deck, n, rank_contexts=True), feahip.FeaGroup(slabs_of(deck, n))):
        g.each("set_preconditioner", precond)
        g.each("update_nodes_with_bc", 1.0); g.each("create_stiffness_and_residual"); g.each("apply_prescribed_bc", 0.0)
        it, res = g.solve_slae(feahip.PCG_ILU, 1e-15, 40000)
        u, e = g.gather("solution"), g.energy()
        g.update_nodes_with_solution()
        out.append((it, res, u, e, g.gather("nodes") - deck.nodes))
        g.close()
    (it0, res0, u0, e0, d0), (it1, res1, u1, e1, d1) = out
    print(f"iterations {it0} / {it1}, residual {res0:.2e} / {res1:.2e}, |du| {rel(u1, u0):.3e}, |dx| {rel(d1, d0):.3e}")
    assert res1 < 1e-14 and abs(it1 - it0) <= 2
    assert rel(u1, u0) < 1e-11 and e1 == pytest.approx(e0, rel=1e-11) and rel(d1, d0) < 1e-11


def test_two_slabs_reproduce_the_oracle(decks_dir):
    """The reference's clamped deck over two slabs: 13 modified-Newton iterations, <u,f> and displacements to 1e-10."""
    deck = feahip.Deck.load(os.path.join(decks_dir, "neohook_brick.sexp"))
    o = OracleSolver(deck)
    od, oits, otol = o.solve(1, deck.max_newton_count, True, deck.desired_tolerance, feahip.CHOLESKY)
    g = feahip.FeaGroup(slabs_of(deck, 2))
    gd, gits, gtol = g.solve(1, deck.max_newton_count, True, deck.desired_tolerance, feahip.CHOLESKY)
    assert gd == od == 1 and list(gits) == list(oits) == [13]
    assert np.abs(gtol - otol).max() < 1e-10 * np.abs(otol).max()
    assert rel(g.gather("nodes") - deck.nodes, o.nodes() - deck.nodes) < 1e-10
    g.close()


@pytest.mark.parametrize("precond", [0, 1])
def test_poisoned_halo_rows_change_nothing(precond, monkeypatch):
    """FEAHIP_TEST_POISON_HALO (tests/test_gpu_sharded.py): the interior product of the overlapped exchange must not read
    a halo row, whichever order the plan lists them in.  Bit for bit the unpoisoned solve."""
    deck = mesh.bar_deck(dims=(6, 96, 6) if precond else (3, 48, 3))
    slabs = slabs_of(deck, 3)

    def run():
        g = feahip.FeaGroup(slabs)
        g.each("set_pcg_variant", 1); g.each("set_preconditioner", precond)
        g.each("update_nodes_with_bc", 1.0); g.each("create_stiffness_and_residual"); g.each("apply_prescribed_bc", 0.0)
        it, res = g.solve_slae(feahip.PCG_ILU, 1e-15, 20000)
        u, e = g.gather("solution"), g.energy()
        g.close()
        return it, res, u, e

    monkeypatch.delenv("FEAHIP_TEST_POISON_HALO", raising=False)
    it0, res0, u0, e0 = run()
    monkeypatch.setenv("FEAHIP_TEST_POISON_HALO", "1")
    it1, res1, u1, e1 = run()
    assert np.isfinite(u1).all() and np.isfinite(res1) and res1 < 1e-14
    assert it1 == it0 and np.array_equal(u1, u0) and e1 == e0


# ------------------------------------------------------------------ 8: generated slabs against the unsharded context
@pytest.mark.parametrize("name", ["tet4", "tet10"])
def test_generated_slabs_against_the_unsharded_context(name):
    """bar_slab cuts node planes, the library cuts library ids: other chunks, other summation order, so not bitwise --
    1e-12 of scale on K and f (the suite's K tolerance), 1e-10 on the solved increment."""
    kw = dict(dims=(3, 24, 3)) if name == "tet4" else dict(dims=(3, 12, 3), quadratic=True)
    deck = mesh.bar_deck(**kw)
    slabs = [mesh.bar_slab(r, 3, **kw).reordered() for r in range(3)]
    x = mesh.deformed_state(deck.nodes, k1=1.03)
    one, K, f = whole_K_f(deck, x=x)
    g = feahip.FeaGroup(slabs)
    seen = np.zeros(len(deck.nodes), dtype=int)
    for r in g.ranks:
        assert r.N < len(deck.nodes) and r.N_global == len(deck.nodes)
        r.set_nodes(x[r.node_global]); r.create_stiffness_and_residual()
        owned_rows_against(r, K, f, 1e-12, 1e-12)
        seen[r.node_global[:r.n_own]] += 1
    assert np.all(seen == 1)
    one.set_nodes(deck.nodes); one.update_nodes_with_bc(1.0); one.create_stiffness_and_residual(); one.apply_prescribed_bc(0.0)
    one.solve_slae(feahip.PCG_ILU, 1e-15, 20000)
    for r in g.ranks:
        r.set_nodes(deck.nodes[r.node_global])
    g.each("update_nodes_with_bc", 1.0); g.each("create_stiffness_and_residual"); g.each("apply_prescribed_bc", 0.0)
    it, res = g.solve_slae(feahip.PCG_ILU, 1e-15, 20000)
    du = rel(g.gather("solution"), one.solution())
    print(f"solve: {it} iterations, residual {res:.2e}, increment {du:.3e} (bound 1e-10)")
    assert res < 1e-14 and du < 1e-10
    g.close(); one.close()


# ------------------------------------------------------------------ 9: prescribed halo dofs
def test_prescribed_halo_dofs_are_cancelled_from_owned_rows():
    """Type-1 constraints on every node of the x = min face straddle every cut: a rank must know the prescribed dofs of
    its halo nodes to cancel their columns from its owned rows."""
    deck = mesh.bar_deck(dims=(3, 24, 3))
    xs = deck.nodes[:, 0]
    face = np.nonzero(np.abs(xs - xs.min()) < 1e-12)[0]
    face = np.setdiff1d(face, deck.presc_node).astype(np.int32)            # (the end faces are clamped already)
    vals = np.zeros((len(face), 3)); vals[:, 0] = 0.01
    deck = copy.copy(deck)
    deck.presc_node = np.ascontiguousarray(np.concatenate([deck.presc_node, face]))
    deck.presc_type = np.ascontiguousarray(np.concatenate([deck.presc_type, np.ones(len(face), dtype=np.int32)]))
    deck.presc_values = np.ascontiguousarray(np.concatenate([deck.presc_values, vals]))
    x = mesh.deformed_state(deck.nodes, k1=1.03, wiggle=1e-2)              # no entry of the pattern is zero by symmetry
    one, K, f = whole_K_f(deck, x=x, lam=0.5, bc=0.5)
    Kd = K.toarray()
    straddles = 0
    for r, slab in enumerate(slabs_of(deck, 3)):
        halo_presc = np.isin(slab.presc_node, np.arange(slab.n_own, len(slab.nodes)))
        straddles += int(halo_presc.any())
        s = feahip.LocalRankSolver(slab, r, 3)
        s.update_nodes_with_bc(0.5); s.set_nodes(x[s.node_global]); s.create_stiffness_and_residual(); s.apply_prescribed_bc(0.5)
        lo, li, lv = s.matrix_yale()
        Kl = sp.csr_matrix((lv, li, lo), shape=(s.ndof, s.ndof)).toarray()
        gd = dofs(s.node_global)
        own = np.arange(3 * s.n_own)
        ref = Kd[gd[own]][:, gd]
        assert np.array_equal(Kl[own] == 0, ref == 0)                      # exactly the entries the unsharded context zeroes
        assert np.abs(Kl[own] - ref).max() < 1e-12 * np.abs(Kd).max()
        df = np.abs(s.forces()[own] - f[gd[own]]).max() / np.abs(f).max()
        print(f"rank {r}: f {df:.3e} of scale (bound 1e-12)")
        assert df < 1e-12
        s.close()
    assert straddles == 3
    one.close()


# ------------------------------------------------------------------ 10: surface loads in local ids
def test_surface_loads_in_local_ids():
    base = mesh.bar_deck(dims=(3, 12, 3))
    top = mesh.block_side_faces(base.nodes, base.elements, 1, True)        # pressure on y = max
    side = mesh.block_side_faces(base.nodes, base.elements, 0, True)       # dead traction on x = max
    faces = np.concatenate([top, side])
    kind = np.concatenate([np.full(len(top), feahip.LOAD_PRESSURE), np.full(len(side), feahip.LOAD_TRACTION)]).astype(np.int32)
    values = np.concatenate([np.tile([2.5, 0, 0], (len(top), 1)), np.tile([0.3, -0.2, 0.1], (len(side), 1))])
    deck = mesh.bar_deck(dims=(3, 12, 3), surface_faces=faces, surface_kind=kind, surface_values=values)
    x = mesh.deformed_state(deck.nodes, k1=1.03)
    one = feahip.FeaSolver(deck)
    one.set_load_factor(0.7); one.set_nodes(x)
    F = one.surface_forces()
    assert np.abs(F).max() > 0
    seen = np.zeros(len(deck.nodes), dtype=int)
    for r, slab in enumerate(slabs_of(deck, 2)):
        assert len(slab.surface_kind) and slab.surface_faces.max() < len(slab.nodes)
        s = feahip.LocalRankSolver(slab, r, 2)
        s.set_load_factor(0.7); s.set_nodes(x[s.node_global])
        own = np.arange(3 * s.n_own)
        d = np.abs(s.surface_forces()[own] - F[dofs(s.node_global)[own]]).max() / np.abs(F).max()
        print(f"rank {r}: surface forces {d:.3e} of scale (bound 1e-13)")
        assert d < 1e-13
        seen[s.node_global[:s.n_own]] += 1
        # another rank's face (no owned node) is dropped silently; a face with a node that is not local is refused
        halo_faces = slab.surface_faces[np.all(slab.surface_faces >= slab.n_own, axis=1)]
        if len(halo_faces):
            s.set_surface_loads(halo_faces[:1], [feahip.LOAD_TRACTION], [[1.0, 1.0, 1.0]])
            assert np.abs(s.surface_forces()).max() == 0
        bad = slab.surface_faces[:1].copy(); bad[0, 0] = len(slab.nodes)
        with pytest.raises(feahip.FeaHipError, match="outside"):
            s.set_surface_loads(bad, slab.surface_kind[:1], slab.surface_values[:1])
        s.close()
    assert np.all(seen == 1)
    one.close()


# ------------------------------------------------------------------ 11: a one-rank slab
def test_one_rank_slab_is_the_unsharded_context(monkeypatch):
    """n_own = n_local: the whole block as one slab, in the deck's own ids.  Against FeaSolver under FEAHIP_RENUMBER=0
    (same ids, same kernels) K and f agree to 1e-12 of scale; bitwise is expected (both build the gather maps of rows
    [0, N) of the same pattern) and printed, not asserted.  Then the one-rank RCCL pattern: communicator + solve."""
    dims = (3, 24, 3)
    deck = mesh.bar_deck(dims=dims)
    slab = mesh.bar_slab(0, 1, dims=dims)
    assert slab.n_own == len(slab.nodes) == len(deck.nodes) and np.array_equal(slab.node_global, np.arange(len(deck.nodes)))
    x = mesh.deformed_state(deck.nodes, k1=1.03)
    monkeypatch.setenv("FEAHIP_RENUMBER", "0")
    one, K, f = whole_K_f(deck, x=x)
    monkeypatch.delenv("FEAHIP_RENUMBER")
    s = feahip.LocalRankSolver(slab, 0, 1)
    assert (s.N, s.n_own, s.E, s.N_global, s.rows_sent, s.rows_received) == (len(deck.nodes),) * 2 + (len(deck.elements), len(deck.nodes), 0, 0)
    s.set_nodes(x); s.create_stiffness_and_residual()
    lo, li, lv = s.matrix_yale()
    print("bitwise K:", np.array_equal(lv, K.data), " bitwise f:", np.array_equal(s.forces(), f))
    owned_rows_against(s, K, f, 1e-12, 1e-12)
    s.comm_init(0, 1, feahip.comm_unique_id())
    assert s.owned_rows() == (0, len(deck.nodes))
    s.set_nodes(deck.nodes); s.update_nodes_with_bc(1.0); s.create_stiffness_and_residual(); s.apply_prescribed_bc(0.0)
    it, res = s.solve_slae(feahip.PCG_ILU, 1e-14, 5000)
    one.set_nodes(deck.nodes); one.update_nodes_with_bc(1.0); one.create_stiffness_and_residual(); one.apply_prescribed_bc(0.0)
    it2, _ = one.solve_slae(feahip.PCG_ILU, 1e-14, 5000)
    assert abs(it - it2) <= 2 and rel(s.solution(), one.solution()) < 1e-11
    assert s.energy() == pytest.approx(one.energy(), rel=1e-11)
    s.close(); one.close()


# ------------------------------------------------------------------ 12: what the constructor refuses
def test_create_refuses_malformed_slabs():
    good = mesh.bar_slab(1, 3, dims=(2, 12, 2))
    n, no = len(good.nodes), good.n_own

    def refused(match, **change):
        s = copy.copy(good)
        for k, v in change.items():
            setattr(s, k, v)
        with pytest.raises(feahip.FeaHipError, match=match):
            feahip.LocalRankSolver(s, 1, 3)

    def edited(a, where, value):
        a = a.copy(); a[where] = value
        return a

    refused(r"\(-1\).*n_own = 0 ", n_own=0)
    refused(rf"n_own = {n + 1} ", n_own=n + 1)
    refused(rf"element 5 refers to local node {n} ", elements=edited(good.elements, (5, 2), n))
    refused(r"element 5 refers to local node -1 ", elements=edited(good.elements, (5, 2), -1))
    refused(r"element 7 has no owned node", elements=edited(good.elements, 7, np.arange(no, no + 4)))
    assert 0 not in good.node_global
    refused(rf"halo node {n} is touched by no element", nodes=np.vstack([good.nodes, [[9.0, 9.0, 9.0]]]),
            node_global=np.append(good.node_global, 0).astype(np.int32), halo_owner=np.append(good.halo_owner, 0).astype(np.int32))
    refused(r"halo_owner\[4\] = 3 outside", halo_owner=edited(good.halo_owner, 4, 3))
    refused(r"halo_owner\[4\] = -1 outside", halo_owner=edited(good.halo_owner, 4, -1))
    refused(r"halo_owner\[4\] = 1: .*this rank", halo_owner=edited(good.halo_owner, 4, 1))
    refused(rf"node_global\[2\] = {good.n_global_nodes} outside", node_global=edited(good.node_global, 2, good.n_global_nodes))
    refused(r"node_global\[9\] repeats node_global\[3\]", node_global=edited(good.node_global, 9, good.node_global[3]))
    refused(rf"prescribed entry 0: local node {n} outside", presc_node=np.array([n], dtype=np.int32),
            presc_type=np.array([7], dtype=np.int32), presc_values=np.zeros((1, 3)))
    s = feahip.LocalRankSolver(good, 1, 3)                                  # and the slab itself is taken
    assert (s.N, s.n_own) == (n, no)
    s.close()

"""The meshes of the PCG iterate tests (test_pcg_reference_cpu.py proves on the oracle's K that each keeps enough
iterates to compare; test_gpu_pcg.py compares them): the smallest that reach each branch of the loop's kernels."""
import numpy as np

import feahip
import mesh


def fan_deck(m=140):
    """The fan of test_node_with_more_neighbours_than_the_spmv_tile: a hub row of m + 3 = 143 blocks."""
    ang = 2 * np.pi * np.arange(m) / m
    ring = np.stack([np.cos(ang), np.sin(ang), np.zeros(m)], axis=1)
    nodes = np.vstack([[0.0, 0.0, 0.0], ring, [0.0, 0.0, 0.7], [0.0, 0.0, -0.7]])
    top, bot = m + 1, m + 2
    el = []
    for i in range(m):
        a, b = 1 + i, 1 + (i + 1) % m
        el.append([0, a, b, top])
        el.append([0, b, a, bot])
    return feahip.Deck(nodes=nodes, elements=np.array(el, dtype=np.int32), ele_type=feahip.TETRAHEDRA4, gauss_nodes_count=1,
                       presc_node=[top, bot, 1], presc_type=[7, 7, 2], presc_values=np.zeros((3, 3)))


def fan_state(deck):
    """its deformed state in that test"""
    return deck.nodes * np.array([1.02, 0.99, 1.05]) + 1e-3 * np.sin(3 * deck.nodes[:, [1, 2, 0]])


# name -> (deck, nodes to set or None, node count or None)
MESHES = {
    "tet4_64_tail_node": (lambda: mesh.bar_deck(dims=(3, 3, 3)), None, 64),        # 3 * 21 + 1: one tail node in the wave loop
    "tet4_63_three_steps": (lambda: mesh.bar_deck(dims=(2, 6, 2)), None, 63),      # exactly three steps of 21 nodes
    "tet4_144": (lambda: mesh.bar_deck(dims=(3, 8, 3)), None, 144),
    "tet4_343_two_workgroups": (lambda: mesh.bar_deck(dims=(6, 6, 6)), None, 343), # > 256 nodes: two workgroups of the vector kernels
    "hex8": (lambda: mesh.bar_deck(dims=(2, 6, 2), hexa=True), None, None),
    "tet10": (lambda: mesh.bar_deck(dims=(2, 4, 2), quadratic=True), None, None),
    "fan_hub_143_blocks": (fan_deck, fan_state, None),                              # the long-row branch of the fused dot
}
# name -> (deck, ranks).  Rows are dealt out in supers of 8 SpMV chunks (shard_chunks below, asserted in
# test_pcg_reference_cpu.py): tet4_144 has two supers -- on 2 ranks the second rank's interior range runs to its last
# chunk (nothing behind it), on 3 ranks rank 0 owns no row at all; the 216-node cube has three -- the middle rank's 8
# chunks all touch a halo column, so enq_spmv_interior launches nothing and k_cgcg_reduce sums no interior partials, and
# rank 0's interior range starts at its first chunk (nothing in front); the 54-node bar is one super -- two ranks
# without rows.
SHARDED = {
    "tet4_144": (lambda: mesh.bar_deck(dims=(3, 8, 3)), (2, 3)),
    "cube_216_no_interior": (lambda: mesh.bar_deck(dims=(5, 5, 5)), (3,)),
    "bar_54_one_super": (lambda: mesh.bar_deck(dims=(2, 5, 2)), (3,)),
}
MULTIGRID_DIMS = (3, 12, 3)
# the environment knobs of the multigrid hierarchy: a test that compares with the reference cycle clears them
AMG_ENV = ("FEAHIP_AMG_TAIL", "FEAHIP_AMG_TAIL_ELL", "FEAHIP_AMG_TAIL_BLOB", "FEAHIP_AMG_TAIL_COP", "FEAHIP_AMG_FUSED_POST",
           "FEAHIP_AMG_FINE_BITS", "FEAHIP_AMG_F32", "FEAHIP_AMG_GAMMA", "FEAHIP_AMG_GAMMA_UNTIL", "FEAHIP_AMG_GAMMA_FROM",
           "FEAHIP_AMG_SWEEPS", "FEAHIP_AMG_COARSEST", "FEAHIP_AMG_OVER")
BATCH_DIMS = (3, 8, 3)


def case(name):
    make, state, count = MESHES[name]
    deck = make()
    if count is not None:
        assert len(deck.nodes) == count
    return deck, (state(deck) if state else None)


CHUNK_ROWS, CHUNK_BLOCKS, SUPER_CHUNKS = 16, 128, 8    # FEA_CHUNK_ROWS, FEA_CHUNK_BLOCKS, FEA_SUPER_CHUNKS (feahip_internal.h)


def spmv_chunks(deck):
    """Host only.  The SpMV chunks of pattern.cpp, restated: consecutive rows in the library's numbering, closed at 16 rows
    or 128 blocks (a row with more blocks than that is a chunk of its own).  (first row of every chunk and N at the end,
    neighbour set of every row -- its blocks --, renumbered?)."""
    N = len(deck.nodes)
    lib, renumbered = feahip.host_numbering(deck.elements, deck.nodes)
    el = lib[np.asarray(deck.elements)]
    nbr = [set([a]) for a in range(N)]
    for e in el:
        for a in e:
            nbr[a].update(e)
    chunk, rows, blocks = [0], 0, 0
    for a in range(N):
        if rows > 0 and (rows == CHUNK_ROWS or blocks + len(nbr[a]) > CHUNK_BLOCKS):
            chunk.append(a); rows = blocks = 0
        rows += 1; blocks += len(nbr[a])
    chunk.append(N)
    return chunk, nbr, renumbered


def shard_chunks(deck, n):
    """Host only.  What install_plan (dist.hip) finds for every rank of FeaGroup(deck, n), restated: the SpMV chunks
    (spmv_chunks above), the rank's rows (shard.cpp: whole supers of 8 chunks, supers s with
    n_super r / n <= s < n_super (r + 1) / n), and the longest run of its chunks whose rows have no column outside the
    rank's rows.  Per rank: dict(row0, row1, chunks, lo, hi) -- enq_spmv_interior multiplies chunks [lo, hi) of the rank,
    enq_spmv_boundary the lo in front and the chunks - hi behind."""
    chunk, nbr, _ = spmv_chunks(deck)
    nchunks = len(chunk) - 1
    nsuper = (nchunks + SUPER_CHUNKS - 1) // SUPER_CHUNKS
    out = []
    for r in range(n):
        c0, c1 = (min(nchunks, (nsuper * k // n) * SUPER_CHUNKS) for k in (r, r + 1))
        row0, row1 = chunk[c0], chunk[c1]
        inside = [all(row0 <= j < row1 for a in range(chunk[k], chunk[k + 1]) for j in nbr[a]) for k in range(c0, c1)]
        best, lo = (0, 0), -1
        for k, ok in enumerate(inside + [False]):
            if ok and lo < 0:
                lo = k
            elif not ok and lo >= 0:
                if k - lo > best[1] - best[0]:
                    best = (lo, k)
                lo = -1
        out.append(dict(row0=row0, row1=row1, chunks=c1 - c0, lo=best[0], hi=best[1]))
    return out


def prescribed_dofs(deck):
    return np.array(sorted(3 * n + j for n, t in zip(deck.presc_node, deck.presc_type) for j in range(3) if t & (1 << j)))


def masked_system(solver, x=None):
    """What the linear solve of the first Newton step sees: nodes moved to the boundary values (or set to x), K and f
    assembled, the prescribed dofs masked.  For FeaSolver and OracleSolver alike."""
    if x is not None:
        solver.set_nodes(x)
    else:
        solver.update_nodes_with_bc(1.0)
    if hasattr(solver, "create_stiffness_and_residual"):
        solver.create_stiffness_and_residual()
    else:
        solver.update_state(); solver.create_stiffness(); solver.create_residual_forces()
    solver.apply_prescribed_bc(0.0)

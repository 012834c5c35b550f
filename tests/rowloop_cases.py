"""The meshes that put the block-row product kernels at the limits of their tile (host only, no device).

Eight kernels share one row loop (spmv_body, k_gershgorin, k_spmv2, k_spmm_km, mass_rows_body, k_mass_blocks / k_mass_lump,
damp_rows_body, k_geom_blocks): a wave owns a chunk of at most 16 block rows and 128 blocks, lane k takes the blocks k and
k + 64, and a row with more than 128 blocks is strided over.  Three of them (spmv_body<double>, k_spmv2,
damp_rows_body<true, .>) stage the chunk's 72-byte blocks through LDS as 16-byte pieces from the 16-byte boundary below
72 b0: at most 577 pieces, the last of which exists only for a 128-block chunk that starts at an odd block.

LIMITS names the smallest meshes that reach each of these shapes and says, as a predicate on the chunk table, which.
tests/test_rowloop_cases_host.py proves the predicates on the CPU; tests/test_gpu_rowloop_limits.py runs the kernels
there."""
import numpy as np

import feahip
from explicit_reference import hub_fan
from pcg_cases import CHUNK_BLOCKS, CHUNK_ROWS, fan_deck, shard_chunks, spmv_chunks

NPMAX = (15 + CHUNK_BLOCKS * 72 + 15) >> 4          # 577: the staged kernels' bound on a chunk's 16-byte pieces


def staged_pieces(b0, nb):
    """16-byte pieces the staged kernels read for a chunk of nb 72-byte blocks that starts at block b0."""
    sh = (72 * b0) & 15
    return (sh + 72 * nb + 15) >> 4


def reordered(deck, order, isolated_before=0, isolated_after=0):
    """The deck with its nodes in the order given (order[k] = old id of the new node k), with isolated nodes -- nodes that
    no element uses -- in front and behind.  They lie away from the body and are left free."""
    order = np.asarray(order, dtype=np.int64)
    assert sorted(order) == list(range(len(deck.nodes)))
    new_id = np.empty(len(order), dtype=np.int64)
    new_id[order] = isolated_before + np.arange(len(order))
    iso = lambda n, z: np.array([[3.0 + k, 3.0, z] for k in range(n)]).reshape(n, 3)
    nodes = np.vstack([iso(isolated_before, 3.0), deck.nodes[order], iso(isolated_after, -3.0)])
    return feahip.Deck(ele_type=deck.ele_type, gauss_nodes_count=deck.gauss_nodes_count, nodes=nodes,
                       elements=new_id[np.asarray(deck.elements)].astype(np.int32), modified_newton=False, solver_type=feahip.CG,
                       presc_node=new_id[np.asarray(deck.presc_node)].astype(np.int32),
                       presc_type=np.asarray(deck.presc_type, dtype=np.int32), presc_values=np.asarray(deck.presc_values))


def hub_variant(spokes, order, isolated_before=0, isolated_after=0):
    """hub_fan(spokes) with its nodes ordered by `order`, a permutation of "hub", "pole", "ring"."""
    d = hub_fan(spokes)
    parts = {"hub": [0], "ring": list(range(1, spokes + 1)), "pole": [spokes + 1]}
    return reordered(d, sum((parts[k] for k in order), []), isolated_before, isolated_after)


def chunk_table(deck):
    """[(r0, r1, b0, nb)] of the SpMV chunks: rows [r0, r1) of the library's numbering, first block, block count."""
    chunk, nbr, _ = spmv_chunks(deck)
    rowptr = np.concatenate([[0], np.cumsum([len(s) for s in nbr])])
    return [(int(r0), int(r1), int(rowptr[r0]), int(rowptr[r1] - rowptr[r0])) for r0, r1 in zip(chunk[:-1], chunk[1:])]


def renumbered(deck):
    return spmv_chunks(deck)[2]


def shapes(table):
    """{(rows, b0, nb)} of a chunk table."""
    return {(r1 - r0, b0, nb) for r0, r1, b0, nb in table}


def _has(*want):
    return lambda deck, table: set(want) <= shapes(table)


def _fan126(deck, table):
    last = table[-1]
    return (set([(1, 0, 129), (1, 885, 128), (1, 1013, 128)]) <= shapes(table) and len(table) == 11
            and (last[1] - last[0], last[2], last[3]) == (1, 1013, 128)
            and (72 * (last[2] + last[3])) % 16 == 8                       # the last block ends 8 bytes past a 16-byte boundary
            and staged_pieces(885, 128) == NPMAX and staged_pieces(1013, 128) == NPMAX)


def rank_first_block(deck, n, rank):
    """kb0 of a rank of FeaGroup(deck, n): the first block of its first row."""
    row0 = shard_chunks(deck, n)[rank]["row0"]
    return next(b0 for r0, _, b0, _ in chunk_table(deck) if r0 == row0)


def _fan126_sharded(deck, table):
    plan = shard_chunks(deck, 2)
    return plan[0]["chunks"] == 8 and plan[1]["chunks"] == 3 and rank_first_block(deck, 2, 1) == 801


def _last_is(shape):
    return lambda deck, table: (table[-1][1] - table[-1][0], table[-1][2], table[-1][3]) == shape


# name -> (deck builder, predicate(deck, chunk table)); chunks are (rows, b0, nb)
LIMITS = {
    # (1, 0, 129): the smallest long row; (1, 885, 128), (1, 1013, 128): full tiles at odd b0, 577 staged pieces, the
    # second the matrix's last chunk, whose last piece ends in the array's padding
    "fan126": (lambda: fan_deck(126), _fan126),
    # eleven chunks are two supers: rank 1 of 2 owns the last three and starts at block 801 (odd kb0)
    "fan126_rank1_of_2": (lambda: fan_deck(126), _fan126_sharded),
    "fan125": (lambda: fan_deck(125), _has((1, 0, 128), (1, 878, 127), (1, 1005, 127))),      # a full tile at b0 = 0
    "fan127": (lambda: fan_deck(127), _has((1, 0, 130), (1, 892, 129), (1, 1021, 129))),      # long rows at either parity
    "hub27_hub_pole_ring": (lambda: hub_variant(27, ("hub", "pole", "ring")), _has((16, 0, 128), (13, 128, 65))),
    "hub66_iso_hub_pole_ring": (lambda: hub_variant(66, ("hub", "pole", "ring"), 1), _has((2, 0, 69), (13, 69, 128))),
    "hub22_iso_hub_ring_pole": (lambda: hub_variant(22, ("hub", "ring", "pole"), 1), _has((16, 0, 95), (9, 95, 64))),
    "hub23_hub_ring_pole": (lambda: hub_variant(23, ("hub", "ring", "pole")), _has((16, 0, 100), (9, 100, 65))),
    "hub29_hub_ring_pole_iso2": (lambda: hub_variant(29, ("hub", "ring", "pole"), 0, 2), _last_is((1, 208, 1))),
}

# shape name -> predicate on a chunk table: what the entries of LIMITS must reach between them
SHAPES = {
    "nb == 1": lambda t: any(nb == 1 for _, _, _, nb in t),
    "nb == 64": lambda t: any(nb == 64 for _, _, _, nb in t),
    "nb == 65": lambda t: any(nb == 65 for _, _, _, nb in t),
    "nb == 128, one row, even b0": lambda t: any(nb == 128 and r1 - r0 == 1 and b0 % 2 == 0 for r0, r1, b0, nb in t),
    "nb == 128, one row, odd b0, last chunk": lambda t: t[-1][3] == 128 and t[-1][1] - t[-1][0] == 1 and t[-1][2] % 2 == 1,
    "nb == 128, several rows, odd b0": lambda t: any(nb == 128 and r1 - r0 > 1 and b0 % 2 == 1 for r0, r1, b0, nb in t),
    "nb == 128 with 16 rows": lambda t: any(nb == 128 and r1 - r0 == CHUNK_ROWS for r0, r1, b0, nb in t),
    "nb == 129": lambda t: any(nb == 129 for _, _, _, nb in t),
    "nb == 130": lambda t: any(nb == 130 for _, _, _, nb in t),
    "np == 577": lambda t: any(nb <= CHUNK_BLOCKS and staged_pieces(b0, nb) == NPMAX for _, _, b0, nb in t),
}


# ---- long-double references and rounding bounds of the products (host only) --------------------------------------------
LD = np.longdouble
U = 2.0 ** -53
RHO = 2.5


def gamma(k):
    """k u / (1 - k u): the relative error of a result that k roundings lie behind, in any order, fused or not, on the scale
    of its expression evaluated with every operand replaced by its absolute value."""
    k = np.asarray(k, dtype=LD)
    return k * U / (1 - k * U)


def limit_state(deck):
    """a smoothly deformed state (pcg_cases.fan_state)"""
    return deck.nodes * np.array([1.02, 0.99, 1.05]) + 1e-3 * np.sin(3 * deck.nodes[:, [1, 2, 0]])


def det3(m):
    return (m[..., 0, 0] * (m[..., 1, 1] * m[..., 2, 2] - m[..., 1, 2] * m[..., 2, 1])
            - m[..., 0, 1] * (m[..., 1, 0] * m[..., 2, 2] - m[..., 1, 2] * m[..., 2, 0])
            + m[..., 0, 2] * (m[..., 1, 0] * m[..., 2, 1] - m[..., 1, 1] * m[..., 2, 0]))


def perm3(m):
    """det3 with every operand replaced by its absolute value and every minus by a plus"""
    m = np.abs(m)
    return (m[..., 0, 0] * (m[..., 1, 1] * m[..., 2, 2] + m[..., 1, 2] * m[..., 2, 1])
            + m[..., 0, 1] * (m[..., 1, 0] * m[..., 2, 2] + m[..., 1, 2] * m[..., 2, 0])
            + m[..., 0, 2] * (m[..., 1, 0] * m[..., 2, 1] + m[..., 1, 1] * m[..., 2, 0]))


def block_rows(deck):
    """(blocks of every row, elements that hold both nodes of every pair [N][N]) in the deck's ids"""
    N = len(deck.nodes)
    pairs = np.zeros((N, N), dtype=np.int64)
    for nd in deck.elements:
        pairs[np.ix_(nd, nd)] += 1
    nb = np.maximum((pairs > 0).sum(axis=1), 1)                            # an isolated node keeps its diagonal block
    return nb, pairs


def mass_rule(deck):
    from dynamics_reference import MASS_POINTS
    return tuple(np.asarray(t, dtype=LD) for t in feahip.element_tables(deck.ele_type, MASS_POINTS[deck.ele_type]))


def mass_long_double(deck, rho=RHO):
    """(m, |m|) [N][N] in long double: the scalar consistent mass by the formula of dynamics_reference.dense_mass,
    m_ab = sum_e rho sum_g w_g det J0_g N_a N_b, and the same expression with every operand replaced by its absolute
    value (det J0 is a sum of signed products: the scale its rounding errors live on is the second)."""
    w, N, dN = mass_rule(deck)
    X = np.asarray(deck.nodes, dtype=LD)
    n = len(X)
    m, mabs = np.zeros((n, n), dtype=LD), np.zeros((n, n), dtype=LD)
    for nd in deck.elements:
        J = np.einsum("gik,kj->gij", dN, X[nd])
        Jabs = np.einsum("gik,kj->gij", np.abs(dN), np.abs(X[nd]))
        wd, wdabs = LD(rho) * w * det3(J), LD(rho) * w * perm3(Jabs)
        assert np.all(wd > 0)
        m[np.ix_(nd, nd)] += np.einsum("g,ga,gb->ab", wd, N, N)
        mabs[np.ix_(nd, nd)] += np.einsum("g,ga,gb->ab", wdabs, np.abs(N), np.abs(N))
    return m, mabs


def mass_entry_roundings(deck):
    """Roundings behind one term rho w_g det J0_g N_a N_b of the device's m (k_mass_elements, k_mass_blocks): an entry of
    J0 is a sum of npe products (npe + 1), det J0 a cofactor expansion (5), rho w det (2), times N_a N_b (2)."""
    return (deck.elements.shape[1] + 1) + 5 + 2 + 2


def mass_row_roundings(deck):
    """[N]: roundings behind row a of y = m x where the device also forms m: the term above, the entry's own sum (its
    Gm points and one addition per element that holds the pair: (Gm + 1) E_ab, the longest of the row), the product with
    x (1) and the row's sum over its blocks (nb_a)."""
    nb, pairs = block_rows(deck)
    gm = len(mass_rule(deck)[0])
    return mass_entry_roundings(deck) + (gm + 1) * pairs.max(axis=1) + 1 + nb


def dof_rows(per_node):
    return np.repeat(np.asarray(per_node), 3)


def scalar_blocks(m):
    """[N][N] -> [3N][3N]: m (x) I"""
    return np.kron(m, np.eye(3, dtype=LD))


def lumped_roundings(deck):
    """(n [N], kappa): roundings behind ml_a = sum_e m_e d_a / sum_b d_b (k_mass_lump) -- m_e, d_a and sum_b d_b each carry
    rho w det (npe + 8) and their own sums over the mass points (Gm + 2), then the npe terms of the denominator, the
    product and the quotient (2) and one addition per element of the node.  Every operand is positive except inside det J0,
    whose relative error is larger by kappa = max_e perm |J0| / det J0."""
    w, N, dN = mass_rule(deck)
    X = np.asarray(deck.nodes, dtype=LD)
    npe, gm = deck.elements.shape[1], len(w)
    kappa = 1.0
    for nd in deck.elements:
        J = np.einsum("gik,kj->gij", dN, X[nd])
        Jabs = np.einsum("gik,kj->gij", np.abs(dN), np.abs(X[nd]))
        kappa = max(kappa, float((perm3(Jabs) / det3(J)).max()))
    count = np.bincount(np.asarray(deck.elements).ravel(), minlength=len(X))
    return 3 * (npe + 8 + gm + 2) + npe + 2 + count, kappa

"""The decks and caps of the LOBPCG iterate tests.  test_lobpcg_reference_cpu.py asserts on the oracle's K that every
(case, k) here meets the guards (the scaled G_M of every step at least 1e-10, both precisions on the same branch, every
deciding ratio / tol outside [1/3, 3]), so that test_gpu_lobpcg.py never has to skip; a (case, k) that fails one is taken
out of this list, not skipped."""
import functools

import numpy as np

import mesh
from dynamics_reference import DENSITIES, free_block, loaded_bar
from hetero_reference import MATERIALS, layered_ids, with_materials
from modal_reference import ModalReference
from pcg_cases import fan_deck

RHO = 1.5
ALL_K = (0, 1, 2, 3, 5, 8, 22)


def _two_materials():
    base = loaded_bar("tet4", (2, 4, 2))
    return with_materials(base, MATERIALS[:2], layered_ids(base, 2))


# name -> (deck, element type, density or one per material, the caps k of the capped solves)
CASES = {
    "tet4": (lambda: loaded_bar("tet4", (3, 8, 3)), "tet4", RHO, ALL_K),
    "hex8": (lambda: loaded_bar("hex8", (3, 8, 3)), "hex8", RHO, ALL_K),
    "tet10": (lambda: loaded_bar("tet10", (2, 4, 2)), "tet10", RHO, ALL_K),
    "fan_143_nodes": (fan_deck, "tet4", RHO, ALL_K),                    # 429 dofs: the last 32-dof Gram tile is partial
    "tet4_two_materials": (_two_materials, "tet4", DENSITIES[:2], ALL_K),
}
PAIRS = [(name, k) for name, c in CASES.items() for k in c[3]]

SMALLEST = lambda: loaded_bar("tet4", (1, 2, 1))                         # 12 nodes, 4 clamped: n_free == 24
MULTIGRID = (lambda: mesh.bar_deck(dims=(3, 12, 3)), (1, 3))
# name -> (deck, ranks): with three ranks rank 0 of the tet4 bar owns no row, and two ranks of the 54-node bar own none
# (pcg_cases.SHARDED)
SHARDED = {
    "tet4": (lambda: loaded_bar("tet4", (3, 8, 3)), (2, 3)),
    "hex8": (lambda: loaded_bar("hex8", (3, 8, 3)), (2, 3)),
    "bar_54_one_super": (lambda: mesh.bar_deck(dims=(2, 5, 2)), (3,)),
}
SHARDED_K = (1, 3, 8)
# name -> (deck, modes, how the shift is chosen): restated and checked on the host alone (test_lobpcg_reference_cpu.py says why)
LOCKED = {
    "tet4": (lambda: loaded_bar("tet4", (3, 8, 3)), 12, None),
    "free_tet4": (lambda: free_block("tet4", (3, 3, 3), parameters=[100, 100]), 12, "two digits of lambda_7"),
}
GRID_STRIDE_DIMS, GRID_STRIDE_K = (40, 40, 40), 3                        # 41^3 = 68921 nodes > 65536


def deck_of(name):
    return CASES[name][0]()


def density(name):
    return CASES[name][2]


@functools.lru_cache(maxsize=None)
def reference(name):
    """The float64 pencil of a case on the oracle's K (modal_reference.py), computed once and read-only."""
    deck = deck_of(name)
    if name == "tet4_two_materials":
        ref = ModalReference(deck, DENSITIES[:2], materials=MATERIALS[:2], ids=layered_ids(deck, 2))
    else:
        ref = ModalReference(deck, RHO)
    for a in (ref.lam, ref.Phi, ref.K, ref.M):
        a.setflags(write=False)
    return ref


def two_digits(v):
    return float(f"{v:.1e}")


def prescribed_mask(deck):
    mask = np.zeros(3 * len(deck.nodes), dtype=bool)
    for n, t in zip(np.asarray(deck.presc_node).ravel(), np.asarray(deck.presc_type).ravel()):
        for j in range(3):
            if int(t) & (1 << j):
                mask[3 * int(n) + j] = True
    return mask

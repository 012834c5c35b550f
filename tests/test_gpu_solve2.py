"""The two-right-hand-side solve on the MI355X (kernels_solve2.hip): the two-vector product against a float64 product
with the Yale matrix, feahip_solve_slae2 against single solves, the freezing of the column that converges first, what
the solve refuses, and bitwise reproducibility."""
import numpy as np
import pytest
import scipy.sparse as sp

import feahip
import mesh
from test_gpu_parity import U_TOL, rel          # the tolerance of u against the direct solve, and its norm

pytestmark = pytest.mark.gpu

SOLVER_TOL, SOLVER_MAX = 1e-15, 20000            # test_linear_solve_matches_direct_solver


def _fan_deck(m=140):
    """A fan of tetrahedra pairs around one node: its block row has m + 3 = 143 blocks, more than the 128-block tile
    (test_node_with_more_neighbours_than_the_spmv_tile)."""
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


SPMV_DECKS = {
    "tet4": lambda: mesh.bar_deck(dims=(3, 3, 3)),
    "tet10": lambda: mesh.bar_deck(dims=(2, 2, 2), quadratic=True),
    "hex8": lambda: mesh.bar_deck(dims=(3, 3, 3), hexa=True),
    "fan": _fan_deck,
}


@pytest.mark.parametrize("kind", sorted(SPMV_DECKS))
def test_spmv2_against_a_float64_product(kind):
    deck = SPMV_DECKS[kind]()
    s = feahip.FeaSolver(deck)
    s.set_nodes(mesh.deformed_state(deck.nodes, k1=1.03))
    s.create_stiffness_and_residual()
    off, idx, val = s.matrix_yale()
    K = sp.csr_matrix((val, idx, off), shape=(s.ndof, s.ndof))
    absK = sp.csr_matrix((np.abs(val), idx, off), shape=(s.ndof, s.ndof))
    nterms = np.diff(off)
    if kind == "fan":
        assert nterms.max() == 3 * 143                                    # the long-row path runs
    rng = np.random.default_rng(17)
    a, b, zero = rng.normal(size=s.ndof), rng.normal(size=s.ndof), np.zeros(s.ndof)
    for x2 in (np.stack([a, b]), np.stack([zero, b]), np.stack([a, zero])):
        y2 = s.spmv2(x2)
        for c in range(2):
            # the worst case of a fixed-order sum of n products: n 2^-52 (|K| |x|) per row
            bound = nterms * 2.0 ** -52 * (absK @ np.abs(x2[c]))
            err = np.abs(y2[c] - K @ x2[c])
            assert np.all(err <= bound), (kind, c, float((err / np.maximum(bound, 1e-300)).max()))
        if not x2[0].any():
            assert not y2[0].any()                                         # nothing of the other column lands here
        if not x2[1].any():
            assert not y2[1].any()
    assert np.array_equal(s.spmv2(np.stack([a, b])), s.spmv2(np.stack([a, b])))
    s.close()


def _masked_system(dims=(6, 36, 6)):
    deck = mesh.bar_deck(dims=dims)
    s = feahip.FeaSolver(deck)
    s.set_pcg_variant(0)
    s.update_nodes_with_bc(1.0)
    s.create_stiffness_and_residual()
    s.apply_prescribed_bc(0.0)
    return deck, s


def _free_dof(deck):
    cd = {3 * n + j for n, t in zip(deck.presc_node, deck.presc_type) for j in range(3) if t & (1 << j)}
    mid = 3 * (len(deck.nodes) // 2)
    return next(k for k in range(mid, 3 * len(deck.nodes)) if k not in cd)


@pytest.mark.parametrize("solver,precond", [(feahip.CG, 0), (feahip.PCG_ILU, 0), (feahip.PCG_ILU, 1)])
def test_solve_slae2_equals_single_solves(solver, precond):
    deck, s = _masked_system()
    if precond:
        s.set_preconditioner(precond)
    f = s.forces()
    f2 = np.zeros(s.ndof)
    f2[_free_dof(deck)] = 1.0                                              # one loaded dof: another difficulty than f
    it, res = s.solve_slae2(f2, solver, SOLVER_TOL, SOLVER_MAX)
    u, u2 = s.solution(), s.solution2()
    assert np.all(it > 0) and np.all(res < 1e-14)
    assert it[0] != it[1], it                                              # the columns stop at different iterations
    # each column is the single solve of its right-hand side
    s.solve_slae(solver, SOLVER_TOL, SOLVER_MAX)
    assert rel(u, s.solution()) < U_TOL
    s.set_forces(f2)
    s.solve_slae(solver, SOLVER_TOL, SOLVER_MAX)
    assert rel(u2, s.solution()) < U_TOL
    s.set_forces(f)
    # the early column is frozen: the iterations that follow leave it as a solve capped at its own count does
    early = int(np.argmin(it))
    itc, _ = s.solve_slae2(f2, solver, SOLVER_TOL, int(it[early]))
    capped = (s.solution(), s.solution2())[early]
    assert itc[early] == it[early]
    assert np.array_equal(capped, (u, u2)[early])
    # the same right-hand side twice: the same bits in both columns
    it, _ = s.solve_slae2(f, solver, SOLVER_TOL, SOLVER_MAX)
    assert it[0] == it[1]
    assert np.array_equal(s.solution(), s.solution2())
    s.close()


def test_solve_slae2_is_reproducible():
    deck, s = _masked_system(dims=(3, 8, 3))
    f2 = np.random.default_rng(5).normal(size=s.ndof)
    cd = [3 * n + j for n, t in zip(deck.presc_node, deck.presc_type) for j in range(3) if t & (1 << j)]
    f2[cd] = 0.0
    out = []
    for _ in range(2):
        it, res = s.solve_slae2(f2, feahip.PCG_ILU, SOLVER_TOL, SOLVER_MAX)
        out.append((it.copy(), res.copy(), s.solution(), s.solution2()))
    for a, b in zip(*out):
        assert np.array_equal(a, b)
    assert np.all(s.solution2()[cd] == 0)                                  # increments at prescribed dofs are exactly 0
    s.close()


def _rc(s, fn):
    with pytest.raises(feahip.FeaHipError) as e:
        fn()
    return str(e.value)


def test_solve_slae2_refusals():
    deck = mesh.bar_deck(dims=(6, 36, 6))                                    # large enough for the multigrid kinds to be set
    f2 = np.zeros(3 * len(deck.nodes))
    s = feahip.FeaSolver(deck)
    msg = _rc(s, lambda: s.solve_slae2(f2, feahip.CG, 1e-12, 10))
    assert f"error {feahip.ESTATE}" in msg and "no stiffness matrix" in msg   # before the first assembly
    s.create_stiffness_and_residual()
    s.apply_prescribed_bc(0.0)
    s.solve_slae2(f2, feahip.CG, 1e-12, 10)                                  # fine now
    s.set_preconditioner(2)
    msg = _rc(s, lambda: s.solve_slae2(f2, feahip.PCG_ILU, 1e-12, 10))
    assert f"error {feahip.EINVAL}" in msg and "preconditioner 2" in msg
    s.set_preconditioner(0)
    s.set_row_shard(0, 2)
    s.create_stiffness_and_residual()
    msg = _rc(s, lambda: s.solve_slae2(f2, feahip.CG, 1e-12, 10))
    assert f"error {feahip.EINVAL}" in msg and "row-sharded" in msg
    msg = _rc(s, lambda: s.spmv2(np.zeros((2, s.ndof))))
    assert f"error {feahip.EINVAL}" in msg
    s.close()
    g = feahip.FeaGroup(deck, 2)
    m = g.ranks[0]
    m.create_stiffness_and_residual()
    msg = _rc(m, lambda: m.solve_slae2(f2, feahip.CG, 1e-12, 10))
    assert f"error {feahip.EINVAL}" in msg and "transport" in msg
    g.close()

"""The node-ordered views of the C ABI on the MI355X (csrc/node_views.h behind get_view / set_view, the block column
helpers and the shared argument check of fea-large_amd/csrc/feahip_api.hip): every entry speaks the CALLER's node ids
whatever the library's numbering is.  One jittered, randomly numbered lattice of 256 nodes -- the smallest bar the
library renumbers (renumber.cpp keeps anything below four cells of 64 nodes as it is) -- and a two-context in-process
group on it for the rows a shard does not own."""
import functools

import numpy as np
import pytest

import feahip
import mesh
from results_reference import cauchy, von_mises

pytestmark = pytest.mark.gpu

DIMS = (3, 15, 3)                                              # 4 x 16 x 4 = 256 nodes
RHO = 1.3
STRETCH = np.array([[1.05, 0.02, 0.01], [0.015, 0.97, 0.03], [-0.01, 0.025, 1.04]])   # all six stress lanes differ


@functools.lru_cache(maxsize=None)
def the_deck():
    return mesh.jitter_permute(mesh.bar_deck(dims=DIMS), amp=0.2, seed=4)


def rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max()


def assembled(s, x, rho=None):
    if rho is not None:
        s.set_mass(rho)
    s.set_nodes(x)
    s.create_stiffness_and_residual()


@pytest.mark.parametrize("renumber", [True, False])
def test_round_trips_are_bit_exact_in_the_callers_order(renumber, monkeypatch):
    """set_nodes / nodes, set_forces / forces, set_velocities / velocities, set_accelerations / accelerations with
    random input, under the library's numbering and with the caller's ids kept (FEAHIP_RENUMBER=0)."""
    deck = the_deck()
    if not renumber:
        monkeypatch.setenv("FEAHIP_RENUMBER", "0")
    s = feahip.FeaSolver(deck)
    assert np.array_equal(s.node_numbering(), np.arange(s.N)) == (not renumber)
    rng = np.random.default_rng(11)
    f, v, a, x = rng.normal(size=s.ndof), rng.normal(size=(s.N, 3)), rng.normal(size=(s.N, 3)), rng.normal(size=(s.N, 3))
    s.set_forces(f)
    assert np.array_equal(s.forces(), f)
    s.set_mass(RHO)
    s.set_velocities(v); s.set_accelerations(a)
    assert np.array_equal(s.velocities(), v) and np.array_equal(s.accelerations(), a)
    assert np.array_equal(s.forces(), f)                       # (each vector its own)
    s.set_nodes(x)
    assert np.array_equal(s.nodes(), x)
    s.close()


def test_update_nodes_with_solution_moves_node_a_by_u_a():
    deck = the_deck()
    s = feahip.FeaSolver(deck)
    assert not np.array_equal(s.node_numbering(), np.arange(s.N))
    x = mesh.deformed_state(deck.nodes, k1=1.07)
    u = 0.01 * np.random.default_rng(12).normal(size=s.ndof)
    s.set_nodes(x)
    s.update_nodes_with_solution(u)
    err = rel(s.nodes(), x + u.reshape(-1, 3))
    print("update_nodes_with_solution: relative error", err)
    assert err < 1e-15
    s.close()


def test_nodal_stresses_are_indexed_by_the_callers_node():
    """A homogeneous stretch x = F X: the stress is F's closed form at every node, so sig6 and von Mises say nothing about
    the order -- the weight (the current volume of the elements around a node) does: a corner of the bar against a node
    in its middle, each read at the caller's index, and the whole field.  Bounds: 1e-12 of the field's scale, what
    tests/test_gpu_results.py holds 4-node tetrahedra to."""
    deck = the_deck()
    s = feahip.FeaSolver(deck)
    assert not np.array_equal(s.node_numbering(), np.arange(s.N))
    x = deck.nodes @ STRETCH.T
    s.set_nodes(x)
    sig6, vm, wt = s.nodal_stresses()
    sig = cauchy(STRETCH, deck.model, deck.parameters[0], deck.parameters[1])
    want6 = np.array([sig[0, 0], sig[1, 1], sig[2, 2], sig[0, 1], sig[1, 2], sig[0, 2]])
    scale = np.abs(want6).max()
    es, ev = np.abs(sig6 - want6).max() / scale, np.abs(vm - von_mises(want6)).max() / scale
    p = x[deck.elements]
    vol = np.abs(np.einsum("ij,ij->i", np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), p[:, 3] - p[:, 0])) / 6.0
    want = np.zeros(s.N)
    for k in range(4):
        np.add.at(want, deck.elements[:, k], vol)
    lo, hi = deck.nodes.min(axis=0), deck.nodes.max(axis=0)
    corner = int(np.argmin(np.abs(deck.nodes - lo).sum(axis=1)))
    inner = int(np.argmin(np.abs(deck.nodes - 0.5 * (lo + hi)).sum(axis=1)))
    assert want[inner] > 4.0 * want[corner]                    # 24 tetrahedra around the one, at most 6 around the other
    ew = np.abs(wt - want).max() / want.max()
    print("nodal stresses: sigma", es, "von Mises", ev, "weight", ew, "corner", wt[corner], want[corner], "inner", wt[inner], want[inner])
    assert abs(wt[corner] - want[corner]) <= 1e-12 * want[corner] and abs(wt[inner] - want[inner]) <= 1e-12 * want[inner]
    assert es <= 1e-12 and ev <= 1e-12 and ew <= 1e-12
    s.close()


@pytest.fixture(scope="module")
def pair():
    """(deck, x, one context, a two-context group), each with mass, nodes x and K assembled; preconditioner 0."""
    deck = the_deck()
    x = mesh.deformed_state(deck.nodes, k1=1.07)
    one = feahip.FeaSolver(deck)
    assembled(one, x, RHO)
    one.set_preconditioner(0)
    g = feahip.FeaGroup(deck, 2)
    g.set_mass(RHO)
    g.each("set_nodes", x); g.each("create_stiffness_and_residual"); g.each("set_preconditioner", 0)
    assert not np.array_equal(one.node_numbering(), np.arange(one.N))
    assert all(len(nd) > 0 for nd in g.nodes) and sum(len(nd) for nd in g.nodes) == one.N
    yield deck, x, one, g
    g.close(); one.close()


def test_apply_preconditioner_reads_zero_off_the_owned_rows(pair):
    """On each context of the group: the nodes it does not own are exactly +0, its own equal the single context's at
    the same caller ids to 1e-13 of the result's scale (block-Jacobi on K's own diagonal blocks, and a shard's K is the
    unsharded one to rounding)."""
    deck, x, one, g = pair
    r = np.random.default_rng(13).normal(size=one.ndof)
    z1 = one.apply_preconditioner(r).reshape(-1, 3)
    assert z1.any()
    for rk, nd in zip(g.ranks, g.nodes):
        z = rk.apply_preconditioner(r).reshape(-1, 3)
        other = np.ones(one.N, dtype=bool); other[nd] = False
        assert other.any() and np.all(z[other] == 0.0) and not np.signbit(z[other]).any()
        err = np.abs(z[nd] - z1[nd]).max() / np.abs(z1).max()
        print("apply_preconditioner: owned rows against the single context", err)
        assert err <= 1e-13


def test_group_spmm_km_equals_the_single_context(pair):
    """FeaGroup.spmm_km stitched over the two contexts against FeaSolver.spmm_km: the column upload and download on the
    whole-vector path and on the owned-rows path."""
    deck, x, one, g = pair
    x8 = np.random.default_rng(14).normal(size=(8, one.ndof))
    y1, z1 = one.spmm_km(x8)
    y2, z2, ys, zs = g.spmm_km(x8, per_rank=True)
    ey, ez = rel(y2, y1), rel(z2, z1)
    print("spmm_km: group against one context, K X", ey, "M X", ez)
    assert ey <= 1e-12 and ez <= 1e-12
    for nd, yr, zr in zip(g.nodes, ys, zs):                    # what a rank does not own reads +0
        other = np.ones(one.N, dtype=bool); other[nd] = False
        for part in (yr.reshape(8, -1, 3)[:, other], zr.reshape(8, -1, 3)[:, other]):
            assert np.all(part == 0.0) and not np.signbit(part).any()


# the texts of the parent commit's four hand-written checks, which callers match on
EIGEN_ENTRIES = {
    "solve_modes": (lambda lib, c, n, tol, it, out: lib.feahip_solve_modes(c, n, tol, it, 0, out, None, None)),
    "solve_modes_sharded": (lambda lib, c, n, tol, it, out: lib.feahip_solve_modes_sharded(c, n, tol, it, 0, out, None, None)),
    "solve_modes_locked": (lambda lib, c, n, tol, it, out: lib.feahip_solve_modes_locked(c, n, 0.0, tol, it, out, None, None, None)),
    "solve_buckling": (lambda lib, c, n, tol, it, out: lib.feahip_solve_buckling(c, n, tol, it, out, None, None, None)),
}
EIGEN_TEXTS = {
    "solve_modes": ("solve_modes: n_modes must be in [1, 8]", "solve_modes: tolerance must be positive",
                    "solve_modes: max_iterations must not be negative", "solve_modes: null lambda"),
    "solve_modes_sharded": ("solve_modes_sharded: n_modes must be in [1, 8]", "solve_modes_sharded: tolerance must be positive",
                            "solve_modes_sharded: max_iterations must not be negative", "solve_modes_sharded: null lambda"),
    "solve_modes_locked": ("solve_modes_locked: n_modes must be in [1, 64]", "solve_modes_locked: tolerance must be positive",
                           "solve_modes_locked: max_iterations must not be negative", "solve_modes_locked: null lambda"),
    "solve_buckling": ("solve_buckling: n_modes must be in [1, 8]", "solve_buckling: tolerance must be positive",
                       "solve_buckling: max_iterations must not be negative", "solve_buckling: null factor"),
}


@pytest.mark.parametrize("entry", sorted(EIGEN_ENTRIES))
def test_eigenvalue_entries_refuse_their_arguments_in_the_same_words(entry, pair):
    deck, x, one, g = pair
    call = EIGEN_ENTRIES[entry]
    out = np.zeros(64)
    good = dict(n=2, tol=1e-8, it=10, out=feahip._d(out))
    bad = (dict(n=0), dict(tol=0.0), dict(it=-1), dict(out=None))
    for change, text in zip(bad, EIGEN_TEXTS[entry]):
        a = dict(good, **change)
        rc = call(one._lib, one._ctx, a["n"], a["tol"], a["it"], a["out"])
        assert rc == feahip.EINVAL
        assert one._lib.feahip_last_error(one._ctx).decode() == text

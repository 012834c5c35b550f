"""The float64 restatement of the multigrid cycle (amg_reference.py), validated on the CPU oracle's K with a hierarchy made
in numpy (aggregates of lattice cells), before the GPU is measured against it (test_gpu_multigrid.py)."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as sla

import amg_reference as ar
import feahip
import mesh
from oracle_binding import OracleSolver

DIMS = (4, 24, 4)
INFO = dict(gamma=2, gamma_from=0, gamma_until=1 << 20, over=2.0, coarse_sweeps=2)


def prescribed_mask(deck):
    m = np.zeros(3 * len(deck.nodes), dtype=bool)
    for n, t in zip(deck.presc_node, deck.presc_type):
        for j in range(3):
            if t & (1 << j):
                m[3 * n + j] = True
    return m


def lattice_levels(pos, cells):
    """Aggregates of lattice cells `cells` wide, twice: per level (agg, doff, type, nagg), then the coarsest sites."""
    out = []
    sites, paired = pos, False
    for w in cells:
        key = np.floor(sites / w + 1e-9).astype(np.int64)
        _, agg = np.unique(key, axis=0, return_inverse=True)
        agg = agg.ravel()
        nagg = agg.max() + 1
        cent = np.zeros((nagg, 3))
        np.add.at(cent, agg, sites)
        cent /= np.bincount(agg, minlength=nagg)[:, None]
        doff = sites - cent[agg]
        if paired:                                         # two block rows per site: translation, rotation
            out.append((np.repeat(agg, 2), np.repeat(doff, 2, axis=0), np.tile([0, 1], len(agg)), nagg))
        else:
            out.append((agg, doff, np.zeros(len(agg), dtype=int), nagg))
        sites, paired = cent, True
    return out


def build_cycle(K, mask, pos, fine_bits=64, coarse_bits=64, info=INFO, cells=(0.5, 1.0), mirror=True):
    """The reference hierarchy for K: stored matrices rounded as the library stores them (the coarse ones mirrored from
    their upper triangle, as k_mirror_lower leaves them), omegas from the restated power iteration."""
    N = K.shape[0] // 3
    lv = []
    lv.append(dict(A=ar.fine_copy(K, fine_bits, np.arange(N)), Dinv=ar.block_inverse(K, N)))
    Kl, first = K, True
    for agg, doff, typ, nagg in lattice_levels(pos, cells):
        P = ar.prolongator(agg, doff, typ, nagg)
        lv[-1]["P"] = P
        C = ar.galerkin(Kl, P, mask if first else None)
        if mirror:
            C = ar.mirror_upper(C)
        C.data = ar.stored(C.data, coarse_bits)
        lv.append(dict(A=C, Dinv=ar.block_inverse(C, C.shape[0] // 3)))
        Kl, first = C, False
    for l, L in enumerate(lv):
        L["omega"] = ar.power_omega(L["A"], ar.blockdiag(L["Dinv"]), np.arange(L["A"].shape[0]))
    return ar.Cycle(lv, info, mask)


@pytest.fixture(scope="module")
def system():
    deck = mesh.bar_deck(dims=DIMS)
    o = OracleSolver(deck)
    o.update_nodes_with_bc(1.0)
    o.update_state(); o.create_stiffness(); o.create_residual_forces(); o.apply_prescribed_bc(0.0)
    K = sp.csr_matrix((o.values().copy(), o.indexes().copy(), o.offsets().copy()), shape=(o.ndof, o.ndof))
    f = o.forces().copy()
    o.solve_slae(feahip.CHOLESKY)
    u = o.solution().copy()
    o.close()
    return deck, K, f, u, prescribed_mask(deck)


def pcg(K, f, apply, tol=1e-12, maxit=5000):
    x = np.zeros_like(f); r = f.copy(); z = apply(r); p = z.copy(); rz = r @ z
    for it in range(1, maxit + 1):
        q = K @ p
        a = rz / (p @ q)
        x += a * p; r -= a * q
        if np.linalg.norm(r) <= tol * np.linalg.norm(f):
            return x, it
        z = apply(r)
        rz, rz0 = r @ z, rz
        p = z + (rz / rz0) * p
    return x, maxit


def rigid_modes(pos):
    c = pos - pos.mean(axis=0)
    modes = []
    for d in range(3):
        t = np.zeros_like(pos); t[:, d] = 1; modes.append(t.ravel())
        w = np.zeros(3); w[d] = 1; modes.append(np.cross(w, c).ravel())
    return modes


def test_bf16_rounding_is_nearest_even():
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -2.5, 0.0, 3.0e-40])
    got = ar.bf16_round(x)
    assert got[0] == 1.0 and got[1] == 1.0                     # tie to even (down)
    assert got[2] == 1.0 + 4 * 2.0 ** -8                       # tie to even (up)
    assert got[3] == 1.0 + 2 * 2.0 ** -8                       # above the tie
    assert got[4] == -2.5 and got[5] == 0.0


@pytest.mark.parametrize("bits", [(64, 64), (16, 32)])
def test_reference_cycle_is_symmetric_positive_linear(system, bits):
    deck, K, f, u, mask = system
    M = build_cycle(K, mask, deck.nodes, fine_bits=bits[0], coarse_bits=bits[1])
    rng = np.random.default_rng(3)
    for _ in range(4):
        a, b = rng.standard_normal(K.shape[0]), rng.standard_normal(K.shape[0])
        Ma, Mb = M.apply(a), M.apply(b)
        assert abs(a @ Mb - b @ Ma) <= 1e-13 * np.linalg.norm(a) * np.linalg.norm(Mb)
        al, be = 0.7, -1.9
        lin = M.apply(al * a + be * b) - (al * Ma + be * Mb)
        assert np.abs(lin).max() <= 1e-13 * np.abs(al * Ma + be * Mb).max()
    vs = [rng.standard_normal(K.shape[0]) for _ in range(32)] + rigid_modes(deck.nodes)
    for v in vs:
        assert v @ M.apply(v) > 0


def test_reference_damping_keeps_jacobi_convergent(system):
    deck, K, f, u, mask = system
    M = build_cycle(K, mask, deck.nodes)
    for L in M.lv:
        # lambda_max(D^-1 A) = lambda_max(S A S), S = D^-1/2 blockwise
        w, V = np.linalg.eigh(L["Dinv"])
        S = ar.blockdiag(np.einsum("nij,nj,nkj->nik", V, np.sqrt(np.maximum(w, 0)), V))
        op = sla.LinearOperator(L["A"].shape, matvec=lambda x, S=S, A=L["A"]: S @ (A @ (S @ x)), dtype=np.float64)
        lam = sla.eigsh(op, k=1, which="LA", return_eigenvectors=False, tol=1e-8)[0]
        assert 0 < L["omega"] * lam < 2, (L["omega"], lam)


def test_reference_pcg_reaches_the_direct_solution_faster_than_block_jacobi(system):
    deck, K, f, u, mask = system
    M = build_cycle(K, mask, deck.nodes, fine_bits=16, coarse_bits=32)
    N = K.shape[0] // 3
    BJ = ar.blockdiag(ar.block_inverse(K, N))
    x_mg, it_mg = pcg(K, f, M.apply)
    x_bj, it_bj = pcg(K, f, lambda r: BJ @ r)
    s = np.abs(u).max()
    assert np.abs(x_mg - u).max() <= 1e-9 * s and np.abs(x_bj - u).max() <= 1e-9 * s
    assert it_mg * 2 < it_bj, (it_mg, it_bj)


def test_over_correction_cap_matters(system):
    """gamma = 1 caps the over-correction at 1 (amg_cycle / tail_args).  Without the cap the operator is visibly another:
    the reference would tell the two apart."""
    deck, K, f, u, mask = system
    info = dict(INFO, gamma=1)
    capped = build_cycle(K, mask, deck.nodes, info=info)
    assert ar.level_params(info, 0) == (1, 1.0)
    uncapped = build_cycle(K, mask, deck.nodes, info=info)
    uncapped_params = ar.level_params
    try:
        ar.level_params = lambda inf, l: (1, inf["over"])
        z1 = uncapped.apply(f)
    finally:
        ar.level_params = uncapped_params
    z0 = capped.apply(f)
    assert np.abs(z1 - z0).max() > 1e-2 * np.abs(z0).max()

"""The multigrid preconditioner (amg.hip) against its float64 restatement (amg_reference.py), on an MI355X.

feahip_apply_preconditioner gives z = M^-1 r of the W-cycle the PCG runs; feahip_amg_info / feahip_amg_level export the
hierarchy as stored.  For every mesh and every variant of the cycle: z agrees with the reference cycle built from the
exported hierarchy, every level's damping with the restated power iteration, every coarse matrix with its restated
Galerkin product in its stored precision, and the device operator is linear, stateless, deterministic, positive and
symmetric.  The whole file runs in about 7 s on an MI355X, where every tolerance below holds."""
import numpy as np
import pytest
import scipy.sparse as sp

import amg_reference as ar
import feahip
import mesh

pytestmark = pytest.mark.gpu

Z_TOL = 1e-12        # z against the reference cycle, relative to max|z|
OMEGA_TOL = 1e-10    # restated power iteration, relative
SYM_TOL = 1e-12      # |a.Mb - b.Ma| / (|a| |Mb|)
LIN_TOL = 1e-13      # linearity, relative to max|alpha Ma + beta Mb|
ENV = ("FEAHIP_AMG_TAIL", "FEAHIP_AMG_TAIL_ELL", "FEAHIP_AMG_TAIL_BLOB", "FEAHIP_AMG_TAIL_COP", "FEAHIP_AMG_FUSED_POST",
       "FEAHIP_AMG_FINE_BITS", "FEAHIP_AMG_F32", "FEAHIP_AMG_GAMMA", "FEAHIP_AMG_GAMMA_UNTIL", "FEAHIP_AMG_GAMMA_FROM",
       "FEAHIP_AMG_SWEEPS", "FEAHIP_AMG_COARSEST", "FEAHIP_AMG_OVER")


def prescribed_mask(deck):
    m = np.zeros(3 * len(deck.nodes), dtype=bool)
    for n, t in zip(deck.presc_node, deck.presc_type):
        for j in range(3):
            if t & (1 << j):
                m[3 * n + j] = True
    return m


def fan_on_block(m=140):
    """A block with, beside it, the fan of m tetrahedron pairs of test_node_with_more_neighbours_than_the_spmv_tile: its hub
    row has m + 3 blocks -- 143, more than the SpMV tile, for the 140 pairs of that test.  The fan alone is too small for a
    hierarchy."""
    b = mesh.bar_deck(dims=(6, 36, 6))
    ang = 2 * np.pi * np.arange(m) / m
    ring = np.stack([np.cos(ang), np.sin(ang), np.zeros(m)], axis=1)
    fan = np.vstack([[0.0, 0.0, 0.0], ring, [0.0, 0.0, 0.7], [0.0, 0.0, -0.7]]) + np.array([4.0, 3.0, 0.5])
    n0 = len(b.nodes)
    top, bot = n0 + m + 1, n0 + m + 2
    el = []
    for i in range(m):
        a, c = n0 + 1 + i, n0 + 1 + (i + 1) % m
        el += [[n0, a, c, top], [n0, c, a, bot]]
    return feahip.Deck(model=b.model, parameters=b.parameters, ele_type=feahip.TETRAHEDRA4, gauss_nodes_count=1,
                       nodes=np.vstack([b.nodes, fan]), elements=np.vstack([b.elements, np.array(el, dtype=np.int32)]),
                       presc_node=np.concatenate([b.presc_node, [top, bot, n0 + 1]]),
                       presc_type=np.concatenate([b.presc_type, [7, 7, 2]]),
                       presc_values=np.vstack([b.presc_values, np.zeros((3, 3))]))


def isolated_node():
    """A block and one node that no element uses: its diagonal block is zero and gets the identity."""
    b = mesh.bar_deck(dims=(6, 36, 6))
    return feahip.Deck(model=b.model, parameters=b.parameters, ele_type=b.ele_type, gauss_nodes_count=b.gauss_nodes_count,
                       nodes=np.vstack([b.nodes, [[3.0, 3.0, 3.0]]]), elements=b.elements, presc_node=b.presc_node,
                       presc_type=b.presc_type, presc_values=b.presc_values)


MESHES = {
    "tet4_bar": lambda: mesh.bar_deck(dims=(6, 36, 6)),
    "tet4_small": lambda: mesh.bar_deck(dims=(3, 12, 3)),        # two levels: the tail's entry matrix fits its LDS
    "tet10_bar": lambda: mesh.bar_deck(dims=(4, 24, 4), quadratic=True),
    "tet10_cylinder_a5": lambda: mesh.cylinder_deck(4, 24, 5, quadratic=True),
    "hex8_block": lambda: mesh.bar_deck(dims=(6, 36, 6), hexa=True),
    "tet4_over_65536_nodes": lambda: mesh.bar_deck(dims=(24, 144, 24)),
    "tet4_fan_hub": fan_on_block,
    "tet4_jittered_permuted": lambda: mesh.jitter_permute(mesh.bar_deck(dims=(6, 36, 6)), amp=0.2, seed=4),
    "tet4_isolated_node": isolated_node,
}
VARIANTS = {
    "default": {},
    "no_tail": {"FEAHIP_AMG_TAIL": "0"},
    "tail_no_ell": {"FEAHIP_AMG_TAIL_ELL": "0"},
    "tail_no_blob": {"FEAHIP_AMG_TAIL_BLOB": "0"},
    "tail_no_cop": {"FEAHIP_AMG_TAIL_COP": "0"},
    "fused_post": {"FEAHIP_AMG_FUSED_POST": "1"},
    "fine_f32": {"FEAHIP_AMG_FINE_BITS": "32"},
    "fine_f64": {"FEAHIP_AMG_FINE_BITS": "64"},
    "coarse_f64": {"FEAHIP_AMG_F32": "0"},
    "v_cycle": {"FEAHIP_AMG_GAMMA": "1"},
    "v_below_1": {"FEAHIP_AMG_GAMMA_UNTIL": "1"},
    "odd_sweeps": {"FEAHIP_AMG_SWEEPS": "3"},
    "shallow": {"FEAHIP_AMG_COARSEST": "1500"},
    "exact": {"FEAHIP_AMG_F32": "0", "FEAHIP_AMG_FINE_BITS": "64"},
}
TAIL_PATHS = set()            # (entry layout, dense coarsest) seen across the cases


def set_env(monkeypatch, env):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def prepared(deck, kind=1, x=None):
    s = feahip.FeaSolver(deck)
    if x is not None:
        s.set_nodes(x)
    s.update_nodes_with_bc(1.0)
    s.create_stiffness_and_residual()
    s.apply_prescribed_bc(0.0)
    s.set_preconditioner(kind)
    return s


def yale(s):
    off, idx, val = s.matrix_yale()
    return sp.csr_matrix((val, idx, off), shape=(s.ndof, s.ndof))


def export(s):
    info = s.amg_info()
    return info, [s.amg_level(l) for l in range(info["levels"])]


def check_galerkin(levels, checks, info):
    for l, C in enumerate(checks["galerkin"]):
        S = ar.bsr(levels[l + 1]["rowptr"], levels[l + 1]["colidx"], levels[l + 1]["K"], levels[l + 1]["N"])
        C = C.tocsr()
        D = abs(S - C).tocoo()
        scale = np.abs(C.data).max()
        ref = np.asarray(C[D.row, D.col]).ravel()
        if info["coarse_f32"]:
            # one f32 ulp of the entry, plus 1e-14 of the level's largest where the double sum cancels
            tol = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64) + 1e-14 * scale
        else:
            tol = 1e-13 * scale
        bad = D.data > tol
        assert not bad.any(), (l + 1, int(bad.sum()), float((D.data - tol).max()))


def check_storage_symmetric(levels, A0):
    """every stored matrix is blockwise symmetric bit for bit: K~_ij == K~_ji^T"""
    if A0 is not None:                                              # (K itself is symmetric to rounding only)
        assert (A0 != A0.T).nnz == 0, "level-0 smoother matrix"
    for l in range(1, len(levels)):
        S = ar.bsr(levels[l]["rowptr"], levels[l]["colidx"], levels[l]["K"], levels[l]["N"])
        assert (S != S.T).nnz == 0, f"level {l}"


def check_operator(s, deck):
    """the device operator against the reference built from its export (one context, or one rank of a row shard)"""
    info, levels = export(s)
    K = yale(s)
    nodes = np.arange(s.N)
    lib = s.node_numbering()[nodes]
    cyc, chk = ar.from_export(K, prescribed_mask(deck), info, levels, nodes, lib)
    for l, L in enumerate(levels):
        assert abs(L["omega"] - chk["omega"][l]) <= OMEGA_TOL * chk["omega"][l], (l, L["omega"], chk["omega"][l])
    A0, K0 = chk["A0"], chk["K0"]
    want = ar.fine_copy(K0, info["fine_bits"], lib)
    assert abs(A0 - want).max() == 0, "the level-0 smoother copy is not K's upper triangle mirrored and rounded"
    check_galerkin(levels, chk, info)
    check_storage_symmetric(levels, A0 if info["fine_bits"] != 64 else None)
    if info["tail_from"] >= 0:
        TAIL_PATHS.add((info["tail_entry"], info["tail_cop"]))
    dofs = ar.owned_dofs(nodes)
    rng = np.random.default_rng(11)
    vs = [rng.standard_normal(s.ndof) for _ in range(4)] + [s.forces()]
    zs = []
    for v in vs:
        z = s.apply_preconditioner(v)
        zr = cyc.apply(v[dofs])
        assert np.abs(z[dofs] - zr).max() <= Z_TOL * np.abs(zr).max()
        rest = np.ones(s.ndof, dtype=bool); rest[dofs] = False
        assert not z[rest].any()
        zs.append(z)
    a, b = vs[0], vs[1]
    Ma, Mb = zs[0], zs[1]
    al, be = 0.3, -2.1
    assert np.abs(s.apply_preconditioner(al * a + be * b) - (al * Ma + be * Mb)).max() <= LIN_TOL * np.abs(al * Ma + be * Mb).max()
    again = s.apply_preconditioner(a)                              # a, b, a: nothing carried between calls
    assert np.array_equal(again, Ma) and np.array_equal(s.apply_preconditioner(b), Mb)
    for v, z in zip(vs, zs):
        assert v[dofs] @ z[dofs] > 0
    assert abs(a[dofs] @ Mb[dofs] - b[dofs] @ Ma[dofs]) <= SYM_TOL * np.linalg.norm(a[dofs]) * np.linalg.norm(Mb[dofs])
    return info, levels


@pytest.mark.parametrize("name", list(MESHES))
def test_multigrid_matches_reference_on_meshes(name, monkeypatch):
    set_env(monkeypatch, {})
    deck = MESHES[name]()
    s = prepared(deck)
    info, levels = check_operator(s, deck)
    if name == "tet4_over_65536_nodes":
        assert s.N > 65536 and levels[0]["bits"] == 16           # the bf16 copy's column index needs its high half
    if name == "tet4_isolated_node":
        assert np.all(levels[0]["K"][levels[0]["rowptr"][-2]:] == 0)  # its block is zero: the identity stands in for D
    s.close()


@pytest.mark.parametrize("bits", [16, 32, 64])
@pytest.mark.parametrize("pairs", [125, 126])
def test_hub_row_at_the_tile_limit(pairs, bits, monkeypatch):
    """A hub row of 128 blocks (a full tile, a chunk of its own) and of 129 (the smallest long row) under the bfloat16, the
    float and the double smoother matrix of level 0: the three bodies of the SpMV and of the fused Jacobi sweep that run
    only inside the cycle."""
    set_env(monkeypatch, {"FEAHIP_AMG_FINE_BITS": str(bits)})
    deck = fan_on_block(pairs)
    s = prepared(deck)
    info, levels = check_operator(s, deck)
    assert info["fine_bits"] == bits and levels[0]["bits"] == bits
    # the hub row has pairs + 3 blocks and is the longest; the two poles of the fan have pairs + 2 (at 126 pairs they are
    # full tiles beside the long hub row); no row of the block comes near
    rows = np.sort(np.diff(levels[0]["rowptr"]))
    assert list(rows[-3:]) == [pairs + 2, pairs + 2, pairs + 3] and rows[-4] < 64, rows[-4:]
    s.close()


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_multigrid_variants_match_reference(variant, monkeypatch):
    set_env(monkeypatch, VARIANTS[variant])
    deck = mesh.bar_deck(dims=(8, 48, 8))
    s = prepared(deck)
    info, _ = check_operator(s, deck)
    want = {"fine_f32": ("fine_bits", 32), "fine_f64": ("fine_bits", 64), "coarse_f64": ("coarse_f32", False),
            "v_cycle": ("gamma", 1), "v_below_1": ("gamma_until", 1), "odd_sweeps": ("coarse_sweeps", 3),
            "fused_post": ("fused_post", True), "no_tail": ("tail_from", -1)}.get(variant)
    if want:
        assert info[want[0]] == want[1], info
    s.close()


def test_tail_paths_are_all_taken():
    """The cases above, together, run the one-workgroup tail with its entry-level product out of LDS, the lane-major
    copy and L2, and with and without the dense coarsest operator (read from the exported flags, not from sizes)."""
    if not TAIL_PATHS:
        pytest.fail("run with the cases above")
    entries = {e for e, _ in TAIL_PATHS}
    cops = {c for _, c in TAIL_PATHS}
    assert entries >= {"lds", "ell", "l2"} and cops == {True, False}, TAIL_PATHS


@pytest.mark.parametrize("n,rank_contexts", [(2, False), (3, False), (2, True), (3, True)])
def test_sharded_multigrid_is_the_block_diagonal_cycle(n, rank_contexts, monkeypatch):
    set_env(monkeypatch, {})
    deck = mesh.bar_deck(dims=(8, 48, 8))
    g = feahip.FeaGroup(deck, n, rank_contexts=rank_contexts)
    for r in g.ranks:
        r.update_nodes_with_bc(1.0); r.create_stiffness_and_residual(); r.apply_prescribed_bc(0.0); r.set_preconditioner(1)
    rng = np.random.default_rng(5)
    v = rng.standard_normal(3 * len(deck.nodes))
    z = g.apply_preconditioner(v)
    want = np.zeros_like(z)
    mask = prescribed_mask(deck)
    for rk, nd in zip(g.ranks, g.nodes):
        info, levels = export(rk)
        K = yale(rk)
        if rank_contexts:                                         # a rank's own nodes are its first n_own local ids
            loc = np.arange(rk.n_own)
            m = np.zeros(3 * rk.N, dtype=bool)
            m.reshape(-1, 3)[:] = mask.reshape(-1, 3)[rk.node_global]
            cyc, chk = ar.from_export(K, m, info, levels, loc, rk.node_numbering()[loc])
            vr = v.reshape(-1, 3)[rk.node_global].ravel()
            want.reshape(-1, 3)[nd] = cyc.apply(vr[ar.owned_dofs(loc)]).reshape(-1, 3)
        else:
            cyc, chk = ar.from_export(K, mask, info, levels, nd, rk.node_numbering()[nd])
            want.reshape(-1, 3)[nd] = cyc.apply(v[ar.owned_dofs(nd)]).reshape(-1, 3)
        for l, L in enumerate(levels):
            assert abs(L["omega"] - chk["omega"][l]) <= OMEGA_TOL * chk["omega"][l]
        check_galerkin(levels, chk, info)
        check_storage_symmetric(levels, chk["A0"])
    assert np.abs(z - want).max() <= Z_TOL * np.abs(want).max()
    g.close()


def test_numeric_setup_follows_K(monkeypatch):
    """Every assertion bitwise against a fresh context holding the same K."""
    set_env(monkeypatch, {})
    deck = mesh.bar_deck(dims=(6, 36, 6))
    x2 = mesh.deformed_state(deck.nodes, k1=1.04)
    v = np.random.default_rng(2).standard_normal(3 * len(deck.nodes))

    def fresh(x=None, bc=True):
        t = feahip.FeaSolver(deck)
        if x is not None:
            t.set_nodes(x)
        t.create_stiffness()
        if bc:
            t.apply_prescribed_bc(0.0)
        t.set_preconditioner(1)
        z = t.apply_preconditioner(v)
        t.close()
        return z

    s = feahip.FeaSolver(deck)
    with pytest.raises(feahip.FeaHipError):                       # no K yet
        s.apply_preconditioner(v)
    s.create_stiffness()
    s.set_preconditioner(1)
    assert np.array_equal(s.apply_preconditioner(v), fresh(bc=False))
    s.apply_prescribed_bc(0.0)
    assert np.array_equal(s.apply_preconditioner(v), fresh())
    s.set_nodes(x2); s.create_stiffness()
    assert np.array_equal(s.apply_preconditioner(v), fresh(x2, bc=False))
    s.apply_prescribed_bc(0.0)
    z2 = fresh(x2)
    assert np.array_equal(s.apply_preconditioner(v), z2)
    # modified Newton: stash, BC, solve; restore, BC, solve ... on the same K
    s.create_stiffness(); s.stash_stiffness(); s.apply_prescribed_bc(0.0)
    assert np.array_equal(s.apply_preconditioner(v), z2)
    s.restore_stiffness()
    assert np.array_equal(s.apply_preconditioner(v), fresh(x2, bc=False))
    s.apply_prescribed_bc(0.0)
    assert np.array_equal(s.apply_preconditioner(v), z2)
    s.restore_stiffness(); s.apply_prescribed_bc(0.0)
    assert np.array_equal(s.apply_preconditioner(v), z2)
    # a row shard and back
    s.set_row_shard(1, 2); s.create_stiffness(); s.apply_prescribed_bc(0.0)
    t = feahip.FeaSolver(deck)
    t.set_nodes(x2); t.set_row_shard(1, 2); t.create_stiffness(); t.apply_prescribed_bc(0.0); t.set_preconditioner(1)
    zt = t.apply_preconditioner(v)
    t.close()
    assert zt.any() and np.array_equal(s.apply_preconditioner(v), zt)
    s.set_row_shard(0, 1); s.create_stiffness(); s.apply_prescribed_bc(0.0)
    assert np.array_equal(s.apply_preconditioner(v), z2)
    s.close()


def test_apply_does_not_disturb_a_solve(monkeypatch):
    set_env(monkeypatch, {})
    deck = mesh.bar_deck(dims=(6, 36, 6))
    for kind in (0, 1):
        a, b = prepared(deck, kind), prepared(deck, kind)
        a.apply_preconditioner(np.ones(a.ndof))
        ra, rb = a.solve_slae(feahip.PCG_ILU, 1e-14, 20000), b.solve_slae(feahip.PCG_ILU, 1e-14, 20000)
        assert ra == rb and np.array_equal(a.solution(), b.solution())
        a.close(); b.close()


@pytest.mark.parametrize("name", ["tet4_bar", "tet4_isolated_node", "tet4_jittered_permuted"])
def test_block_jacobi_is_the_inverse_diagonal(name):
    deck = MESHES[name]()
    s = prepared(deck, kind=0)
    K = yale(s)
    N = s.N
    a, i, j = np.meshgrid(np.arange(N), np.arange(3), np.arange(3), indexing="ij")
    d = np.asarray(K[(3 * a + i).ravel(), (3 * a + j).ravel()]).reshape(N, 3, 3)
    det = np.linalg.det(d)
    ok = (det != 0) & np.isfinite(det)                            # k_precond_build: a singular block gets the identity
    m = np.tile(np.eye(3), (N, 1, 1))
    m[ok] = np.linalg.inv(d[ok])
    if name == "tet4_isolated_node":
        assert not ok[-1]
    r = np.random.default_rng(1).standard_normal(s.ndof)
    want = np.einsum("nij,nj->ni", m, r.reshape(-1, 3)).ravel()
    assert np.abs(s.apply_preconditioner(r) - want).max() <= 1e-14 * np.abs(want).max()
    s.close()

"""A float64 numpy/scipy restatement of the multigrid preconditioner (fea-large_amd/csrc/amg.hip).

Given K (matrix_yale, the caller's dof ids), the level-0 prescribed-dof mask and a hierarchy in the layout that
FeaSolver.amg_level exports (per level: N, rowptr, colidx, K [nnzb][3][3] as stored, agg, doff, type, omega), this
module applies the same operator M^-1 the W-cycle applies, restates the Jacobi damping of every level from its power
iteration and the coarse matrices from their Galerkin products.  Every rule cites the line of amg.hip it restates.

Vectors of level 0 are indexed by the rank's own nodes (`nodes`, caller ids); coarse levels by the library's aggregate
ids (aggregate A of level l is block rows 2A, 2A+1 of level l+1).
"""
import numpy as np
import scipy.sparse as sp


def bsr(rowptr, colidx, blocks, n_rows, n_cols=None):
    """3x3 block-CSR -> scalar CSR (3 n_rows x 3 n_cols)."""
    n_cols = n_rows if n_cols is None else n_cols
    return sp.bsr_matrix((np.asarray(blocks, dtype=np.float64).reshape(-1, 3, 3), np.asarray(colidx), np.asarray(rowptr)),
                         shape=(3 * n_rows, 3 * n_cols)).tocsr()


def bf16_round(a):
    """k_to_bf16 (amg.hip:294-310): double -> float, then round to nearest even on the upper 16 bits; returned widened."""
    u = np.asarray(a, dtype=np.float64).astype(np.float32).view(np.uint32).astype(np.uint64)
    b = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF
    return (b << 16).astype(np.uint32).view(np.float32).astype(np.float64)


def stored(a, bits):
    """a value of a double matrix as the level stores it: bfloat16, float or double, widened back."""
    a = np.asarray(a, dtype=np.float64)
    if bits == 16:
        return bf16_round(a)
    if bits == 32:
        return a.astype(np.float32).astype(np.float64)
    return a.copy()


def mirror_upper(A):
    """The scalar upper triangle and its transpose: what k_mirror_lower (coarse levels, amg.hip:122-136) and sym_value
    (the level-0 copies of k_to_bf16 / k_to_f32, amg.hip:274-283) store, so that the stored matrix is symmetric bit for bit."""
    U = sp.triu(A, 1)
    return (U + U.T + sp.diags(A.diagonal())).tocsr()


def fine_copy(K0, bits, libid):
    """the level-0 smoother's matrix for the rank's diagonal block K0: K itself (64), or its upper triangle mirrored and
    rounded (k_to_f32, k_to_bf16).  "Upper" is in the library's node order (libid of every node of K0)."""
    if bits == 64:
        return K0.copy()
    p = owned_dofs(np.argsort(libid))
    ip = np.argsort(p)
    A = mirror_upper(K0.tocsr()[p][:, p]).tocsr()[ip][:, ip]
    A.data = stored(A.data, bits)
    return A


def block_inverse(A, N):
    """k_block_inverse (amg.hip:142-162): the inverse of every diagonal 3x3 block; a zero diagonal entry becomes 1 first,
    a block with determinant 0 or NaN gets the identity."""
    a, i, j = np.meshgrid(np.arange(N), np.arange(3), np.arange(3), indexing="ij")
    d = np.asarray(A.tocsr()[(3 * a + i).ravel(), (3 * a + j).ravel()]).reshape(N, 3, 3)
    ii = np.arange(3)
    dd = d[:, ii, ii]
    dd[dd == 0.0] = 1.0
    d[:, ii, ii] = dd
    det = np.linalg.det(d)
    ok = (det != 0.0) & np.isfinite(det)
    m = np.tile(np.eye(3), (N, 1, 1))
    if ok.any():
        m[ok] = np.linalg.inv(d[ok])
    return m


def blockdiag(minv):
    N = minv.shape[0]
    return sp.bsr_matrix((minv, np.arange(N), np.arange(N + 1)), shape=(3 * N, 3 * N)).tocsr()


def start_vector(libdof):
    """k_fill_pattern (amg.hip:264-268): 1 + 0.37 ((t * 2654435761) mod 2^32 >> 24) / 256 at the library's dof t."""
    t = np.asarray(libdof, dtype=np.uint64)
    h = ((t * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(24)
    return 1.0 + 0.37 * h.astype(np.float64) / 256.0


def power_omega(A, Dinv, libdof, steps=8):
    """amg_numeric's power iteration (amg.hip:970-988): 8 products v = D^-1 A v,
    normalised between them (k_scale_by_norm), omega = 4 / (3 * 1.1 * |v_8|); a zero or NaN norm gives lambda 2."""
    v = start_vector(libdof)
    nrm2 = 0.0
    for it in range(steps):
        v = Dinv @ (A @ v)
        nrm2 = float(v @ v)
        if it < steps - 1 and nrm2 > 0:
            v = v / np.sqrt(nrm2)
    lam = np.sqrt(nrm2) if (nrm2 > 0 and nrm2 == nrm2) else 2.0
    return 4.0 / (3.0 * 1.1 * lam)


def rot(d):
    """R(d) w = w x d (k_prolong, amg.hip:246-248)."""
    return np.array([[0.0, d[2], -d[1]], [-d[2], 0.0, d[0]], [d[1], -d[0], 0.0]])


def prolongator(agg, doff, typ, nagg):
    """P: a translation row i of aggregate A is [I | R(d_i)] on A's coarse dofs 6A..6A+5, a rotation row [0 | I]
    (k_prolong, amg.hip:233-252; k_galerkin's comment, amg.hip:24-30).  Rows with agg < 0 (other ranks) are empty."""
    agg = np.asarray(agg)
    rows, cols, vals = [], [], []
    d = np.asarray(doff, dtype=np.float64).reshape(-1, 3)
    typ = np.asarray(typ)
    for i in np.nonzero(agg >= 0)[0]:
        A = agg[i]
        if typ[i]:
            blk = np.hstack([np.zeros((3, 3)), np.eye(3)])
        else:
            blk = np.hstack([np.eye(3), rot(d[i])])
        r, c = np.nonzero(blk != 0.0)
        rows.append(3 * i + r); cols.append(6 * A + c); vals.append(blk[r, c])
    if not rows:
        return sp.csr_matrix((3 * len(agg), 6 * nagg))
    return sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(3 * len(agg), 6 * nagg))


def galerkin(K, P, mask=None):
    """k_galerkin (amg.hip:37-115): P' K P, on level 0 with the prescribed dofs' rows and columns of K left out."""
    if mask is not None:
        keep = sp.diags((~np.asarray(mask, dtype=bool)).astype(np.float64))
        K = keep @ K @ keep
    return (P.T @ K @ P).tocsr()


def level_params(info, l):
    """gamma and over-correction of level l (amg_cycle, amg.hip:1121 and 1130; tail_args, amg.hip:1033-1034:
    `gamma = (l < gamma_from || l >= gamma_until) ? 1 : gamma`, `over = gamma >= 2 ? over : fmin(over, 1)`)."""
    g = 1 if (l < info["gamma_from"] or l >= info["gamma_until"]) else info["gamma"]
    return g, (info["over"] if g >= 2 else min(info["over"], 1.0))


class Cycle:
    """The W-cycle of amg_cycle (amg.hip:1097-1140) / t_cycle (the one-workgroup tail) in float64.

    levels: list of dicts with A (the smoother's stored matrix, scalar CSR), Dinv (N x 3 x 3), omega and, above the
    coarsest level, P (prolongator to the next level).  mask: level-0 prescribed dofs (bool, 3N) or None."""

    def __init__(self, levels, info, mask=None):
        self.lv, self.info = levels, info
        self.mask = None if mask is None else np.asarray(mask, dtype=bool)
        for L in self.lv:
            L["D"] = blockdiag(L["Dinv"])
            if L.get("P") is not None:
                L["PT"] = L["P"].T.tocsr()

    def _cycle(self, l, r):
        L = self.lv[l]
        om, D, A = L["omega"], L["D"], L["A"]
        x = om * (D @ r)                                            # k_smooth_first (amg.hip:190): x = omega D^-1 r
        if L.get("P") is None:                                      # coarsest (amg.hip:1104-1118): `sweeps` damped Jacobi sweeps
            for _ in range(self.info["coarse_sweeps"]):
                x = x + om * (D @ (r - A @ x))
            return x
        gamma, over = level_params(self.info, l)
        mask = self.mask if l == 0 else None
        for _ in range(gamma):                                      # coarse correction, gamma times
            res = r - A @ x
            if mask is not None:
                res = np.where(mask, 0.0, res)                      # k_restrict (amg.hip:207-230): masked residual
            xc = self._cycle(l + 1, L["PT"] @ res)
            u = L["P"] @ xc
            if mask is not None:
                u = np.where(mask, 0.0, u)                          # k_prolong (amg.hip:234-252): masked update
            x = x + over * u
        return x + om * (D @ (r - A @ x))                           # post-smoothing, k_smooth_next (amg.hip:196)

    def apply(self, r):
        return self._cycle(0, np.asarray(r, dtype=np.float64))


def owned_dofs(nodes):
    nodes = np.asarray(nodes)
    return (3 * nodes[:, None] + np.arange(3)[None, :]).ravel()


def from_export(K, mask, info, levels, nodes, libid, restate=True):
    """The reference for one rank, built from an exported hierarchy.

    K: the double matrix (scalar CSR, the caller's dof ids); mask: prescribed dofs (3N bools); levels: amg_level dicts;
    nodes: the rank's own nodes (caller ids, the order of the vectors); libid: library id of each of them (the power
    iteration's start vector is written in library dof ids).

    Returns (Cycle, checks): the cycle uses the exported omegas and stored matrices; checks holds what the reference
    restates on its own -- omega of every level, the Galerkin product of every coarse level (double), and the level-0
    smoother's matrix rounded from K."""
    dofs = owned_dofs(nodes)
    K0 = K.tocsr()[dofs][:, dofs]
    m0 = np.asarray(mask, dtype=bool)[dofs]
    L0 = levels[0]
    A0 = bsr(L0["rowptr"], L0["colidx"], L0["K"], L0["N"]).tocsr()[dofs][:, dofs]
    lv = [dict(A=A0, Dinv=block_inverse(K0, len(nodes)), omega=L0["omega"])]    # level 0: D from the double K
    checks = dict(omega=[], galerkin=[], K0=K0, A0=A0)
    for l in range(len(levels)):
        Lx = levels[l]
        if l > 0:
            A = bsr(Lx["rowptr"], Lx["colidx"], Lx["K"], Lx["N"])
            lv.append(dict(A=A, Dinv=block_inverse(A, Lx["N"]), omega=Lx["omega"]))   # below: D from the stored blocks
        if Lx["Nc"] > 0:
            agg = Lx["agg"][nodes] if l == 0 else Lx["agg"]
            doff = Lx["doff"][nodes] if l == 0 else Lx["doff"]
            typ = Lx["type"][nodes] if l == 0 else Lx["type"]
            lv[l]["P"] = prolongator(agg, doff, typ, Lx["Nc"] // 2)
    if restate:
        for l, L in enumerate(lv):
            ld = 3 * np.asarray(libid)[:, None] + np.arange(3)[None, :] if l == 0 else np.arange(3 * levels[l]["N"])
            checks["omega"].append(power_omega(L["A"], blockdiag(L["Dinv"]), np.ravel(ld)))
            if L.get("P") is not None:
                Kl = K0 if l == 0 else L["A"]
                checks["galerkin"].append(galerkin(Kl, L["P"], m0 if l == 0 else None))
    return Cycle(lv, info, m0), checks

"""Linear buckling restated in float64 numpy / scipy: dense K and K_sigma from the oracle's element_stiffness(e) pair
(kc, ks), every element from the oracle solver of ITS material as tests/hetero_reference.py does it (one material is a
table of one), K masked as feahip_apply_prescribed_bc(0.0) documents, and scipy.linalg.eigh(Ksig_ff, K_ff) on the free
dofs.  Also the column decks the buckling tests share, the stop test's ratio, and a float64 emulation of the driver's
Rayleigh-Ritz step that sizes max_iterations.  Nothing here calls the library under test."""
import functools

import numpy as np
import scipy.linalg

import feahip
import mesh
from hetero_reference import HeteroRestatement

END_MOTION = -0.02
COLUMNS = {                                               # kind: (cells, size)
    "tet4": ((2, 8, 2), (1.0, 8.0, 1.0)),
    "hex8": ((2, 8, 2), (1.0, 8.0, 1.0)),
    "tet10": ((1, 4, 1), (1.0, 4.0, 1.0)),
}


def column_deck(kind, end_motion=END_MOTION, dims=None, size=None, model=feahip.MODEL_COMPRESSIBLE_NEOHOOKEAN, **kw):
    """A column along y at origin 0, Neo-Hookean (100, 100), clamped at y = 0, the far end prescribed (0, end_motion, 0),
    type 7 -- or, with end_motion None, the far end free (a clamped-free column for a traction in kw)."""
    dims = COLUMNS[kind][0] if dims is None else dims
    size = COLUMNS[kind][1] if size is None else size
    if kind == "hex8":
        nodes, el = mesh.hex_block(*dims, origin=(0.0, 0.0, 0.0), size=size)
        et, g = feahip.HEXAHEDRA8, 8
    else:
        nodes, el = mesh.kuhn_block(*dims, kind == "tet10", origin=(0.0, 0.0, 0.0), size=size)
        et, g = (feahip.TETRAHEDRA10, 5) if kind == "tet10" else (feahip.TETRAHEDRA4, 1)
    bot = np.nonzero(np.abs(nodes[:, 1]) < 1e-12)[0]
    ids, vals = bot, np.zeros((len(bot), 3))
    if end_motion is not None:
        top = np.nonzero(np.abs(nodes[:, 1] - size[1]) < 1e-12)[0]
        ids = np.concatenate([bot, top])
        vals = np.vstack([vals, np.tile([0.0, end_motion, 0.0], (len(top), 1))])
    kw.setdefault("solver_tolerance", 1e-13)
    kw.setdefault("desired_tolerance", 1e-14)
    kw.setdefault("max_newton_count", 30)
    kw.setdefault("modified_newton", False)
    kw.setdefault("solver_type", feahip.CG)
    return feahip.Deck(model=model, parameters=[100.0, 100.0], ele_type=et, gauss_nodes_count=g, nodes=nodes, elements=el,
                       presc_node=ids.astype(np.int32), presc_type=np.full(len(ids), 7, np.int32), presc_values=vals, **kw)


def _table(deck, materials, ids):
    table = materials is not None
    mats = np.asarray(materials if table else [deck.parameters[:2]], dtype=np.float64).reshape(-1, 2)
    ids = np.asarray(ids if table else np.zeros(len(deck.elements)), dtype=np.int64)
    return mats, ids


def newton_state(deck, materials=None, ids=None):
    """The nodes after ONE load increment of full Newton to the deck's desired_tolerance (1e-14 on the column decks), on
    the oracle with a dense direct solve."""
    h = HeteroRestatement(deck, *_table(deck, materials, ids))
    try:
        done, its, x = h.solve(1, deck.max_newton_count, deck.desired_tolerance)
        assert done == 1, its
    finally:
        h.close()
    return x


def element_pairs(deck, x, materials=None, ids=None):
    """[(kc, ks)] of every element at the nodes x."""
    mats, ids = _table(deck, materials, ids)
    h = HeteroRestatement(deck, mats, ids)
    try:
        for o in h.solvers:
            o.set_nodes(x)
            assert o.update_state() == 0
        return [tuple(np.array(m) for m in h.solvers[ids[e]].element_stiffness(e)) for e in range(h.E)]
    finally:
        h.close()


def identity_deviation(ks, npe):
    """How far the 3x3 blocks of an element's Ks are from a scalar times the identity: the largest |off-diagonal entry|
    and the largest difference among the three diagonal entries, over all node pairs."""
    b = np.asarray(ks).reshape(npe, 3, npe, 3).transpose(0, 2, 1, 3)
    off = np.abs(b * (1.0 - np.eye(3))).max()
    d = np.stack([b[..., 0, 0], b[..., 1, 1], b[..., 2, 2]], axis=-1)
    return max(off, (d.max(axis=-1) - d.min(axis=-1)).max())


def dense_pair(deck, x, materials=None, ids=None):
    """(K unmasked, Ksig symmetrised, K masked, mask[3N]) dense at the nodes x, every element's (kc, ks) from the oracle
    solver of its material."""
    mats, ids = _table(deck, materials, ids)
    h = HeteroRestatement(deck, mats, ids)
    try:
        for o in h.solvers:
            o.set_nodes(np.asarray(x, dtype=np.float64))
            assert o.update_state() == 0
        K, Ks = np.zeros((h.ndof, h.ndof)), np.zeros((h.ndof, h.ndof))
        for e in range(h.E):
            kc, ks = h.solvers[ids[e]].element_stiffness(e)
            d = h.dofs[e]
            K[np.ix_(d, d)] += kc + ks
            Ks[np.ix_(d, d)] += ks
        Km, _ = h.masked(K, np.zeros(h.ndof))
    finally:
        h.close()
    return K, 0.5 * (Ks + Ks.T), Km, h.mask


class BucklingReference:
    """K (masked) and Ksig (unmasked) dense at the nodes x, mask[3N], nu[free dofs] ascending, Phi[3N][free dofs] (zero on
    the prescribed dofs, K-orthonormal), min_eig_K of the free block."""

    def __init__(self, deck, x, materials=None, ids=None):
        _, self.Ksig, self.K, self.mask = dense_pair(deck, x, materials, ids)
        self.free = np.nonzero(~self.mask)[0]
        ff = np.ix_(self.free, self.free)
        Kf = 0.5 * (self.K[ff] + self.K[ff].T)
        self.min_eig_K = float(np.linalg.eigvalsh(Kf)[0])
        self.nu, vec = scipy.linalg.eigh(self.Ksig[ff], Kf)
        self.Phi = np.zeros((len(self.mask), len(self.free)))
        self.Phi[self.free] = vec

    def factor(self, n):
        nu = self.nu[:n]
        return np.where(nu < 0, 1.0 - 1.0 / np.where(nu < 0, nu, -1.0), np.inf)

    def residual_ratio(self, nu, phi):
        """||Ksig phi - nu K phi|| / (||Ksig phi|| + |nu| ||K phi||), the Ksig-product zeroed on the prescribed dofs: the
        stop test's formula."""
        Kp, Sp = self.K @ phi, np.where(self.mask, 0.0, self.Ksig @ phi)
        return np.linalg.norm(Sp - nu * Kp) / (np.linalg.norm(Sp) + abs(nu) * np.linalg.norm(Kp))

    def emulate(self, n_modes, tol, max_it, seed=5):
        """The driver's step in float64: blocks of eight columns [X, W, P], W = D^-1 (Ksig X - K X diag(nu)) with the 3x3
        block-Jacobi inverse of the masked K, Rayleigh-Ritz on the K-orthonormalised basis (directions below 1e-12 of the
        largest dropped, P_new = the [W, P] part of X_new, a rank drop restarts without P); the products of X and P are
        carried by recurrence and made again every 20 steps, and the stop test is repeated on fresh products of a
        re-orthonormalised X before the return.  The start block is another one than the library's hash.  Returns
        (nu[n_modes], ratio[n_modes], steps)."""
        n = len(self.mask)
        K, S = self.K, np.where(self.mask[:, None], 0.0, self.Ksig)
        Dinv = np.zeros((n, n))
        for a in range(n // 3):
            s = slice(3 * a, 3 * a + 3)
            Dinv[s, s] = np.linalg.inv(K[s, s])
        free = ~self.mask

        def ritz(GM, GK):
            GM, GK = 0.5 * (GM + GM.T), 0.5 * (GK + GK.T)
            d = 1.0 / np.sqrt(np.diag(GM))
            w, V = np.linalg.eigh(d[:, None] * GM * d[None, :])
            keep = w > 1e-12 * w.max()
            Q = d[:, None] * V[:, keep] / np.sqrt(w[keep])
            t, Z = np.linalg.eigh(Q.T @ GK @ Q)
            C = Q @ Z[:, :8]
            Cp = C.copy()
            Cp[:8] = 0.0
            return t[:8], C, Cp, int(keep.sum())

        def ritz_on_x(X):
            nu, C, _, _ = ritz(X.T @ (K @ X), X.T @ (S @ X))
            X = X @ C
            return nu, X, K @ X, S @ X

        def ratios(nu, KX, SX):
            return np.linalg.norm(SX - KX * nu, axis=0) / (np.linalg.norm(SX, axis=0) + np.abs(nu) * np.linalg.norm(KX, axis=0))

        X = np.where(free[:, None], np.random.default_rng(seed).uniform(-1.0, 1.0, size=(n, 8)), 0.0)
        nu, X, KX, SX = ritz_on_x(X)
        P = KP = SP = None
        it, must_step = 0, False
        while True:
            if it > 0 and it % 20 == 0 and not must_step:
                KX, SX = K @ X, S @ X
                if P is not None:
                    KP, SP = K @ P, S @ P
            ratio = ratios(nu, KX, SX)
            W = np.where(free[:, None], Dinv @ (SX - KX * nu), 0.0)
            stop = bool(np.all(ratio[:n_modes] <= tol)) and not must_step
            must_step = False
            if stop or it >= max_it:
                nu, X, KX, SX = ritz_on_x(X)
                ratio = ratios(nu, KX, SX)
                if np.all(ratio[:n_modes] <= tol) or it >= max_it:
                    return nu[:n_modes], ratio[:n_modes], it
                must_step = True
                continue
            B, KB, SB = [X, W], [KX, K @ W], [SX, S @ W]
            if P is not None:
                B, KB, SB = B + [P], KB + [KP], SB + [SP]
            B, KB, SB = np.hstack(B), np.hstack(KB), np.hstack(SB)
            nu, C, Cp, rank = ritz(B.T @ KB, B.T @ SB)
            X, KX, SX = B @ C, KB @ C, SB @ C
            P, KP, SP = (B @ Cp, KB @ Cp, SB @ Cp) if rank == B.shape[1] else (None, None, None)
            it += 1


@functools.lru_cache(maxsize=None)
def column_reference(kind, end_motion=END_MOTION):
    """(deck, x, BucklingReference) of a column deck at its Newton state, computed once and read-only."""
    deck = column_deck(kind, end_motion)
    x = newton_state(deck)
    ref = BucklingReference(deck, x)
    for a in (x, ref.nu, ref.Phi, ref.K, ref.Ksig):
        a.setflags(write=False)
    return deck, x, ref


TRACTION = 0.2                                            # about a quarter of Euler's clamped-free load of the column


def traction_column(traction=TRACTION):
    """The TET4 column clamped at y = 0 with its far end free, under a compressive dead traction (0, -traction, 0) on the
    far end face, applied in one load increment."""
    free_end = column_deck("tet4", end_motion=None)
    faces = mesh.block_side_faces(free_end.nodes, free_end.elements, 1, True)
    return column_deck("tet4", end_motion=None, surface_faces=faces,
                       surface_kind=np.full(len(faces), feahip.LOAD_TRACTION, np.int32),
                       surface_values=np.tile([0.0, -traction, 0.0], (len(faces), 1)))

"""A body of several materials, restated in numpy on the oracle: one OracleSolver per (lambda, mu) pair on the same
deck, and every element's stiffness (Kc + Ksigma), residual, F and sigma taken from the solver of ITS material.  K is
dense; prescribed dofs are masked as feahip_apply_prescribed_bc documents (rows and columns zeroed, the diagonal
kept, f = 0 there for lambda = 0); the Newton loop is the reference's solve() with a dense direct solve."""
import copy

import numpy as np

import mesh
from oracle_binding import OracleSolver

MATERIALS = np.array([[100.0, 100.0], [400.0, 250.0], [30.0, 80.0]])


def scattered_ids(deck):
    """id = (7 e + 3) % 3: every chunk of elements holds all three materials."""
    e = np.arange(len(deck.elements))
    return ((7 * e + 3) % 3).astype(np.int32)


def layered_ids(deck, nmat=3):
    """Layers along y by the element centroid."""
    y = deck.nodes[deck.elements].mean(axis=1)[:, 1]
    lo, hi = deck.nodes[:, 1].min(), deck.nodes[:, 1].max()
    return np.minimum((nmat * (y - lo) / (hi - lo)).astype(np.int32), nmat - 1)


def perturbed(nodes, amp=0.02):
    """A smooth displacement of about 2 % of the body's size on top of the nodes: F != I everywhere."""
    x = np.asarray(nodes, dtype=np.float64)
    L = x.max(axis=0) - x.min(axis=0)
    s = (x - x.min(axis=0)) / L
    d = np.stack([np.sin(1.3 * s[:, 1] + 0.4) * np.cos(0.9 * s[:, 2]),
                  0.8 * s[:, 1] + 0.3 * np.sin(1.1 * s[:, 0]),
                  np.cos(0.7 * s[:, 0] + 1.2 * s[:, 1])], axis=1)
    return x + amp * L.min() * d


def with_materials(deck, materials, ids):
    """A copy of the deck that carries the table."""
    d = copy.copy(deck)
    d.materials = np.ascontiguousarray(materials, dtype=np.float64).reshape(-1, 2)
    d.element_material = np.ascontiguousarray(ids, dtype=np.int32)
    return d


class HeteroRestatement:
    def __init__(self, deck, materials, ids):
        self.deck = deck
        self.ids = np.asarray(ids, dtype=np.int64)
        self.N, self.E, self.npe = len(deck.nodes), len(deck.elements), deck.elements.shape[1]
        self.ndof = 3 * self.N
        self.solvers = []
        for lam, mu in np.asarray(materials, dtype=np.float64).reshape(-1, 2):
            d = copy.copy(deck)
            d.parameters = np.array([lam, mu])
            self.solvers.append(OracleSolver(d))
        self.dofs = (3 * deck.elements[:, :, None] + np.arange(3)[None, None, :]).reshape(self.E, -1)
        self.mask = np.zeros(self.ndof, dtype=bool)
        self.cval = np.zeros(self.ndof)
        for nd, ty, v in zip(deck.presc_node, deck.presc_type, deck.presc_values):
            for j in range(3):
                if ty & (1 << j):
                    self.mask[3 * nd + j] = True
                    self.cval[3 * nd + j] = v[j]

    def close(self):
        for o in self.solvers:
            o.close()

    def assemble(self, x):
        """(K dense, f, F[E][G][3][3], sigma[E][G][3][3]) at the nodes x, before any boundary condition."""
        self.bad = 0                                          # Gauss points with a non-positive Jacobian (geometry only)
        for o in self.solvers:
            o.set_nodes(x)
            self.bad = max(self.bad, o.update_state())
        K, f = np.zeros((self.ndof, self.ndof)), np.zeros(self.ndof)
        Fs = [o.graddefs() for o in self.solvers]
        Ss = [o.stresses() for o in self.solvers]
        F, S = np.empty_like(Fs[0]), np.empty_like(Ss[0])
        for e in range(self.E):
            o = self.solvers[self.ids[e]]
            kc, ks = o.element_stiffness(e)
            d = self.dofs[e]
            K[np.ix_(d, d)] += kc + ks
            f[d] += o.element_residual(e)
            F[e], S[e] = Fs[self.ids[e]][e], Ss[self.ids[e]][e]
        return K, f, F, S

    def yale_values(self, K, offsets, indexes):
        """The entries of the dense K at the positions of a Yale pattern."""
        rows = np.repeat(np.arange(self.ndof), np.diff(offsets))
        return K[rows, indexes]

    def masked(self, K, f):
        K, f = K.copy(), f.copy()
        diag = K[self.mask, self.mask].copy()
        K[self.mask, :] = 0.0
        K[:, self.mask] = 0.0
        K[self.mask, self.mask] = diag
        f[self.mask] = 0.0
        return K, f

    def solve(self, load_increments, max_newton, desired_tolerance):
        """The reference's solve() with full Newton: (steps done, iterations per step, nodes [N][3])."""
        x = np.array(self.deck.nodes, dtype=np.float64)
        its = []
        for step in range(load_increments):
            x = x + self.cval.reshape(-1, 3)
            it = 0
            while True:
                it += 1
                K, f, _, _ = self.assemble(x)
                K, f = self.masked(K, f)
                u = np.linalg.solve(K, f)
                tol = float(f @ u)
                x = x + u.reshape(-1, 3)
                if not (abs(tol) > desired_tolerance and it < max_newton):
                    break
            its.append(it)
            if it == max_newton:
                return step, its, x
        return load_increments, its, x


def arclength_hetero(deck, *args, **kw):
    """arclength_reference.arclength on a deck with a material table: the same loop, its K and T taken from the
    heterogeneous restatement instead of the single oracle."""
    from unittest import mock

    import arclength_reference as ar

    class HeteroArc(ar.Restatement):
        def __init__(self, d):
            super().__init__(d)
            self.h = HeteroRestatement(d, d.materials, d.element_material)

        def system(self, x, lam):
            K, f, _, _ = self.h.assemble(x)
            K, _ = self.h.masked(K, f)
            F = self.external(x)
            R = lam * F + f
            R[self.mask] = 0.0
            return K, R, F, self.h.bad

        def close(self):
            self.h.close()
            super().close()

    with mock.patch.object(ar, "Restatement", HeteroArc):
        return ar.arclength(deck, *args, **kw)

"""Result recovery restated in float64 numpy on the oracle: the volume-weighted nodal average of the Cauchy stress from
the oracle's own stresses(), detj() and graddefs() per Gauss point (through tests/hetero_reference.py, which takes every
element's state from the oracle solver of ITS material), the strain-energy potentials of the two models, and the
reactions as minus the oracle's unmasked residual minus the applied loads.  Nothing here calls the library under test."""
import numpy as np

import feahip
from hetero_reference import HeteroRestatement, perturbed

SIG6 = ((0, 0), (1, 1), (2, 2), (0, 1), (1, 2), (0, 2))       # xx yy zz xy yz xz


def smooth_field(nodes, amp=0.12):
    """A smooth, non-homogeneous displacement large enough for max|F - I| >= 0.05 on the test bars."""
    return perturbed(nodes, amp)


def psi(F, model, lam, mu):
    """Strain-energy density per reference volume of the two models, F[..., 3, 3]."""
    F = np.asarray(F, dtype=np.float64)
    if model == feahip.MODEL_COMPRESSIBLE_NEOHOOKEAN:
        lnJ = np.log(np.linalg.det(F))
        trb = np.einsum("...ij,...ij->...", F, F)
        return 0.5 * mu * (trb - 3.0) - mu * lnJ + 0.5 * lam * lnJ ** 2
    E = 0.5 * (np.einsum("...ki,...kj->...ij", F, F) - np.eye(3))
    trE = np.einsum("...ii->...", E)
    return 0.5 * lam * trE ** 2 + mu * np.einsum("...ij,...ij->...", E, E)


def cauchy(F, model, lam, mu):
    """sigma(F) of the two models in closed form (what fd_constitutive documents)."""
    J = np.linalg.det(F)
    if model == feahip.MODEL_COMPRESSIBLE_NEOHOOKEAN:
        return (mu * (F @ F.T - np.eye(3)) + lam * np.log(J) * np.eye(3)) / J
    E = 0.5 * (F.T @ F - np.eye(3))
    return F @ (lam * np.trace(E) * np.eye(3) + 2.0 * mu * E) @ F.T / J


def von_mises(sig6):
    """sqrt(3/2 s:s) of the symmetric tensors given as xx yy zz xy yz xz, [..., 6]."""
    s = np.asarray(sig6, dtype=np.float64)
    p = s[..., :3].sum(axis=-1) / 3.0
    dev = s[..., :3] - p[..., None]
    return np.sqrt(1.5 * ((dev ** 2).sum(axis=-1) + 2.0 * (s[..., 3:] ** 2).sum(axis=-1)))


class ResultsRestatement:
    def __init__(self, deck):
        self.deck = deck
        table = len(getattr(deck, "materials", [])) > 0
        self.mats = np.asarray(deck.materials if table else [deck.parameters[:2]], dtype=np.float64).reshape(-1, 2)
        self.ids = np.asarray(deck.element_material if table else np.zeros(len(deck.elements)), dtype=np.int64)
        self.h = HeteroRestatement(deck, self.mats, self.ids)
        self.w = feahip.element_tables(deck.ele_type, deck.gauss_nodes_count)[0]
        self.N, self.E, self.npe = self.h.N, self.h.E, self.h.npe
        self.faces = None
        if len(getattr(deck, "surface_kind", [])):
            import arclength_reference as ar
            self.faces, self.owner = ar.ordered_faces(deck), ar.face_owners(deck)

    def close(self):
        self.h.close()

    def state(self, x):
        """(F[E][G][3][3], sigma[E][G][3][3], det J[E][G]) of the oracle at the nodes x, every element with its material."""
        h = self.h
        for o in h.solvers:
            o.set_nodes(x)
            o.update_state()
        Fs = [o.graddefs().copy() for o in h.solvers]
        Ss = [o.stresses().copy() for o in h.solvers]
        e = np.arange(self.E)
        F = np.stack(Fs)[self.ids, e]
        S = np.stack(Ss)[self.ids, e]
        return F, S, h.solvers[0].detj().copy()

    def nodal_stresses(self, x, material=-1):
        """(sig6[N][6], von Mises[N], weight[N]) over all elements, or over those of one material."""
        _, S, dj = self.state(x)
        vol = self.w[None, :] * np.abs(dj)
        sel = np.ones(self.E, dtype=bool) if material < 0 else self.ids == material
        se = np.einsum("eg,egij->eij", vol, S)[sel]
        ve = vol.sum(axis=1)[sel]
        conn = self.deck.elements[sel]
        num, den = np.zeros((self.N, 3, 3)), np.zeros(self.N)
        for k in range(self.npe):
            np.add.at(num, conn[:, k], se)
            np.add.at(den, conn[:, k], ve)
        sig = np.where(den[:, None, None] > 0, num / np.where(den > 0, den, 1.0)[:, None, None], 0.0)
        sig6 = np.stack([sig[:, i, j] for i, j in SIG6], axis=1)
        return sig6, von_mises(sig6), den

    def element_energy(self, x):
        F, _, dj = self.state(x)
        lam, mu = self.mats[self.ids, 0][:, None], self.mats[self.ids, 1][:, None]
        dj0 = dj / np.linalg.det(F)
        return (self.w[None, :] * dj0 * psi(F, self.deck.model, lam, mu)).sum(axis=1)

    def energy(self, x):
        """(W, w_node[N]): the strain energy and the nodal shares W_e / npe."""
        We = self.element_energy(x)
        wn = np.zeros(self.N)
        for k in range(self.npe):
            np.add.at(wn, self.deck.elements[:, k], We / self.npe)
        return float(We.sum()), wn

    def internal(self, x):
        """The oracle's residual before masking, f = -T(x), from its element residuals."""
        h = self.h
        for o in h.solvers:
            o.set_nodes(x)
            o.update_state()
        f = np.zeros(h.ndof)
        for e in range(h.E):
            f[h.dofs[e]] += h.solvers[h.ids[e]].element_residual(e)
        return f

    def external(self, x):
        """F_surf(x) at load factor 1."""
        if self.faces is None:
            return np.zeros(self.h.ndof)
        from test_surface_loads import reference_forces
        d = self.deck
        return reference_forces(d, x, self.faces, self.owner, d.surface_kind, d.surface_values, 1.0).ravel()

    def reactions(self, x, lam, body=None):
        """r = T(x) - lambda (F_surf(x) + F_body) on the prescribed dofs, zero elsewhere."""
        F = self.external(x) + (0.0 if body is None else body)
        r = -self.internal(x) - lam * F
        r[~self.h.mask] = 0.0
        return r

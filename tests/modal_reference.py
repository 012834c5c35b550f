"""Modal analysis restated in float64 numpy / scipy: K from the oracle at given nodes (tests/hetero_reference.py takes
every element's stiffness from the oracle solver of its material; one material is a table of one), masked as
feahip_apply_prescribed_bc(0.0) documents, M the consistent mass of tests/dynamics_reference.py, and scipy.linalg.eigh on
the free dofs.  Nothing here calls the library under test."""
import numpy as np
import scipy.linalg

from dynamics_reference import dense_mass
from hetero_reference import HeteroRestatement


class ModalReference:
    """lam[free dofs] ascending, Phi[3N][free dofs] (zero on the prescribed dofs, M-orthonormal), K (masked) and M
    (unmasked) dense, mask[3N]."""

    def __init__(self, deck, rho, x=None, materials=None, ids=None):
        table = materials is not None
        mats = np.asarray(materials if table else [deck.parameters[:2]], dtype=np.float64).reshape(-1, 2)
        ids = np.asarray(ids if table else np.zeros(len(deck.elements)), dtype=np.int64)
        h = HeteroRestatement(deck, mats, ids)
        try:
            K, f, _, _ = h.assemble(np.asarray(deck.nodes if x is None else x, dtype=np.float64))
            assert h.bad == 0
            self.K, _ = h.masked(K, f)
            self.K_unmasked = K
        finally:
            h.close()
        self.mask = h.mask
        self.M = dense_mass(deck, rho, ids)
        self.free = np.nonzero(~self.mask)[0]
        Kf, Mf = self.K[np.ix_(self.free, self.free)], self.M[np.ix_(self.free, self.free)]
        self.lam, vec = scipy.linalg.eigh(0.5 * (Kf + Kf.T), 0.5 * (Mf + Mf.T))
        self.Phi = np.zeros((len(self.mask), len(self.free)))
        self.Phi[self.free] = vec

    def residual_ratio(self, lam, phi):
        """||K phi - lam M phi|| / (||K phi|| + |lam| ||M phi||) with the M-product zeroed on the prescribed dofs."""
        Kp, Mp = self.K @ phi, np.where(self.mask, 0.0, self.M @ phi)
        return np.linalg.norm(Kp - lam * Mp) / (np.linalg.norm(Kp) + abs(lam) * np.linalg.norm(Mp))

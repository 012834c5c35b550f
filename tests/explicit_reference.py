"""Explicit dynamics restated in float64 numpy: the HRZ-lumped mass from the element tables, the Gershgorin bound on
the dense K of tests/hetero_reference.py, and the central-difference loop of feahip_solve_explicit with T from the
oracle (state, external forces and body force of tests/dynamics_reference.py).  Nothing here calls the library under
test."""
import numpy as np

import feahip
from dynamics_reference import MASS_POINTS, DynamicsRestatement


def hrz_lumped_mass(deck, rho, ids=None):
    """ml[N] = sum_e m_e d_a / sum_b d_b with m_e = sum_g rho_e w_g det J0_g and d_a = sum_g rho_e w_g det J0_g N_a(g)^2."""
    rho = np.atleast_1d(np.asarray(rho, dtype=np.float64))
    rho_e = np.full(len(deck.elements), rho[0]) if len(rho) == 1 else rho[np.asarray(ids)]
    w, N, dN = feahip.element_tables(deck.ele_type, MASS_POINTS[deck.ele_type])
    X = np.asarray(deck.nodes, dtype=np.float64)
    ml = np.zeros(len(X))
    for e, nd in enumerate(deck.elements):
        J = np.einsum("gik,kj->gij", dN, X[nd])
        wd = rho_e[e] * w * np.linalg.det(J)
        assert np.all(wd > 0)
        d = np.einsum("g,ga->a", wd, N * N)
        np.add.at(ml, nd, wd.sum() * d / d.sum())
    return ml


def body_mass(deck, rho, ids=None):
    """sum_e rho_e V_e by the mass rule."""
    rho = np.atleast_1d(np.asarray(rho, dtype=np.float64))
    rho_e = np.full(len(deck.elements), rho[0]) if len(rho) == 1 else rho[np.asarray(ids)]
    w, _, dN = feahip.element_tables(deck.ele_type, MASS_POINTS[deck.ele_type])
    X = np.asarray(deck.nodes, dtype=np.float64)
    return float(sum(rho_e[e] * (w * np.linalg.det(np.einsum("gik,kj->gij", dN, X[nd]))).sum()
                     for e, nd in enumerate(deck.elements)))


def gershgorin_bound(K, ml):
    """max_i (sum_j |K_ij|) / ml(node of i): an upper bound of the largest eigenvalue of M_L^-1 K."""
    return float((np.abs(K).sum(axis=1) / np.repeat(ml, 3)).max())


def omega_max(K, ml):
    """sqrt of the largest eigenvalue of M_L^-1/2 K M_L^-1/2 (dense eigh)."""
    s = 1.0 / np.sqrt(np.repeat(ml, 3))
    A = K * s[:, None] * s[None, :]
    return float(np.sqrt(np.linalg.eigvalsh(0.5 * (A + A.T)).max()))


def hub_fan(spokes=150):
    """Linear tetrahedra around one hub node whose block row has spokes + 2 blocks (the hub, the ring and the pole: 152,
    more than the 128-block tile, for the 150 spokes of the default): a ring of `spokes` nodes around the hub, a pole
    above; tetrahedron k = (hub, ring k, ring k + 1, pole).  Clamped at the pole, so the hub is free."""
    ang = 2.0 * np.pi * np.arange(spokes) / spokes
    ring = np.stack([np.cos(ang), np.sin(ang), 0.05 * np.cos(3 * ang)], axis=1)
    nodes = np.vstack([[0.0, 0.0, 0.0], ring, [0.0, 0.0, 0.8]])
    hub, pole = 0, spokes + 1
    el = np.array([[hub, 1 + k, 1 + (k + 1) % spokes, pole] for k in range(spokes)], dtype=np.int32)
    return feahip.Deck(ele_type=feahip.TETRAHEDRA4, gauss_nodes_count=1, nodes=nodes, elements=el, modified_newton=False,
                       solver_type=feahip.CG, presc_node=np.array([pole], dtype=np.int32), presc_type=np.array([7], dtype=np.int32),
                       presc_values=np.zeros((1, 3)))


class ExplicitRestatement(DynamicsRestatement):
    """The Newmark restatement's state plus the lumped mass, the stable step and the loop of feahip_solve_explicit."""

    def __init__(self, deck, rho, body=None):
        super().__init__(deck, rho, body)
        self.ml = hrz_lumped_mass(deck, rho, self.h.ids)
        self.ml3 = np.repeat(self.ml, 3)
        self.perturb = None                                   # (rng, relative size): noise on the residual, an experiment

    def residual(self, x):
        """lambda (F_surf + F_body) - T(x), from the oracle's element residuals alone."""
        h = self.h
        self.bad = 0                                          # Gauss points with det J <= 0 at x
        for o in h.solvers:
            o.set_nodes(x)
            self.bad = max(self.bad, o.update_state())
        f = np.zeros(h.ndof)
        for e in range(h.E):
            f[h.dofs[e]] += h.solvers[h.ids[e]].element_residual(e)
        R = self.lam * self.external(x) + f
        if self.perturb is not None:
            rng, eps = self.perturb
            R = R + eps * np.abs(R).max() * rng.uniform(-1.0, 1.0, len(R))
        return R

    def tangent(self, x=None):
        K, _, _, _ = self.h.assemble(self.x if x is None else x)
        return K

    def bound(self, x=None):
        return gershgorin_bound(self.tangent(x), self.ml)

    def stable_step(self, x=None):
        return 2.0 / np.sqrt(self.bound(x))

    def kinetic_energy(self):
        return 0.5 * float((self.ml3 * self.v.ravel() ** 2).sum())

    def explicit(self, n_steps, dt=0.0, safety=0.9, restep=0, dlambda=0.0):
        """([(x, v, a) after every step], [dt of every step])."""
        traj, dts = [], []
        m, cv = self.mask, self.cval
        for step in range(n_steps):
            if dt == 0.0 and (step == 0 or (restep > 0 and step % restep == 0)):
                h = safety * self.stable_step()
            elif dt != 0.0:
                h = dt
            vh = (self.v + 0.5 * h * self.a).ravel()
            vh[m] = 0.0
            x = (self.x.ravel() + h * vh + dlambda * cv).reshape(-1, 3)
            self.lam += dlambda
            R = self.residual(x)
            a = R / self.ml3
            a[m] = 0.0
            vh[m] = dlambda * cv[m] / h
            self.x, self.a = x, a.reshape(-1, 3)
            self.v = (vh + 0.5 * h * a).reshape(-1, 3)
            self.t += h
            traj.append((self.x.copy(), self.v.copy(), self.a.copy()))
            dts.append(h)
        return traj, dts

"""Implicit dynamics restated in float64 numpy: the consistent mass matrix from the element tables, K and T from the
oracle (through tests/hetero_reference.py, which takes every element's stiffness and residual from the oracle solver
of its material), dead tractions from tests/test_surface_loads.py, and the Newmark loop of feahip_solve_dynamic with
dense solves.  Nothing here calls the library under test."""
import numpy as np

import feahip
import mesh
from hetero_reference import HeteroRestatement

MASS_POINTS = {feahip.TETRAHEDRA4: 4, feahip.TETRAHEDRA10: 27, feahip.HEXAHEDRA8: 8}
DENSITIES = np.array([1.5, 0.7, 3.1])


def element_volumes_and_mass(deck, rho_e):
    """(V[E], M scalar [N][N]): M_ab = sum_e rho_e sum_g w_g det J0_g N_a N_b with the mass rule of the element type."""
    w, N, dN = feahip.element_tables(deck.ele_type, MASS_POINTS[deck.ele_type])
    X = np.asarray(deck.nodes, dtype=np.float64)
    n = len(X)
    M = np.zeros((n, n))
    V = np.zeros(len(deck.elements))
    for e, nd in enumerate(deck.elements):
        J = np.einsum("gik,kj->gij", dN, X[nd])               # J[g][i][j] = sum_k dN[g][i][k] X[k][j]
        wd = w * np.linalg.det(J)
        assert np.all(wd > 0)
        V[e] = wd.sum()
        M[np.ix_(nd, nd)] += rho_e[e] * np.einsum("g,ga,gb->ab", wd, N, N)
    return V, M


def dense_mass(deck, rho, ids=None):
    """The 3N x 3N consistent mass: rho a number, or one density per material id."""
    rho = np.atleast_1d(np.asarray(rho, dtype=np.float64))
    rho_e = np.full(len(deck.elements), rho[0]) if len(rho) == 1 else rho[np.asarray(ids)]
    _, M = element_volumes_and_mass(deck, rho_e)
    return np.kron(M, np.eye(3))


def free_block(kind="tet4", dims=(2, 2, 2), **kw):
    """An unconstrained block: no prescribed node at all."""
    if kind == "hex8":
        nodes, el = mesh.hex_block(*dims, origin=(0.0, 0.0, 0.0), size=(1.0, 1.0, 1.0))
        return feahip.Deck(ele_type=feahip.HEXAHEDRA8, gauss_nodes_count=8, nodes=nodes, elements=el, modified_newton=False,
                           solver_type=feahip.CG, **kw)
    quad = kind == "tet10"
    nodes, el = mesh.kuhn_block(*dims, quad, origin=(0.0, 0.0, 0.0), size=(1.0, 1.0, 1.0))
    return feahip.Deck(ele_type=feahip.TETRAHEDRA10 if quad else feahip.TETRAHEDRA4, gauss_nodes_count=5 if quad else 1,
                       nodes=nodes, elements=el, modified_newton=False, solver_type=feahip.CG, **kw)


def loaded_bar(kind="tet4", dims=(2, 4, 2), traction=10.0, model=feahip.MODEL_COMPRESSIBLE_NEOHOOKEAN, end_motion=None, **kw):
    """A bar along y clamped at y = 0; a dead traction along y on the far end, or (end_motion = dy per increment) the
    far end prescribed instead."""
    size = (1.0, 2.0, 1.0)
    if kind == "hex8":
        nodes, el = mesh.hex_block(*dims, origin=(0.0, 0.0, 0.0), size=size)
        et, g = feahip.HEXAHEDRA8, 8
    else:
        nodes, el = mesh.kuhn_block(*dims, kind == "tet10", origin=(0.0, 0.0, 0.0), size=size)
        et, g = (feahip.TETRAHEDRA10, 5) if kind == "tet10" else (feahip.TETRAHEDRA4, 1)
    bot = np.nonzero(np.abs(nodes[:, 1]) < 1e-12)[0]
    ids, types, vals = bot, np.full(len(bot), 7), np.zeros((len(bot), 3))
    if end_motion is not None:
        top = np.nonzero(np.abs(nodes[:, 1] - size[1]) < 1e-12)[0]
        ids, types = np.concatenate([bot, top]), np.concatenate([types, np.full(len(top), 7)])
        vals = np.vstack([vals, np.tile([0.0, end_motion, 0.0], (len(top), 1))])
    else:
        faces = mesh.block_side_faces(nodes, el, 1, True)
        kw.update(surface_faces=faces, surface_kind=np.full(len(faces), feahip.LOAD_TRACTION, np.int32),
                  surface_values=np.tile([0.0, traction, 0.0], (len(faces), 1)))
    kw.setdefault("solver_tolerance", 1e-13)
    kw.setdefault("desired_tolerance", 1e-14)
    return feahip.Deck(model=model, parameters=[100.0, 100.0], ele_type=et, gauss_nodes_count=g, nodes=nodes, elements=el,
                       presc_node=ids.astype(np.int32), presc_type=types.astype(np.int32), presc_values=vals,
                       max_newton_count=30, modified_newton=False, solver_type=feahip.CG, **kw)


class DynamicsRestatement:
    """State (x, v, a, t, load factor) and the loops of feahip_solve, feahip_consistent_acceleration and
    feahip_solve_dynamic on it."""

    def __init__(self, deck, rho, body=None, solve=np.linalg.solve):
        self.deck = deck
        table = len(getattr(deck, "materials", [])) > 0
        mats = deck.materials if table else np.array([deck.parameters[:2]])
        ids = deck.element_material if table else np.zeros(len(deck.elements), dtype=np.int64)
        self.h = HeteroRestatement(deck, mats, ids)
        self.mask, self.cval = self.h.mask, self.h.cval
        self.M = dense_mass(deck, rho, ids)
        b = np.zeros(3) if body is None else np.asarray(body, dtype=np.float64)
        self.Fbody = self.M @ np.tile(b, len(deck.nodes))
        self.x = np.array(deck.nodes, dtype=np.float64)
        self.v, self.a = np.zeros_like(self.x), np.zeros_like(self.x)
        self.t, self.lam = 0.0, 0.0
        self.solve_dense = solve
        self.faces = None
        if len(getattr(deck, "surface_kind", [])):
            import arclength_reference as ar
            self.faces, self.owner = ar.ordered_faces(deck), ar.face_owners(deck)

    def close(self):
        self.h.close()

    def external(self, x):
        """F_surf(x) + F_body at load factor 1."""
        F = self.Fbody.copy()
        if self.faces is not None:
            from test_surface_loads import reference_forces
            d = self.deck
            F += reference_forces(d, x, self.faces, self.owner, d.surface_kind, d.surface_values, 1.0)
        return F

    def residual_and_stiffness(self, x):
        K, f, _, _ = self.h.assemble(x)
        return K, self.lam * self.external(x) + f

    def consistent_acceleration(self):
        _, R = self.residual_and_stiffness(self.x)
        Mm, Rm = self.h.masked(self.M, R)
        self.a = self.solve_dense(Mm, Rm).reshape(-1, 3)

    def static(self, increments, max_newton, tol):
        its = []
        for step in range(increments):
            self.x = self.x + self.cval.reshape(-1, 3)
            self.lam += 1.0
            it = 0
            while True:
                it += 1
                K, R = self.residual_and_stiffness(self.x)
                K, R = self.h.masked(K, R)
                u = self.solve_dense(K, R)
                e = float(R @ u)
                self.x = self.x + u.reshape(-1, 3)
                if not (abs(e) > tol and it < max_newton):
                    break
            its.append(it)
            if it == max_newton:
                return step, its
        return increments, its

    def newmark(self, n_steps, dt, beta, gamma, dlambda, max_newton, tol):
        """(steps done, Newton iterations per step, [(x, v, a) after every completed step])."""
        a0 = 1.0 / (beta * dt * dt)
        its, traj = [], []
        for step in range(n_steps):
            xt = self.x + dt * self.v + dt * dt * (0.5 - beta) * self.a
            vt = self.v + dt * (1.0 - gamma) * self.a
            x = self.x + dlambda * self.cval.reshape(-1, 3)
            self.lam += dlambda
            it = 0
            while True:
                it += 1
                K, R = self.residual_and_stiffness(x)
                R = R - a0 * (self.M @ (x - xt).ravel())
                K, R = self.h.masked(K + a0 * self.M, R)
                u = self.solve_dense(K, R)
                e = float(R @ u)
                x = x + u.reshape(-1, 3)
                if not (abs(e) > tol and it < max_newton):
                    break
            its.append(it)
            if it == max_newton:
                self.lam -= dlambda
                return step, its, traj
            self.a = a0 * (x - xt)
            self.v = vt + gamma * dt * self.a
            self.x = x
            self.t += dt
            traj.append((self.x.copy(), self.v.copy(), self.a.copy()))
        return n_steps, its, traj

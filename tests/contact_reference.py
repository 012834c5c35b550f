"""Frictionless node-to-rigid-surface contact restated in float64 numpy: reference-area weights of the contact nodes,
gaps and normals of the five obstacle kinds, forces, diagonal blocks, potential, augmentation, and the loops that use
them -- a static Newton loop on the CPU oracle with the contact term added to its values() and forces() views, and the
explicit loop of tests/explicit_reference.py with the contact force in the residual.  Nothing here calls the library
under test."""
import math

import numpy as np

PLANE, SPHERE, SPHERE_INSIDE, CYLINDER, CYLINDER_INSIDE = 0, 1, 2, 3, 4


# ---- weights ----------------------------------------------------------------------------------------------------------
def _tri_points():
    """The 6-point degree-4 rule on the unit triangle (area 1/2): [(xi, eta, w)]."""
    s10, r = math.sqrt(10.0), math.sqrt(38.0 - 44.0 * math.sqrt(0.4))
    d = math.sqrt(213125.0 - 53320.0 * s10)
    out = []
    for a, w in (((8 - s10 + r) / 18, (620 + d) / 3720), ((8 - s10 - r) / 18, (620 - d) / 3720)):
        out += [(a, a, 0.5 * w), (1 - 2 * a, a, 0.5 * w), (a, 1 - 2 * a, 0.5 * w)]
    return out


def _tri6(xi, eta):
    L = np.array([1 - xi - eta, xi, eta])
    dL = np.array([[-1.0, 1.0, 0.0], [-1.0, 0.0, 1.0]])
    pairs = [(0, 1), (1, 2), (2, 0)]
    N = np.concatenate([L * (2 * L - 1), [4 * L[a] * L[b] for a, b in pairs]])
    dN = [np.concatenate([(4 * L - 1) * dL[k], [4 * (dL[k][a] * L[b] + L[a] * dL[k][b]) for a, b in pairs]]) for k in range(2)]
    return N, dN[0], dN[1]


def _quad4(xi, eta):
    sx, se = np.array([-1.0, 1.0, 1.0, -1.0]), np.array([-1.0, -1.0, 1.0, 1.0])
    return 0.25 * (1 + sx * xi) * (1 + se * eta), 0.25 * sx * (1 + se * eta), 0.25 * se * (1 + sx * xi)


def face_weights(X):
    """(w[npf], area) of one face with the reference nodes X[npf][3] in a face order (corners around, then the mid-sides
    (0,1) (1,2) (2,0)): tri3 A/3; quad4 the row sums of int N_a dA by 2 x 2 Gauss; tri6 the HRZ lumping."""
    npf = len(X)
    if npf == 3:
        A = 0.5 * np.linalg.norm(np.cross(X[1] - X[0], X[2] - X[0]))
        return np.full(3, A / 3.0), A
    if npf == 4:
        q = 1.0 / math.sqrt(3.0)
        pts, shape = [(a, b, 1.0) for b in (-q, q) for a in (-q, q)], _quad4
    else:
        pts, shape = _tri_points(), _tri6
    lump, A = np.zeros(npf), 0.0
    for xi, eta, w in pts:
        N, dx, de = shape(xi, eta)
        dA = w * np.linalg.norm(np.cross(dx @ X, de @ X))
        A += dA
        lump += (N * N if npf == 6 else N) * dA
    return (lump * A / lump.sum() if npf == 6 else lump), A


def _ring_order(X):
    """The corners of a flat quad in the order around it (the caller's faces come in any node order)."""
    c = X.mean(axis=0)
    n = np.cross(X[1] - X[0], X[2] - X[0])
    if np.linalg.norm(n) < 1e-12 * np.linalg.norm(X[1] - X[0]) ** 2:
        n = np.cross(X[1] - X[0], X[3] - X[0])
    e1 = X[0] - c
    e2 = np.cross(n, e1)
    return np.argsort([math.atan2((p - c) @ e2, (p - c) @ e1) for p in X])


def canonical_face(X0, face, elements=None):
    """The face's nodes in an order face_weights understands, whatever order the caller gave them in: a quad around its
    centre; a tri6 corners first (a corner is a node that is no midpoint of two others), then the mid-sides in place."""
    face = np.asarray(face)
    X = X0[face]
    if len(face) == 3:
        return face
    if len(face) == 4:
        return face[_ring_order(X)]
    mids = {}
    for k in range(6):
        for i in range(6):
            for j in range(i + 1, 6):
                if k not in (i, j) and np.allclose(X[k], 0.5 * (X[i] + X[j]), atol=1e-9 * (1 + np.abs(X).max())):
                    mids[k] = (i, j)
    corners = [k for k in range(6) if k not in mids]
    assert len(corners) == 3, "a straight-sided 6-node face is expected"
    mid_of = {frozenset(v): k for k, v in mids.items() if set(v) <= set(corners)}
    c0, c1, c2 = corners
    return face[[c0, c1, c2, mid_of[frozenset((c0, c1))], mid_of[frozenset((c1, c2))], mid_of[frozenset((c2, c0))]]]


def contact_weights(X0, faces):
    """(nodes[n] ascending, w[n]): every face's weights summed at its nodes."""
    X0 = np.asarray(X0, dtype=np.float64)
    w = {}
    for f in faces:
        fc = canonical_face(X0, f)
        wf, _ = face_weights(X0[fc])
        for a, v in zip(fc, wf):
            w[int(a)] = w.get(int(a), 0.0) + v
    nodes = np.array(sorted(w), dtype=np.int64)
    return nodes, np.array([w[a] for a in nodes])


# ---- obstacles --------------------------------------------------------------------------------------------------------
def obstacle(kind, point, direction=(0.0, 0.0, 0.0), radius=0.0, travel=(0.0, 0.0, 0.0)):
    d = np.asarray(direction, dtype=np.float64)
    if kind in (PLANE, CYLINDER, CYLINDER_INSIDE):
        d = d / np.linalg.norm(d)
    else:
        d = np.zeros(3)
    return {"kind": kind, "point": np.asarray(point, dtype=np.float64), "direction": d, "radius": float(radius),
            "travel": np.asarray(travel, dtype=np.float64)}


def pair(ob, x, lam):
    """(g, n[3], rho, s, P[3][3]) of one node against one obstacle at load factor lam; None where rho = 0."""
    c = ob["point"] + lam * ob["travel"]
    a = ob["direction"]
    q = x - c
    if ob["kind"] == PLANE:
        return q @ a, a.copy(), 1.0, 0.0, np.zeros((3, 3))
    P = np.eye(3)
    if ob["kind"] in (CYLINDER, CYLINDER_INSIDE):
        P = P - np.outer(a, a)
        q = P @ q
    rho = np.linalg.norm(q)
    if rho == 0.0:
        return None
    s = 1.0 if ob["kind"] in (SPHERE, CYLINDER) else -1.0
    return s * (rho - ob["radius"]), s * q / rho, rho, s, P


class Contact:
    """The contact term of a mesh: nodes, weights, obstacles, penalty and the multipliers mu[n][n_obs]."""

    def __init__(self, X0, faces, obstacles, penalty):
        self.nodes, self.w = contact_weights(X0, faces)
        self.obstacles = list(obstacles)
        self.eps = float(penalty)
        self.mu = np.zeros((len(self.nodes), len(self.obstacles)))

    def pairs(self, x, lam):
        """[(i, o, g, n, rho, s, P, t)] of every pair that has a normal, node-major, obstacles in their order."""
        out = []
        for i, a in enumerate(self.nodes):
            for o, ob in enumerate(self.obstacles):
                p = pair(ob, x[a], lam)
                if p is None:
                    continue
                g, n, rho, s, P = p
                out.append((i, o, g, n, rho, s, P, max(0.0, self.mu[i, o] - self.eps * g)))
        return out

    def forces(self, x, lam):
        F = np.zeros((len(x), 3))
        for i, o, g, n, rho, s, P, t in self.pairs(x, lam):
            F[self.nodes[i]] += self.w[i] * t * n
        return F.ravel()

    def blocks(self, x, lam, curvature=True):
        """{node: K_c[3][3]} = -dF_c/dx of the node's own block (nodes without an active pair are absent)."""
        B = {}
        for i, o, g, n, rho, s, P, t in self.pairs(x, lam):
            if t > 0.0:
                k = self.eps * np.outer(n, n)
                if curvature:
                    k = k - s * t * (P - np.outer(n, n)) / rho
                B[int(self.nodes[i])] = B.get(int(self.nodes[i]), np.zeros((3, 3))) + self.w[i] * k
        return B

    def bound_blocks(self, x, lam):
        """{node: sum_o w eps n n'} over EVERY pair, whatever its gap: what the stable-step estimate adds."""
        B = {}
        for i, o, g, n, rho, s, P, t in self.pairs(x, lam):
            B[int(self.nodes[i])] = B.get(int(self.nodes[i]), np.zeros((3, 3))) + self.w[i] * self.eps * np.outer(n, n)
        return B

    def potential(self, x, lam):
        return sum(self.w[i] * t * t / (2.0 * self.eps) for i, o, g, n, rho, s, P, t in self.pairs(x, lam))

    def info(self, x, lam):
        """(active pairs, largest penetration over them or 0, sum w t, Pi_c)."""
        act = [(self.w[i], t, -g) for i, o, g, n, rho, s, P, t in self.pairs(x, lam) if t > 0.0]
        return (len(act), max([0.0] + [p for _, _, p in act]), sum(w * t for w, t, _ in act),
                sum(w * t * t / (2.0 * self.eps) for w, t, _ in act))

    def status(self, x, lam):
        """(gap[N]: smallest over the obstacles, +inf elsewhere; pressure[N]: summed t)."""
        gap, t_sum = np.full(len(x), np.inf), np.zeros(len(x))
        for i, o, g, n, rho, s, P, t in self.pairs(x, lam):
            gap[self.nodes[i]] = min(gap[self.nodes[i]], g)
            t_sum[self.nodes[i]] += t
        return gap, t_sum

    def augment(self, x, lam):
        for i, o, g, n, rho, s, P, t in self.pairs(x, lam):
            self.mu[i, o] = t


# ---- the static Newton loop on the oracle ----------------------------------------------------------------------------
def add_blocks_csr(offsets, indexes, values, blocks):
    """values (per-dof CSR, full pattern, sorted columns) += the 3 x 3 diagonal blocks {node: B}."""
    for a, B in blocks.items():
        for i in range(3):
            r = 3 * a + i
            cols = indexes[offsets[r]:offsets[r + 1]]
            for j in range(3):
                k = np.searchsorted(cols, 3 * a + j)
                assert cols[k] == 3 * a + j
                values[offsets[r] + k] += B[i, j]


def solve_static(oracle, contact, load_increments, max_newton, desired_tolerance, solver_type, augment_max=0,
                 gap_tolerance=0.0, curvature=True, solver_tolerance=1e-14, solver_max_iter=20000):
    """feahip_solve with contact, full Newton, on an OracleSolver: (its per increment, tolerance log, steps done).
    Per iteration: state, K and f of the oracle, the contact term added to both views, prescribed dofs, solve, energy,
    update.  After a converged increment, up to augment_max multiplier updates, each followed by the same iterations."""
    its, tol_log, lam = [], [], 0.0
    off, idx = oracle.offsets(), oracle.indexes()
    step = 0
    for step in range(load_increments):
        oracle.update_nodes_with_bc(1.0)
        lam += 1.0

        def newton_pass():
            k = 0
            while True:
                k += 1
                oracle.update_state()
                oracle.create_stiffness()
                oracle.create_residual_forces()
                x = oracle.nodes()
                add_blocks_csr(off, idx, oracle.values(), contact.blocks(x, lam, curvature))
                oracle.forces()[:] += contact.forces(x, lam)
                oracle.apply_prescribed_bc(0.0)
                oracle.solve_slae(solver_type, solver_tolerance, solver_max_iter)
                tol = oracle.energy()
                tol_log.append(tol)
                oracle.update_nodes_with_solution()
                if not (abs(tol) > desired_tolerance and k < max_newton):
                    return k

        it = k = newton_pass()
        for _ in range(augment_max):
            if k == max_newton or contact.info(oracle.nodes(), lam)[1] <= gap_tolerance:
                break
            contact.augment(oracle.nodes(), lam)
            k = newton_pass()
            it += k
        its.append(it)
        if k == max_newton:
            break
    else:
        step = load_increments
    oracle.update_state()
    return its, np.array(tol_log), step


def reactions(oracle, contact, lam):
    """-(f - T + F_c) on the prescribed dofs, zero elsewhere (the unmasked residual at the nodes in force)."""
    oracle.update_state()
    oracle.create_residual_forces()
    f = oracle.forces().copy() + contact.forces(oracle.nodes(), lam)
    r = np.zeros_like(f)
    d = oracle.deck
    for a, t in zip(d.presc_node, d.presc_type):
        for j in range(3):
            if t & (1 << j):
                r[3 * a + j] = -f[3 * a + j]
    return r

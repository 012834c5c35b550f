"""Crisfield's cylindrical arc length on the surface loads, restated in numpy: the loop of feahip_solve_arclength
(include/fea_hip.h) with the oracle's K, T and prescribed-dof masking (oracle_binding.OracleSolver), the surface
forces of tests/test_surface_loads.py (reference_forces) and a dense direct solve.  Also the shallow-arch deck the
arc-length tests share, and plain load control on the same primitives (the oracle's own solve() knows no loads)."""
import math

import numpy as np

import feahip
import mesh
from oracle_binding import OracleSolver
from test_surface_loads import reference_forces


def arch_deck(nx=16, span=10.0, rise=1.0, thickness=0.25, width=1.0, load=0.08, **kw):
    """A shallow HEX8 arch strip: nx x 1 x 1 bricks along x, the midline a parabola of the given rise, every dof
    prescribed on both end faces, a dead traction (0, -load, 0) per unit load factor on the top faces of the two
    middle bricks.  Neo-Hookean, lambda = mu = 100.  Under load control it snaps through: with the defaults (found on
    the CPU: rise 0.5 over thickness 0.25 is too shallow to have a limit point, load 0.02 needs more than 40 steps to
    pass it) the load factor rises to 2.19 at step 5, falls to 1.97 at step 10 and rises from there."""
    nodes, el = mesh.hex_block(nx, 1, 1, origin=(0.0, 0.0, 0.0), size=(span, thickness, width))
    s = nodes[:, 0] / span
    nodes = nodes.copy()
    nodes[:, 1] += 4.0 * rise * s * (1.0 - s)
    ends = np.nonzero((nodes[:, 0] < 1e-9) | (nodes[:, 0] > span - 1e-9))[0].astype(np.int32)
    faces, owner, _ = mesh.boundary_faces(el)
    mid = np.nonzero((owner == nx // 2 - 1) | (owner == nx // 2))[0]
    # the top face of a brick: the one whose four nodes are the brick's upper (y) layer
    top = np.array([f for f in mid if _is_top(el[owner[f]], faces[f])], dtype=np.int64)
    kw.setdefault("load_increments_count", 1000)
    kw.setdefault("max_newton_count", 25)
    kw.setdefault("desired_tolerance", 1e-22)
    kw.setdefault("modified_newton", False)
    kw.setdefault("solver_type", feahip.CHOLESKY)
    kw.setdefault("solver_tolerance", 1e-15)
    return feahip.Deck(model=feahip.MODEL_COMPRESSIBLE_NEOHOOKEAN, parameters=[100.0, 100.0], ele_type=feahip.HEXAHEDRA8,
                       gauss_nodes_count=8, nodes=nodes, elements=el, presc_node=ends,
                       presc_type=np.full(len(ends), 7, np.int32), presc_values=np.zeros((len(ends), 3)),
                       surface_faces=np.ascontiguousarray(faces[top]), surface_kind=np.full(len(top), feahip.LOAD_TRACTION, np.int32),
                       surface_values=np.tile([0.0, -load, 0.0], (len(top), 1)), **kw)


def _is_top(elem, face):
    """hex_block's local axis s is y: the face made of the brick's local nodes 2, 3, 6, 7."""
    return set(int(a) for a in face) == set(int(elem[k]) for k in (2, 3, 6, 7))


def face_owners(deck):
    """The element every loaded face of the deck belongs to."""
    faces, owner, _ = mesh.boundary_faces(deck.elements)
    nc = 4 if deck.elements.shape[1] == 8 else 3
    table = {tuple(sorted(int(a) for a in f[:nc])): int(e) for f, e in zip(faces, owner)}
    npf = deck.surface_faces.shape[1]
    out = []
    for f in deck.surface_faces:
        corners = sorted(int(a) for a in f)
        if npf == 6:                                # the corners of a 6-node face: the three nodes of some boundary face
            corners = next(list(k) for k in table if set(k) <= set(corners))
        out.append(table[tuple(corners)])
    return np.array(out, dtype=np.int32)


def ordered_faces(deck):
    """The deck's loaded faces in their element's face order (the deck may list a face's nodes in any order)."""
    faces, _, _ = mesh.boundary_faces(deck.elements)
    by_set = {frozenset(int(a) for a in f): f for f in faces}
    return np.array([by_set[frozenset(int(a) for a in f)] for f in deck.surface_faces], dtype=np.int32)


class Restatement:
    """K (dense, prescribed dofs masked), R = lambda F - T and F at a configuration."""

    def __init__(self, deck):
        self.deck = deck
        self.o = OracleSolver(deck)
        self.faces, self.owner = ordered_faces(deck), face_owners(deck)
        self.mask = np.zeros(3 * len(deck.nodes), dtype=bool)
        for nd, ty in zip(deck.presc_node, deck.presc_type):
            for j in range(3):
                if ty & (1 << j):
                    self.mask[3 * nd + j] = True

    def external(self, x):
        d = self.deck
        F = reference_forces(d, x, self.faces, self.owner, d.surface_kind, d.surface_values, 1.0)
        F[self.mask] = 0.0
        return F

    def system(self, x, lam):
        """(K, R, F, bad): bad = Gauss points with a non-positive Jacobian."""
        o = self.o
        o.set_nodes(x)
        bad = o.update_state()
        o.create_stiffness()
        o.create_residual_forces()
        o.apply_prescribed_bc(0.0)
        n = o.ndof
        off, idx, val = o.offsets(), o.indexes(), o.values()
        K = np.zeros((n, n))
        rows = np.repeat(np.arange(n), np.diff(off))
        K[rows, idx] = val
        F = self.external(x)
        R = lam * F + o.forces()
        R[self.mask] = 0.0
        return K, R, F, bad

    def close(self):
        self.o.close()


def arclength(deck, lambda_max, max_steps, max_newton, desired_tolerance, x0=None):
    """The loop of feahip_solve_arclength.  Returns dict(lam=[...], its=[...], tol=[...], x=[x per step], dl=[dl per
    step], rc=0 or feahip.ENOTCONVERGED, resid=[|R_free| / (lambda |F|) at every converged point])."""
    rs = Restatement(deck)
    xn = (deck.nodes if x0 is None else x0).astype(float).copy()
    n = xn.size
    lam_n, dl = 0.0, 0.0
    Dprev = np.zeros(n)
    out = dict(lam=[], its=[], tol=[], x=[], dl=[], resid=[], rc=0)
    for step in range(max_steps):
        if lam_n >= lambda_max:
            break
        K, _, F, bad = rs.system(xn, lam_n)
        if bad:
            out["rc"] = feahip.ENOTCONVERGED
            break
        v = np.linalg.solve(K, F)
        vnorm = math.sqrt(v @ v)
        sgn = -1.0 if (step > 0 and Dprev @ v < 0.0) else 1.0
        if step == 0:
            dl = vnorm
        converged = False
        for cut in range(9):
            if cut > 0:
                dl *= 0.5
            Dlam = sgn * dl / vnorm
            Du = Dlam * v
            failed = False
            for it in range(1, max_newton + 1):
                K, R, F, bad = rs.system(xn + Du.reshape(-1, 3), lam_n + Dlam)
                if bad:
                    failed = True
                    break
                try:
                    sol = np.linalg.solve(K, np.stack([R, F], axis=1))
                except np.linalg.LinAlgError:
                    failed = True
                    break
                dR, dF = sol[:, 0], sol[:, 1]
                w = Du + dR
                qa, qb, qc = dF @ dF, 2.0 * (Du @ dF + dR @ dF), w @ w - dl * dl
                disc = qb * qb - 4.0 * qa * qc
                if not qa > 0.0 or not disc >= 0.0:
                    failed = True
                    break
                q = -0.5 * (qb + math.copysign(1.0, qb if qb != 0.0 else 1.0) * math.sqrt(disc))
                r1 = q / qa
                r2 = qc / q if q != 0.0 else r1
                fwd = Du @ w
                dlam = r1 if fwd + r1 * (Du @ dF) >= fwd + r2 * (Du @ dF) else r2
                tol = dR @ R + dlam * (dF @ R)
                out["tol"].append(tol)
                Du = Du + (dR + dlam * dF)
                Dlam += dlam
                if not tol == tol:
                    failed = True
                    break
                if abs(tol) <= desired_tolerance:
                    converged = True
                    break
            if converged:
                break
        if not converged:
            out["rc"] = feahip.ENOTCONVERGED
            break
        xn = xn + Du.reshape(-1, 3)
        lam_n += Dlam
        Dprev = Du
        _, R, F, _ = rs.system(xn, lam_n)
        out["lam"].append(lam_n); out["its"].append(it); out["x"].append(xn.copy()); out["dl"].append(dl)
        out["resid"].append(math.sqrt(R @ R) / (abs(lam_n) * math.sqrt(F @ F)))
    rs.close()
    out["lam"] = np.array(out["lam"]); out["its"] = np.array(out["its"], dtype=np.int32)
    return out


def load_control(deck, factors, max_newton, desired_tolerance):
    """Plain load control on the same primitives: full Newton at every factor, the energy test of the reference.
    Returns (steps done, [x per finished step]); stops at the first factor that does not converge."""
    rs = Restatement(deck)
    x = deck.nodes.astype(float).copy()
    xs = []
    for lam in factors:
        ok = False
        for _ in range(max_newton):
            K, R, _, bad = rs.system(x, lam)
            if bad:
                break
            try:
                u = np.linalg.solve(K, R)
            except np.linalg.LinAlgError:
                break
            tol = u @ R
            x = x + u.reshape(-1, 3)
            if not np.isfinite(tol) or np.abs(u).max() > 1e3:
                break
            if abs(tol) <= desired_tolerance:
                ok = True
                break
        if not ok:
            break
        xs.append(x.copy())
    rs.close()
    return len(xs), xs


def extrema(lam):
    """Indices i with lam[i] a strict interior local maximum or minimum of the log."""
    lam = np.asarray(lam)
    return [i for i in range(1, len(lam) - 1) if (lam[i] - lam[i - 1]) * (lam[i + 1] - lam[i]) < 0]

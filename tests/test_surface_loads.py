"""Surface loads on the MI355X: follower pressure and dead traction on boundary faces (kernels_surface.hip), checked
against an independent numpy statement of F_a = int N_a t da, inside the residual, through finite-strain and Lame
solutions, sharded, and from the command line."""
import math
import os
import subprocess

import numpy as np
import pytest

import feahip
import mesh
from test_oracle_closed_form import nh_closed_form

pytestmark = pytest.mark.gpu


# ---- numpy restatement ----------------------------------------------------------------------------------------------
def _shape(npf, xi, eta):
    """N[npf], dN/dxi[npf], dN/deta[npf] of the face on its parameter domain (triangle: xi, eta >= 0, xi + eta <= 1,
    corners then mid-sides (0,1) (1,2) (2,0); quad: [-1, 1]^2, corners counter-clockwise)."""
    if npf == 3:
        return np.array([1 - xi - eta, xi, eta]), np.array([-1.0, 1.0, 0.0]), np.array([-1.0, 0.0, 1.0])
    if npf == 6:
        L = np.array([1 - xi - eta, xi, eta])
        dL = np.array([[-1.0, 1.0, 0.0], [-1.0, 0.0, 1.0]])
        pairs = [(0, 1), (1, 2), (2, 0)]
        N = np.concatenate([L * (2 * L - 1), [4 * L[a] * L[b] for a, b in pairs]])
        dN = [np.concatenate([(4 * L - 1) * dL[k], [4 * (dL[k][a] * L[b] + L[a] * dL[k][b]) for a, b in pairs]])
              for k in range(2)]
        return N, dN[0], dN[1]
    sx, se = np.array([-1.0, 1.0, 1.0, -1.0]), np.array([-1.0, -1.0, 1.0, 1.0])
    return (0.25 * (1 + sx * xi) * (1 + se * eta), 0.25 * sx * (1 + se * eta), 0.25 * se * (1 + sx * xi))


def _rule(npf, kind):
    """(xi, eta, w).  'high': collapsed Gauss-Legendre 6 x 6 on the triangle, 5 x 5 Gauss on the quad -- more than
    exact for n da times N.  'kernel': the points the library integrates with (1 point; 6-point degree 4; 2 x 2)."""
    if kind == "high":
        g, w = np.polynomial.legendre.leggauss(6 if npf != 4 else 5)
        if npf == 4:
            return [(a, b, wa * wb) for a, wa in zip(g, w) for b, wb in zip(g, w)]
        u, wu = 0.5 * (g + 1), 0.5 * w
        return [(a, b * (1 - a), wa * wb * (1 - a)) for a, wa in zip(u, wu) for b, wb in zip(u, wu)]
    if npf == 3:
        return [(1 / 3, 1 / 3, 0.5)]
    if npf == 4:
        q = 1 / math.sqrt(3)
        return [(a, b, 1.0) for b in (-q, q) for a in (-q, q)]
    s10, r = math.sqrt(10.0), math.sqrt(38.0 - 44.0 * math.sqrt(0.4))
    d = math.sqrt(213125.0 - 53320.0 * s10)
    out = []
    for a, w in (((8 - s10 + r) / 18, (620 + d) / 3720), ((8 - s10 - r) / 18, (620 - d) / 3720)):
        out += [(a, a, 0.5 * w), (1 - 2 * a, a, 0.5 * w), (a, 1 - 2 * a, 0.5 * w)]
    return out


def _flip(npf):
    return {3: [0, 2, 1], 6: [0, 2, 1, 5, 4, 3], 4: [0, 3, 2, 1]}[npf]


def reference_forces(deck, x, faces, elems, kind, values, lam):
    """[3N]: faces oriented away from their element's centroid in the configuration they are integrated on."""
    F = np.zeros((len(x), 3))
    npf = faces.shape[1]
    for f in range(len(faces)):
        P = x if kind[f] == feahip.LOAD_PRESSURE else deck.nodes
        nd = faces[f]
        xa = P[nd]
        nrm = np.cross(xa[1] - xa[0], xa[2] - xa[0])
        if nrm @ (xa[:3].mean(axis=0) - P[deck.elements[elems[f]]].mean(axis=0)) < 0:
            nd = nd[_flip(npf)]
            xa = P[nd]
        for xi, eta, w in _rule(npf, "high" if kind[f] == feahip.LOAD_PRESSURE else "kernel"):
            N, dx, de = _shape(npf, xi, eta)
            n = np.cross(dx @ xa, de @ xa)
            t = -values[f][0] * n if kind[f] == feahip.LOAD_PRESSURE else values[f] * np.linalg.norm(n)
            F[nd] += w * np.outer(N, t)
    return lam * F.ravel()


def _decks():
    return {"tet4": mesh.bar_deck(dims=(2, 3, 2)),
            "tet10": mesh.bar_deck(dims=(2, 2, 2), quadratic=True),
            "hex8": mesh.bar_deck(dims=(2, 3, 2), hexa=True)}


def _shuffled(faces, seed=3):
    rng = np.random.default_rng(seed)
    return np.array([rng.permutation(f) for f in faces], dtype=np.int32)


@pytest.mark.parametrize("kind", ["tet4", "tet10", "hex8"])
def test_surface_forces_match_numpy_restatement(kind):
    deck = mesh.jitter_permute(_decks()[kind])                     # caller ids permuted, nodes off the lattice
    faces, elems, _ = mesh.boundary_faces(deck.elements)
    rng = np.random.default_rng(11)
    load_kind = (np.arange(len(faces)) % 2).astype(np.int32)       # pressure and dead traction alternate
    values = rng.normal(size=(len(faces), 3))
    s = feahip.FeaSolver(deck)
    s.set_surface_loads(_shuffled(faces), load_kind, values)
    s.set_load_factor(1.7)
    for x in (deck.nodes, mesh.deformed_state(deck.nodes, k1=1.08, wiggle=2e-2)):
        s.set_nodes(x)
        got = s.surface_forces()
        want = reference_forces(deck, x, faces, elems, load_kind, values, 1.7)
        assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max()
        assert np.array_equal(s.surface_forces(), got)              # no atomics: the same bits again
    s.close()


@pytest.mark.parametrize("kind", ["tet4", "tet10", "hex8"])
def test_pressure_resultants(kind):
    deck = _decks()[kind]
    s = feahip.FeaSolver(deck)
    p = 0.75
    top = mesh.block_side_faces(deck.nodes, deck.elements, 1, True)   # y = 7, area 1, outward +y
    s.set_surface_loads(_shuffled(top), np.zeros(len(top), np.int32), np.tile([p, 0, 0], (len(top), 1)))
    s.set_load_factor(1.0)
    tot = s.surface_forces().reshape(-1, 3).sum(axis=0)
    assert np.abs(tot - np.array([0.0, -p, 0.0])).max() < 1e-14
    # a pressure over the whole closed boundary of the deformed block: no resultant
    faces, _, _ = mesh.boundary_faces(deck.elements)
    s.set_surface_loads(faces, np.zeros(len(faces), np.int32), np.tile([p, 0, 0], (len(faces), 1)))
    s.set_nodes(mesh.deformed_state(deck.nodes, k1=1.1, wiggle=2e-2))
    F = s.surface_forces().reshape(-1, 3)
    assert np.abs(F.sum(axis=0)).max() < 1e-13 * np.abs(F).sum()
    s.close()


@pytest.mark.parametrize("kind", ["tet4", "tet10", "hex8"])
def test_residual_composition_and_clearing(kind):
    deck = mesh.jitter_permute(_decks()[kind])
    x = mesh.deformed_state(deck.nodes, k1=1.05)
    faces, _, _ = mesh.boundary_faces(deck.elements)
    load_kind = (np.arange(len(faces)) % 2).astype(np.int32)
    values = np.random.default_rng(5).normal(size=(len(faces), 3))
    plain = feahip.FeaSolver(deck)
    s = feahip.FeaSolver(deck)
    s.set_surface_loads(faces, load_kind, values)
    assert s.load_factor() == 0.0
    s.update_nodes_with_bc(1.0)
    plain.update_nodes_with_bc(1.0)
    assert s.load_factor() == 1.0                                   # one increment of the loads per step
    for o in (s, plain):
        o.set_nodes(x)
    plain.create_residual_forces()
    f0 = plain.forces()
    F1 = s.surface_forces()
    s.set_load_factor(2.5)
    s.create_residual_forces()
    f = s.forces()
    assert np.abs(f - (f0 + 2.5 * F1)).max() <= 1e-14 * np.abs(f0).max()
    s.create_stiffness_and_residual()
    assert np.abs(s.forces() - f).max() <= 1e-14 * np.abs(f0).max()  # with the stiffness (another volume kernel for TET4)
    assert s.time_kernel(5, 1, 3) > 0
    # cleared: K and f bitwise those of a context that never had loads
    s.set_surface_loads([], [], [])
    s.create_stiffness_and_residual()
    plain.create_stiffness_and_residual()
    assert np.array_equal(s.forces(), plain.forces())
    assert np.array_equal(s.matrix_yale()[2], plain.matrix_yale()[2])
    assert np.all(s.surface_forces() == 0)
    with pytest.raises(feahip.FeaHipError, match="no surface loads"):
        s.time_kernel(5, 1, 1)
    s.close(); plain.close()


def test_bad_faces_are_refused_with_the_face_named():
    deck = _decks()["tet4"]
    s = feahip.FeaSolver(deck)
    faces, _, _ = mesh.boundary_faces(deck.elements)
    table = mesh.element_faces(4)
    bset = {tuple(sorted(f)) for f in faces}
    interior = next(deck.elements[e][table[lf]] for e in range(len(deck.elements)) for lf in range(4)
                    if tuple(sorted(deck.elements[e][table[lf]])) not in bset)
    bad = np.vstack([faces[:3], interior[None, :]])
    with pytest.raises(feahip.FeaHipError, match="surface face 3 .*interior face"):
        s.set_surface_loads(bad, np.zeros(4, np.int32), np.ones((4, 3)))
    with pytest.raises(feahip.FeaHipError, match="has 3 nodes, not 4"):
        s.set_surface_loads(np.zeros((2, 4), np.int32), np.zeros(2, np.int32), np.ones((2, 3)))
    s.close()


# ---- finite strain: uniaxial bar, Neo-Hookean ------------------------------------------------------------------------
def _uniaxial_bar(kind, value, steps):
    nodes, el = mesh.kuhn_block(2, 4, 2, origin=(0.0, 0.0, 0.0), size=(1.0, 2.0, 1.0))
    eps = 1e-12
    types = (np.where(np.abs(nodes[:, 0]) < eps, 1, 0) | np.where(np.abs(nodes[:, 1]) < eps, 2, 0)
             | np.where(np.abs(nodes[:, 2]) < eps, 4, 0))
    sel = np.nonzero(types)[0].astype(np.int32)
    top = mesh.block_side_faces(nodes, el, 1, True)
    vals = np.tile([value, 0.0, 0.0] if kind == feahip.LOAD_PRESSURE else [0.0, value, 0.0], (len(top), 1))
    return feahip.Deck(model=feahip.MODEL_COMPRESSIBLE_NEOHOOKEAN, parameters=[100.0, 100.0], ele_type=feahip.TETRAHEDRA4,
                       gauss_nodes_count=1, nodes=nodes, elements=el, presc_node=sel, presc_type=types[sel].astype(np.int32),
                       presc_values=np.zeros((len(sel), 3)), surface_faces=_shuffled(top),
                       surface_kind=np.full(len(top), kind, np.int32), surface_values=vals, load_increments_count=steps,
                       max_newton_count=80, desired_tolerance=1e-24, modified_newton=False, solver_type=feahip.CG,
                       solver_tolerance=1e-15)


def _stretch_for(target):
    """k1 with target(k1) = 0, by bisection on [1, 2]."""
    lo, hi = 1.0, 2.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if target(mid) > 0:
            hi = mid
        else:
            lo = mid
    return 0.5 * (lo + hi)


def test_uniaxial_bar_under_follower_pressure_and_dead_traction():
    steps, per_step = 4, 10.0
    lam = float(steps)
    out = {}
    for kind in (feahip.LOAD_PRESSURE, feahip.LOAD_TRACTION):
        deck = _uniaxial_bar(kind, -per_step if kind == feahip.LOAD_PRESSURE else per_step, steps)
        s = feahip.FeaSolver(deck)
        done, its, _ = s.solve()
        assert done == steps
        assert s.load_factor() == lam
        X, x = deck.nodes, s.nodes()
        inside = X[:, 1] > 0
        k1 = x[inside, 1] / X[inside, 1]
        k2 = x[X[:, 0] > 0, 0] / X[X[:, 0] > 0, 0]
        assert np.ptp(k1) < 1e-10 and np.ptp(k2) < 1e-10             # homogeneous
        if kind == feahip.LOAD_PRESSURE:                              # Cauchy sigma_yy = -lambda p on the current face
            want = _stretch_for(lambda k: nh_closed_form(k)[1] - lam * per_step)
        else:                                                         # nominal: sigma_yy k2^2 = lambda t0
            want = _stretch_for(lambda k: nh_closed_form(k)[1] * nh_closed_form(k)[0] ** 2 - lam * per_step)
        assert abs(k1.mean() - want) < 1e-8, (kind, k1.mean(), want)
        assert abs(k2.mean() - nh_closed_form(want)[0]) < 1e-8
        out[kind] = k1.mean()
        s.close()
    # same nominal value, different loads: the dead traction's Cauchy stress grows as the face shrinks (k2 < 1)
    assert out[feahip.LOAD_TRACTION] - out[feahip.LOAD_PRESSURE] > 1e-2


# ---- Lame: quarter ring under internal pressure ----------------------------------------------------------------------
def _radial(deck, x):
    r = np.hypot(deck.nodes[:, 0], deck.nodes[:, 1])
    u = x - deck.nodes
    return r, (u[:, 0] * deck.nodes[:, 0] + u[:, 1] * deck.nodes[:, 1]) / r, u


def test_lame_quarter_ring_under_internal_pressure():
    """Small-strain plane strain, lambda = mu = 100: u(r) = a r + b / r with sigma_rr(1) = -p, sigma_rr(2) = 0, so
    a = p / 1200, b = p / 150: u(1) = 3p/400, u(1.5) = p (1.5/1200 + 8/1800), u(2) = p/200.  Quadratic tets, 4 cells
    per quarter as the oracle's ring; a reversed sign would push the ring inwards."""
    p = 0.01
    deck = mesh.lame_quarter_deck(2, 4, 1, p=p, load_increments_count=1, max_newton_count=30, desired_tolerance=1e-26,
                                  modified_newton=False)
    s = feahip.FeaSolver(deck)
    done, _, _ = s.solve()
    assert done == 1
    r, ur, u = _radial(deck, s.nodes())
    assert np.abs(u[:, 2]).max() < 2e-3 * p / 200                  # plane strain (mid-plane nodes drift by the mesh's asymmetry only)
    for radius, expect in ((1.0, 3 * p / 400), (1.5, p * (1.5 / 1200 + 8 / 1800)), (2.0, p / 200)):
        sel = np.abs(r - radius) < 1e-9
        assert sel.sum() >= 8
        assert np.abs(ur[sel] - expect).max() < 0.01 * expect, (radius, ur[sel].min(), ur[sel].max(), expect)
    s.close()


@pytest.mark.parametrize("rank_contexts", [False, True])
@pytest.mark.parametrize("n", [2, 3])
def test_sharded_pressure_ring_equals_one_context(n, rank_contexts):
    deck = mesh.lame_quarter_deck(3, 12, 8, zhi=2.0, p=1.0, load_increments_count=2, max_newton_count=30,
                                  desired_tolerance=1e-22, modified_newton=False)
    one = feahip.FeaSolver(deck)
    done, its, _ = one.solve()
    assert done == 2
    x1 = one.nodes()
    g = feahip.FeaGroup(deck, n, rank_contexts=rank_contexts)
    gd, gits, _ = g.solve(2, 30, False, 1e-22, feahip.CG, 1e-14, 20000)
    assert gd == 2
    xg = g.gather("nodes")
    assert np.abs(xg - x1).max() < 1e-10, np.abs(xg - x1).max()
    assert np.abs(x1 - deck.nodes).max() > 1e-3                      # the load did move the ring
    g.close(); one.close()


def test_command_line_solves_a_pressure_deck(tmp_path):
    deck = mesh.lame_quarter_deck(2, 4, 1, p=1.0, load_increments_count=2, max_newton_count=30, desired_tolerance=1e-20,
                                  modified_newton=False)
    path = tmp_path / "ring.sexp"
    deck.save(str(path))
    exe = os.path.join(os.path.dirname(feahip.LIB_PATH), "feasolver_hip")
    res = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    assert "Load increment 2 finished" in res.stdout
    s = feahip.FeaSolver(feahip.Deck.load(str(path)))
    done, _, _ = s.solve()
    assert done == 2
    u = s.nodes() - deck.nodes
    msh = (tmp_path / "ring.msh").read_text().splitlines()
    last = [i for i, l in enumerate(msh) if l == "$NodeData"][-1]
    rows = np.array([[float(v) for v in msh[last + 9 + a].split()] for a in range(len(deck.nodes))])
    assert np.array_equal(rows[:, 0], np.arange(1, len(deck.nodes) + 1))
    assert np.abs(rows[:, 1:4] - u).max() < 1e-6                    # %f in the file
    assert np.abs(u).max() > 1e-3
    s.close()

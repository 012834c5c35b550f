"""The numpy restatement of the contact term (tests/contact_reference.py) against itself and against closed forms, on
the CPU: finite differences, the weights, a frictionless platen on a uniaxial block, and the augmentation."""
import numpy as np
import pytest

import feahip
import mesh
import contact_reference as cr
from contact_cases import PLATEN_STEPS, PLATEN_TOLERANCE, platen_contact, platen_deck, sphere_contact, sphere_deck, SPHERE_STEPS
from oracle_binding import OracleSolver
from test_oracle_closed_form import nh_closed_form


def five_obstacles():
    """One obstacle of each kind around the unit cube [0, 1]^3."""
    return [cr.obstacle(cr.PLANE, (0.0, 0.9, 0.0), (0.1, -1.0, 0.2), travel=(0.0, -0.05, 0.0)),
            cr.obstacle(cr.SPHERE, (0.5, 1.3, 0.5), radius=0.5, travel=(0.0, -0.1, 0.0)),
            cr.obstacle(cr.SPHERE_INSIDE, (0.4, 0.5, 0.5), radius=0.8, travel=(0.05, 0.0, 0.0)),
            cr.obstacle(cr.CYLINDER, (-0.2, 0.5, 0.0), (0.1, 0.2, 1.0), radius=0.4, travel=(0.02, 0.0, 0.0)),
            cr.obstacle(cr.CYLINDER_INSIDE, (0.5, 0.0, 0.5), (0.05, 1.0, -0.1), radius=0.6)]


def _sampled_contact(seed):
    """A contact whose 'mesh' is a cloud of random points in the unit cube (each its own contact node, random weights,
    random multipliers), thinned to the nodes at least 1e-3 (in t / eps) from the switching surface t = 0 of every pair."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-0.1, 1.1, size=(60, 3))
    c = cr.Contact.__new__(cr.Contact)
    c.obstacles, c.eps = five_obstacles(), 37.0
    c.nodes, c.w = np.arange(len(x)), rng.uniform(0.5, 2.0, len(x))
    c.mu = rng.uniform(0.0, 3.0, size=(len(x), 5)) * (rng.uniform(size=(len(x), 5)) < 0.7)
    lam = 0.6
    keep = np.ones(len(x), dtype=bool)
    for i, o, g, n, rho, s, P, t in c.pairs(x, lam):
        if abs(c.mu[i, o] - c.eps * g) < 1e-3 * c.eps or rho < 0.05:
            keep[i] = False
    x = x[keep]
    c.nodes, c.w, c.mu = np.arange(len(x)), c.w[keep], c.mu[keep]
    return c, x, lam


@pytest.mark.parametrize("seed", [1, 2])
def test_blocks_and_forces_are_derivatives(seed):
    c, x, lam = _sampled_contact(seed)
    pairs = c.pairs(x, lam)
    for kind in range(5):                                         # every kind both pressing and separated
        ts = [t for i, o, g, n, rho, s, P, t in pairs if c.obstacles[o]["kind"] == kind]
        assert any(t > 0 for t in ts) and any(t == 0 for t in ts)
    h = 1e-6
    F = c.forces(x, lam).reshape(-1, 3)
    B = c.blocks(x, lam)
    fscale, kscale = np.abs(F).max(), max(np.abs(b).max() for b in B.values())
    for a in range(len(x)):
        Kfd, Ffd = np.zeros((3, 3)), np.zeros(3)
        for j in range(3):
            xp, xm = x.copy(), x.copy()
            xp[a, j] += h
            xm[a, j] -= h
            Kfd[:, j] = -(c.forces(xp, lam).reshape(-1, 3)[a] - c.forces(xm, lam).reshape(-1, 3)[a]) / (2 * h)
            Ffd[j] = -(c.potential(xp, lam) - c.potential(xm, lam)) / (2 * h)
        assert np.abs(Kfd - B.get(a, np.zeros((3, 3)))).max() <= 1e-6 * kscale
        assert np.abs(Ffd - F[a]).max() <= 1e-6 * fscale


def test_augmentation_is_the_pressure():
    c, x, lam = _sampled_contact(3)
    t = {(i, o): t for i, o, g, n, rho, s, P, t in c.pairs(x, lam)}
    c.augment(x, lam)
    assert all(c.mu[i, o] == v for (i, o), v in t.items()) and np.all(c.mu >= 0)


@pytest.mark.parametrize("kind", ["tet4", "tet10", "hex8"])
def test_weights_sum_to_the_area(kind):
    deck = {"tet4": mesh.bar_deck(dims=(2, 3, 2)), "tet10": mesh.bar_deck(dims=(2, 2, 2), quadratic=True),
            "hex8": mesh.bar_deck(dims=(2, 3, 2), hexa=True)}[kind]
    deck = mesh.jitter_permute(deck) if kind != "tet10" else deck     # (straight-sided 6-node faces)
    faces, _, _ = mesh.boundary_faces(deck.elements)
    area = 0.0
    for f in faces:
        fc = cr.canonical_face(deck.nodes, f)
        w, A = cr.face_weights(deck.nodes[fc])
        assert np.all(w > 0) and abs(w.sum() - A) <= 1e-14 * A
        area += A
    nodes, w = cr.contact_weights(deck.nodes, faces)
    assert abs(w.sum() - area) <= 1e-13 * area
    if kind != "tet10":
        return
    assert abs(area - 2 * (1 * 6 + 1 * 6 + 1 * 1)) <= 1e-12 * area    # the block of kuhn_block: 1 x 6 x 1
    X = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0.5, 0, 0], [0.5, 0.5, 0], [0, 0.5, 0]], dtype=float)
    w, A = cr.face_weights(X)
    assert np.allclose(w[:3] / A, 0.0526, atol=5e-5) and np.allclose(w[3:] / A, 0.2807, atol=5e-5)
    assert np.allclose(w[:3] / A, 3.0 / 57.0, rtol=1e-12) and np.allclose(w[3:] / A, 16.0 / 57.0, rtol=1e-12)


# ---- the platen: a frictionless plane pressing the top face of a uniaxial block ------------------------------------------
def run_platen(kind, penalty, augment_max=0, gap_tolerance=0.0, tolerance=1e-12):
    deck = platen_deck(kind)
    faces, c = platen_contact(deck, penalty)
    o = OracleSolver(deck)
    its, tol_log, done = cr.solve_static(o, c, PLATEN_STEPS, 30, tolerance, feahip.CG, augment_max, gap_tolerance)
    assert done == PLATEN_STEPS
    return deck, c, o, its, tol_log


@pytest.mark.parametrize("kind", ["tet4", "hex8"])
def test_platen_closed_form(kind):
    deck, c, o, its, _ = run_platen(kind, 1e4)
    x, lam = o.nodes(), float(PLATEN_STEPS)
    ymin, ymax = deck.nodes[:, 1].min(), deck.nodes[:, 1].max()
    top = c.nodes
    k1 = (x[top, 1].mean() - ymin) / (ymax - ymin)
    k2, syy = nh_closed_form(k1)
    A0 = (np.ptp(deck.nodes[:, 0])) * (np.ptp(deck.nodes[:, 2]))
    force = c.forces(x, lam).reshape(-1, 3).sum(axis=0)
    want = syy * A0 * k2 * k2                                     # compression: sigma_yy < 0, the platen pushes along -y
    assert abs(force[1] - want) <= 1e-9 * abs(want)
    assert abs(force[1] + c.info(x, lam)[2]) <= 1e-12 * abs(want) # the normal is -y everywhere: sum w t is the force
    pen = np.array([-g for i, oo, g, n, rho, s, P, t in c.pairs(x, lam)])
    assert np.ptp(pen) <= 1e-12 and pen.min() > 0


def test_platen_tet10_force_balance():
    deck, c, o, its, _ = run_platen("tet10", 1e4)
    lam = float(PLATEN_STEPS)
    F = c.forces(o.nodes(), lam).reshape(-1, 3).sum(axis=0)
    R = cr.reactions(o, c, lam).reshape(-1, 3).sum(axis=0)
    assert np.abs(F + R).max() <= 1e-9 * np.abs(F).max()


def test_augmentation_closes_the_gap():
    deck, c, o, its, _ = run_platen("tet4", 1e3, augment_max=4, gap_tolerance=1e-7)
    assert c.info(o.nodes(), float(PLATEN_STEPS))[1] <= 1e-7
    assert np.all(c.mu > 0)
    deck, c0, o0, its0, _ = run_platen("tet4", 1e3)
    assert c0.info(o0.nodes(), float(PLATEN_STEPS))[1] > 1e-3
    assert sum(its) > sum(its0)


# ---- the sphere on the clamped pad: the iteration counts the GPU test pins, and their margins ----------------------------
def test_sphere_iteration_counts_do_not_hang_on_a_borderline():
    """tests/test_gpu_contact.py asks the library for the restatement's Newton iterations per increment at the energy
    tolerance 1e-14: every increment's last logged tolerance lies at least 100 times below it and the one before at least
    100 times above (at 1e-12 the fourth increment's fourth iteration logs 1.1e-12: a coin toss)."""
    tol = 1e-14
    deck = sphere_deck()
    faces, c = sphere_contact(deck)
    o = OracleSolver(deck)
    its, tol_log, done = cr.solve_static(o, c, SPHERE_STEPS, 30, tol, feahip.CG)
    assert done == SPHERE_STEPS and its == [4, 4, 4, 5]
    k = 0
    for n in its:
        assert abs(tol_log[k + n - 1]) <= tol / 100 and abs(tol_log[k + n - 2]) >= 100 * tol
        k += n
    nocurv = cr.solve_static(OracleSolver(deck), sphere_contact(deck)[1], SPHERE_STEPS, 30, tol, feahip.CG, curvature=False)[0]
    assert all(a > b for a, b in zip(nocurv, its))                # why the curvature term is in: [5, 6, 7, 7] at 1e-12


@pytest.mark.parametrize("kind", ["tet4", "tet10", "hex8"])
def test_platen_iteration_counts_do_not_hang_on_a_borderline(kind):
    """The same margins for the platen decks at PLATEN_TOLERANCE (eps = 1e4, no augmentation): three iterations an
    increment on every deck, the last logged tolerance 100 times below, the one before 100 times above."""
    deck, c, o, its, tol_log = run_platen(kind, 1e4, tolerance=PLATEN_TOLERANCE)
    assert its == [3, 3, 3]
    k = 0
    for n in its:
        assert abs(tol_log[k + n - 1]) <= PLATEN_TOLERANCE / 100 and abs(tol_log[k + n - 2]) >= 100 * PLATEN_TOLERANCE
        k += n

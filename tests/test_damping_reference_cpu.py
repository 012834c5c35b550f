"""The restatement the GPU damping tests compare against (tests/damping_reference.py), checked on its own: C
diagonalises on a mode and the Newmark loop carries it, the damped central differences relax to the static solution
and keep the undamped stability limit, and no Newton count of the shared release cases hangs on a borderline
comparison.  No GPU."""
import numpy as np
import pytest

from damping_reference import COEFFICIENTS, DampedDynamics, DampedExplicit, damped_release, oscillator_newmark
from dynamics_reference import loaded_bar
from explicit_reference import omega_max

MODAL_TOL = 1e-7      # of the initial amplitude at eps = 1e-6: a factor 60 over the worst deviation measured (1.6e-9, hex8)
RELAX_TOL = 1e-12     # of max|x - x0| after 1250 steps (measured 5.4e-15; 5.5e-13 after 1000)


def first_mode(r):
    """(omega, phi) of the lowest mode of (K(X0), M) on the free dofs, phi M-orthonormal and zero on the prescribed ones."""
    free = ~r.mask
    K = r.h.assemble(r.x)[0][np.ix_(free, free)]
    M = r.M[np.ix_(free, free)]
    L = np.linalg.cholesky(M)
    A = np.linalg.solve(L, np.linalg.solve(L, 0.5 * (K + K.T)).T)
    lam, Y = np.linalg.eigh(0.5 * (A + A.T))
    phi = np.zeros(len(r.mask))
    phi[free] = np.linalg.solve(L.T, Y[:, 0])
    return float(np.sqrt(lam[0])), phi


@pytest.mark.parametrize("kind,dims", [("tet4", (2, 4, 2)), ("hex8", (2, 4, 2)), ("tet10", (1, 2, 1))])
def test_a_mode_decays_like_its_oscillator(kind, dims):
    deck = loaded_bar(kind, dims)
    r = DampedDynamics(deck, 1.5)                               # load factor 0: the traction is there and not applied
    omega, phi = first_mode(r)
    assert abs(phi @ r.M @ phi - 1.0) <= 1e-12
    eps = 1e-6
    alpha, beta_k = 0.04 * omega, 0.1 / omega
    r.set_damping(alpha, beta_k)                                # K_d = K(X0)
    X0 = r.x.copy()
    r.x = X0 + eps * phi.reshape(-1, 3)
    r.consistent_acceleration()
    dt = 2.0 * np.pi / omega / 20.0
    done, its, traj = r.newmark(40, dt, 0.25, 0.5, 0.0, deck.max_newton_count, deck.desired_tolerance)
    r.close()
    assert done == 40
    q = np.array([phi @ r.M @ (x - X0).ravel() / eps for x, _, _ in traj])
    want = oscillator_newmark(1.0, alpha + beta_k * omega ** 2, omega ** 2, 1.0, 0.0, 40, dt)
    dev = np.abs(q - want).max()
    print(kind, "omega", omega, "zeta", 0.5 * (alpha / omega + beta_k * omega), "Newton", sorted(set(its)), "deviation", dev,
          "amplitude after 2 periods", q[-1])
    assert 0.3 < q[-1] < 0.5                                    # exp(-0.07 * 4 pi) = 0.41: it did decay
    assert dev <= MODAL_TOL


def test_dynamic_relaxation_reaches_the_static_solution():
    deck = loaded_bar("tet4", (2, 4, 2))
    s = DampedDynamics(deck, 1.5)
    done, _ = s.static(1, deck.max_newton_count, deck.desired_tolerance)
    want = s.x.copy()
    s.close()
    assert done == 1
    r = DampedExplicit(deck, 1.5)
    K = r.tangent()
    free = ~r.mask
    s3 = 1.0 / np.sqrt(r.ml3[free])
    omega1 = float(np.sqrt(np.linalg.eigvalsh(K[np.ix_(free, free)] * s3[:, None] * s3[None, :]).min()))
    assert omega1 < omega_max(K, r.ml)
    r.set_damping(2.0 * omega1)
    dt = 0.5 * r.stable_step()
    r.lam = 1.0                                                 # the traction at once
    r.explicit(1250, dt, keep=False)
    r.close()
    scale = np.abs(want - deck.nodes).max()
    err = np.abs(r.x - want).max() / scale
    print("relaxation: omega_1", omega1, "dt", dt, "error after 1250 steps", err, "max|v|", np.abs(r.v).max())
    assert err <= RELAX_TOL


def test_the_damped_scheme_keeps_the_undamped_stability_limit():
    """One oscillator, u'' + alpha u' + omega^2 u = 0, in the loop of DampedExplicit at 0.99 of 2 / omega with
    alpha = omega: bounded over 10 000 steps (the undamped limit holds for every mass-proportional C >= 0)."""
    omega = 3.0
    alpha, h = omega, 0.99 * 2.0 / omega
    u, v = 1.0, 0.0
    a = -omega * omega * u - alpha * v
    most = 0.0
    for _ in range(10000):
        vh = v + 0.5 * h * a
        u = u + h * vh
        a = (-omega * omega * u - alpha * vh) / (1.0 + 0.5 * alpha * h)
        v = vh + 0.5 * h * a
        most = max(most, abs(u))
    print("largest |u|", most, "last", u)
    assert most <= 1.0 and abs(u) <= 1e-6


@pytest.mark.parametrize("key", list(COEFFICIENTS))
@pytest.mark.parametrize("name", ["tet4_a5", "tet10", "hex8", "tet4_table", "end_motion", "tet4"])
def test_no_newton_count_of_the_release_cases_is_borderline(name, key):
    """Every |<u, R>| of the restatement is a factor 100 away from the tolerance, on either side: a rounding-level
    difference on the GPU cannot change a Newton count.  The A5 case converges linearly (its tangent is not exact: the
    energies fall by 40 to 300 per iteration), so no tolerance is 100 away from two neighbours; there the factor is the
    2.5 that NEWTON_TOL_A5 reaches, against a difference of a few 1e-5 between the GPU's energies and these
    (tests/damping_reference.py)."""
    done, its, traj, energies, tol = damped_release(name, key)
    assert done == len(traj) == (3 if name == "end_motion" else 4) and len(energies) == sum(its)
    factor = 2.5 if name == "tet4_a5" else 100.0
    margin = min(max(e / tol, tol / e) for e in energies)
    print(name, key, "Newton counts", its, "tolerance", tol, "closest energy: a factor", margin)
    assert margin >= factor

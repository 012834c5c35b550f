"""Rayleigh damping restated in float64 numpy: C = alpha M + beta_k K_d dense, with K_d the plain tangent of
tests/hetero_reference.py at the x of set_damping and M the mass of the loop that runs -- the consistent mass in the
damped Newmark loop and the damped consistent acceleration, the HRZ-lumped mass in the damped central-difference loop.
Nothing here calls the library under test."""
import numpy as np

from dynamics_reference import DynamicsRestatement
from explicit_reference import ExplicitRestatement


def rayleigh(omega1, zeta1, omega2, zeta2):
    """(alpha, beta_k) with zeta_i = (alpha / omega_i + beta_k omega_i) / 2, from the 2 x 2 system itself."""
    A = 0.5 * np.array([[1.0 / omega1, omega1], [1.0 / omega2, omega2]])
    a, b = np.linalg.solve(A, np.array([zeta1, zeta2]))
    return float(a), float(b)


def oscillator_newmark(m, c, k, u0, v0, n_steps, dt, beta=0.25, gamma=0.5):
    """u after every Newmark step of m u'' + c u' + k u = 0 from (u0, v0), with a(0) from the equation."""
    u, v = float(u0), float(v0)
    a = -(c * v + k * u) / m
    a0, c1 = 1.0 / (beta * dt * dt), gamma / (beta * dt)
    out = []
    for _ in range(n_steps):
        ut = u + dt * v + dt * dt * (0.5 - beta) * a
        vt = v + dt * (1.0 - gamma) * a
        # m a0 (u - ut) + c (vt + c1 (u - ut)) + k u = 0
        u = ((m * a0 + c * c1) * ut - c * vt) / (m * a0 + c * c1 + k)
        a = a0 * (u - ut)
        v = vt + gamma * dt * a
        out.append(u)
    return np.array(out)


class DampedDynamics(DynamicsRestatement):
    """DynamicsRestatement with C = alpha M + beta_k K_d in the Newmark loop and the consistent acceleration."""

    alpha = beta_k = 0.0
    C = None

    def set_damping(self, alpha, beta_k, x=None):
        self.alpha, self.beta_k = float(alpha), float(beta_k)
        self.Kd = self.h.assemble(self.x if x is None else x)[0].copy() if beta_k > 0 else np.zeros_like(self.M)
        self.C = self.alpha * self.M + self.beta_k * self.Kd

    def consistent_acceleration(self):
        _, R = self.residual_and_stiffness(self.x)
        if self.C is not None:
            R = R - self.C @ self.v.ravel()
        Mm, Rm = self.h.masked(self.M, R)
        self.a = self.solve_dense(Mm, Rm).reshape(-1, 3)

    def newmark(self, n_steps, dt, beta, gamma, dlambda, max_newton, tol, energies=None):
        """(steps done, Newton iterations per step, [(x, v, a) after every completed step]); energies: a list that takes
        |<u, R>| of every iteration."""
        if self.C is None:
            self.set_damping(0.0, 0.0)
        a0, c1 = 1.0 / (beta * dt * dt), gamma / (beta * dt)
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
                d = (x - xt).ravel()
                w = vt.ravel() + c1 * d
                R = R - a0 * (self.M @ d) - self.C @ w
                K, R = self.h.masked(K + a0 * self.M + c1 * self.C, R)
                u = self.solve_dense(K, R)
                e = float(R @ u)
                if energies is not None:
                    energies.append(abs(e))
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


class DampedExplicit(ExplicitRestatement):
    """ExplicitRestatement with C = alpha M_L: M_L a = f - alpha M_L v with the end-of-step v = vh + h/2 a."""

    alpha = 0.0

    def set_damping(self, alpha, beta_k=0.0):
        assert beta_k == 0.0, "the explicit loop takes mass-proportional damping only"
        self.alpha = float(alpha)

    def explicit(self, n_steps, dt, dlambda=0.0, keep=True):
        """[(x, v, a) after every step] at the fixed step dt (keep=False: nothing is kept, for long runs)."""
        traj = []
        m, cv, h, al = self.mask, self.cval, dt, self.alpha
        for step in range(n_steps):
            vh = (self.v + 0.5 * h * self.a).ravel()
            vh[m] = 0.0
            x = (self.x.ravel() + h * vh + dlambda * cv).reshape(-1, 3)
            self.lam += dlambda
            R = self.residual(x)
            a = (R / self.ml3 - al * vh) / (1.0 + 0.5 * al * h)
            a[m] = 0.0
            vh[m] = dlambda * cv[m] / h
            self.x, self.a = x, a.reshape(-1, 3)
            self.v = (vh + 0.5 * h * a).reshape(-1, 3)
            self.t += h
            if keep:
                traj.append((self.x.copy(), self.v.copy(), self.a.copy()))
        return traj


# ---- the damped release cases the GPU trajectory tests and their CPU guard share -------------------------------------
COEFFICIENTS = {"alpha": (0.5, 0.0), "beta": (0.0, 0.01), "both": (0.5, 0.01)}
# The Newton tolerance on |<u, R>| of the release cases, chosen so that no count hangs on a borderline comparison.  On the
# neo-Hookean cases Newton converges quadratically: under the three coefficient pairs the third iteration's energy lies in
# [1.5e-18, 5.8e-12] and the fourth's is rounding (<= 4e-25), so 1e-21 is a factor 1000 from both.  The A5 tangent is not
# exact and its energies fall by 40 to 300 per iteration, linearly: no tolerance is a factor 100 from two neighbours.  There
# 1.6e-14 is the best choice, a factor >= 2.5 from every energy.  That is enough: at an energy of 1e-14 the iterate is
# sqrt(1e-14 / K) ~ 1e-8 from the solution, the GPU's x differs from the restatement's by the 1.5e-13 of the perturbation
# experiment, so the energies of the two differ by a few 1e-5 of themselves.
NEWTON_TOL = 1e-21
NEWTON_TOL_A5 = 1.6e-14
_RELEASES = {}


def release_deck(name):
    """(deck, rho) of the release case `name` of tests/test_gpu_dynamics.py, with the Newton tolerance above."""
    from hetero_reference import MATERIALS, scattered_ids, with_materials
    from dynamics_reference import DENSITIES, loaded_bar
    from test_gpu_dynamics import CASES
    deck = loaded_bar(**CASES[name], desired_tolerance=NEWTON_TOL_A5 if name == "tet4_a5" else NEWTON_TOL)
    if name == "tet4_table":
        deck = with_materials(deck, MATERIALS, scattered_ids(deck))
    return deck, (DENSITIES if name == "tet4_table" else 1.5)


def damped_release(name, key):
    """(steps done, Newton counts, trajectory, |<u, R>| of every iteration, tolerance) of the release case `name` under
    COEFFICIENTS[key], K_d taken at the reference configuration -- computed once, shared, never written to."""
    if (name, key) not in _RELEASES:
        from test_gpu_dynamics import DT
        deck, rho = release_deck(name)
        r = DampedDynamics(deck, rho)
        r.set_damping(*COEFFICIENTS[key])
        energies = []
        if name == "end_motion":
            out = r.newmark(3, DT, 0.25, 0.5, 1.0, deck.max_newton_count, deck.desired_tolerance, energies)
        else:
            r.lam = 1.0
            out = r.newmark(4, DT, 0.25, 0.5, 0.0, deck.max_newton_count, deck.desired_tolerance, energies)
        r.close()
        for st in out[2]:
            for arr in st:
                arr.setflags(write=False)
        _RELEASES[(name, key)] = (*out, energies, deck.desired_tolerance)
    return _RELEASES[(name, key)]

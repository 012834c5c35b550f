"""Arc-length continuation on the MI355X (feahip_solve_arclength) against its numpy restatement
(tests/arclength_reference.py): the uniaxial bar, the snap-through of a shallow arch, equilibrium and the arc-length
constraint at logged points, follower pressure against load control, the error returns and the command line."""
import os
import re
import subprocess

import numpy as np
import pytest

import feahip
import mesh
import arclength_reference as ar
from test_arclength_reference_cpu import bar_deck

pytestmark = pytest.mark.gpu

U_TOL = 1e-10            # tests/test_gpu_fullpath.py: displacements within 1e-10 relative
ARCH_STEPS = 16          # past the maximum (step 5) and the minimum (step 10) of the load factor


def rel(a, b):
    s = np.abs(b).max()
    return np.abs(a - b).max() / (s if s > 0 else 1.0)


@pytest.fixture(scope="module")
def arch():
    deck = ar.arch_deck()
    return deck, ar.arclength(deck, 1e9, ARCH_STEPS, deck.max_newton_count, deck.desired_tolerance)


def test_bar_follows_the_restatement():
    deck = bar_deck()
    want = ar.arclength(deck, 4.0, 12, deck.max_newton_count, deck.desired_tolerance)
    s = feahip.FeaSolver(deck)
    n, lam, its, _, rc = s.solve_arclength(4.0, 12)
    assert rc == 0 and n == len(want["lam"])
    assert np.array_equal(its, want["its"])
    assert rel(lam, want["lam"]) < U_TOL
    assert rel(s.nodes() - deck.nodes, want["x"][-1] - deck.nodes) < U_TOL
    assert s.load_factor() == lam[-1]
    s.close()


def test_arch_passes_its_limit_points(arch):
    deck, want = arch
    s = feahip.FeaSolver(deck)
    n, lam, its, _, rc = s.solve_arclength(1e9, ARCH_STEPS, solver_type=feahip.CHOLESKY)
    assert rc == 0 and n == ARCH_STEPS
    ext = ar.extrema(lam)
    assert len(ext) == 2 and ext == ar.extrema(want["lam"])               # non-monotone, the extrema on the same steps
    assert np.array_equal(its, want["its"])
    assert rel(lam, want["lam"]) < U_TOL
    assert rel(s.nodes() - deck.nodes, want["x"][-1] - deck.nodes) < U_TOL
    s.close()


def test_arch_equilibrium_and_constraint(arch):
    deck, want = arch
    xs, lams = [], []
    for steps in (1, 2, 7, ARCH_STEPS):                                    # rising, falling and rising again
        s = feahip.FeaSolver(deck)
        n, lam, _, _, _ = s.solve_arclength(1e9, steps, solver_type=feahip.CHOLESKY)
        assert n == steps
        xs.append(s.nodes()); lams.append(lam[-1])
        # equilibrium: the residual over the free dofs at the logged point, relative to lambda |F|
        s.create_residual_forces()
        R = s.forces()
        s.set_load_factor(1.0)
        F = s.surface_forces()
        free = np.ones(s.ndof, dtype=bool)
        for nd, ty in zip(deck.presc_node, deck.presc_type):
            for j in range(3):
                if ty & (1 << j):
                    free[3 * nd + j] = False
        got = np.linalg.norm(R[free]) / (abs(lam[-1]) * np.linalg.norm(F[free]))
        print(f"step {steps}: |R|/(lambda |F|) = {got:.3e}, restatement {want['resid'][steps - 1]:.3e}")
        assert got <= 10.0 * want["resid"][steps - 1]
        s.close()
    # the constraint |Du| = dl: no cut on this path, so the second step has the first one's length
    dl = np.linalg.norm(xs[0] - deck.nodes)
    assert abs(np.linalg.norm(xs[1] - xs[0]) / dl - 1.0) <= 1e-12
    assert abs(dl / want["dl"][0] - 1.0) < U_TOL


def test_follower_pressure_agrees_with_load_control():
    deck = mesh.lame_quarter_deck(2, 4, 1, p=1.0, load_increments_count=3, max_newton_count=30, desired_tolerance=1e-22,
                                  modified_newton=False)
    s = feahip.FeaSolver(deck)
    n, lam, _, _, rc = s.solve_arclength(1e9, 3, solver_tolerance=1e-15)
    assert rc == 0 and n == 3 and np.all(np.diff(lam) > 0)
    xa = s.nodes()
    s.close()
    # load control to the last logged factor: Newton at every logged factor through set_load_factor
    c = feahip.FeaSolver(deck)
    for l in lam:
        c.set_load_factor(float(l))
        for _ in range(30):
            c.create_stiffness_and_residual()
            c.apply_prescribed_bc(0.0)
            c.solve_slae(feahip.CG, 1e-15, 20000)
            tol = c.energy()
            c.update_nodes_with_solution()
            if abs(tol) <= 1e-22:
                break
    assert rel(xa - deck.nodes, c.nodes() - deck.nodes) < U_TOL
    assert np.abs(xa - deck.nodes).max() > 1e-3
    c.close()


def test_errors(arch):
    deck, _ = arch
    plain = feahip.FeaSolver(mesh.bar_deck(dims=(2, 3, 2)))
    with pytest.raises(feahip.FeaHipError, match=f"error {feahip.ESTATE}.*no surface loads"):
        plain.solve_arclength(1.0, 2)
    plain.close()
    s = feahip.FeaSolver(deck)
    n, lam, _, _, rc = s.solve_arclength(1e9, 4, max_newton=1, check=False)   # one corrector iteration never converges
    assert rc == feahip.ENOTCONVERGED and n == 0 and len(lam) == 0
    assert np.array_equal(s.nodes(), deck.nodes) and s.load_factor() == 0.0  # back at the last converged point
    s.close()


def test_command_line_follows_the_arch(arch, tmp_path):
    deck, want = arch
    exe = os.path.join(os.path.dirname(feahip.LIB_PATH), "feasolver_hip")
    d = ar.arch_deck(load_increments_count=1000)
    d.arclength_max = 8
    path = tmp_path / "arch.sexp"
    d.save(str(path))
    res = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    lam = np.array([float(m) for m in re.findall(r"Arc-length step \d+ finished: load factor (\S+),", res.stdout)])
    assert len(lam) == 8 and rel(lam, want["lam"][:8]) < U_TOL
    assert os.path.exists(tmp_path / "arch.msh")
    # the same deck with :max 0 takes the load-control path
    d.arclength_max = 0
    d.load_increments_count = 2
    d.save(str(path))
    res = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    assert "Arc-length" not in res.stdout and "Load increment 2 finished" in res.stdout

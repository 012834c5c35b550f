"""Explicit dynamics on the GPU against tests/explicit_reference.py: the HRZ-lumped mass, the Gershgorin stable step,
the central-difference steps of feahip_solve_explicit on one context, on row shards and on rank contexts, the adaptive
step, the interchange with Newmark, the refusals, the inversion report and the command line.

Bound of the trajectories: x within 5.6e-10 of max|x - x0|, v of max|v|, a of max|a| -- ten times the spread of the
experiment of DESIGN.md section 12.  The project holds f to 1e-12 of its scale and no linear solve amplifies it; the
restatement's residual perturbed at 1e-12 of max|f| in every step (three seeds) moves x, v or a by 2.1e-11 to 5.6e-11
over the 20 steps of the seven cases below (hex8 the largest; section 13 has the table): a = f / ml divides by nodal
masses that differ by a factor of ten to thirty between a corner and an interior node, so 1e-12 of max|f| is a few
1e-11 of max|a|."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import feahip
from dynamics_reference import DENSITIES, free_block, loaded_bar
from explicit_reference import ExplicitRestatement, gershgorin_bound, hrz_lumped_mass, hub_fan, omega_max
from hetero_reference import MATERIALS, scattered_ids, with_materials

pytestmark = pytest.mark.gpu

ML_TOL = 1e-13       # relative, per node: sums of a few positive terms
DT_TOL = 1e-12       # relative: row sums of |K| at K's parity with the oracle (1e-12 of scale)
X_TOL = 5.6e-10      # ten times the largest spread: see the module docstring
SHARD_TOL = 1e-12    # sharded against unsharded, of max|x - x0|
FREE_TOL = 1e-11     # as tests/test_gpu_dynamics.py::test_free_flight
DIMS = (2, 4, 2)
BIG = (4, 12, 4)     # 325 nodes: several chunks of the gather kernel, and rows for every rank of two shards or three rank contexts
V0 = np.array([1.0, -2.0, 0.5])
GRAVITY = np.array([0.3, -9.81, 1.1])
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dynamics", "explicit_bar.sexp")


def rel(a, b, scale=None):
    s = np.abs(b).max() if scale is None else scale
    return np.abs(np.asarray(a) - np.asarray(b)).max() / (s if s > 0 else 1.0)


def case_deck(name):
    """(deck, density, body force, load factor at the start, dlambda, steps)"""
    if name in ("tet4", "tet10", "hex8"):
        return loaded_bar(name, DIMS), 1.5, None, 0.0, 0.05, 20          # a traction ramped up over the run
    if name == "big":
        return loaded_bar("tet4", BIG), 1.5, None, 0.0, 0.05, 20
    if name == "table":
        d = loaded_bar("tet4", DIMS)
        return with_materials(d, MATERIALS, scattered_ids(d)), DENSITIES, None, 0.0, 0.05, 20
    if name == "end_motion":
        return loaded_bar("tet4", DIMS, end_motion=0.002), 1.5, None, 0.0, 1.0, 20
    if name == "gravity":
        return free_block("tet4", DIMS), 1.5, GRAVITY, 1.0, 0.0, 20
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(dt = 0.5 dt_G at the reference state, trajectory, kinetic energy at the end) of the restatement -- computed once,
    shared, never written to."""
    deck, rho, body, lam, dlam, steps = case_deck(name)
    r = ExplicitRestatement(deck, rho, body)
    r.lam = lam
    dt = 0.5 * r.stable_step()
    traj, _ = r.explicit(steps, dt, dlambda=dlam)
    ke = r.kinetic_energy()
    r.close()
    for st in traj:
        for arr in st:
            arr.setflags(write=False)
    return dt, traj, ke


def make_solver(name, cls=feahip.FeaSolver, *args, **kw):
    deck, rho, body, lam, dlam, steps = case_deck(name)
    s = cls(deck, *args, **kw)
    s.set_mass(rho)
    if body is not None:
        s.set_body_force(body)
    if isinstance(s, feahip.FeaGroup):
        s.each("set_load_factor", lam)
    else:
        s.set_load_factor(lam)
    return s, deck, dlam, steps


def check_state(tag, got, want, x0, rows=None, tol=X_TOL):
    rows = slice(None) if rows is None else rows
    (x, v, a), (xw, vw, aw) = got, want
    ex = rel(x[rows], xw[rows], np.abs(xw - x0).max())
    ev, ea = rel(v[rows], vw[rows], np.abs(vw).max()), rel(a[rows], aw[rows], np.abs(aw).max())
    print(tag, "x", ex, "v", ev, "a", ea)
    assert ex <= tol and ev <= tol and ea <= tol


# ---- lumped mass ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("table", [False, True])
@pytest.mark.parametrize("kind", ["tet4", "tet10", "hex8"])
def test_lumped_mass_matches_the_restatement(kind, table):
    deck = loaded_bar(kind, DIMS)
    ids = scattered_ids(deck)
    if table:
        deck = with_materials(deck, MATERIALS, ids)
    rho = DENSITIES if table else 2.5
    want = hrz_lumped_mass(deck, rho, ids)
    s = feahip.FeaSolver(deck)
    s.set_mass(rho)
    ml = s.lumped_mass()
    print(kind, table, "lumped mass", np.abs(ml / want - 1.0).max())
    assert np.abs(ml / want - 1.0).max() <= ML_TOL
    assert np.array_equal(s.lumped_mass(), ml)
    s.set_mass(rho)                                                    # built again: the same bits
    assert np.array_equal(s.lumped_mass(), ml)
    s.close()


@pytest.mark.parametrize("form", ["shards2", "ranks3"])
def test_lumped_mass_on_shards(form):
    deck = loaded_bar("tet4", BIG)
    ids = scattered_ids(deck)
    deck = with_materials(deck, MATERIALS, ids)
    want = hrz_lumped_mass(deck, DENSITIES, ids)
    g = feahip.FeaGroup(deck, 2) if form == "shards2" else feahip.FeaGroup(deck, 3, rank_contexts=True)
    g.set_mass(DENSITIES)
    for rk, nd in zip(g.ranks, g.nodes):                               # authoritative on owned rows, zero elsewhere
        ml = rk.lumped_mass()
        own = ml[:rk.n_own] if g.rank_contexts else ml[nd]
        other = ml[rk.n_own:] if g.rank_contexts else np.delete(ml, nd)
        assert np.abs(own / want[nd] - 1.0).max() <= ML_TOL and (len(other) == 0 or np.abs(other).max() == 0.0)
    ml = g.lumped_mass()
    assert np.abs(ml / want - 1.0).max() <= ML_TOL and np.array_equal(g.lumped_mass(), ml)
    g.close()


# ---- stable step ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def step_reference(name):
    """(Gershgorin step, dense 2 / omega_max) of the restatement at the reference state"""
    deck = hub_fan() if name == "hub" else (free_block(name[5:], DIMS) if name.startswith("free_") else loaded_bar(name, BIG if name == "tet4" else DIMS))
    r = ExplicitRestatement(deck, 1.5)
    K = r.tangent()
    dt_g, dt_dense = 2.0 / np.sqrt(gershgorin_bound(K, r.ml)), 2.0 / omega_max(K, r.ml)
    r.close()
    return deck, dt_g, dt_dense


@pytest.mark.parametrize("name", ["tet4", "tet10", "hex8", "free_tet4", "free_tet10", "free_hex8", "hub"])
def test_stable_step_matches_the_restatement(name):
    deck, dt_g, dt_dense = step_reference(name)
    s = feahip.FeaSolver(deck)
    s.set_mass(1.5)
    dt = s.stable_step()
    print(name, "stable step", dt, "restatement", dt_g, rel(dt, dt_g), "dense limit", dt_dense, "tightness", dt / dt_dense)
    assert rel(dt, dt_g) <= DT_TOL and dt <= dt_dense
    assert s.stable_step() == dt
    s.close()
    if name == "tet4":                                                 # the max all-reduce of the in-process group
        for g in (feahip.FeaGroup(deck, 2), feahip.FeaGroup(deck, 3, rank_contexts=True)):
            g.set_mass(1.5)
            assert g.stable_step() == dt
            g.close()


# ---- trajectories ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tet4", "tet10", "hex8", "big", "table", "end_motion", "gravity"])
def test_trajectory_matches_the_restatement(name):
    """20 steps at 0.5 dt_G with a fixed dt, every state compared: a traction ramped by dlambda, a prescribed end
    motion (v and a at the prescribed nodes included), gravity on the free block."""
    dt, traj, ke = reference(name)
    s, deck, dlam, steps = make_solver(name)
    for k in range(steps):
        done, log = s.solve_explicit(1, dt, dlambda=dlam)
        assert done == 1 and list(log) == [dt]
        check_state(f"{name} step {k + 1}", (s.nodes(), s.velocities(), s.accelerations()), traj[k], deck.nodes)
    assert abs(s.time() - steps * dt) <= 1e-12 * steps * dt
    e = s.kinetic_energy()
    print(name, "kinetic energy", e, ke)
    assert abs(e - ke) <= 1e-10 * ke
    s.set_velocities(s.velocities())                                   # the partial sums of the step are dropped: the same sum again
    assert abs(s.kinetic_energy() - e) <= 1e-14 * e
    s.close()


@pytest.mark.parametrize("form", ["shards2", "ranks3"])
def test_sharded_trajectory_is_the_unsharded_one(form):
    dt, traj, ke = reference("big")
    one, deck, dlam, steps = make_solver("big")
    done, _ = one.solve_explicit(steps, dt, dlambda=dlam)
    assert done == steps
    want = (one.nodes(), one.velocities(), one.accelerations())
    e_one = one.kinetic_energy()
    one.close()
    check_state("one context, 20 steps in one call", want, traj[-1], deck.nodes)
    g, _, _, _ = (make_solver("big", feahip.FeaGroup, 2) if form == "shards2" else make_solver("big", feahip.FeaGroup, 3, rank_contexts=True))
    done, log = g.solve_explicit(steps, dt, dlambda=dlam)
    assert done == steps and np.all(log == dt)
    got = (g.gather("nodes"), g.gather("velocities"), g.gather("accelerations"))
    check_state(form, got, want, deck.nodes, tol=SHARD_TOL)
    for rk, nd in zip(g.ranks, g.nodes):
        if g.rank_contexts:                                            # halo x is the owner's
            x = rk.nodes()
            assert rel(x, want[0][rk.node_global], np.abs(want[0] - deck.nodes).max()) <= SHARD_TOL
        else:
            check_state(form + " rank", (rk.nodes(), rk.velocities(), rk.accelerations()), want, deck.nodes, nd, SHARD_TOL)
            touching = np.isin(deck.elements, nd).any(axis=1)          # halo: the other nodes of the elements at its rows
            halo = np.setdiff1d(np.unique(deck.elements[touching]), nd)
            assert len(halo) > 0
            assert rel(rk.nodes()[halo], want[0][halo], np.abs(want[0] - deck.nodes).max()) <= SHARD_TOL
    e = g.kinetic_energy()
    print(form, "kinetic energy", e, e_one)
    assert abs(e - e_one) <= 1e-12 * e_one
    g.close()


def stretching_velocity(deck):
    """v = (0, 2 y, 0.5 y): every node above the clamped end moves from the first step on, so the tangent -- and the
    estimate -- changes within a few steps (a bar released from rest keeps its first estimate exactly until the wave
    reaches the row that decides the bound)."""
    y = deck.nodes[:, 1]
    return np.stack([np.zeros_like(y), 2.0 * y, 0.5 * y], axis=1)


def test_adaptive_step_follows_the_estimates():
    deck, rho, _, _, _, _ = case_deck("tet4")
    r = ExplicitRestatement(deck, rho)
    r.v = stretching_velocity(deck)
    traj, dts = r.explicit(6, 0.0, safety=0.8, restep=3, dlambda=0.1)
    r.close()
    assert dts[0] == dts[1] == dts[2] and dts[3] == dts[4] == dts[5] and abs(dts[3] / dts[0] - 1.0) > 1e-4
    s, _, _, _ = make_solver("tet4")
    s.set_velocities(stretching_velocity(deck))
    done, log = s.solve_explicit(6, 0.0, safety=0.8, restep=3, dlambda=0.1)
    print("adaptive dt", log, dts)
    assert done == 6 and log[0] == log[1] == log[2] and log[3] == log[4] == log[5]
    assert rel(log[0], dts[0]) <= 1e-10 and rel(log[3], dts[3]) <= 1e-10
    check_state("adaptive", (s.nodes(), s.velocities(), s.accelerations()), traj[-1], deck.nodes)
    s.close()
    s, _, _, _ = make_solver("tet4")                                   # restep <= 0: one estimate
    s.set_velocities(stretching_velocity(deck))
    done, log = s.solve_explicit(5, 0.0, safety=0.8, restep=0, dlambda=0.1)
    assert done == 5 and np.all(log == log[0]) and rel(log[0], dts[0]) <= 1e-10
    s.close()


def test_free_flight():
    deck = free_block()
    s = feahip.FeaSolver(deck)
    s.set_mass(2.0)
    s.set_velocities(np.tile(V0, (s.N, 1)))
    done, _ = s.solve_explicit(3, 0.01)
    assert done == 3 and abs(s.time() - 0.03) < 1e-15
    x, v, a = s.nodes(), s.velocities(), s.accelerations()
    want = deck.nodes + V0 * 0.03
    print("free flight", rel(x, want), rel(v, np.tile(V0, (s.N, 1))), np.abs(a).max())
    assert rel(x, want) <= FREE_TOL and rel(v, np.tile(V0, (s.N, 1))) <= FREE_TOL
    assert np.abs(a).max() <= FREE_TOL * np.abs(V0).max() / 0.01
    s.close()


def test_explicit_and_newmark_steps_interchange():
    deck, rho, _, _, _, _ = case_deck("tet4")
    r = ExplicitRestatement(deck, rho)
    r.lam = 1.0
    dt = 0.5 * r.stable_step()
    r.explicit(10, dt)
    done_w, its_w, traj = r.newmark(2, 4 * dt, 0.25, 0.5, 0.0, deck.max_newton_count, deck.desired_tolerance)
    r.close()
    s = feahip.FeaSolver(deck)
    s.set_mass(rho)
    s.set_load_factor(1.0)
    assert s.solve_explicit(10, dt)[0] == 10
    done, its, _ = s.solve_dynamic(2, 4 * dt, 0.25, 0.5, 0.0)
    assert done == done_w == 2 and list(its) == its_w
    check_state("10 explicit + 2 Newmark", (s.nodes(), s.velocities(), s.accelerations()), traj[-1], deck.nodes)
    assert abs(s.time() - 18 * dt) <= 1e-13 * 18 * dt
    s.close()


def test_refusals():
    deck, rho, _, _, _, _ = case_deck("tet4")
    s = feahip.FeaSolver(deck)

    def refused(code, what, fn, *args, **kw):
        with pytest.raises(feahip.FeaHipError, match=what) as e:
            fn(*args, **kw)
        assert f"error {code}:" in str(e.value)

    for fn, args in ((s.lumped_mass, ()), (s.stable_step, ()), (s.kinetic_energy, ()), (s.solve_explicit, (1, 0.01))):
        refused(feahip.ESTATE, "no mass on this context", fn, *args)
    for what in (10, 11):
        refused(feahip.EINVAL, rf"time_kernel\({what}\): no mass", s.time_kernel, what)
    s.set_mass(rho)
    refused(feahip.EINVAL, "dt must not be negative", s.solve_explicit, 1, -0.01)
    refused(feahip.EINVAL, "n_steps must not be negative", s.solve_explicit, -1, 0.01)
    for safety in (0.0, 1.5, -0.1, float("nan")):
        refused(feahip.EINVAL, r"safety must be in \(0, 1\]", s.solve_explicit, 1, 0.0, safety=safety)
    assert s.solve_explicit(1, 0.01, safety=7.0)[0] == 1               # ignored with a fixed dt
    assert s.time_kernel(10, 1, 2) > 0 and s.time_kernel(11, 1, 2) > 0
    s.close()


def inverted_tets(deck, x):
    """Linear tetrahedra whose signed volume at x is not of the sign it has at the deck's nodes."""
    e = deck.elements

    def vol(X):
        return np.linalg.det(np.stack([X[e[:, 1]] - X[e[:, 0]], X[e[:, 2]] - X[e[:, 0]], X[e[:, 3]] - X[e[:, 0]]], axis=1))
    return int((vol(x) * np.sign(vol(deck.nodes)) <= 0).sum())


def test_inversion_ends_the_loop_at_the_next_check():
    """The far end is pushed in by 0.3 per step against layers 0.5 thick: the restatement, on the same schedule, has no
    inverted tetrahedron after the first step and some after the second.  With restep = 1 the check before step 3 finds
    them; steps_done counts the steps up to the check before."""
    deck = loaded_bar("tet4", DIMS, end_motion=-0.3)
    r = ExplicitRestatement(deck, 1.5)
    bad = []
    for k in range(2):
        r.explicit(1, 0.0, safety=0.5, restep=1, dlambda=1.0)
        bad.append(inverted_tets(deck, r.x))
    r.close()
    assert bad[0] == 0 and bad[1] > 0
    s = feahip.FeaSolver(deck)
    s.set_mass(1.5)
    done, log, rc = s.solve_explicit(6, 0.0, safety=0.5, restep=1, dlambda=1.0, check=False)
    print("inversion", done, log, rc)
    assert rc == feahip.ENOTCONVERGED and done == 1 and len(log) == 2
    assert b"inverted elements" in s._lib.feahip_last_error(s._ctx)
    assert np.isfinite(s.nodes()).all()                                # the state is left as it is
    s.close()


@pytest.mark.parametrize("kind", ["tet4", "tet10", "hex8"])
def test_fixed_step_reports_an_inverted_mesh(kind):
    """One step with a caller-given dt that pushes the far end 0.6 into layers 0.5 thick: the interior is at rest, so
    the top layer is inverted whatever the element type; the check after the last step says so (no stiffness assembly
    is involved, and the residual-only assembly of the 10-node and 8-node elements does not count)."""
    deck = loaded_bar(kind, DIMS, end_motion=-0.6)
    s = feahip.FeaSolver(deck)
    s.set_mass(1.5)
    done, log, rc = s.solve_explicit(1, 0.005, dlambda=1.0, check=False)
    assert rc == feahip.ENOTCONVERGED and done == 0 and list(log) == [0.005]
    assert b"inverted elements" in s._lib.feahip_last_error(s._ctx)
    assert s.update_state() > 0
    s.close()
    s = feahip.FeaSolver(loaded_bar(kind, DIMS, end_motion=-0.1))      # a mesh that stays valid: no report
    s.set_mass(1.5)
    assert s.solve_explicit(1, 0.005, dlambda=1.0)[0] == 1
    s.close()


def test_command_line_reproduces_the_python_trajectory(tmp_path):
    p = tmp_path / "explicit_bar.sexp"
    with open(GOLDEN) as f:
        p.write_text(f.read())
    d = feahip.Deck.load(str(p))
    assert d.dynamics["scheme"] == "explicit" and d.dynamics["steps"] == 20
    s = feahip.FeaSolver(d)                                            # the mass comes with the deck
    done, log = s.solve_explicit()
    assert done == 20
    u = s.nodes() - d.nodes
    s.close()
    exe = os.path.join(os.path.dirname(feahip.LIB_PATH), "feasolver_hip")
    out = subprocess.run([exe, str(p)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    dts = [float(m) for m in re.findall(r"Explicit step \d+ finished: time \S+ dt (\S+)", out.stdout)]
    assert len(dts) == 20 and np.array_equal(np.array(dts), log)
    lines = (tmp_path / "explicit_bar.msh").read_text().splitlines()
    at = max(i for i, ln in enumerate(lines) if ln == "$NodeData")
    n = len(d.nodes)
    start = next(i for i in range(at, len(lines)) if lines[i].strip() == str(n)) + 1
    got = np.array([[float(v) for v in ln.split()[1:4]] for ln in lines[start:start + n]])
    assert np.abs(u).max() > 1e-3 and np.abs(got - u).max() <= 1e-6    # the file holds six decimals

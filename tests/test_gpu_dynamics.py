"""Implicit dynamics on the GPU against tests/dynamics_reference.py: the consistent mass, the body force, the
consistent acceleration and the Newmark steps of feahip_solve_dynamic, on one context, on row shards and on rank
contexts, and from the command line."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import feahip
import mesh
from dynamics_reference import DENSITIES, DynamicsRestatement, dense_mass, free_block, loaded_bar
from hetero_reference import MATERIALS, scattered_ids, with_materials

pytestmark = pytest.mark.gpu

M_TOL = 1e-13        # of max|y|: shorter sums of positive terms than K's parity (1e-12 of scale)
FREE_TOL = 1e-11     # closed forms of the unconstrained body
U_TOL = 1e-10        # of max|x - x0|: the bound the project holds the full path to (tests/test_gpu_fullpath.py)
NH, A5 = feahip.MODEL_COMPRESSIBLE_NEOHOOKEAN, feahip.MODEL_A5
V0 = np.array([1.0, -2.0, 0.5])
B = np.array([0.3, -9.81, 1.1])
# a tenth of the first axial period of the 2-long clamped bar: T = 4 L / c, c = sqrt(E / rho), E = mu (3 lambda + 2 mu) / (lambda + mu) = 250
DT = 0.1 * 4 * 2.0 / np.sqrt(250.0 / 1.5)


def rel(a, b, scale=None):
    s = np.abs(b).max() if scale is None else scale
    return np.abs(np.asarray(a) - np.asarray(b)).max() / (s if s > 0 else 1.0)


def mass_deck(kind):
    if kind == "tet4":
        return mesh.jitter_permute(mesh.bar_deck(dims=(3, 4, 3)))      # renumbered, 80 rows: five 16-row chunks, more than one workgroup of four
    if kind == "tet10":
        return mesh.bar_deck(dims=(2, 2, 2), quadratic=True)
    return mesh.bar_deck(dims=(2, 3, 2), hexa=True)


@pytest.mark.parametrize("table", [False, True])
@pytest.mark.parametrize("kind", ["tet4", "tet10", "hex8"])
def test_mass_spmv_matches_the_dense_mass(kind, table):
    deck = mass_deck(kind)
    ids = scattered_ids(deck)
    if table:
        deck = with_materials(deck, MATERIALS, ids)
    rho = DENSITIES if table else 2.5
    M = dense_mass(deck, rho, ids)
    rng = np.random.default_rng(5)
    s = feahip.FeaSolver(deck)
    s.set_mass(rho)
    for x in (np.ones(s.ndof), rng.standard_normal(s.ndof)):
        y, want = s.mass_spmv(x), M @ x
        print(kind, table, "mass_spmv", rel(y, want))
        assert rel(y, want) <= M_TOL
    y1 = s.mass_spmv(x)
    s.set_mass(rho)                                                    # twice: the same bits
    assert np.array_equal(s.mass_spmv(x), y1)
    assert np.abs(s.velocities()).max() == 0.0 and np.abs(s.accelerations()).max() == 0.0 and s.time() == 0.0
    s.close()


def test_free_flight():
    deck = free_block()
    s = feahip.FeaSolver(deck)
    s.set_mass(2.0)
    s.set_velocities(np.tile(V0, (s.N, 1)))
    done, its, _ = s.solve_dynamic(3, 0.01, 0.25, 0.5, 0.0, max_newton=10, desired_tolerance=1e-20, solver_tolerance=1e-15)
    assert done == 3 and abs(s.time() - 0.03) < 1e-15
    x, v, a = s.nodes(), s.velocities(), s.accelerations()
    want = deck.nodes + V0 * 0.03
    print("free flight", rel(x, want), rel(v, np.tile(V0, (s.N, 1))), np.abs(a).max())
    assert rel(x, want) <= FREE_TOL and rel(v, np.tile(V0, (s.N, 1))) <= FREE_TOL
    assert np.abs(a).max() <= FREE_TOL * np.abs(V0).max() / 0.01       # a = 0 to rounding on the scale v / dt
    s.close()


def test_free_fall():
    deck = free_block()
    s = feahip.FeaSolver(deck)
    s.set_mass(2.0)
    s.set_body_force(B)
    s.set_load_factor(1.0)
    s.consistent_acceleration(feahip.CG, 1e-15, 2000)
    a = s.accelerations()
    print("consistent acceleration", rel(a, np.tile(B, (s.N, 1))))
    assert rel(a, np.tile(B, (s.N, 1))) <= FREE_TOL
    done, _, _ = s.solve_dynamic(3, 0.01, 0.25, 0.5, 0.0, max_newton=10, desired_tolerance=1e-20, solver_tolerance=1e-15)
    assert done == 3
    t = 0.03
    x, v, a = s.nodes(), s.velocities(), s.accelerations()
    print("free fall", rel(x, deck.nodes + 0.5 * B * t * t), rel(v, np.tile(B * t, (s.N, 1))), rel(a, np.tile(B, (s.N, 1))))
    assert rel(x, deck.nodes + 0.5 * B * t * t) <= FREE_TOL
    assert rel(v, np.tile(B * t, (s.N, 1))) <= FREE_TOL and rel(a, np.tile(B, (s.N, 1))) <= FREE_TOL
    s.close()


CASES = {
    "tet4": dict(kind="tet4", dims=(4, 12, 4)),
    "tet4_a5": dict(kind="tet4", dims=(2, 4, 2), model=A5),
    "tet10": dict(kind="tet10", dims=(1, 2, 1)),
    "hex8": dict(kind="hex8", dims=(2, 4, 2)),
    "tet4_table": dict(kind="tet4", dims=(2, 4, 2)),
    "end_motion": dict(kind="tet4", dims=(2, 4, 2), end_motion=0.01),
}


def case_deck(name):
    deck = loaded_bar(**CASES[name])
    if name == "tet4_table":
        deck = with_materials(deck, MATERIALS, scattered_ids(deck))
    return deck, (DENSITIES if name == "tet4_table" else 1.5)


@functools.lru_cache(maxsize=None)
def released(name):
    """(steps done, Newton counts, trajectory) of the restatement -- computed once, shared, never written to."""
    deck, rho = case_deck(name)
    r = DynamicsRestatement(deck, rho)
    if name == "end_motion":
        out = r.newmark(3, DT, 0.25, 0.5, 1.0, deck.max_newton_count, deck.desired_tolerance)
    else:
        r.lam = 1.0
        out = r.newmark(4, DT, 0.25, 0.5, 0.0, deck.max_newton_count, deck.desired_tolerance)
    r.close()
    for st in out[2]:
        for arr in st:
            arr.setflags(write=False)
    return out


def run_released(s, name, steps=None):
    if name == "end_motion":
        return s.solve_dynamic(3 if steps is None else steps, DT, 0.25, 0.5, 1.0)
    return s.solve_dynamic(4 if steps is None else steps, DT, 0.25, 0.5, 0.0)


def check_state(tag, x, v, a, want, deck, rows=None):
    """x, v and a alike within U_TOL of max|x - x0| (the numbers, whatever their units)."""
    xw, vw, aw = want
    rows = slice(None) if rows is None else rows
    scale = np.abs(xw - deck.nodes).max()
    ex, ev, ea = rel(x[rows], xw[rows], scale), rel(v[rows], vw[rows], scale), rel(a[rows], aw[rows], scale)
    print(tag, "x", ex, "v", ev, "a", ea)
    assert ex <= U_TOL and ev <= U_TOL and ea <= U_TOL


@pytest.mark.parametrize("name", ["tet4", "tet4_a5", "tet10", "hex8", "tet4_table", "end_motion"])
def test_trajectory_matches_the_restatement(name):
    """Release of a loaded bar (load factor 1, dlambda = 0, 4 steps) and, for end_motion, a prescribed end motion
    (dlambda = 1, 3 steps): x, v, a of every step -- v and a at the prescribed nodes included -- and the Newton counts."""
    deck, rho = case_deck(name)
    done_w, its_w, traj = released(name)
    s = feahip.FeaSolver(deck)
    s.set_mass(rho)
    if name != "end_motion":
        s.set_load_factor(1.0)
    for k in range(len(traj)):                                         # step by step: every state is compared
        done, its, _ = run_released(s, name, 1)
        assert done == 1 and int(its[0]) == its_w[k], (k, its, its_w)
        check_state(f"{name} step {k + 1}", s.nodes(), s.velocities(), s.accelerations(), traj[k], deck)
    assert done_w == len(traj)
    assert abs(s.time() - len(traj) * DT) < 1e-14
    s.close()


def test_static_gravity_ramp():
    deck = loaded_bar(kind="tet4", dims=(2, 4, 2), traction=0.0)
    g = np.array([0.0, -3.0, 1.0])
    r = DynamicsRestatement(deck, 1.5, body=g)
    done_w, its_w = r.static(2, deck.max_newton_count, deck.desired_tolerance)
    r.close()
    s = feahip.FeaSolver(deck)
    s.set_mass(1.5)
    s.set_body_force(g)
    done, its, _ = s.solve(2, modified_newton=False)
    print("static gravity", rel(s.nodes() - deck.nodes, r.x - deck.nodes))
    assert done == done_w == 2 and list(its[:2]) == its_w
    assert rel(s.nodes() - deck.nodes, r.x - deck.nodes) <= U_TOL
    s.close()


def gravity_deck(**kw):
    d = loaded_bar(kind="tet4", dims=(4, 12, 4), traction=0.0)
    keys = ("model", "parameters", "ele_type", "gauss_nodes_count", "nodes", "elements", "presc_node", "presc_type", "presc_values",
            "max_newton_count", "desired_tolerance", "modified_newton", "solver_type", "solver_tolerance")
    return feahip.Deck(**{k: getattr(d, k) for k in keys}, **kw)


def test_body_force_follows_the_shard_and_the_material_ids():
    """The static path keeps F_body current: a mass set before the rows were cut (the deck's, installed at creation, then
    feahip_group_init) gives every rank the gravity of ITS rows; new ids of a table of the same size give the new
    gravity; a table of another size is refused by the next residual assembly."""
    g = np.array([0.0, -3.0, 1.0])
    deck = gravity_deck(density=1.5, body_force=g)
    one = feahip.FeaSolver(deck)
    done, its, _ = one.solve(2, modified_newton=False)
    want = one.nodes()
    one.close()
    grp = feahip.FeaGroup(deck, 2)                                     # mass and body force installed, THEN the shards
    done_g, its_g, _ = grp.solve(2, deck.max_newton_count, False, deck.desired_tolerance, deck.solver_type, deck.solver_tolerance)
    got = grp.gather("nodes")
    grp.close()
    print("sharded static gravity", rel(got - deck.nodes, want - deck.nodes))
    assert done == done_g == 2 and list(its) == list(its_g) and rel(got - deck.nodes, want - deck.nodes) <= U_TOL
    # per-material densities: the ids change under the mass
    plain = gravity_deck()
    ids = scattered_ids(plain)
    ids2 = ((ids + 1) % 3).astype(np.int32)

    def gravity_residual(s):
        s.set_load_factor(1.0)
        s.create_residual_forces()
        return s.forces()

    a = feahip.FeaSolver(with_materials(plain, MATERIALS, ids))
    a.set_mass(DENSITIES)
    a.set_body_force(g)
    f1 = gravity_residual(a)
    a.set_materials(MATERIALS, ids2)
    f2 = gravity_residual(a)
    b = feahip.FeaSolver(with_materials(plain, MATERIALS, ids2))
    b.set_mass(DENSITIES)
    b.set_body_force(g)
    assert np.array_equal(f2, gravity_residual(b)) and not np.array_equal(f1, f2)
    b.close()
    a.set_materials(MATERIALS[:2], ids % 2)
    with pytest.raises(feahip.FeaHipError, match="material count changed") as e:
        a.create_residual_forces()
    assert f"error {feahip.ESTATE}:" in str(e.value)
    with pytest.raises(feahip.FeaHipError, match="material count changed"):
        a.solve(1, modified_newton=False)
    a.set_mass(None)                                                   # cleared: the static path runs again, without gravity
    a.create_residual_forces()
    a.close()


@pytest.mark.parametrize("form", ["shards2", "ranks3"])
def test_sharded_trajectory_is_the_unsharded_one(form):
    deck, rho = case_deck("tet4")
    one = feahip.FeaSolver(deck)
    one.set_mass(rho)
    one.set_load_factor(1.0)
    x = np.random.default_rng(7).standard_normal(one.ndof)
    y_one = one.mass_spmv(x)
    run_released(one, "tet4")
    want = (one.nodes(), one.velocities(), one.accelerations())
    one.close()
    g = feahip.FeaGroup(deck, 2) if form == "shards2" else feahip.FeaGroup(deck, 3, rank_contexts=True)
    g.set_mass(rho)
    g.each("set_load_factor", 1.0)
    y = np.zeros((len(deck.nodes), 3))
    for rk, nd in zip(g.ranks, g.nodes):                               # the ranks' products add up to the unsharded one
        if g.rank_contexts:
            yr = rk.mass_spmv(x.reshape(-1, 3)[rk.node_global].ravel()).reshape(-1, 3)
            assert np.abs(yr[rk.n_own:]).max() == 0.0
            y[rk.node_global[:rk.n_own]] += yr[:rk.n_own]
        else:
            y += rk.mass_spmv(x).reshape(-1, 3)
    print(form, "mass_spmv", rel(y.ravel(), y_one))
    assert rel(y.ravel(), y_one) <= M_TOL
    done, its, _ = g.solve_dynamic(4, DT, 0.25, 0.5, 0.0, deck.max_newton_count, deck.desired_tolerance, deck.solver_type,
                                   deck.solver_tolerance, deck.solver_max_iter)
    assert done == 4 and list(its) == released("tet4")[1]
    check_state(form, g.gather("nodes"), g.gather("velocities"), g.gather("accelerations"), want, deck)
    for rk, nd in zip(g.ranks, g.nodes):                               # ... on each rank's owned rows, and the restatement's
        if g.rank_contexts:                                            # local arrays: the owned rows are the first n_own
            full = [np.full((len(deck.nodes), 3), np.nan) for _ in range(3)]
            for out, loc in zip(full, (rk.nodes(), rk.velocities(), rk.accelerations())):
                out[nd] = loc[:rk.n_own]
            check_state(form + " rank", *full, released("tet4")[2][-1], deck, nd)
        else:
            check_state(form + " rank", rk.nodes(), rk.velocities(), rk.accelerations(), released("tet4")[2][-1], deck, nd)
    g.close()


def test_a_collective_error_on_another_rank_reaches_the_callers_handle():
    """feahip_consistent_acceleration is made on ONE handle and drives the group: when a rank other than that handle's
    refuses (here rank 1 has no mass), the code is that rank's and the handle the caller holds names the reason."""
    g = feahip.FeaGroup(mesh.bar_deck(dims=(2, 2, 2)), 2)
    r0 = g.ranks[0]
    r0.set_mass(1.5)                                                   # rank 0 only
    rc = r0._lib.feahip_consistent_acceleration(r0._ctx, feahip.PCG_ILU, 1e-14, 100)
    msg = r0._lib.feahip_last_error(r0._ctx).decode()
    print("rc", rc, "last_error of the caller's handle:", repr(msg))
    assert rc == feahip.ESTATE
    assert msg and "feahip_consistent_acceleration" in msg
    g.close()


def one_newton_iteration(s):
    s.update_nodes_with_bc(1.0)
    s.create_stiffness_and_residual()
    off, idx, val = s.matrix_yale()
    f = s.forces()
    s.apply_prescribed_bc(0.0)
    s.solve_slae()
    return val, f, s.solution()


@pytest.mark.parametrize("kind", ["tet4", "tet10", "hex8"])
def test_a_cleared_mass_changes_no_bit(kind):
    deck = mass_deck(kind)
    fresh = feahip.FeaSolver(deck)
    want = one_newton_iteration(fresh)
    fresh.close()
    s = feahip.FeaSolver(deck)
    s.set_mass(2.0)
    s.set_body_force([0.0, -9.81, 0.0])
    s.set_mass(None)
    got = one_newton_iteration(s)
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
    s.close()


def test_refusals():
    deck, _ = case_deck("tet4_table")
    s = feahip.FeaSolver(deck)
    lib, ctx = s._lib, s._ctx

    def refused(code, what, fn, *args):
        with pytest.raises(feahip.FeaHipError, match=what) as e:
            fn(*args)
        assert f"error {code}:" in str(e.value)

    # without a mass
    refused(feahip.ESTATE, "no mass on this context", s.solve_dynamic, 1, DT, 0.25, 0.5, 0.0)
    refused(feahip.ESTATE, "no mass on this context", s.set_body_force, [0, 0, 1])
    refused(feahip.ESTATE, "no mass on this context", s.velocities)
    refused(feahip.ESTATE, "no mass on this context", s.consistent_acceleration)
    refused(feahip.ESTATE, "no mass on this context", s.mass_spmv, np.zeros(s.ndof))
    for what in (8, 9):
        refused(feahip.EINVAL, rf"time_kernel\({what}\): no mass", s.time_kernel, what)
    # feahip_set_mass
    refused(feahip.EINVAL, "density 1 is not finite and positive", s.set_mass, [1.0, -2.0, 1.0])
    refused(feahip.EINVAL, "density 0 is not finite and positive", s.set_mass, [np.nan])
    refused(feahip.EINVAL, r"2 densities: one, or one per material \(3 in force\)", s.set_mass, [1.0, 2.0])
    w, N, dN = feahip.element_tables(deck.ele_type, 4)
    rho = np.array([1.0])
    assert lib.feahip_set_mass(ctx, 1, feahip._d(rho), 4, None, feahip._d(N), feahip._d(dN)) == feahip.EINVAL
    assert b"null array" in lib.feahip_last_error(ctx)
    assert lib.feahip_set_mass(ctx, 1, feahip._d(rho), 4, feahip._d(w), feahip._d(N), feahip._d(-dN)) == feahip.EINVAL
    assert b"det J0 <= 0 at a mass point of element 0" in lib.feahip_last_error(ctx)
    refused(feahip.ESTATE, "no mass on this context", s.velocities)     # the context is left as it was
    # the step
    s.set_mass(DENSITIES)
    refused(feahip.EINVAL, "dt must be positive", s.solve_dynamic, 1, 0.0, 0.25, 0.5, 0.0)
    refused(feahip.EINVAL, "beta must be positive", s.solve_dynamic, 1, DT, 0.0, 0.5, 0.0)
    refused(feahip.EINVAL, "gamma must not be negative", s.solve_dynamic, 1, DT, 0.25, -0.1, 0.0)
    # a bad call leaves the mass in force
    y = s.mass_spmv(np.ones(s.ndof))
    refused(feahip.EINVAL, "density 2 is not finite and positive", s.set_mass, [1.0, 2.0, 0.0])
    assert np.array_equal(s.mass_spmv(np.ones(s.ndof)), y)
    # arc length with a body force
    s.set_body_force([0.0, -1.0, 0.0])
    refused(feahip.EINVAL, "a body force is set", s.solve_arclength, 2.0, 2)
    s.set_body_force(None)
    # a table of another size drops the per-material mass
    s.set_materials(MATERIALS[:2], scattered_ids(deck) % 2)
    refused(feahip.ESTATE, "material count changed", s.solve_dynamic, 1, DT, 0.25, 0.5, 0.0)
    refused(feahip.ESTATE, "material count changed", s.mass_spmv, np.ones(s.ndof))
    s.set_mass(2.0)                                                    # a new mass is a new start
    assert s.mass_spmv(np.ones(s.ndof)).sum() > 0
    s.close()


def test_command_line_reproduces_the_python_trajectory(tmp_path):
    deck, _ = case_deck("tet4_a5")
    kw = {k: getattr(deck, k) for k in ("model", "parameters", "ele_type", "gauss_nodes_count", "nodes", "elements", "presc_node",
                                         "presc_type", "presc_values", "surface_faces", "surface_kind", "surface_values",
                                         "max_newton_count", "desired_tolerance", "modified_newton", "solver_type",
                                         "solver_tolerance")}
    d = feahip.Deck(**kw, density=1.5, body_force=[0.0, 0.0, -2.0], dynamics=dict(steps=3, dt=float(DT), dlambda=1.0))
    p = tmp_path / "dyn.sexp"
    d.save(str(p))
    s = feahip.FeaSolver(feahip.Deck.load(str(p)))                     # mass and body force come with the deck
    done, its, _ = s.solve_dynamic()
    assert done == 3
    u = s.nodes() - d.nodes
    s.close()
    exe = os.path.join(os.path.dirname(feahip.LIB_PATH), "feasolver_hip")
    out = subprocess.run([exe, str(p)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    counts = [int(m) for m in re.findall(r"Dynamic step \d+ finished: time \S+ (\d+) iterations", out.stdout)]
    assert counts == [int(k) for k in its]
    lines = (tmp_path / "dyn.msh").read_text().splitlines()
    at = max(i for i, ln in enumerate(lines) if ln == "$NodeData")      # the last step's displacements
    n = len(d.nodes)
    start = next(i for i in range(at, len(lines)) if lines[i].strip() == str(n)) + 1
    got = np.array([[float(v) for v in ln.split()[1:4]] for ln in lines[start:start + n]])
    assert np.abs(u).max() > 1e-3 and np.abs(got - u).max() <= 1e-6    # the file holds six decimals

"""Rayleigh damping on the GPU against tests/damping_reference.py: the product C v, the damped Newmark trajectories and
the damped consistent acceleration, row shards and rank contexts, the damped explicit steps and the dynamic relaxation,
the bits of a context without damping, the refusals and the command line."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import feahip
from damping_reference import COEFFICIENTS, DampedDynamics, DampedExplicit, damped_release, release_deck
from dynamics_reference import DENSITIES, DynamicsRestatement, dense_mass, loaded_bar
from explicit_reference import hub_fan
from hetero_reference import MATERIALS, scattered_ids, with_materials
from test_gpu_dynamics import DT, check_state, mass_deck, rel

pytestmark = pytest.mark.gpu

C_TOL = 1e-12        # of max|y|: K's parity bound with the oracle, the one M_TOL's comment in test_gpu_dynamics.py cites
U_TOL = 1e-10        # of max|x - x0|, as tests/test_gpu_dynamics.py
# the consistent acceleration, of max|a|: f is held to 1e-12 of its scale and C v to C_TOL; a = M^-1 (f - C v) amplifies
# that by the condition of the consistent mass on the free dofs, which the test prints (below 100 on these meshes)
A_TOL = 1e-10
X_TOL = 5.6e-10      # explicit steps: the bound of tests/test_gpu_explicit.py
RELAX_TOL = 1e-10    # the relaxed state against feahip_solve's, of max|x - x0|
DIMS = (2, 4, 2)
PAIRS = [(0.7, 0.0), (0.0, 0.013), (0.7, 0.013)]


# ---- a: the product ---------------------------------------------------------------------------------------------------
def spmv_deck(name):
    if name in ("tet4", "tet10", "hex8"):
        return mass_deck(name), 2.5
    if name == "hub":
        return hub_fan(), 2.5                                       # a row longer than the 128-block tile
    d = mass_deck("tet4")
    return with_materials(d, MATERIALS, scattered_ids(d)), DENSITIES


@functools.lru_cache(maxsize=None)
def dense_parts(name):
    """(M, K(X0)) dense -- computed once, shared, never written to."""
    deck, rho = spmv_deck(name)
    r = DynamicsRestatement(deck, rho)
    K = r.h.assemble(r.x)[0].copy()
    M = r.M.copy()
    r.close()
    K.setflags(write=False); M.setflags(write=False)
    return M, K


@pytest.mark.parametrize("name", ["tet4", "tet10", "hex8", "hub", "table"])
def test_damping_spmv_matches_the_dense_product(name):
    deck, rho = spmv_deck(name)
    M, K = dense_parts(name)
    rng = np.random.default_rng(11)
    vs = (np.ones(3 * len(deck.nodes)), rng.standard_normal(3 * len(deck.nodes)))
    s = feahip.FeaSolver(deck)
    s.set_mass(rho)
    for alpha, beta in PAIRS:
        s.set_damping(alpha, beta)
        assert s.damping() == (alpha, beta)
        C = alpha * M + beta * K
        for v in vs:
            y, want = s.damping_spmv(v), C @ v
            # K_d 1 = 0 (a translation strains nothing): with beta_k alone the exact product of the ones is zero and
            # max|y| is no scale; the terms that were summed are
            terms = (np.abs(C) @ np.abs(v)).max()
            scale = np.abs(want).max() if np.abs(want).max() > 1e-6 * terms else terms
            print(name, alpha, beta, "damping_spmv", rel(y, want, scale), "of", scale)
            assert rel(y, want, scale) <= C_TOL
        assert np.array_equal(s.damping_spmv(vs[1]), y)                # twice: the same bits
    s.close()
    if name == "tet4":                                                 # beta_k alone needs no mass
        s = feahip.FeaSolver(deck)
        s.set_damping(0.0, 0.013)
        assert rel(s.damping_spmv(vs[1]), 0.013 * (K @ vs[1])) <= C_TOL
        s.close()


def test_the_snapshot_is_the_tangent_at_the_state_of_the_call():
    deck = loaded_bar("tet4", DIMS)
    s = feahip.FeaSolver(deck)
    done, _, _ = s.solve(1, modified_newton=False)                     # one static increment of the traction
    assert done == 1
    x = s.nodes()
    u, f = s.solution(), s.forces()
    s.set_damping(0.0, 0.02)
    assert np.array_equal(s.nodes(), x) and np.array_equal(s.solution(), u) and np.array_equal(s.forces(), f)
    r = DynamicsRestatement(deck, 1.5)
    K = r.h.assemble(x)[0]
    K0 = r.h.assemble(deck.nodes)[0]
    r.close()
    v = np.random.default_rng(3).standard_normal(s.ndof)
    y = s.damping_spmv(v)
    print("snapshot at the deformed state", rel(y, 0.02 * (K @ v)), "against K(X0)", rel(y, 0.02 * (K0 @ v)))
    assert rel(y, 0.02 * (K @ v)) <= C_TOL and rel(y, 0.02 * (K0 @ v)) > 1e-6
    s.set_nodes(deck.nodes * np.array([1.0, 1.1, 1.0]))                # x moves on: the snapshot stays
    s.create_stiffness_and_residual()
    assert np.array_equal(s.damping_spmv(v), y)
    s.set_materials(MATERIALS, scattered_ids(deck))                    # ... and under another material table
    assert np.array_equal(s.damping_spmv(v), y)
    s.close()


# ---- b: trajectories --------------------------------------------------------------------------------------------------
def run_release(s, name, deck, steps):
    dl = 1.0 if name == "end_motion" else 0.0
    if isinstance(s, feahip.FeaGroup):
        return s.solve_dynamic(steps, DT, 0.25, 0.5, dl, deck.max_newton_count, deck.desired_tolerance, deck.solver_type,
                               deck.solver_tolerance, deck.solver_max_iter)
    return s.solve_dynamic(steps, DT, 0.25, 0.5, dl)


@pytest.mark.parametrize("key", list(COEFFICIENTS))
@pytest.mark.parametrize("name", ["tet4", "tet4_a5", "tet10", "hex8", "tet4_table", "end_motion"])
def test_damped_trajectory_matches_the_restatement(name, key):
    """The release cases of tests/test_gpu_dynamics.py under the three coefficient pairs: x, v, a of every step and the
    Newton counts (tests/test_damping_reference_cpu.py holds every count away from a borderline comparison)."""
    deck, rho = release_deck(name)
    done_w, its_w, traj, _, _ = damped_release(name, key)
    s = feahip.FeaSolver(deck)
    s.set_mass(rho)
    s.set_damping(*COEFFICIENTS[key])
    if name != "end_motion":
        s.set_load_factor(1.0)
    for k in range(len(traj)):
        done, its, _ = run_release(s, name, deck, 1)
        assert done == 1 and int(its[0]) == its_w[k], (k, its, its_w)
        check_state(f"{name} {key} step {k + 1}", s.nodes(), s.velocities(), s.accelerations(), traj[k], deck)
    assert done_w == len(traj)
    s.close()


# ---- c: the consistent acceleration -----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["tet4", "tet10", "hex8"])
def test_damped_consistent_acceleration(kind):
    deck = loaded_bar(kind, DIMS if kind != "tet10" else (1, 2, 1))
    rng = np.random.default_rng(17)
    v = rng.standard_normal(deck.nodes.shape)
    x = deck.nodes + 0.01 * rng.standard_normal(deck.nodes.shape)
    x[deck.presc_node] = deck.nodes[deck.presc_node]
    r = DampedDynamics(deck, 1.5)
    r.set_damping(0.5, 0.01)                                           # K_d = K(X0)
    r.x, r.v, r.lam = x.copy(), v.copy(), 1.0
    r.consistent_acceleration()
    undamped = DynamicsRestatement.consistent_acceleration
    want = r.a.copy()
    undamped(r)
    free = ~r.mask
    cond = np.linalg.cond(r.M[np.ix_(free, free)])
    plain = r.a.copy()
    r.close()
    s = feahip.FeaSolver(deck)
    s.set_mass(1.5)
    s.set_damping(0.5, 0.01)
    s.set_nodes(x)
    s.set_velocities(v)
    s.set_load_factor(1.0)
    s.consistent_acceleration(feahip.CG, 1e-15, 5000)
    a = s.accelerations()
    print(kind, "damped consistent acceleration", rel(a, want), "cond(M)", cond, "the damping moves it by", rel(plain, want))
    assert rel(plain, want) > 1e-3 and rel(a, want) <= A_TOL
    s.close()


# ---- d: shards and ranks ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["shards2", "ranks3"])
def test_sharded_damped_trajectory_is_the_unsharded_one(form):
    deck, rho = release_deck("tet4")
    coef = COEFFICIENTS["both"]
    one = feahip.FeaSolver(deck)
    one.set_mass(rho)
    one.set_damping(*coef)
    one.set_load_factor(1.0)
    v = np.random.default_rng(7).standard_normal(one.ndof)
    y_one = one.damping_spmv(v)
    run_release(one, "tet4", deck, 4)
    want = (one.nodes(), one.velocities(), one.accelerations())
    one.close()
    if form == "shards2":
        deck.damping = coef                                            # with the deck: taken again once the rows are cut
        g = feahip.FeaGroup(deck, 2)
    else:
        g = feahip.FeaGroup(deck, 3, rank_contexts=True)
        g.set_damping(*coef)
    assert all(rk.damping() == coef for rk in g.ranks)
    presc = set(int(p) for p in deck.presc_node)
    assert any(not (presc & set(int(a) for a in nd)) for nd in g.nodes)   # a rank that owns no prescribed node
    g.set_mass(rho)
    g.each("set_load_factor", 1.0)
    y = np.zeros((len(deck.nodes), 3))
    for rk, nd in zip(g.ranks, g.nodes):                               # the ranks' products add up to the unsharded one
        if g.rank_contexts:
            yr = rk.damping_spmv(v.reshape(-1, 3)[rk.node_global].ravel()).reshape(-1, 3)
            assert np.abs(yr[rk.n_own:]).max() == 0.0
            y[rk.node_global[:rk.n_own]] += yr[:rk.n_own]
        else:
            y += rk.damping_spmv(v).reshape(-1, 3)
    print(form, "damping_spmv", rel(y.ravel(), y_one))
    assert rel(y.ravel(), y_one) <= C_TOL
    done, its, _ = run_release(g, "tet4", deck, 4)
    assert done == 4 and list(its) == damped_release("tet4", "both")[1]
    check_state(form, g.gather("nodes"), g.gather("velocities"), g.gather("accelerations"), want, deck)
    g.consistent_acceleration(deck.solver_type, 1e-15, 5000)           # M a = f - C v at the state reached: a again
    ea = rel(g.gather("accelerations"), want[2])
    print(form, "consistent acceleration at the state reached", ea)
    assert ea <= A_TOL
    g.close()


# ---- e: explicit ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def relaxation_case():
    """(deck, alpha = 2 omega_1 of the lumped system, dt = 0.5 dt_G, 20 steps of the restatement) -- computed once."""
    deck = loaded_bar("tet4", DIMS)
    r = DampedExplicit(deck, 1.5)
    K = r.tangent()
    free = ~r.mask
    s3 = 1.0 / np.sqrt(r.ml3[free])
    alpha = 2.0 * float(np.sqrt(np.linalg.eigvalsh(K[np.ix_(free, free)] * s3[:, None] * s3[None, :]).min()))
    dt = 0.5 * r.stable_step()
    r.set_damping(alpha)
    r.lam = 1.0
    traj = r.explicit(20, dt)
    r.close()
    for st in traj:
        for arr in st:
            arr.setflags(write=False)
    return deck, alpha, dt, traj


def test_damped_explicit_steps_match_the_restatement():
    deck, alpha, dt, traj = relaxation_case()
    s = feahip.FeaSolver(deck)
    s.set_mass(1.5)
    s.set_damping(alpha, 0.0)
    s.set_load_factor(1.0)
    for k, (xw, vw, aw) in enumerate(traj):
        done, _ = s.solve_explicit(1, dt)
        assert done == 1
        x, v, a = s.nodes(), s.velocities(), s.accelerations()
        ex, ev, ea = rel(x, xw, np.abs(xw - deck.nodes).max()), rel(v, vw), rel(a, aw)
        if k in (0, len(traj) - 1):
            print("damped explicit step", k + 1, "x", ex, "v", ev, "a", ea)
        assert ex <= X_TOL and ev <= X_TOL and ea <= X_TOL
    s.close()


def test_dynamic_relaxation_reaches_the_static_solution():
    deck, alpha, dt, _ = relaxation_case()
    st = feahip.FeaSolver(deck)
    done, _, _ = st.solve(1, modified_newton=False)
    want = st.nodes()
    st.close()
    assert done == 1
    s = feahip.FeaSolver(deck)
    s.set_mass(1.5)
    s.set_damping(alpha, 0.0)
    s.set_load_factor(1.0)                                             # the traction at once
    done, _ = s.solve_explicit(1250, dt)
    err = rel(s.nodes(), want, np.abs(want - deck.nodes).max())
    print("relaxed after 1250 steps: error", err, "max|v|", np.abs(s.velocities()).max())
    assert done == 1250 and err <= RELAX_TOL
    s.close()


def test_the_explicit_loop_refuses_stiffness_proportional_damping():
    deck = loaded_bar("tet4", DIMS)
    s = feahip.FeaSolver(deck)
    s.set_mass(1.5)
    s.set_damping(0.5, 0.01)
    with pytest.raises(feahip.FeaHipError, match=r"beta_k = 0\.01") as e:
        s.solve_explicit(1, 0.001)
    assert f"error {feahip.EINVAL}:" in str(e.value)
    assert s.stable_step() > 0.0                                       # (the estimate needs no damping and takes none)
    s.close()
    g = feahip.FeaGroup(deck, 2)
    g.set_mass(1.5)
    g.ranks[1].set_damping(0.0, 0.01)                                  # one member is enough
    with pytest.raises(feahip.FeaHipError, match="beta_k"):
        g.solve_explicit(1, 0.001)
    g.close()


# ---- f: without damping -----------------------------------------------------------------------------------------------
def undamped_run(deck, how):
    s = feahip.FeaSolver(deck)
    s.set_mass(1.5)
    if how == "zero":
        s.set_damping(0.0, 0.0)
    elif how == "cleared":
        s.set_damping(0.5, 0.01)
        s.set_damping(0.0, 0.0)
    assert s.damping() == (0.0, 0.0)
    s.set_load_factor(1.0)
    assert s.solve_dynamic(3, DT, 0.25, 0.5, 0.0)[0] == 3
    out = [s.nodes(), s.velocities(), s.accelerations(), s.matrix_yale()[2]]
    assert s.solve_explicit(20, 0.002)[0] == 20
    out += [s.nodes(), s.velocities(), s.accelerations()]
    s.close()
    return out


@pytest.mark.parametrize("kind", ["tet4", "tet10", "hex8"])
def test_no_damping_changes_no_bit(kind):
    deck = loaded_bar(kind, DIMS if kind != "tet10" else (1, 2, 1))
    want = undamped_run(deck, "never")
    for how in ("zero", "cleared"):
        for a, b in zip(undamped_run(deck, how), want):
            assert np.array_equal(a, b), how


# ---- g: refusals and states -------------------------------------------------------------------------------------------
def test_refusals_and_states():
    deck = loaded_bar("tet4", (4, 12, 4))
    s = feahip.FeaSolver(deck)

    def refused(code, what, fn, *args):
        with pytest.raises(feahip.FeaHipError, match=what) as e:
            fn(*args)
        assert f"error {code}:" in str(e.value)

    for what in (21, 22):
        refused(feahip.EINVAL, rf"time_kernel\({what}\): no damping", s.time_kernel, what)
    refused(feahip.ESTATE, "no damping on this context", s.damping_spmv, np.zeros(s.ndof))
    s.set_damping(0.0, 0.01)
    v = np.random.default_rng(2).standard_normal(s.ndof)
    y = s.damping_spmv(v)
    for bad in ((-1.0, 0.0), (0.0, -1e-3), (np.nan, 0.0), (0.0, np.inf)):
        refused(feahip.EINVAL, "finite and not negative", s.set_damping, *bad)
    assert s.damping() == (0.0, 0.01) and np.array_equal(s.damping_spmv(v), y)    # the context is left as it was
    # alpha > 0 without a mass: refused where it is used
    s.set_damping(0.5, 0.01)
    refused(feahip.ESTATE, "no mass on this context", s.damping_spmv, v)
    refused(feahip.ESTATE, "no mass on this context", s.solve_dynamic, 1, DT, 0.25, 0.5, 0.0)
    refused(feahip.EINVAL, r"time_kernel\(22\): no mass", s.time_kernel, 22)
    s.set_mass(1.5)
    M = dense_mass(deck, 1.5)
    assert rel(s.damping_spmv(v), 0.5 * (M @ v) + y) <= C_TOL          # the alpha part follows the new mass
    assert s.time_kernel(21, 1, 2) > 0.0 and s.time_kernel(22, 1, 2) > 0.0
    refused(feahip.EINVAL, r"time_kernel\(21\): no damping with beta_k > 0", _with(s, 0.5, 0.0).time_kernel, 21)
    # the row shard changes under the snapshot
    s.set_damping(0.5, 0.01)
    s.set_row_shard(1, 2)
    refused(feahip.ESTATE, "row shard changed", s.damping_spmv, v)
    refused(feahip.ESTATE, "row shard changed", s.time_kernel, 22)
    refused(feahip.ESTATE, "row shard changed", s.consistent_acceleration)
    s.set_damping(0.5, 0.01)                                           # set again: the rows of the new shard
    y2 = s.damping_spmv(v).reshape(-1, 3)
    own = s.owned_nodes()
    rest = np.setdiff1d(np.arange(len(deck.nodes)), own)
    want = (0.5 * (M @ v) + y).reshape(-1, 3)
    assert 0 < len(own) < len(deck.nodes) and np.abs(y2[rest]).max() == 0.0
    assert rel(y2[own], want[own], np.abs(want).max()) <= C_TOL
    s.close()


def _with(s, alpha, beta):
    s.set_damping(alpha, beta)
    return s


# ---- h: the command line ----------------------------------------------------------------------------------------------
def test_command_line_reproduces_the_python_trajectory(tmp_path):
    deck = loaded_bar("tet4", DIMS)
    kw = {k: getattr(deck, k) for k in ("model", "parameters", "ele_type", "gauss_nodes_count", "nodes", "elements", "presc_node",
                                         "presc_type", "presc_values", "surface_faces", "surface_kind", "surface_values",
                                         "max_newton_count", "desired_tolerance", "modified_newton", "solver_type",
                                         "solver_tolerance")}
    d = feahip.Deck(**kw, density=1.5, dynamics=dict(steps=3, dt=float(DT), dlambda=1.0), damping=(0.5, 0.01))
    p = tmp_path / "damped.sexp"
    d.save(str(p))
    back = feahip.Deck.load(str(p))
    assert back.damping == (0.5, 0.01)
    s = feahip.FeaSolver(back)                                         # mass and damping come with the deck
    assert s.damping() == (0.5, 0.01)
    done, its, _ = s.solve_dynamic()
    assert done == 3
    u = s.nodes() - d.nodes
    s.close()
    plain = feahip.FeaSolver(feahip.Deck(**kw, density=1.5, dynamics=dict(steps=3, dt=float(DT), dlambda=1.0)))
    plain.solve_dynamic()
    moved = np.abs(plain.nodes() - d.nodes - u).max()
    plain.close()
    exe = os.path.join(os.path.dirname(feahip.LIB_PATH), "feasolver_hip")
    out = subprocess.run([exe, str(p)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert re.search(r"^Damping: alpha 0\.5, beta 0\.01\S*$", out.stdout, flags=re.M)
    counts = [int(m) for m in re.findall(r"Dynamic step \d+ finished: time \S+ (\d+) iterations", out.stdout)]
    assert counts == [int(k) for k in its]
    lines = (tmp_path / "damped.msh").read_text().splitlines()
    at = max(i for i, ln in enumerate(lines) if ln == "$NodeData")      # the last step's displacements
    n = len(d.nodes)
    start = next(i for i in range(at, len(lines)) if lines[i].strip() == str(n)) + 1
    got = np.array([[float(v) for v in ln.split()[1:4]] for ln in lines[start:start + n]])
    print("the damping moves the end state by", moved)
    assert moved > 1e-4 and np.abs(got - u).max() <= 1e-6              # the file holds six decimals

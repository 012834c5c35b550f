"""Random-vibration fatigue on the MI355X (kernels_stress_fatigue.hip) against the restatement of tests/fatigue_reference.py
and the library's own long-double host entry: four forms of the caller's own in one launch against four launches of the
combine kernel, bit for bit; the four spectral moments under a PSD against host_moment_form fed to the restatement; rates,
damages and status against host_fatigue at the device's own moments; the corners (one live frequency, a static PSD, a
stress basis of one material); what the entries leave of the context's state, hooks 31 and 32, stale state, refusals,
reproducibility; and feasolver_hip on a deck with the three keys."""
import os
import re
import subprocess

import numpy as np
import pytest

import fatigue_reference as fr
import feahip
from dynamics_reference import loaded_bar
from hetero_reference import MATERIALS, layered_ids, with_materials
from test_fatigue_host import relative_tolerance, within
from test_gpu_combine import _psd
from test_gpu_modal_locked import DECKS, RHO, reference, solver
from test_gpu_modal_stress import held
from test_gpu_response import CASES, _refused, rayleigh_for, tip_load

pytestmark = pytest.mark.gpu

LD = fr.LD
CURVES = ((3.0, 1e3), (5.5, 2.5e7))


def three_frequencies(lam, correction):
    """The grid of tests/test_gpu_modal_stress.py: the static point (or one well below the first mode), one near the first
    resonance, one above the last mode."""
    w1, wm = np.sqrt(lam[0]), np.sqrt(lam[-1])
    return np.array([0.0 if correction else 0.05 * w1, 0.98 * w1, 1.2 * max(wm, 2.0 * w1)])


# ---- 1. four forms of the caller's own -----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,m,correction", CASES)
def test_four_forms_against_the_restatement_and_the_combine_kernel(kind, m, correction):
    """Indefinite with b and s, semidefinite alone, negative definite with b, a positive diagonal with s: all different, so a
    wrong table offset or output stride shows in the comparison with response_stress_combine, form by form, bit by bit."""
    ref, s, lam, q, T, Ts, _ = held(kind, m, correction)
    rng = np.random.default_rng(300 + m)
    G = rng.standard_normal((m, m))
    scale = np.abs(Ts).max() / np.abs(T).max() if correction else 1.0      # so that the three terms are of one size
    sym = lambda A: (A + A.T) / 2
    forms = [(sym(G + G.T) * scale * scale, rng.standard_normal(m) * scale, 0.8),
             (sym(G @ G.T) * scale * scale, None, None),
             (-sym(G @ G.T) * scale * scale, rng.standard_normal(m) * scale, None),
             (np.diag(rng.uniform(0.5, 2.0, m)) * scale * scale, None, 1.7)]
    mom = s.response_stress_moments([f[0] for f in forms], [f[1] for f in forms], [f[2] for f in forms])
    full = [(C, np.zeros(m) if b is None else b, 0.0 if s0 is None else s0) for C, b, s0 in forms]
    want, bound, raw = fr.seven_moments(T, Ts, full)
    err = np.abs(mom - want)
    print(kind, m, "largest error / bound", (err / np.where(bound > 0, bound, 1.0)).max(), "negative beyond the bound", int((raw < -bound).sum()))
    assert mom.shape == (len(T[0]), 7, 4) and np.all(err <= bound) and np.all(mom >= 0)
    assert (raw < -bound).any() and not mom[raw < -bound].any()          # exactly 0 where the form is negative
    assert np.array_equal(mom, s.response_stress_moments([f[0] for f in forms], [f[1] for f in forms], [f[2] for f in forms]))
    for k, (C, b, s0) in enumerate(full):
        out6, vm = s.response_stress_combine(C, b, s0)
        assert np.array_equal(np.sqrt(mom[:, :6, k]), out6) and np.array_equal(np.sqrt(mom[:, 6, k]), vm), k
    # b4 and s4 left out altogether
    plain = s.response_stress_moments([f[0] for f in forms])
    want0, bound0, _ = fr.seven_moments(T, Ts, [(C, np.zeros(m), 0.0) for C, _, _ in forms])
    assert np.all(np.abs(plain - want0) <= bound0) and np.array_equal(plain[:, :, 1], mom[:, :, 1])
    s.close()


# ---- 2. under a PSD ------------------------------------------------------------------------------------------------------
def close(name, got, ref, plain, exact):
    """Every entry of got within relative_tolerance(plain, exact) of ref, relative to ref."""
    tol, gap = relative_tolerance(plain, exact)
    err = np.abs(got - ref)
    worst = float((err / np.where(ref != 0, np.abs(ref), 1.0)).max()) if ref.size else 0.0
    print(f"{name}: relative error {worst:.3e}, float64 gap {gap:.3e}, tolerance {tol:.3e}")
    assert np.all(err <= tol * np.abs(ref))


def check_statistics(what, mom, rates, damage, status, b, A, limit=0.02):
    """rates, damage and status of the device against host_fatigue at the device's own moments: status equal, values within
    100 times the float64-to-long-double gap of the restatement at those moments (at least 1e-13, at most 1e-10), a pair
    excused only where the long-double alpha2 or a Dirlik parameter lies within 1e-9 of its threshold."""
    hr, hd, hs = feahip.host_fatigue(mom, b, A)
    er, ed, es, near = fr.fatigue(mom, b, A, LD)
    pr, pd, _, _ = fr.fatigue(mom, b, A, np.float64)
    keep = ~near
    print(what, "pairs", status.size, "excused", int(near.sum()), "status counts", np.bincount(status.reshape(-1), minlength=5))
    assert near.sum() <= limit * status.size
    assert np.array_equal(status[keep], hs[keep]) and np.array_equal(hs[keep], es[keep])
    assert np.all(np.isfinite(rates)) and np.all(np.isfinite(damage))
    for k, name in enumerate(("nu0", "nup")):
        within(f"{what} {name} (host entry against the restatement)", hr[keep][:, k], er[keep][:, k], pr[keep][:, k])
        close(f"{what} {name}", rates[keep][:, k], hr[keep][:, k], pr[keep][:, k], er[keep][:, k])
    for k, name in enumerate(feahip.FATIGUE_DAMAGE):
        within(f"{what} {name} (host entry against the restatement)", hd[keep][:, k], ed[keep][:, k], pd[keep][:, k])
        close(f"{what} {name}", damage[keep][:, k], hd[keep][:, k], pd[keep][:, k], ed[keep][:, k])
    return hs


@pytest.mark.parametrize("kind,m,correction", CASES)
def test_moments_and_statistics_under_a_psd(kind, m, correction):
    ref, s, lam, q, T, Ts, (alpha, beta) = held(kind, m, correction)
    omega, S = three_frequencies(lam, correction), np.array([1.0, 2.0, 0.5])
    forms = [feahip.host_moment_form(lam, q, omega, S, alpha, beta, None, correction, order) for order in fr.ORDERS]
    want, bound, raw = fr.seven_moments(T, Ts, forms)
    # on the CPU, before the device is asked: the restatement excuses no pair on these inputs
    for b, A in CURVES:
        assert not fr.fatigue(want, b, A, LD)[3].any()
    rms6, rvm, _ = s.response_stress_random(omega, S, alpha, beta)
    for b, A in CURVES:
        mom, rates, damage, status = s.response_stress_fatigue(omega, S, alpha, beta, None, b, A)
        assert np.array_equal(np.sqrt(mom[:, :6, 0]), rms6) and np.array_equal(np.sqrt(mom[:, 6, 0]), rvm)
        err = np.abs(mom - want)
        print(kind, m, "moments: largest error / bound by order", [(err[..., k] / np.where(bound[..., k] > 0, bound[..., k], 1.0)).max() for k in range(4)])
        assert np.all(err <= bound) and np.all(mom >= 0)
        hs = check_statistics(f"{kind} {m} b {b}", mom, rates, damage, status, b, A)
        live = hs != feahip.FATIGUE_NO_STRESS
        assert live.any() and np.all(damage[live][:, 2] <= damage[live][:, 0])
        again = s.response_stress_fatigue(omega, S, alpha, beta, None, b, A)
        for x, y in zip((mom, rates, damage, status), again):
            assert np.array_equal(x, y)                                  # the same bits on every call
    s.close()


# ---- 3. corners ------------------------------------------------------------------------------------------------------------
def test_one_live_frequency_and_a_static_psd():
    kind, m, correction = CASES[1]
    ref, s, lam, q, T, Ts, (alpha, beta) = held(kind, m, correction)
    omega = three_frequencies(lam, correction)
    b, A = CURVES[0]
    # the interior point alone: m_n = w^n m0 up to rounding, alpha2 = 1
    mom, rates, damage, status = s.response_stress_fatigue(omega, [0.0, 2.0, 0.0], alpha, beta, None, b, A)
    live = status != feahip.FATIGUE_NO_STRESS
    print("one frequency: stressed pairs", int(live.sum()), "of", status.size)
    assert live.sum() > 0.5 * status.size and np.all(status[live] == feahip.FATIGUE_NARROW)
    assert np.all(damage[live][:, 0] == damage[live][:, 1]) and np.all(damage[live][:, 0] == damage[live][:, 2]) and np.all(damage[live] > 0)
    assert np.all(np.abs(rates[live] - omega[1] / (2 * np.pi)) <= 1e-7 * omega[1])
    assert not rates[~live].any() and not damage[~live].any()
    check_statistics("one frequency", mom, rates, damage, status, b, A)
    # the static point alone (with the correction): m0 > 0 and nothing else
    assert correction and omega[0] == 0.0
    mom, rates, damage, status = s.response_stress_fatigue(omega, [1.0, 0.0, 0.0], alpha, beta, None, b, A)
    assert mom[..., 0].max() > 0 and not mom[..., 1:].any()
    assert np.all(status == feahip.FATIGUE_NO_STRESS) and not rates.any() and not damage.any()
    s.close()


def test_a_stress_basis_of_one_material():
    """The layered body of test_selection_by_material with three vectors of no physical meaning as the modes held: the
    pairs of the nodes outside the material have zero rows in the store and in T_s."""
    base = loaded_bar("tet4", (2, 4, 2))
    ids = layered_ids(base)
    deck = with_materials(base, MATERIALS, ids)
    n = len(deck.nodes)
    phi = np.random.default_rng(7).standard_normal((3, n, 3))
    s = solver(deck)
    s.response_set_basis([4.0, 9.0, 25.0], phi.reshape(3, -1))
    s.response_load(tip_load(deck), True, feahip.CG, 1e-14, 20000)
    s.response_stress_basis(1)
    omega, S = np.array([0.0, 1.9, 7.0]), np.array([1.0, 2.0, 0.5])
    mom, rates, damage, status = s.response_stress_fatigue(omega, S, 0.1, 0.0, None, *CURVES[0])
    outside = ~np.isin(np.arange(n), deck.elements[ids == 1])
    assert outside.any() and not outside.all()
    assert not mom[outside].any() and not rates[outside].any() and not damage[outside].any()
    assert np.all(status[outside] == feahip.FATIGUE_NO_STRESS) and np.all(status[~outside][:, 6] != feahip.FATIGUE_NO_STRESS)
    for a in (mom, rates, damage):
        assert np.all(np.isfinite(a))
    assert damage[~outside][:, 6].min() > 0
    check_statistics("one material", mom, rates, damage, status, *CURVES[0])
    s.close()


# ---- 4. state, hooks, stale state, refusals, reproducibility -------------------------------------------------------------------
def _run(deck, ref, m, omega, S, alpha, beta):
    s = solver(deck)
    s.response_set_basis(ref.lam[:m], ref.Phi[:, :m].T)
    s.response_base_load((1.0, 0.5, 0.0), True, feahip.CG, 1e-14, 20000)
    s.response_stress_basis()
    out = (*s.response_stress_fatigue(omega, S, alpha, beta, 0.01, *CURVES[1]),
           s.response_stress_moments(np.stack([np.eye(m) * (k + 1) for k in range(4)]), np.ones((4, m)), np.ones(4)))
    s.close()
    return out


def test_state_is_left_alone_and_two_cold_runs_agree():
    kind, m = "tet4", 24
    ref, deck = reference(kind), DECKS[kind]()
    alpha, beta = rayleigh_for(ref, m)
    omega = np.linspace(0.0, 1.2 * np.sqrt(ref.lam[m - 1]), 33)
    S = _psd(omega)
    rng = np.random.default_rng(2)
    s = solver(deck)
    s.set_velocities(rng.standard_normal((s.N, 3)))
    s.set_accelerations(rng.standard_normal((s.N, 3)))
    s.set_time(0.375)
    s.set_load_factor(0.5)
    s.response_set_basis(ref.lam[:m], ref.Phi[:, :m].T)
    s.response_base_load((1.0, 0.5, 0.0), True, feahip.CG, 1e-14, 20000)
    state = lambda: (s.nodes(), s.velocities(), s.accelerations(), np.array(s.time()), np.array(s.load_factor()), s.locked_modes(),
                     s.response_static(), s.forces(), s.solution(), s.matrix_yale()[2])
    sweep = s.response_sweep(omega[:9], alpha, beta, 0.01)
    combined = s.response_combine(np.eye(m), np.ones(m), 1.0)
    s.response_stress_basis()
    stress_combined = s.response_stress_combine(np.eye(m), np.ones(m), 1.0)
    store = (s.modal_stresses(), s.response_static_stress())
    before = state()
    C4 = np.stack([np.eye(m) * (k + 1) for k in range(4)])
    for entry in (lambda: s.response_stress_moments(C4, np.ones((4, m)), np.ones(4)),
                  lambda: s.response_stress_fatigue(omega, S, alpha, beta, 0.01, *CURVES[0])):
        entry()
        for a, b in zip(before, state()):
            assert np.array_equal(a, b)
        assert all(np.array_equal(a, b) for a, b in zip(store, (s.modal_stresses(), s.response_static_stress())))
        assert s.time_kernel(23, 1, 2) > 0.0 and s.time_kernel(26, 1, 2) > 0.0 and s.time_kernel(28, 1, 2) > 0.0
    assert s.time_kernel(31, 1, 2) > 0.0 and s.time_kernel(32, 1, 2) > 0.0
    for a, b in zip(before, state()):
        assert np.array_equal(a, b)
    for a, b in zip(sweep, s.response_sweep(omega[:9], alpha, beta, 0.01)):
        assert np.array_equal(a, b)
    assert np.array_equal(combined, s.response_combine(np.eye(m), np.ones(m), 1.0))
    for a, b in zip(stress_combined, s.response_stress_combine(np.eye(m), np.ones(m), 1.0)):
        assert np.array_equal(a, b)
    s.close()
    for a, b in zip(_run(deck, ref, m, omega, S, alpha, beta), _run(deck, ref, m, omega, S, alpha, beta)):
        assert np.array_equal(a, b)


def test_refusals_stale_state_and_hooks():
    kind = "tet4"
    ref, deck = reference(kind), DECKS[kind]()
    F = tip_load(deck)
    lam, phi = np.array([9.0, 4.0, 25.0]), ref.Phi[:, :3].T.copy()
    C4, omega, S = np.stack([np.eye(3)] * 4), np.array([0.5, 1.0, 1.5]), np.ones(3)
    s = solver(deck)
    moments = lambda: s.response_stress_moments(C4)
    fatigue = lambda: s.response_stress_fatigue(omega, S, 0.1, 0.0, None, 3.0, 1e3)
    hooks = (lambda: s.time_kernel(31, 1, 1), lambda: s.time_kernel(32, 1, 1))
    for call in (moments, fatigue, *hooks):
        assert "no modes held" in _refused(s, feahip.ESTATE, call)
    s.response_set_basis(lam, phi)
    s.response_stress_basis()                                            # without a load
    for call in (moments, fatigue, *hooks):
        assert "no load held" in _refused(s, feahip.ESTATE, call)
    s.response_load(F, True)                                             # a new load: T_s is stale
    for call in (moments, fatigue, *hooks):
        assert "a load was made" in _refused(s, feahip.ESTATE, call)
    s.response_stress_basis()
    assert "no stress moments" in _refused(s, feahip.ESTATE, hooks[0])
    assert "no fatigue rates" in _refused(s, feahip.ESTATE, hooks[1])
    assert np.isfinite(moments()).all()
    assert s.time_kernel(31, 1, 2) > 0.0
    assert "no fatigue rates" in _refused(s, feahip.ESTATE, hooks[1])   # moments, but no S-N curve yet
    assert all(np.isfinite(a).all() for a in fatigue())
    assert s.time_kernel(31, 1, 2) > 0.0 and s.time_kernel(32, 1, 2) > 0.0
    # the S-N curve
    for b, A in ((0.999, 1e3), (64.001, 1e3), (np.nan, 1e3), (np.inf, 1e3), (3.0, 0.0), (3.0, -1.0), (3.0, np.inf), (3.0, np.nan)):
        assert "S-N curve" in _refused(s, feahip.EINVAL, lambda: s.response_stress_fatigue(omega, S, 0.1, 0.0, None, b, A))
    assert all(np.isfinite(a).all() for a in s.response_stress_fatigue(omega, S, 0.1, 0.0, None, 1.0, 1e-3))
    assert all(np.isfinite(a).all() for a in s.response_stress_fatigue(omega, S, 0.1, 0.0, None, 64.0, 1e300))
    # what response_stress_random and response_stress_combine refuse
    _refused(s, feahip.EINVAL, lambda: s.response_stress_fatigue(omega[::-1], S, 0.1, 0.0, None, 3.0, 1e3))
    _refused(s, feahip.EINVAL, lambda: s.response_stress_fatigue(omega, -S, 0.1, 0.0, None, 3.0, 1e3))
    _refused(s, feahip.EINVAL, lambda: s.response_stress_fatigue(omega, S, -0.1, 0.0, None, 3.0, 1e3))
    bad = C4.copy()
    bad[2, 0, 1] = 1e-300
    assert "symmetric" in _refused(s, feahip.EINVAL, lambda: s.response_stress_moments(bad))
    assert "not finite" in _refused(s, feahip.EINVAL, lambda: s.response_stress_moments(C4, [None, None, [0.0, np.nan, 0.0], None]))
    assert "not finite" in _refused(s, feahip.EINVAL, lambda: s.response_stress_moments(C4, None, [0.0, 0.0, 0.0, np.inf]))
    assert s.time_kernel(31, 1, 2) > 0.0 and s.time_kernel(32, 1, 2) > 0.0   # a refused call leaves the last forms in force
    # a new basis drops the moments: the store is another one
    s.response_stress_basis()
    assert "no stress moments" in _refused(s, feahip.ESTATE, hooks[0])
    assert "no fatigue rates" in _refused(s, feahip.ESTATE, hooks[1])
    fatigue()
    # whatever fills the locked store invalidates the stress store, and with it these entries
    s.response_set_basis(lam, phi)
    s.response_load(F, False)
    for call in (moments, fatigue, *hooks):
        assert "no stress store" in _refused(s, feahip.ESTATE, call)
    s.response_stress_basis()
    assert np.isfinite(moments()).all()
    # a row shard, a rank context
    s.set_row_shard(0, 2)
    for call in (moments, fatigue, *hooks):
        assert "row-sharded" in _refused(s, feahip.EINVAL, call)
    s.close()
    r = feahip.RankSolver(deck, 0, 2)
    assert "feahip_create_rank" in _refused(r, feahip.EINVAL, lambda: r.response_stress_moments(C4))
    r.close()


# ---- 5. the command line --------------------------------------------------------------------------------------------------
def test_feasolver_hip_runs_a_deck_with_the_fatigue_keys(tmp_path):
    """The (3, 8, 3) TET4 bar of the :stress t test, (random ...) with :base and the three keys: the log line, the two
    one-component $NodeData sections behind everything else, the damage field against response_stress_fatigue on the same
    state to the ten digits of the file, and without the keys the old output byte for byte."""
    def make(**kw):
        d = loaded_bar("tet4", (3, 8, 3), density=RHO, modal_count=12, load_increments_count=1, **kw)
        d.surface_values = np.tile([0.05, 0.015, 0.0], (len(d.surface_kind), 1))
        return d
    section = dict(random_points=[(0.0, 0.0), (0.5, 1.0), (4.0, 1.0), (5.0, 0.0)], random_zeta=0.02, random_per_mode=8,
                   random_background=33, random_base=(1.0, 0.0, 0.0), random_stress=True)
    b, A, duration = 4.0, 1e6, 3600.0
    decks = {"old": make(**section), "fatigue": make(**section, random_sn_exponent=b, random_sn_coefficient=A, random_duration=duration)}
    exe = os.path.join(os.path.dirname(feahip.LIB_PATH), "feasolver_hip")
    out = {}
    for name, d in decks.items():
        path = tmp_path / f"{name}.sexp"
        d.save(str(path))
        out[name] = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
        assert out[name].returncode == 0, out[name].stderr
    old = (tmp_path / "old.msh").read_text()
    new = (tmp_path / "fatigue.msh").read_text()
    assert "fatigue" not in out["old"].stdout and "Fatigue" not in old
    keep = "".join(l for l in out["fatigue"].stdout.splitlines(True) if not l.startswith("Random fatigue:"))
    assert keep == out["old"].stdout
    assert new.startswith(old)
    n_nodes = len(decks["old"].nodes)
    titles = re.findall(r'^"([^"]+)"$', new[len(old):], re.M)
    assert titles == ["Fatigue damage (Dirlik)", "Zero-upcrossing rate"]
    hit = re.search(r"^Random fatigue: damage = (\S+) \(Dirlik\), node (\d+), nu0 = (\S+), life = (\S+)$", out["fatigue"].stdout, re.M)
    assert hit, out["fatigue"].stdout
    got = {}
    for title in titles:
        body = new[new.index(f'"{title}"'):].splitlines()
        assert body[5] == "1" and body[6] == str(n_nodes) and body[7 + n_nodes] == "$EndNodeData"
        got[title] = np.array([float(l.split()[1]) for l in body[7:7 + n_nodes]])
    D, node, nu0, life = float(hit.group(1)), int(hit.group(2)), float(hit.group(3)), float(hit.group(4))
    print("damage", D, "node", node, "nu0", nu0, "life", life)
    rows = got["Fatigue damage (Dirlik)"]
    assert D > 0 and abs(rows.max() - D) <= 1e-9 * D and abs(rows[node - 1] - D) <= 1e-9 * D
    assert abs(got["Zero-upcrossing rate"][node - 1] - nu0) <= 1e-9 * nu0 and abs(life * D - duration) <= 1e-12 * duration
    # the Python entries on the state the command line reached: the solved nodes, its modes, the base load
    d = decks["fatigue"]
    s = feahip.FeaSolver(d)
    s.set_mass(RHO)
    done, _, _ = s.solve(load_increments=1)
    assert done == 1
    lam = s.solve_modes_locked(12, 0.0, d.modal_tolerance, d.modal_max)[0]
    s.response_base_load((1.0, 0.0, 0.0), True)
    s.response_stress_basis()
    two_pi = 6.283185307179586
    wr, Sr = two_pi * d.random_points[:, 0], d.random_points[:, 1] / two_pi
    grid = feahip.host_random_grid(lam, 0.0, 0.0, 0.02, wr[0], wr[-1], d.random_background, d.random_per_mode, wr)
    _, rates, damage, status = s.response_stress_fatigue(grid, feahip.host_psd_value(wr, Sr, grid), 0.0, 0.0, 0.02, b, A)
    for title, mine in (("Fatigue damage (Dirlik)", duration * damage[:, 6, 1]), ("Zero-upcrossing rate", rates[:, 6, 0])):
        want = got[title]
        print(title, "command line against Python", np.abs(mine - want).max() / want.max())
        assert np.all(np.abs(mine - want) <= 1e-9 * want.max())
    assert not (status[:, 6] & feahip.FATIGUE_NO_STRESS).any()
    s.close()

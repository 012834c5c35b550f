"""Stress from mode superposition on the MI355X (kernels_modal_stress.hip, kernels_stress_combine.hip) against the float64
restatement of tests/stress_reference.py: the linearised nodal stress of one vector at moved nodes, the selection by
material, the stress store of one to sixty-four modes and T_s, the nine-form von Mises combination, the RMS under a PSD
against the trapezoid rule over the stresses of the sweep's fields, the rules of a response spectrum, the library's own
nodal stresses differenced, what the entries leave of the context's state, reproducibility, stale state, refusals and
hooks 27 and 28, and feasolver_hip on a deck with :stress t in both sections.

T_s equals stress_increment(u_s) to the bit: both go through the same kernels as a panel with one live column."""
import os
import re
import subprocess

import numpy as np
import pytest

import combine_reference as cr
import feahip
import stress_reference as sr
from dynamics_reference import loaded_bar
from hetero_reference import MATERIALS, layered_ids, with_materials
from response_reference import EPS
from results_reference import smooth_field, von_mises
from test_gpu_combine import SPECTRUM_SA, SPECTRUM_W, _psd
from test_gpu_modal_locked import DECKS, RHO, reference, solver
from test_gpu_response import CASES, _refused, rayleigh_for, tip_load
from test_gpu_transient import half_sine, loaded, period
from test_stress_reference_cpu import GAP_STEP, difference_gap

pytestmark = pytest.mark.gpu

MODELS = {"neohookean": feahip.MODEL_COMPRESSIBLE_NEOHOOKEAN, "a5": feahip.MODEL_A5}


def check_nodal(what, r, got, want, A):
    bound = r.bound(A)
    err = np.abs(got - want)
    print(what, "largest error / bound", (err / np.where(bound > 0, bound, 1.0)).max(), "chain", r.chain())
    assert got.shape == want.shape and np.all(err <= bound)


# ---- 1. one vector ---------------------------------------------------------------------------------------------------
INCREMENTS = [("fan", "neohookean")] + [(k, m) for k in ("tet10", "hex8") for m in sorted(MODELS)]


@pytest.mark.parametrize("kind,model", INCREMENTS)
def test_stress_increment_against_the_restatement(kind, model):
    """The fan's 143 nodes leave a partial last wave and its hub has 280 visits: many rounds of the node pass.  TET10
    (2, 4, 2) and HEX8 (3, 8, 3) with both models; the nodes moved by smooth_field(nodes, 0.12)."""
    deck = DECKS["fan"]() if kind == "fan" else loaded_bar(kind, (2, 4, 2) if kind == "tet10" else (3, 8, 3), model=MODELS[model])
    s = feahip.FeaSolver(deck)
    s.set_nodes(smooth_field(deck.nodes, 0.12))
    x = s.nodes()
    du = 0.1 * np.random.default_rng(21).standard_normal(3 * len(deck.nodes))
    r = sr.StressRestatement(deck)
    want, A = r.nodal(x, du[None, :])
    got = s.stress_increment(du)
    check_nodal(f"{kind} {model}", r, got, want[0], A[0])
    assert np.abs(got).max() > 0 and np.array_equal(got, s.stress_increment(du))
    assert np.array_equal(x, s.nodes())
    r.close()
    s.close()


def test_selection_by_material():
    base = loaded_bar("tet4", (2, 4, 2))
    ids = layered_ids(base)
    deck = with_materials(base, MATERIALS, ids)
    s = feahip.FeaSolver(deck)
    s.set_nodes(smooth_field(deck.nodes, 0.12))
    x = s.nodes()
    du = 0.1 * np.random.default_rng(22).standard_normal(3 * len(deck.nodes))
    r = sr.StressRestatement(deck)
    for material in (-1, 1):
        want, A = r.nodal(x, du[None, :], material)
        got = s.stress_increment(du, material)
        check_nodal(f"material {material}", r, got, want[0], A[0])
        if material >= 0:
            outside = ~np.isin(np.arange(len(deck.nodes)), deck.elements[ids == material])
            assert outside.any() and not outside.all() and not got[outside].any() and got[~outside].any(axis=1).all()
    for bad in (len(MATERIALS), -2):
        _refused(s, feahip.EINVAL, lambda: s.stress_increment(du, bad))
    r.close()
    s.close()


# ---- 2. the stress store -----------------------------------------------------------------------------------------------
def moved(deck):
    return smooth_field(deck.nodes, 0.12)


@pytest.mark.parametrize("kind,m,correction", CASES)
def test_stress_basis_against_the_restatement(kind, m, correction):
    """A single column, a full panel, a partial last panel, three panels and all eight, at moved nodes (a prestressed
    state): every column against the restatement of that column, T_s to the bit stress_increment(u_s)."""
    ref, s, lam, Phi, q, u_s, _ = loaded(kind, m, correction)
    deck = DECKS[kind]()
    s.set_nodes(moved(deck))
    x = s.nodes()
    s.response_stress_basis()
    T, Ts = s.modal_stresses(), s.response_static_stress()
    r = sr.StressRestatement(deck)
    want, A = r.nodal(x, np.vstack([Phi.T, u_s[None, :]]))
    check_nodal(f"{kind} {m} modes", r, T, want[:m], A[:m])
    check_nodal(f"{kind} {m} T_s", r, Ts, want[m], A[m])
    assert np.array_equal(Ts, s.stress_increment(u_s))
    assert correction == bool(Ts.any())
    assert np.array_equal(T[1:3], s.modal_stresses(1, min(2, m - 1)))
    r.close()
    s.close()


def test_a_permuted_installation_returns_the_modes_by_ascending_lam():
    kind, m = "tet4", 20
    ref, deck = reference(kind), DECKS[kind]()
    lam, Phi = ref.lam[:m], ref.Phi[:, :m]
    perm = np.random.default_rng(3).permutation(m)
    a, b = solver(deck), solver(deck)
    a.response_set_basis(lam, Phi.T)
    b.response_set_basis(lam[perm], Phi.T[perm])
    a.response_stress_basis()
    b.response_stress_basis()
    assert np.array_equal(a.modal_stresses(), b.modal_stresses())
    coef = np.random.default_rng(4).standard_normal(m)
    fa, fb = a.response_stress_field(coef), b.response_stress_field(coef)
    T = a.modal_stresses()
    sig6, vm = sr.field(T, None, coef)
    slack = (m + 2) * EPS * np.einsum("k,kac->ac", np.abs(coef), np.abs(T))
    assert np.all(np.abs(fa[0] - sig6) <= slack) and np.all(np.abs(fb[0] - sig6) <= slack)
    assert np.all(np.abs(fa[1] - vm) <= 1e-13 * vm.max() + 8 * np.abs(slack).sum(axis=1))
    a.close()
    b.close()


# ---- 3. the forms ------------------------------------------------------------------------------------------------------
def held(kind, m, correction):
    ref, s, lam, Phi, q, u_s, damping = loaded(kind, m, correction)
    s.response_stress_basis()
    return ref, s, lam, q, s.modal_stresses(), s.response_static_stress(), damping


def check_forms(what, T, Ts, form, absolute, out6, vm):
    """out6^2 and vm^2 within the restatement's bounds of max(v, 0), exactly 0 where the form is negative beyond the
    bound.  Returns the number of such values."""
    v6, b6, vvm, bvm = sr.stress_combine(T, Ts, *form, absolute)
    e6 = np.abs(out6 * out6 - np.maximum(v6, 0.0))
    print(what, "out6^2: largest error / bound", (e6 / np.where(b6 > 0, b6, 1.0)).max())
    assert out6.shape == v6.shape and np.all(e6 <= b6) and not out6[v6 < -b6].any() and np.all(out6 >= 0)
    negative = int((v6 < -b6).sum())
    if vm is not None:
        ev = np.abs(vm * vm - np.maximum(vvm, 0.0))
        print(what, "vm^2: largest error / bound", (ev / np.where(bvm > 0, bvm, 1.0)).max())
        assert vm.shape == vvm.shape and np.all(ev <= bvm) and not vm[vvm < -bvm].any() and np.all(vm >= 0)
        negative += int((vvm < -bvm).sum())
    return negative


@pytest.mark.parametrize("kind,m,correction", CASES)
def test_stress_combine_against_the_restatement(kind, m, correction):
    ref, s, lam, q, T, Ts, _ = held(kind, m, correction)
    rng = np.random.default_rng(200 + m)
    G = rng.standard_normal((m, m))
    b, s0 = rng.standard_normal(m), 0.8
    scale = np.abs(Ts).max() / np.abs(T).max() if correction else 1.0      # so that the three terms are of one size
    negative = 0
    # (one column: a 1 x 1 C has one sign, so a negative definite one stands beside the two, and every form is negative)
    for name, Cm in (("indefinite", G + G.T), ("semidefinite", G @ G.T)) + ((("negative definite", -(G @ G.T)),) if m == 1 else ()):
        Cm = (Cm + Cm.T) / 2
        form = (Cm * scale * scale, b * scale, s0)
        out6, vm = s.response_stress_combine(*form)
        negative += check_forms(f"{kind} {m} {name}", T, Ts, form, False, out6, vm)
        again = s.response_stress_combine(*form)
        assert np.array_equal(out6, again[0]) and np.array_equal(vm, again[1])   # the same bits on every call
    assert negative > 0                                                 # some values did come out negative, and exactly 0
    # rank one: the von Mises stress of the combination feahip_response_stress_field returns
    a = rng.standard_normal(m)
    out6, vm = s.response_stress_combine(np.outer(a, a))
    sig6, fvm = s.response_stress_field(a)
    v6, b6, vvm, bvm = sr.stress_combine(T, None, np.outer(a, a))
    slack = (m + 2) * EPS * np.einsum("k,kac->ac", np.abs(a), np.abs(T))
    assert np.all(np.abs(out6 * out6 - sig6 * sig6) <= b6 + 2 * np.abs(sig6) * slack + slack ** 2)
    vslack = 12 * von_mises(np.abs(sig6)) * np.abs(slack).sum(axis=1) + 16 * EPS * fvm * fvm
    assert np.all(np.abs(vm * vm - fvm * fvm) <= bvm + vslack)
    s.close()


@pytest.mark.parametrize("kind,m,correction", [CASES[1], CASES[3]])
def test_random_vibration_against_the_trapezoid_rule_over_the_fields(kind, m, correction):
    """Three frequencies.  rms6^2 and rms_vm^2 against the form of host_random_form, and against sum_j wt_j S_j of the
    squared stresses (von Mises: of the real and of the imaginary part) the restatement gives for the fields of
    feahip_response_field, within the bound of the form plus that of the restatement on either part."""
    ref, s, lam, q, T, Ts, (alpha, beta) = held(kind, m, correction)
    deck = DECKS[kind]()
    w1, wm = np.sqrt(lam[0]), np.sqrt(lam[-1])
    omega = np.array([0.0 if correction else 0.05 * w1, 0.98 * w1, 1.2 * max(wm, 2.0 * w1)])
    S = np.array([1.0, 2.0, 0.5])
    form = feahip.host_random_form(lam, q, omega, S, alpha, beta, None, correction, 0)
    rms6, rvm, cov = s.response_stress_random(omega, S, alpha, beta)
    assert np.array_equal(cov, form[0])
    check_forms(f"{kind} {m} random", T, Ts, form, False, rms6, rvm)
    v6, b6, vvm, bvm = sr.stress_combine(T, Ts, *form)
    r = sr.StressRestatement(deck)
    g = cr.trapezoid_weights(omega) * S
    tot6, totv, sl6, slv = np.zeros_like(rms6), np.zeros_like(rvm), np.zeros_like(rms6), np.zeros_like(rvm)
    # every column of the store is within bound(A_k) of the restatement's, so a combination is within sum_k |c_k| bound(A_k)
    _, Acol = r.nodal(deck.nodes, np.vstack([ref.Phi[:, :m].T, s.response_static()[None, :]]))
    coef = feahip.host_response_coefficients(lam, q, omega, alpha, beta, None, correction)
    for j, w in enumerate(omega):
        u = s.response_field(w, alpha, beta)
        parts, Ap = r.nodal(deck.nodes, np.vstack([u.real, u.imag]))
        for p in (0, 1):
            c = np.abs(coef[j, :m].real if p == 0 else coef[j, :m].imag)
            delta = 2 * (r.bound(Ap[p]) + r.bound(np.einsum("k,kac->ac", c, Acol[:m]) + (p == 0) * correction * Acol[m]))
            tot6 += g[j] * parts[p] ** 2
            sl6 += g[j] * (2 * np.abs(parts[p]) * delta + delta ** 2)
            vmp = von_mises(parts[p])
            totv += g[j] * vmp ** 2
            dv = 3 * np.abs(delta).sum(axis=1)
            slv += g[j] * (2 * vmp * dv + dv ** 2)
    ratio = lambda err, bound: (err / np.where(bound > 0, bound, 1.0)).max()
    print("against the fields: largest error / bound", ratio(np.abs(rms6 ** 2 - tot6), b6 + sl6 + 8 * EPS * tot6),
          ratio(np.abs(rvm ** 2 - totv), bvm + slv + 8 * EPS * totv))
    assert np.all(np.abs(rms6 ** 2 - tot6) <= b6 + sl6 + 8 * EPS * tot6)
    assert np.all(np.abs(rvm ** 2 - totv) <= bvm + slv + 8 * EPS * totv)
    r.close()
    s.close()


@pytest.mark.parametrize("kind,m,correction", CASES)
def test_spectrum_rules(kind, m, correction):
    """SRSS and CQC against host_spectrum_form fed to the restatement; ABS on the magnitudes of the components, and refused
    with a von Mises output."""
    ref, s, lam, q, T, Ts, (alpha, beta) = held(kind, m, correction)
    top = SPECTRUM_W * (np.sqrt(lam[-1]) / 40.0)
    sa = feahip.host_spectrum_value(top, SPECTRUM_SA, np.sqrt(lam), loglog=True)
    for rule in (feahip.SRSS, feahip.CQC, feahip.ABS):
        zpa = 0.5 if correction and rule != feahip.ABS else 0.0
        peak6, pvm, a = s.response_stress_spectrum(top, SPECTRUM_SA, rule, alpha, beta, 0.03, zpa, loglog=True)
        assert np.all(np.abs(a - cr.modal_peaks(lam, q, sa, 0)) <= 8 * EPS * np.abs(a))
        form = feahip.host_spectrum_form(lam, q, sa, rule, alpha, beta, np.full(m, 0.03), correction, zpa, 0)
        assert (pvm is None) == (rule == feahip.ABS)
        check_forms(f"{kind} {m} rule {rule}", T, Ts, form, rule == feahip.ABS, peak6, pvm)
        assert peak6.max() > 0
    assert "ABS" in _refused(s, feahip.EINVAL, lambda: s.response_stress_spectrum(top, SPECTRUM_SA, feahip.ABS, alpha, beta, 0.03,
                                                                                  loglog=True, von_mises=True))
    s.close()


# ---- 4. the library's own nodal stresses, differenced ----------------------------------------------------------------------
def test_central_difference_of_the_nodal_stresses_at_the_reference_configuration():
    """TET4 (1, 3, 1) at x = X0: within 10 times the gap tests/test_stress_reference_cpu.py records for the same mesh,
    increment and step."""
    deck = loaded_bar("tet4", (1, 3, 1))
    du, T, gap, _ = difference_gap("tet4")
    s = feahip.FeaSolver(deck)
    got = s.stress_increment(du)
    step = GAP_STEP * du.reshape(-1, 3)
    s.set_nodes(deck.nodes + step)
    hi = s.nodal_stresses()[0]
    s.set_nodes(deck.nodes - step)
    lo = s.nodal_stresses()[0]
    err = np.abs((hi - lo) / (2 * GAP_STEP) - got).max()
    print("difference of the library's nodal stresses against stress_increment", err, "recorded gap", gap)
    assert err <= 10 * gap
    s.close()


# ---- 5. state, reproducibility, stale state, refusals, hooks -----------------------------------------------------------------
def _run(deck, ref, m, omega, S, alpha, beta):
    s = solver(deck)
    s.response_set_basis(ref.lam[:m], ref.Phi[:, :m].T)
    s.response_base_load((1.0, 0.5, 0.0), True, feahip.CG, 1e-14, 20000)
    s.response_stress_basis()
    out = (s.modal_stresses(), s.response_static_stress(), *s.response_stress_random(omega, S, alpha, beta, 0.01),
           *s.response_stress_spectrum(SPECTRUM_W, SPECTRUM_SA, feahip.CQC, alpha, beta, 0.01, 0.5)[::2],
           s.response_stress_spectrum(SPECTRUM_W, SPECTRUM_SA, feahip.ABS, alpha, beta, 0.01)[0],
           *s.response_stress_field(np.linspace(-1.0, 1.0, m), 0.3))
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

    def every_stress_entry():
        s.stress_increment(np.ones(3 * len(deck.nodes)))
        s.response_stress_basis()
        s.modal_stresses()
        s.response_static_stress()
        s.response_stress_field(np.ones(m), 1.0)
        s.response_stress_combine(np.eye(m), np.ones(m), 1.0)
        s.response_stress_random(omega, S, alpha, beta, 0.01)
        s.response_stress_spectrum(SPECTRUM_W, SPECTRUM_SA, feahip.CQC, alpha, beta, 0.01, 0.5)
        s.response_stress_spectrum(SPECTRUM_W, SPECTRUM_SA, feahip.ABS, alpha, beta, 0.01)
        assert s.time_kernel(27, 1, 2) > 0.0 and s.time_kernel(28, 1, 2) > 0.0

    # the sweep's table (hook 23) and the form of the displacement combination (hook 26)
    sweep = s.response_sweep(omega[:9], alpha, beta, 0.01)
    combined = s.response_combine(np.eye(m), np.ones(m), 1.0)
    before = state()
    every_stress_entry()
    store = (s.modal_stresses(), s.response_static_stress())
    assert s.time_kernel(27, 1, 2) > 0.0                                # hook 27 writes a scratch panel, not the store
    assert all(np.array_equal(a, b) for a, b in zip(store, (s.modal_stresses(), s.response_static_stress())))
    assert s.time_kernel(23, 1, 2) > 0.0 and s.time_kernel(26, 1, 2) > 0.0
    for a, b in zip(before, state()):
        assert np.array_equal(a, b)
    for a, b in zip(sweep, s.response_sweep(omega[:9], alpha, beta, 0.01)):
        assert np.array_equal(a, b)
    assert np.array_equal(combined, s.response_combine(np.eye(m), np.ones(m), 1.0))
    # the last chunk of a transient (hook 25): it shares the buffer of the sweep's table, so a phase of its own
    g = half_sine(40, period(ref) / 40, 0.4 * period(ref))
    trans = s.response_transient(g, period(ref) / 40, alpha, beta, 0.01)
    every_stress_entry()
    assert s.time_kernel(25, 1, 2) > 0.0 and s.time_kernel(26, 1, 2) > 0.0
    for a, b in zip(trans, s.response_transient(g, period(ref) / 40, alpha, beta, 0.01)):
        assert np.array_equal(a, b)
    for a, b in zip(before, state()):
        assert np.array_equal(a, b)
    s.close()
    for a, b in zip(_run(deck, ref, m, omega, S, alpha, beta), _run(deck, ref, m, omega, S, alpha, beta)):
        assert np.array_equal(a, b)


def test_refusals_stale_state_and_hooks():
    kind = "tet4"
    ref, deck = reference(kind), DECKS[kind]()
    F = tip_load(deck)
    n3 = 3 * len(deck.nodes)
    lam, phi = np.array([9.0, 4.0, 25.0]), ref.Phi[:, :3].T.copy()
    Cm, omega, S = np.eye(3), np.array([0.5, 1.0, 1.5]), np.ones(3)
    spec = ([1.0, 10.0], [1.0, 2.0])
    s = feahip.FeaSolver(deck)
    s.set_mass(RHO)
    assert np.isfinite(s.stress_increment(np.ones(n3))).all()             # no modes, no load needed
    forms = (lambda: s.response_stress_combine(Cm), lambda: s.response_stress_random(omega, S, 0.1),
             lambda: s.response_stress_spectrum(*spec))
    reads = (lambda: s.modal_stresses(), lambda: s.response_static_stress(), lambda: s.response_stress_field(np.ones(3)))
    for call in (s.response_stress_basis, *reads, *forms, lambda: s.time_kernel(27, 1, 1), lambda: s.time_kernel(28, 1, 1)):
        assert "no modes held" in _refused(s, feahip.ESTATE, call)
    s.response_set_basis(lam, phi)
    for call in (*reads, lambda: s.time_kernel(27, 1, 1)):
        assert "no stress store" in _refused(s, feahip.ESTATE, call)
    s.response_stress_basis()                                            # without a load: T_s = 0
    assert not s.response_static_stress().any() and s.modal_stresses().shape == (3, len(deck.nodes), 6)
    assert s.time_kernel(27, 1, 2) > 0.0
    for call in forms:
        assert "no load held" in _refused(s, feahip.ESTATE, call)
    s.response_load(F, True)                                             # a new load: T_s is stale
    for call in (*reads, *forms):
        assert "a load was made" in _refused(s, feahip.ESTATE, call)
    s.response_stress_basis()
    assert s.response_static_stress().any()
    assert "no stress form" in _refused(s, feahip.ESTATE, lambda: s.time_kernel(28, 1, 1))
    for call in forms:
        assert np.isfinite(call()[0]).all()
        assert s.time_kernel(28, 1, 2) > 0.0
    bad = np.eye(3)
    bad[0, 1] = 1e-300
    assert "symmetric" in _refused(s, feahip.EINVAL, lambda: s.response_stress_combine(bad))
    assert "not finite" in _refused(s, feahip.EINVAL, lambda: s.response_stress_combine(Cm, [0.0, np.nan, 0.0]))
    assert "not finite" in _refused(s, feahip.EINVAL, lambda: s.response_stress_field([0.0, np.inf, 0.0]))
    assert "not finite" in _refused(s, feahip.EINVAL, lambda: s.stress_increment(np.full(n3, np.nan)))
    _refused(s, feahip.EINVAL, lambda: s.modal_stresses(2, 2))
    # whatever fills or drops the locked store invalidates the stress store
    s.response_set_basis(lam, phi)
    for call in reads:
        assert "no stress store" in _refused(s, feahip.ESTATE, call)
    s.response_load(F, False)
    s.response_stress_basis()
    s.create_stiffness_and_residual()
    s.modal_deflate(phi, np.zeros((8, n3)))
    for call in (*reads, *forms):
        assert "no modes held" in _refused(s, feahip.ESTATE, call)
    s.solve_modes_locked(2, 0.0, 1e-6, 500)
    for call in reads[:2]:
        assert "no stress store" in _refused(s, feahip.ESTATE, call)
    s.response_load(F, True)
    s.response_stress_basis()
    assert np.isfinite(s.response_stress_combine(np.eye(2), [1.0, 1.0], 1.0)[1]).all()
    # a row shard, a rank context
    s.set_row_shard(0, 2)
    for call in (s.response_stress_basis, lambda: s.stress_increment(np.ones(n3)), lambda: s.modal_stresses(),
                 lambda: s.response_stress_combine(np.eye(2)), lambda: s.time_kernel(27, 1, 1)):
        assert "row-sharded" in _refused(s, feahip.EINVAL, call)
    s.close()
    r = feahip.RankSolver(deck, 0, 2)
    assert "feahip_create_rank" in _refused(r, feahip.EINVAL, lambda: r.stress_increment(np.ones(r.ndof)))
    assert "feahip_create_rank" in _refused(r, feahip.EINVAL, r.response_stress_basis)
    assert "feahip_create_rank" in _refused(r, feahip.EINVAL, lambda: r.response_stress_combine(Cm))
    r.close()


# ---- 6. the command line --------------------------------------------------------------------------------------------------
def test_feasolver_hip_runs_a_deck_with_the_stress_key(tmp_path):
    """A (3, 8, 3) TET4 bar under a lateral traction, twelve locked modes, (spectrum ...) and (random ...) with :base and
    :stress t: the two log lines, the two one-component $NodeData sections behind the old ones, whose largest entry is the
    logged value at the logged node, the values against the Python entries on the same state, and without the key the old
    output byte for byte."""
    def make(**kw):
        d = loaded_bar("tet4", (3, 8, 3), density=RHO, modal_count=12, load_increments_count=1, **kw)
        d.surface_values = np.tile([0.05, 0.015, 0.0], (len(d.surface_kind), 1))
        return d
    sections = dict(spectrum_points=[(0.01, 0.1), (0.5, 2.0), (5.0, 2.0), (50.0, 0.5)], spectrum_rule="cqc", spectrum_zeta=0.02,
                    spectrum_interp="loglog", spectrum_base=(1.0, 0.0, 0.0), spectrum_zpa=0.5,
                    random_points=[(0.0, 0.0), (0.5, 1.0), (4.0, 1.0), (5.0, 0.0)], random_zeta=0.02, random_per_mode=8,
                    random_background=33, random_base=(1.0, 0.0, 0.0))
    decks = {"old": make(**sections), "stress": make(**sections, spectrum_stress=True, random_stress=True)}
    exe = os.path.join(os.path.dirname(feahip.LIB_PATH), "feasolver_hip")
    out = {}
    for name, d in decks.items():
        path = tmp_path / f"{name}.sexp"
        d.save(str(path))
        out[name] = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
        assert out[name].returncode == 0, out[name].stderr
    old = (tmp_path / "old.msh").read_text()
    new = (tmp_path / "stress.msh").read_text()
    assert "von Mises" not in out["old"].stdout and "von Mises stress" not in old
    keep = "".join(l for l in out["stress"].stdout.splitlines(True) if "von Mises:" not in l)
    assert keep == out["old"].stdout
    n_nodes = len(decks["old"].nodes)
    titles = re.findall(r'^"([^"]+)"$', new, re.M)
    assert [t for t in titles if "von Mises stress" not in t] == re.findall(r'^"([^"]+)"$', old, re.M)
    assert titles[-4:] == ["Spectrum peak displacement", "Spectrum peak von Mises stress", "RMS displacement", "RMS von Mises stress"]
    got = {}
    for title, pattern in (("Spectrum peak von Mises stress", r"^Spectrum peak von Mises: vm = (\S+), node (\d+), rule cqc, 12 modes$"),
                           ("RMS von Mises stress", r"^Random RMS von Mises: vm = (\S+), node (\d+), (\d+) grid points, 12 modes$")):
        hit = re.search(pattern, out["stress"].stdout, re.M)
        assert hit, out["stress"].stdout
        body = new[new.index(f'"{title}"'):].splitlines()
        assert body[5] == "1" and body[6] == str(n_nodes) and body[7 + n_nodes] == "$EndNodeData"
        rows = np.array([float(l.split()[1]) for l in body[7:7 + n_nodes]])
        vm, node = float(hit.group(1)), int(hit.group(2))
        print(title, vm, "node", node)
        assert vm > 0 and abs(rows.max() - vm) <= 1e-9 * vm and abs(rows[node - 1] - vm) <= 1e-9 * vm
        got[title] = rows
    # the Python entries on the state the command line reached: the solved nodes, its modes, the base load
    d = decks["stress"]
    s = feahip.FeaSolver(d)
    s.set_mass(RHO)
    done, _, _ = s.solve(load_increments=1)
    assert done == 1
    lam = s.solve_modes_locked(12, 0.0, d.modal_tolerance, d.modal_max)[0]
    s.response_base_load((1.0, 0.0, 0.0), True)
    s.response_stress_basis()
    two_pi = 6.283185307179586
    w, sa = two_pi * d.spectrum_points[:, 0], d.spectrum_points[:, 1]
    _, pvm, _ = s.response_stress_spectrum(w, sa, feahip.CQC, 0.0, 0.0, 0.02, 0.5, loglog=True)
    # fea_random_run: the table from per Hz over Hz to per rad/s over rad/s, the grid of host_random_grid over its band with
    # its abscissae as breakpoints, the PSD read there by host_psd_value
    wr, Sr = two_pi * d.random_points[:, 0], d.random_points[:, 1] / two_pi
    grid = feahip.host_random_grid(lam, 0.0, 0.0, 0.02, wr[0], wr[-1], d.random_background, d.random_per_mode, wr)
    assert len(grid) == int(re.search(r"^Random RMS von Mises: .* (\d+) grid points", out["stress"].stdout, re.M).group(1))
    _, rvm, _ = s.response_stress_random(grid, feahip.host_psd_value(wr, Sr, grid), 0.0, 0.0, 0.02)
    # the file holds ten digits of every entry (%.9e), and two cold runs of the library give the same bits
    for title, mine in (("Spectrum peak von Mises stress", pvm), ("RMS von Mises stress", rvm)):
        want = got[title]
        print(title, "command line against Python", np.abs(mine - want).max() / want.max())
        assert np.all(np.abs(mine - want) <= 1e-9 * want.max())
    s.close()

"""Response spectrum and random vibration on the MI355X (kernels_combine.hip): the combine kernel alone on an exact basis
against the float64 restatement of tests/combine_reference.py, the RMS under a PSD against the same restatement and
against the fields of the sweep, the three rules of a response spectrum, one mode against the transient, the missing mass
against a dense solve, the whole chain -- modes from feahip_solve_modes_locked -- against the dense direct solve, what the
entries leave of the context's state, reproducibility, refusals and stale state, hook 26, and feasolver_hip with a
(spectrum ...) and a (random ...) section."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import combine_reference as cr
import feahip
from dynamics_reference import loaded_bar
from modal_reference import ModalReference
from response_reference import EPS, coefficients, direct, response, rounding_bound, static_solve
from test_gpu_modal_locked import DECKS, RHO, reference, solver
from test_gpu_response import CASES, _refused, rayleigh_for, tip_load
from test_gpu_transient import half_sine, loaded, period

pytestmark = pytest.mark.gpu

_dp = C.POINTER(C.c_double)


def check_form(ref, Phi, u_s, form, absolute, out, what=""):
    """out^2 within 4 (m + 5) eps A + 4 eps v of the restatement's max(v, 0), exactly 0 on the prescribed dofs and where
    the form is negative beyond the bound.  Returns (v, bound)."""
    m = Phi.shape[1]
    v, A = cr.combine(Phi, u_s, *form, absolute)
    bound = cr.combine_bound(m, v, A)
    free = ~ref.mask
    err = np.abs(out * out - np.maximum(v, 0.0))
    print(what, "out^2: largest error / bound", (err[free] / bound[free]).max())
    assert out.shape == v.shape and np.all(err <= bound)
    assert not out[ref.mask].any() and not out[v < -bound].any() and np.all(out >= 0)
    return v, bound


@pytest.mark.parametrize("kind,m,correction", CASES)
def test_kernel_on_an_exact_basis(kind, m, correction):
    """A single column, a full panel, a partial last panel, three panels and all eight; 143 nodes leave a partial last
    wave.  A random symmetric C with entries of either sign, so the form is negative on some dofs, a random b and s, the
    mode values as they are and their magnitudes; a positive semidefinite C; a C of one entry."""
    ref, s, lam, Phi, q, u_s, _ = loaded(kind, m, correction)
    rng = np.random.default_rng(100 + m)
    G = rng.standard_normal((m, m))
    b, s0 = rng.standard_normal(m), 0.8
    scale = np.abs(u_s).max() / np.abs(Phi).max() if correction else 1.0   # so that the three terms are of one size
    negative = 0
    for name, Cm in (("indefinite", G + G.T), ("semidefinite", G @ G.T)):
        Cm = (Cm + Cm.T) / 2
        for absolute in (False, True):
            form = (Cm * scale * scale, b * scale, s0)
            out = s.response_combine(*form, absolute)
            v, bound = check_form(ref, Phi, u_s, form, absolute, out, f"{kind} {m} {name} absolute={absolute}")
            negative += int((v < -bound).sum())
            assert np.array_equal(out, s.response_combine(*form, absolute))    # the same bits on every call
    assert m == 1 or negative > 0                                       # some dofs did come out negative, and exactly 0
    # b = None is b = 0, and without a correction b and s do not matter
    out = s.response_combine(G @ G.T)
    assert np.array_equal(out, s.response_combine(G @ G.T, np.zeros(m), 0.0))
    if not correction:
        assert np.array_equal(out, s.response_combine(G @ G.T, b, s0))
    # one entry: |phi_ik| sqrt(C_kk) within 2 ulp
    for k in sorted({0, m // 2, m - 1}):
        one = np.zeros((m, m))
        one[k, k] = 2.7
        want = np.abs(Phi[:, k]).astype(cr.LD) * np.sqrt(cr.LD(2.7))     # (exact to 11 more bits: the 2 ulp are the kernel's)
        for absolute in (False, True):
            out = s.response_combine(one, None, 0.0, absolute)
            assert np.all(np.abs(out - want) <= 2 * np.spacing(want.astype(np.float64)))
    s.close()


def test_the_table_follows_the_store_columns():
    """The pairs installed in another order than ascending lam: C, b and the outputs stay by ascending mode."""
    kind, m = "tet4", 24
    ref, deck = reference(kind), DECKS[kind]()
    lam, Phi = ref.lam[:m], ref.Phi[:, :m]
    perm = np.random.default_rng(3).permutation(m)
    s = solver(deck)
    s.response_set_basis(lam[perm], Phi.T[perm])
    assert np.array_equal(s.locked_modes(), Phi.T)
    q, _, _ = s.response_load(tip_load(deck, 0.1), True, feahip.CG, 1e-14, 20000)
    u_s = s.response_static()
    rng = np.random.default_rng(4)
    G = rng.standard_normal((m, m))
    scale = np.abs(u_s).max() / np.abs(Phi).max()
    form = ((G + G.T) * scale * scale, rng.standard_normal(m) * scale, 0.5)
    check_form(ref, Phi, u_s, form, False, s.response_combine(*form), "permuted store")
    sa = np.linspace(1.0, 2.0, m)
    w = np.sqrt(lam)
    peak, a = s.response_spectrum(w, sa, feahip.CQC, zeta=0.05)
    assert np.all(np.abs(a - q * sa / lam) <= 4 * EPS * np.abs(a))
    check_form(ref, Phi, u_s, feahip.host_spectrum_form(lam, q, sa, feahip.CQC, zeta=0.05), False, peak, "permuted store, CQC")
    s.close()


def _psd(omega):
    """Positive, not smooth on the grid, zero at the last point."""
    return (1.0 + 0.5 * np.cos(3.0 * np.arange(len(omega)))) * (omega < omega[-1])


@pytest.mark.parametrize("kind,m,correction", CASES)
def test_random_vibration(kind, m, correction):
    """2, 3 and 257 frequencies, the three quantities.  The form is the host builder's, fed with the GPU's own q (the
    builder is held to its restatement in tests/test_combine_host.py), the sum over it the float64 restatement with the GPU's
    own u_s.  At 3 frequencies also sum_j wt_j S_j w_j^(2p) |field_j|^2 over the fields of feahip_response_field, within
    the sum of both bounds: a field's parts are each within rounding_bound of the restatement's."""
    ref, s, lam, Phi, q, u_s, (alpha, beta) = loaded(kind, m, correction)
    w1, wm = np.sqrt(lam[0]), np.sqrt(lam[-1])
    free = ~ref.mask
    for n_freq in (2, 3, 257):
        omega = np.linspace(0.0 if correction else 0.05 * w1, 1.2 * max(wm, 2.0 * w1), n_freq)
        if n_freq == 3:
            omega[1] = 0.98 * w1
        S = _psd(omega) if n_freq > 2 else np.array([1.0, 2.0])
        for quantity in (0, 1, 2):
            form = feahip.host_random_form(lam, q, omega, S, alpha, beta, None, correction, quantity)
            rms, cov = s.response_random(omega, S, alpha, beta, None, quantity)
            assert np.array_equal(cov, form[0])
            v, bound = check_form(ref, Phi, u_s, form, False, rms, f"{kind} {m} n_freq={n_freq} quantity={quantity}")
            assert rms[free].max() > 0
            if n_freq == 3:
                g = cr.trapezoid_weights(omega) * S * omega ** (2 * quantity)
                coef = feahip.host_response_coefficients(lam, q, omega, alpha, beta, None, correction)[:, :m]   # the GPU's rows
                delta = np.sqrt(2.0) * rounding_bound(Phi, coef, u_s if correction else None)
                total, slack = np.zeros(len(rms)), np.zeros(len(rms))
                for j, w in enumerate(omega):
                    mag = np.abs(s.response_field(w, alpha, beta))
                    total += g[j] * mag * mag
                    slack += g[j] * (2 * mag * delta[j] + delta[j] ** 2)
                slack += 8 * EPS * total
                print("against the fields: largest error / bound", (np.abs(rms * rms - total)[free] / (bound + slack)[free]).max())
                assert np.all(np.abs(rms * rms - total) <= bound + slack)
    s.close()


SPECTRUM_W, SPECTRUM_SA = np.array([0.5, 5.0, 50.0, 500.0]), np.array([0.2, 2.0, 2.0, 0.5])


@pytest.mark.parametrize("kind,m,correction", CASES)
def test_spectrum_rules(kind, m, correction):
    """SRSS, CQC and ABS on the tip load and a spectrum read log-log, the three quantities, the missing mass where the load
    is held with the correction: each against the restatement with the host builder's form; ABS >= CQC and ABS >= SRSS on
    every dof up to the bounds."""
    ref, s, lam, Phi, q, u_s, (alpha, beta) = loaded(kind, m, correction)
    top = SPECTRUM_W * (np.sqrt(lam[-1]) / 40.0)                        # the plateau and both slopes lie among the modes
    sa = feahip.host_spectrum_value(top, SPECTRUM_SA, np.sqrt(lam), loglog=True)
    for quantity in (0, 1, 2):
        pk, sq, bd = {}, {}, {}
        for rule in (feahip.SRSS, feahip.CQC, feahip.ABS):
            zpa = 0.5 if correction and quantity == 0 and rule != feahip.ABS else 0.0
            peak, a = s.response_spectrum(top, SPECTRUM_SA, rule, alpha, beta, 0.03, zpa, quantity, loglog=True)
            assert np.all(np.abs(a - cr.modal_peaks(lam, q, sa, quantity)) <= 8 * EPS * np.abs(a))
            form = feahip.host_spectrum_form(lam, q, sa, rule, alpha, beta, np.full(m, 0.03), correction, zpa, quantity)
            v, bound = check_form(ref, Phi, u_s, form, rule == feahip.ABS, peak, f"{kind} {m} rule {rule} quantity {quantity} zpa {zpa}")
            if zpa:                                                     # without it, for the comparison of the rules
                peak, _ = s.response_spectrum(top, SPECTRUM_SA, rule, alpha, beta, 0.03, 0.0, quantity, loglog=True)
                form = feahip.host_spectrum_form(lam, q, sa, rule, alpha, beta, np.full(m, 0.03), correction, 0.0, quantity)
                v, bound = check_form(ref, Phi, u_s, form, False, peak)
            pk[rule], sq[rule], bd[rule] = peak, peak * peak, bound
        for rule in (feahip.SRSS, feahip.CQC):
            assert np.all(sq[feahip.ABS] + bd[feahip.ABS] >= sq[rule] - bd[rule])
        if m == 1:                                                      # one mode: |phi_i1| |a_1| whatever the rule
            want = np.abs(Phi[:, 0]) * np.abs(a[0])
            for rule in pk:
                assert np.all(np.abs(pk[rule] - want) <= 4 * EPS * want)
    s.close()


def test_one_mode_against_the_transient():
    """("fan", 1) under a base load without the correction and a half-sine: the largest |q(t_n)| from the history of the
    probe dof with the largest |phi|, handed to the spectrum entry as sa = lam max|q| / |q_1|.  Both fields are |phi_i|
    times the same number, rounded once more: 8 eps relative."""
    ref, s, lam, Phi, q, u_s, _ = loaded("fan", 1, False, base=(1.0, 0.5, 0.25))
    T1 = period(ref)
    dt = 3 * T1 / 257
    g = half_sine(258, dt, 0.4 * T1)
    dof = int(np.abs(Phi[:, 0]).argmax())
    peak_t, _, hist, _ = s.response_transient(g, dt, zeta=0.02, probes=[dof])
    q_max = np.abs(hist[0]).max() / abs(Phi[dof, 0])
    sa = lam[0] * q_max / abs(q[0])
    assert q_max > 0 and peak_t.max() > 0
    for rule in (feahip.SRSS, feahip.CQC, feahip.ABS):
        peak, a = s.response_spectrum([1.0, 2.0], [sa, sa], rule, zeta=0.02)
        moving = peak_t > 0
        print("rule", rule, "largest relative difference / eps", (np.abs(peak - peak_t)[moving] / peak_t[moving]).max() / EPS)
        assert np.all(np.abs(peak - peak_t) <= 8 * EPS * peak_t) and not peak[ref.mask].any()
    s.close()


def test_missing_mass():
    """A bar of 36 free dofs with all modes of its dense pencil installed: the rigid residual u_s - Phi (q / lam) is zero,
    so zpa moves the peak by no more than the rounding bounds and the square of the PCG's error, 1e-8 of u_s (DESIGN.md
    section 22).  With 8 of them and a zero spectrum the peak is zpa |u_s - Phi (q / lam)| of the dense solve, within that
    1e-8 of the largest u_s."""
    deck = loaded_bar("tet4", (1, 3, 1))
    ref = ModalReference(deck, RHO)
    n_free = int((~ref.mask).sum())
    assert n_free == 36 and np.all(ref.lam[:n_free] > 0)
    F = tip_load(deck, 0.1)
    Fm = np.where(ref.mask, 0.0, F)
    us_ref = static_solve(ref.K, ref.mask, F)
    zpa = 3.0
    s = solver(deck)
    for m in (n_free, 8):
        lam, Phi = ref.lam[:m], ref.Phi[:, :m]
        s.response_set_basis(lam, Phi.T)
        q, _, _ = s.response_load(F, True, feahip.CG, 1e-14, 20000)
        u_s = s.response_static()
        pcg = 1e-8 * np.abs(us_ref).max()
        assert np.abs(u_s - us_ref).max() <= pcg
        w = np.sqrt(lam)
        if m == n_free:
            sa = np.full(m, 2.0)
            for rule in (feahip.SRSS, feahip.CQC):
                with_zpa, _ = s.response_spectrum(w, sa, rule, zeta=0.05, zpa=zpa)
                without, _ = s.response_spectrum(w, sa, rule, zeta=0.05)
                _, b1 = check_form(ref, Phi, u_s, feahip.host_spectrum_form(lam, q, sa, rule, zeta=0.05, static_correction=True, zpa=zpa), False, with_zpa)
                _, b0 = check_form(ref, Phi, u_s, feahip.host_spectrum_form(lam, q, sa, rule, zeta=0.05, static_correction=True), False, without)
                gap = np.abs(with_zpa ** 2 - without ** 2)
                print("all modes, rule", rule, "largest gap / bound", (gap / (b0 + b1 + (2 * zpa * pcg) ** 2))[~ref.mask].max())
                assert np.all(gap <= b0 + b1 + (2 * zpa * pcg) ** 2)
        else:
            peak, _ = s.response_spectrum(w, np.zeros(m), feahip.SRSS, zpa=zpa)
            want = zpa * np.abs(us_ref - Phi @ ((Phi.T @ Fm) / lam))
            form = feahip.host_spectrum_form(lam, q, np.zeros(m), feahip.SRSS, static_correction=True, zpa=zpa)
            _, bound = check_form(ref, Phi, u_s, form, False, peak)
            delta = zpa * pcg
            print("8 modes: largest |peak - want| / largest want", np.abs(peak - want).max() / want.max())
            assert want.max() > 1e-3 * zpa * np.abs(us_ref).max()       # there is a residual to speak of
            assert np.all(np.abs(peak * peak - want * want) <= bound + 2 * want * delta + delta * delta)
    s.close()


@pytest.mark.parametrize("kind,m", [("tet4", 24), ("hex8", 20), ("tet10", 16)])
def test_end_to_end_against_the_dense_direct_solve(kind, m):
    """Modes from the locked solve at 1e-8, the tip load, Rayleigh damping of 2 % at the first and the m-th frequency, a
    flat PSD from 0 to 1.2 w_m on the helper's grid.  The exact RMS is the same quadrature over the dense direct solve with
    every mode; trunc is the error of the float64 restatement with the REFERENCE's first m pairs, with and without the
    correction.  The GPU's corrected field may add 1e-4 (the argument of tests/test_gpu_response.py); the uncorrected one
    is farther from the exact RMS.  Errors are the largest over the dofs, relative to the largest exact RMS."""
    ref, deck = reference(kind), DECKS[kind]()
    lam, Phi = ref.lam[:m], ref.Phi[:, :m]
    F = tip_load(deck)
    alpha, beta = rayleigh_for(ref, m)
    omega = feahip.host_random_grid(lam, alpha, beta, None, 0.0, 1.2 * np.sqrt(lam[-1]), 33, 8)
    S = np.ones_like(omega)
    g = cr.trapezoid_weights(omega) * S
    rms_of = lambda u: np.sqrt((g[:, None] * np.abs(u) ** 2).sum(axis=0))
    exact = rms_of(np.array([direct(ref.K, ref.M, ref.mask, F, w, alpha, beta) for w in omega]))
    scale = exact.max()
    q_ref = Phi.T @ np.where(ref.mask, 0.0, F)
    with_c = rms_of(response(Phi, coefficients(lam, q_ref, omega, alpha, beta, None, True), static_solve(ref.K, ref.mask, F)))
    without = rms_of(response(Phi, coefficients(lam, q_ref, omega, alpha, beta, None, False)))
    trunc, trunc_u = np.abs(with_c - exact).max() / scale, np.abs(without - exact).max() / scale
    print(kind, len(omega), "grid points; reference alone: uncorrected", trunc_u, "corrected", trunc)
    s = solver(deck)
    s.solve_modes_locked(m, 0.0, 1e-8, 2000)
    err = {}
    for correction in (True, False):
        s.response_load(F, correction, feahip.CG, 1e-14, 20000)
        rms, _ = s.response_random(omega, S, alpha, beta)
        err[correction] = np.abs(rms - exact).max() / scale
    s.close()
    print(kind, "GPU against the exact RMS: corrected", err[True], "uncorrected", err[False], "largest exact RMS", scale)
    assert err[True] <= 2 * trunc + 1e-4
    assert err[False] > err[True]


def _run(deck, ref, m, omega, S, alpha, beta):
    s = solver(deck)
    s.response_set_basis(ref.lam[:m], ref.Phi[:, :m].T)
    s.response_base_load((1.0, 0.5, 0.0), True, feahip.CG, 1e-14, 20000)
    out = (*s.response_random(omega, S, alpha, beta, 0.01, 2),
           *s.response_spectrum(SPECTRUM_W, SPECTRUM_SA, feahip.CQC, alpha, beta, 0.01, 0.5),
           *s.response_spectrum(SPECTRUM_W, SPECTRUM_SA, feahip.ABS, alpha, beta, 0.01))
    s.close()
    return out


def test_state_is_left_alone_and_two_cold_runs_agree():
    kind, m = "tet4", 24
    ref, deck = reference(kind), DECKS[kind]()
    alpha, beta = rayleigh_for(ref, m)
    omega = np.linspace(0.0, 1.2 * np.sqrt(ref.lam[m - 1]), 257)
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
    before = state()
    s.response_combine(np.eye(m), np.ones(m), 1.0, True)
    assert s.time_kernel(23, 1, 2) > 0.0                                # the sweep's table is still there
    s.response_random(omega, S, alpha, beta, 0.01, 1)
    s.response_spectrum(SPECTRUM_W, SPECTRUM_SA, feahip.CQC, alpha, beta, 0.01, 0.5)
    assert s.time_kernel(26, 1, 2) > 0.0 and s.time_kernel(23, 1, 2) > 0.0
    for a, b in zip(before, state()):
        assert np.array_equal(a, b)
    for a, b in zip(sweep, s.response_sweep(omega[:9], alpha, beta, 0.01)):
        assert np.array_equal(a, b)
    g = half_sine(40, period(ref) / 40, 0.4 * period(ref))
    trans = s.response_transient(g, period(ref) / 40, alpha, beta, 0.01)
    s.response_spectrum(SPECTRUM_W, SPECTRUM_SA, feahip.ABS, alpha, beta, 0.01)
    assert s.time_kernel(25, 1, 2) > 0.0 and s.time_kernel(26, 1, 2) > 0.0   # and so is the transient's last chunk
    for a, b in zip(trans, s.response_transient(g, period(ref) / 40, alpha, beta, 0.01)):
        assert np.array_equal(a, b)
    for a, b in zip(before, state()):
        assert np.array_equal(a, b)
    s.close()
    for a, b in zip(_run(deck, ref, m, omega, S, alpha, beta), _run(deck, ref, m, omega, S, alpha, beta)):
        assert np.array_equal(a, b)


def test_refusals_and_stale_state():
    kind = "tet4"
    ref, deck = reference(kind), DECKS[kind]()
    F = tip_load(deck)
    n3 = 3 * len(deck.nodes)
    lam, phi = np.array([9.0, 4.0, 25.0]), ref.Phi[:, :3].T.copy()       # any three columns serve here; lam out of order
    Cm, omega, S = np.eye(3), np.array([0.5, 1.0, 1.5]), np.ones(3)
    spec = ([1.0, 10.0], [1.0, 2.0])
    s = feahip.FeaSolver(deck)
    lib, ctx = s._lib, s._ctx
    s.set_mass(RHO)
    calls = (lambda: s.response_combine(Cm), lambda: s.response_random(omega, S, 0.1), lambda: s.response_spectrum(*spec))
    for call in calls:
        assert "no modes held" in _refused(s, feahip.ESTATE, call)
    _refused(s, feahip.ESTATE, lambda: s.time_kernel(26, 1, 1))
    s.response_set_basis(lam, phi)
    for call in calls:
        assert "no load held" in _refused(s, feahip.ESTATE, call)
    s.response_load(F, False)
    assert "no form" in _refused(s, feahip.ESTATE, lambda: s.time_kernel(26, 1, 1))
    for call in calls:
        assert np.isfinite(call()[0]).all()
        assert s.time_kernel(26, 1, 2) > 0.0
    # the generic form
    out = np.zeros(n3)
    op, cp = out.ctypes.data_as(_dp), Cm.ctypes.data_as(_dp)
    assert lib.feahip_response_combine(ctx, None, None, 0.0, 0, op) == feahip.EINVAL
    assert lib.feahip_response_combine(ctx, cp, None, 0.0, 0, None) == feahip.EINVAL
    assert lib.feahip_response_combine(ctx, cp, None, 0.0, 0, op) == 0
    bad = np.eye(3)
    bad[0, 1] = 1e-300
    assert "symmetric" in _refused(s, feahip.EINVAL, lambda: s.response_combine(bad))
    bad[1, 0], bad[0, 1] = -0.0, 0.0
    assert "symmetric" in _refused(s, feahip.EINVAL, lambda: s.response_combine(bad))       # to the bit
    for v in (np.nan, np.inf, -np.inf, 1e308):                           # (twice 1e308 is not finite)
        bad = np.eye(3)
        bad[0, 2] = bad[2, 0] = v
        assert "not finite" in _refused(s, feahip.EINVAL, lambda: s.response_combine(bad))
    for v in (np.nan, np.inf):
        bad = np.eye(3)
        bad[1, 1] = v
        assert "not finite" in _refused(s, feahip.EINVAL, lambda: s.response_combine(bad))
        assert "not finite" in _refused(s, feahip.EINVAL, lambda: s.response_combine(Cm, [0.0, v, 0.0]))
        assert "not finite" in _refused(s, feahip.EINVAL, lambda: s.response_combine(Cm, None, v))
    # random vibration
    rms = np.zeros(n3)
    wp, sp, rp = omega.ctypes.data_as(_dp), S.ctypes.data_as(_dp), rms.ctypes.data_as(_dp)
    assert lib.feahip_response_random(ctx, 3, None, sp, 0.1, 0.0, None, 0, rp, None) == feahip.EINVAL
    assert lib.feahip_response_random(ctx, 3, wp, None, 0.1, 0.0, None, 0, rp, None) == feahip.EINVAL
    assert lib.feahip_response_random(ctx, 3, wp, sp, 0.1, 0.0, None, 0, None, None) == feahip.EINVAL
    assert lib.feahip_response_random(ctx, 3, wp, sp, 0.1, 0.0, None, 0, rp, None) == 0     # modal_cov may be NULL
    for n in (1, 0, -1, feahip.RANDOM_MAX_FREQ + 1):
        assert lib.feahip_response_random(ctx, n, wp, sp, 0.1, 0.0, None, 0, rp, None) == feahip.EINVAL
        assert b"n_freq" in lib.feahip_last_error(ctx)
    for kw in (dict(omega=[0.5, 0.5, 1.5]), dict(omega=[1.0, 0.5, 1.5]), dict(omega=[-0.5, 1.0, 1.5]), dict(omega=[0.5, 1.0, np.inf]),
               dict(omega=[0.5, np.nan, 1.5]), dict(S=[1.0, -1.0, 1.0]), dict(S=[1.0, np.inf, 1.0]), dict(S=[np.nan, 1.0, 1.0]),
               dict(quantity=-1), dict(quantity=3), dict(alpha=-0.1), dict(alpha=np.nan), dict(beta=-0.1), dict(beta=np.inf),
               dict(zeta=[0.0, -0.1, 0.0]), dict(zeta=np.nan),
               dict(omega=[0.5, 2.0, 2.5], alpha=0.0)):                   # the last: w^2 = lam_k undamped
        a = dict(omega=omega, S=S, alpha=0.1, beta=0.0, zeta=None, quantity=0)
        a.update(kw)
        _refused(s, feahip.EINVAL, lambda: s.response_random(**a))
    # the spectrum
    pk = np.zeros(n3)
    w2, s2 = np.array(spec[0]), np.array(spec[1])
    xp, yp, pp = w2.ctypes.data_as(_dp), s2.ctypes.data_as(_dp), pk.ctypes.data_as(_dp)
    tail = (0, 0, 0.0, 0.0, None, 0.0, 0)
    assert lib.feahip_response_spectrum(ctx, 2, None, yp, *tail, pp, None) == feahip.EINVAL
    assert lib.feahip_response_spectrum(ctx, 2, xp, None, *tail, pp, None) == feahip.EINVAL
    assert lib.feahip_response_spectrum(ctx, 2, xp, yp, *tail, None, None) == feahip.EINVAL
    assert lib.feahip_response_spectrum(ctx, 2, xp, yp, *tail, pp, None) == 0               # modal_peak may be NULL
    assert lib.feahip_response_spectrum(ctx, 0, xp, yp, *tail, pp, None) == feahip.EINVAL
    for kw in (dict(w=[1.0, 1.0]), dict(w=[2.0, 1.0]), dict(w=[1.0, np.nan]), dict(sa=[1.0, -2.0]), dict(sa=[1.0, np.inf]),
               dict(rule=-1), dict(rule=3), dict(quantity=-1), dict(quantity=3), dict(zpa=0.5), dict(zpa=-0.5), dict(zpa=np.nan),
               dict(alpha=-0.1), dict(beta=np.inf), dict(zeta=[0.0, -0.1, 0.0])):   # zpa: the load is held without the correction
        a = dict(w=spec[0], sa=spec[1], rule=feahip.CQC, alpha=0.0, beta=0.0, zeta=None, zpa=0.0, quantity=0)
        a.update(kw)
        _refused(s, feahip.EINVAL, lambda: s.response_spectrum(**a))
    s.response_load(F, True)
    s.response_spectrum(*spec, feahip.CQC, zpa=0.5)
    for kw in (dict(quantity=1), dict(quantity=2), dict(rule=feahip.ABS)):
        assert "zpa" in _refused(s, feahip.EINVAL, lambda: s.response_spectrum(*spec, **dict(dict(rule=feahip.SRSS, zpa=0.5), **kw)))
    s.response_set_basis([0.0, 4.0, 25.0], phi)                          # a zero mode: no spectrum, but an RMS at w > 0
    s.response_load(F, False)
    assert "not positive" in _refused(s, feahip.EINVAL, lambda: s.response_spectrum(*spec))
    assert np.isfinite(s.response_random(omega, S, 0.1)[0]).all()
    # whatever fills or drops the store invalidates the load and the form
    s.response_set_basis(lam, phi)
    for call in calls:
        assert "no load held" in _refused(s, feahip.ESTATE, call)
    _refused(s, feahip.ESTATE, lambda: s.time_kernel(26, 1, 1))
    s.response_load(F, False)
    assert "no form" in _refused(s, feahip.ESTATE, lambda: s.time_kernel(26, 1, 1))   # the old form was laid out for the old store
    s.response_combine(Cm)
    s.create_stiffness_and_residual()
    s.modal_deflate(phi, np.zeros((8, n3)))
    for call in calls:
        assert "no modes held" in _refused(s, feahip.ESTATE, call)
    s.solve_modes_locked(2, 0.0, 1e-6, 500)
    assert "no load held" in _refused(s, feahip.ESTATE, lambda: s.response_combine(np.eye(2)))
    s.response_load(F, True)
    assert np.isfinite(s.response_combine(np.eye(2), [1.0, 1.0], 1.0)).all()
    # a row shard
    s.set_row_shard(0, 2)
    for call in (lambda: s.response_combine(np.eye(2)), *calls[1:]):
        assert "row-sharded" in _refused(s, feahip.EINVAL, call)
    s.close()
    r = feahip.RankSolver(deck, 0, 2)
    assert "feahip_create_rank" in _refused(r, feahip.EINVAL, lambda: r.response_combine(Cm))
    assert "feahip_create_rank" in _refused(r, feahip.EINVAL, lambda: r.response_random(omega, S, 0.1))
    assert "feahip_create_rank" in _refused(r, feahip.EINVAL, lambda: r.response_spectrum(*spec))
    r.close()


def test_feasolver_hip_runs_a_deck_with_each_section(tmp_path):
    """A lateral traction on the bar's end, one load increment, twelve locked modes.  (spectrum ...) with the surface load
    and with :base, (random ...) with :base, both together: the log line of each, its $NodeData section, whose largest
    entry is the logged value, and the grid's point count.  Without the sections, the old output."""
    def make(**kw):
        d = loaded_bar("tet4", (3, 8, 3), density=RHO, modal_count=12, load_increments_count=1, **kw)
        d.surface_values = np.tile([0.05, 0.015, 0.0], (len(d.surface_kind), 1))
        return d
    spectrum = dict(spectrum_points=[(0.01, 0.1), (0.5, 2.0), (5.0, 2.0), (50.0, 0.5)], spectrum_rule="cqc", spectrum_zeta=0.02,
                    spectrum_interp="loglog")
    random = dict(random_points=[(0.0, 0.0), (0.5, 1.0), (4.0, 1.0), (5.0, 0.0)], random_zeta=0.02, random_per_mode=8,
                  random_background=33, random_base=(1.0, 0.0, 0.0))
    decks = {"plain": make(), "spectrum": make(**spectrum), "base": make(**spectrum, spectrum_base=(1.0, 0.0, 0.0), spectrum_zpa=0.5),
             "random": make(**random), "both": make(**spectrum, **random)}
    exe = os.path.join(os.path.dirname(feahip.LIB_PATH), "feasolver_hip")
    out = {}
    for name, d in decks.items():
        path = tmp_path / f"{name}.sexp"
        d.save(str(path))
        out[name] = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
        assert out[name].returncode == 0, out[name].stderr
    old = (tmp_path / "plain.msh").read_text()
    assert "Spectrum" not in out["plain"].stdout and "Random" not in out["plain"].stdout and "Spectrum" not in old and "RMS" not in old
    strip = lambda text: "".join(l for l in text.splitlines(True) if not l.startswith(("Spectrum", "Random")))
    n_nodes = len(decks["plain"].nodes)

    def section(name, title):
        msh = (tmp_path / f"{name}.msh").read_text()
        assert msh.startswith(old) and strip(out[name].stdout) == out["plain"].stdout
        tail = msh[len(old):]
        body = tail[tail.index(f'"{title}"'):].splitlines()
        rows = np.array([[float(x) for x in l.split()[1:]] for l in body[7:7 + n_nodes]])
        assert body[6] == str(n_nodes) and body[7 + n_nodes] == "$EndNodeData" and rows.shape == (n_nodes, 3)
        return tail, rows

    for name in ("spectrum", "base", "both"):
        hit = re.search(r"^Spectrum peak: \|u\| = (\S+), node (\d+) dof ([012]), rule cqc, 12 modes$", out[name].stdout, re.M)
        assert hit, out[name].stdout
        tail, rows = section(name, "Spectrum peak displacement")
        peak, node, dof = float(hit.group(1)), int(hit.group(2)), int(hit.group(3))
        print(name, "spectrum peak", peak, "node", node, "dof", dof)
        assert peak > 0 and abs(rows.max() - peak) <= 1e-9 * peak and abs(rows[node - 1, dof] - peak) <= 1e-9 * peak
        assert re.findall(r'^"([^"]+)"$', tail, re.M) == ["Spectrum peak displacement"] + (["RMS displacement"] if name == "both" else [])
    for name in ("random", "both"):
        hit = re.search(r"^Random RMS: \|u\| = (\S+), node (\d+) dof ([012]), (\d+) grid points, 12 modes$", out[name].stdout, re.M)
        assert hit, out[name].stdout
        tail, rows = section(name, "RMS displacement")
        rms, node, dof, n_grid = float(hit.group(1)), int(hit.group(2)), int(hit.group(3)), int(hit.group(4))
        print(name, "RMS", rms, "node", node, "dof", dof, "grid points", n_grid)
        assert rms > 0 and abs(rows.max() - rms) <= 1e-9 * rms and abs(rows[node - 1, dof] - rms) <= 1e-9 * rms
        assert 33 <= n_grid <= 33 + 12 * 8 + 4
        assert tail.count("$NodeData") == (2 if name == "both" else 1)
    # the RMS is the same beside a spectrum section: the load is made again
    assert re.search(r"^Random RMS: .*$", out["random"].stdout, re.M).group(0) == re.search(r"^Random RMS: .*$", out["both"].stdout, re.M).group(0)

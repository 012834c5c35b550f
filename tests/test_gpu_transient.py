"""Transient response by mode superposition and base excitation on the MI355X (kernels_transient.hip): the sweep kernel
alone on an exact basis against the restatement of tests/transient_reference.py fed with the library's own host table,
the chunk boundaries of a long history, the base load against the dense mass matrix, the whole chain -- modes from
feahip_solve_modes_locked -- against the exact dense solution, a stiff step and a free body, what the entries leave of
the context's state, reproducibility, refusals and stale state, and feasolver_hip with a (transient ...) section."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import feahip
import transient_reference as tr
from dynamics_reference import loaded_bar
from modal_reference import ModalReference
from response_reference import EPS, static_solve
from test_gpu_modal_locked import DECKS, N_MODES, RHO, reference, shift_of, solver
from test_gpu_response import _refused, decided, rayleigh_for, tip_load

pytestmark = pytest.mark.gpu

_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
CHUNK = feahip.TRANSIENT_CHUNK


def period(ref):
    return 2 * np.pi / np.sqrt(ref.lam[0])


def half_sine(points, dt, length, start=0):
    """sin(pi (t - t0) / length) on [t0, t0 + length), t0 = start dt, zero elsewhere."""
    t = (np.arange(points) - start) * dt
    return np.where((t >= 0) & (t < length), np.sin(np.pi * np.clip(t, 0, length) / length), 0.0)


def check_peaks(ref, Phi, coef, u_s, g, peak, at):
    """peak to the rounding bound, peak_at the restatement's argmax where that is decided, a step within the bound of
    the largest elsewhere; at least 95 % of the free dofs decided; zero on the prescribed dofs.  Returns (u, bound)."""
    u, bound = tr.response(Phi, coef, u_s, g), tr.rounding_bound(Phi, coef, u_s, g)
    mag, worst = np.abs(u), bound.max(axis=0)
    free = ~ref.mask
    print("peak: largest error / bound", (np.abs(peak - mag.max(axis=0))[free] / worst[free]).max())
    assert np.all(np.abs(peak - mag.max(axis=0)) <= worst)
    best, sure = decided(mag, worst)
    print("peak_at: decided", (sure & free).sum(), "of", free.sum(), "free dofs; steps", at[free].min(), "..", at[free].max())
    assert (sure & free).sum() >= 0.95 * free.sum()
    assert np.array_equal(at[sure & free], best[sure & free])
    assert np.all(mag[at, np.arange(len(at))] >= mag.max(axis=0) - 2 * worst)
    assert not peak[ref.mask].any() and not at[ref.mask].any()
    return u, bound


def loaded(kind, m, correction, base=None):
    """A context with the reference's first m pairs installed and the tip load (or a base load) held: (ref, s, lam, Phi,
    q, u_s, damping)."""
    ref, deck = reference(kind), DECKS[kind]()
    lam, Phi = ref.lam[:m], ref.Phi[:, :m]
    s = solver(deck)
    s.response_set_basis(lam, Phi.T)
    if base is None:
        q, _, _ = s.response_load(tip_load(deck, 0.1), correction, feahip.CG, 1e-14, 20000)
    else:
        q = s.response_base_load(base, correction, feahip.CG, 1e-14, 20000)[0]
    return ref, s, lam, Phi, q, s.response_static(), rayleigh_for(ref, m)


def probes_of(ref):
    n3 = len(ref.mask)
    return np.array([0, 4, n3 // 2, n3 - 2, n3 - 1, int(np.nonzero(ref.mask)[0][0]) if ref.mask.any() else 1], dtype=np.int32)


CASES = [("fan", 1, False), ("tet10", 8, True), ("hex8", 20, True), ("tet4", 24, False), ("tet4", 64, True)]


@pytest.mark.parametrize("kind,m,correction", CASES)
def test_kernel_on_an_exact_basis(kind, m, correction):
    """A single column, a full panel, a partial last panel, three panels and all eight; 143 nodes leave a partial last
    wave.  Histories of 1, 3 and 257 steps, a half-sine of 0.4 T1 and a step.  The restatement takes the GPU's own q and
    u_s (both checked in tests/test_gpu_response.py) and the library's own host table."""
    ref, s, lam, Phi, q, u_s, (alpha, beta) = loaded(kind, m, correction)
    T1 = period(ref)
    dt = 3 * T1 / 257
    probes = probes_of(ref)
    for n_steps in (1, 3, 257):
        for g in (half_sine(n_steps + 1, dt, 0.4 * T1), np.ones(n_steps + 1)):
            snaps = sorted({0, n_steps // 2, n_steps})
            coef = feahip.host_transient_coefficients(lam, q, g, dt, alpha, beta, None, correction)[:, :m]
            peak, at, hist, snap = s.response_transient(g, dt, alpha, beta, None, 0, probes, snaps)
            u, bound = check_peaks(ref, Phi, coef, u_s if correction else None, g, peak, at)
            assert hist.shape == (len(probes), n_steps + 1) and snap.shape == (len(snaps), len(ref.mask))
            assert np.all(np.abs(hist - u[:, probes].T) <= bound[:, probes].T)
            for k, n in enumerate(snaps):
                assert np.all(np.abs(snap[k] - u[n]) <= bound[n])
                assert not snap[k][ref.mask].any()
                assert np.array_equal(snap[k][probes], hist[:, n])         # the host sums the probes in the kernel's order
    if kind == "hex8":                                                   # velocity and acceleration: no static term
        g = half_sine(258, dt, 0.4 * T1)
        for quantity in (1, 2):
            coef = feahip.host_transient_coefficients(lam, q, g, dt, alpha, beta, None, correction, quantity)[:, :m]
            peak, at, hist, snap = s.response_transient(g, dt, alpha, beta, None, quantity, probes, [100])
            u, bound = check_peaks(ref, Phi, coef, None, g, peak, at)
            assert np.all(np.abs(hist - u[:, probes].T) <= bound[:, probes].T) and np.all(np.abs(snap[0] - u[100]) <= bound[100])
            assert np.array_equal(snap[0][probes], hist[:, 100])
    # the same value at every step: the lowest step on every dof
    peak, at, _, _ = s.response_transient(np.zeros(40), dt, alpha, beta)
    assert not peak.any() and not at.any()
    s.close()


@pytest.mark.parametrize("kind,m", [("fan", 1), ("tet4", 24)])
def test_chunk_boundaries(kind, m):
    """Histories of FEA_TRANSIENT_CHUNK, one more and 2 FEA_TRANSIENT_CHUNK + 3 points: one launch, a second launch of one
    row, three launches.  The step puts every peak early in the first chunk; the half-sine is delayed to begin at the
    first row of the second chunk, so every peak lies in a later one, or, where there is none or it has one row, to
    straddle the end of the first."""
    correction = kind != "fan"
    ref, s, lam, Phi, q, u_s, (alpha, beta) = loaded(kind, m, correction)
    T1 = period(ref)
    dt = 3 * T1 / 257
    probes = probes_of(ref)
    for points in (CHUNK, CHUNK + 1, 2 * CHUNK + 3):
        start = CHUNK if points > CHUNK + 1 else CHUNK - 60
        for name, g in (("step", np.ones(points)), ("delayed half-sine", half_sine(points, dt, 0.4 * T1, start))):
            snaps = [0, CHUNK - 1, min(CHUNK, points - 1), points - 1]
            coef = feahip.host_transient_coefficients(lam, q, g, dt, alpha, beta, None, correction)[:, :m]
            peak, at, hist, snap = s.response_transient(g, dt, alpha, beta, None, 0, probes, snaps)
            print(kind, points, name)
            u, bound = check_peaks(ref, Phi, coef, u_s if correction else None, g, peak, at)
            free = ~ref.mask
            if name == "step":
                assert at[free].max() < CHUNK
            elif start == CHUNK:
                assert at[free].min() >= CHUNK
            assert np.all(np.abs(hist - u[:, probes].T) <= bound[:, probes].T)
            for k, n in enumerate(snaps):
                assert np.all(np.abs(snap[k] - u[n]) <= bound[n]) and np.array_equal(snap[k][probes], hist[:, n])
    s.close()


@pytest.mark.parametrize("kind,m", [("tet4", 24), ("hex8", 20), ("tet10", 16)])
def test_base_load(kind, m):
    """q within the projection's bound of Phi' mask(-M r) with the dense M over all dofs -- the columns of the prescribed
    dofs take part --, gamma = -q, eff_mass = gamma^2, total_mass = r' M r = |r|^2 times the bar's mass 3.0, and u_s within
    1e-8 of the dense solve (the bound of tests/test_gpu_response.py)."""
    ref, deck = reference(kind), DECKS[kind]()
    lam, Phi = ref.lam[:m], ref.Phi[:, :m]
    s = solver(deck)
    s.response_set_basis(lam, Phi.T)
    carried = {}
    for direction in ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (0.3, -2.0, 0.5)):
        F, r, total_ref = tr.base_load(ref.M, ref.mask, direction)
        q, gamma, eff, total, its, _ = s.response_base_load(direction, True, feahip.CG, 1e-14, 20000)
        qb = 2 * len(F) * EPS * (np.abs(Phi) * (np.abs(ref.M) @ np.abs(r))[:, None]).sum(axis=0)
        print(kind, direction, "q: largest error / bound", (np.abs(q - Phi.T @ F) / qb).max(), "sum of m_eff", eff.sum(), "of", total)
        assert q.shape == (m,) and np.all(np.abs(q - Phi.T @ F) <= qb)
        assert np.array_equal(gamma, -q) and np.array_equal(eff, gamma * gamma) and its > 0
        assert abs(total - total_ref) <= 1e-12 * total_ref and abs(total - 3.0 * np.dot(direction, direction)) <= 1e-12 * total
        assert eff.sum() <= total * (1 + 1e-12)
        carried[direction] = eff.sum()
        u, want = s.response_static(), static_solve(ref.K, ref.mask, F)
        assert np.abs(u - want).max() <= 1e-8 * np.abs(want).max() and not u[ref.mask].any()
    if kind == "tet4":                                                   # what the reference's first 24 modes carry
        assert abs(carried[(1.0, 0.0, 0.0)] - 2.824) <= 1e-3 and abs(carried[(0.0, 0.0, 1.0)] - 2.824) <= 1e-3
        assert abs(carried[(0.0, 1.0, 0.0)] - 2.692) <= 1e-3
    # without the correction: no solve, u_s zero, the same q
    q0 = s.response_base_load((1.0, 0.0, 0.0), False)
    assert q0[4] == 0 and not s.response_static().any()
    # the load is held for the transient as for the sweep
    g = half_sine(65, period(ref) / 40, 0.4 * period(ref))
    coef = feahip.host_transient_coefficients(lam, q0[0], g, period(ref) / 40, 0.0, 0.0, 0.02, False)[:, :m]
    peak, at, _, _ = s.response_transient(g, period(ref) / 40, zeta=0.02)
    check_peaks(ref, Phi, coef, None, g, peak, at)
    assert np.isfinite(s.response_sweep([1.0], 0.1)[0]).all()
    s.close()


@pytest.mark.parametrize("kind,m", [("tet4", 24), ("hex8", 20), ("tet10", 16)])
def test_end_to_end_against_the_exact_dense_solution(kind, m):
    """Modes from the locked solve at 1e-8, Rayleigh damping of 2 % at the first and the m-th frequency, the tip load under
    a half-sine of 0.4 T1, 257 steps of 3 T1 / 257.  The exact solution is the restatement with ALL modes of the dense
    pencil, which Rayleigh damping leaves uncoupled.  trunc is the error of the restatement with the REFERENCE's first m
    pairs and the correction; the GPU may add 1e-4 (the argument of tests/test_gpu_response.py).  Errors are the largest
    over steps and dofs, relative to the largest |u| of the exact solution."""
    ref, deck = reference(kind), DECKS[kind]()
    F = tip_load(deck)
    Fm = np.where(ref.mask, 0.0, F)
    alpha, beta = rayleigh_for(ref, m)
    T1 = period(ref)
    dt, g = 3 * T1 / 257, half_sine(258, 3 * T1 / 257, 0.4 * T1)
    full = tr.coefficients(ref.lam, ref.Phi.T @ Fm, g, dt, alpha, beta, None, False).astype(np.float64)
    exact = tr.response(ref.Phi, full)
    scale = np.abs(exact).max()
    lam, Phi = ref.lam[:m], ref.Phi[:, :m]
    q_ref = Phi.T @ Fm
    with_c = tr.response(Phi, tr.coefficients(lam, q_ref, g, dt, alpha, beta, None, True).astype(np.float64), static_solve(ref.K, ref.mask, F), g)
    without = tr.response(Phi, tr.coefficients(lam, q_ref, g, dt, alpha, beta, None, False).astype(np.float64))
    trunc = np.abs(with_c - exact).max() / scale
    trunc_u = np.abs(without - exact).max() / scale
    print(kind, "reference alone: uncorrected", trunc_u, "corrected", trunc, "ratio", trunc_u / trunc)
    s = solver(deck)
    s.solve_modes_locked(m, 0.0, 1e-8, 2000)
    probes, err = probes_of(ref), {}
    for correction in (True, False):
        s.response_load(F, correction, feahip.CG, 1e-14, 20000)
        peak, at, hist, snap = s.response_transient(g, dt, alpha, beta, None, 0, probes, np.arange(258))
        err[correction] = np.abs(snap - exact).max() / scale
        assert np.array_equal(snap[:, probes].T, hist)
        assert np.all(np.abs(peak - np.abs(snap).max(axis=0)) == 0) and np.array_equal(at, np.abs(snap).argmax(axis=0))
        if correction:
            print(kind, "GPU against the exact solution", err[True], "trunc", trunc)
            assert err[True] <= 2 * trunc + 1e-4
            assert np.abs(hist - exact[:, probes].T).max() / scale <= 2 * trunc + 1e-4
        else:
            gap = np.abs(snap - without).max() / scale
            print(kind, "uncorrected: GPU against the restatement", gap, "against the exact solution", err[False])
            assert gap <= 1e-4
    s.close()
    print(kind, "uncorrected / corrected error", err[False] / err[True])
    assert err[False] >= 10 * err[True]


def test_a_stiff_step_and_a_free_body():
    """omega_max dt = 50 on the 24 pairs of tet4: nothing blows up, the result is within the rounding bound.  The free
    block with the modes of a solve with a shift (its six rigid modes come back as +-1e-12 of the shift's scale) runs
    without the correction; the correction is refused."""
    kind, m = "tet4", 24
    ref, s, lam, Phi, q, u_s, (alpha, beta) = loaded(kind, m, True)
    dt = 50.0 / np.sqrt(lam[-1])
    g = half_sine(65, dt, 9.5 * dt)
    for damping in (dict(alpha=0.0, beta=0.0), dict(alpha=alpha, beta=beta)):
        coef = feahip.host_transient_coefficients(lam, q, g, dt, zeta=None, static_correction=True, **damping)[:, :m]
        peak, at, _, _ = s.response_transient(g, dt, **damping)
        assert np.isfinite(peak).all() and peak.max() < 100 * np.abs(u_s).max()
        check_peaks(ref, Phi, coef, u_s, g, peak, at)
    s.close()
    kind = "free_tet4"
    ref, deck, m = reference(kind), DECKS[kind](), N_MODES["free_tet4"]
    F = tip_load(deck, 0.1)
    s = solver(deck)
    lam, _, _, _ = s.solve_modes_locked(m, shift_of(kind), 1e-8, 2000)
    Phi = s.locked_modes().T
    assert "shift" in _refused(s, feahip.EINVAL, lambda: s.response_load(F, True))
    assert "shift" in _refused(s, feahip.EINVAL, lambda: s.response_base_load((1.0, 0.0, 0.0), True))
    q, its, _ = s.response_load(F, False)
    dt = 2 * np.pi / np.sqrt(ref.lam[6]) / 20
    g = half_sine(101, dt, 8 * dt)
    coef = feahip.host_transient_coefficients(lam, q, g, dt, zeta=0.02, static_correction=False)[:, :m]
    peak, at, _, _ = s.response_transient(g, dt, zeta=0.02)
    assert np.isfinite(peak).all()
    check_peaks(ref, Phi, coef, None, g, peak, at)
    s.close()


def _run(deck, ref, m, g, dt, alpha, beta):
    s = solver(deck)
    s.response_set_basis(ref.lam[:m], ref.Phi[:, :m].T)
    base = s.response_base_load((1.0, 0.5, 0.0), True, feahip.CG, 1e-14, 20000)
    out = s.response_transient(g, dt, alpha, beta, 0.01, 0, [7, 8], [3, len(g) - 1])
    s.close()
    return (*base[:4], *out)


def test_state_is_left_alone_and_two_cold_runs_agree():
    kind, m = "tet4", 24
    ref, deck = reference(kind), DECKS[kind]()
    alpha, beta = rayleigh_for(ref, m)
    dt = period(ref) / 40
    g = half_sine(CHUNK + 40, dt, 0.4 * period(ref), 20)
    rng = np.random.default_rng(2)
    s = solver(deck)
    s.set_velocities(rng.standard_normal((s.N, 3)))
    s.set_accelerations(rng.standard_normal((s.N, 3)))
    s.set_time(0.375)
    s.set_load_factor(0.5)
    s.response_set_basis(ref.lam[:m], ref.Phi[:, :m].T)
    state = lambda: (s.nodes(), s.velocities(), s.accelerations(), np.array(s.time()), np.array(s.load_factor()), s.locked_modes())
    before = state()
    s.response_base_load((1.0, 0.5, 0.0), True, feahip.CG, 1e-14, 20000)
    s.response_transient(g, dt, alpha, beta, 0.01, 0, [7, 8], [3, len(g) - 1])
    s.response_transient(g[:50], dt, alpha, beta, 0.01, 2, [7], [0])
    for a, b in zip(before, state()):
        assert np.array_equal(a, b)

    def assemble_and_solve(t):
        t.create_stiffness_and_residual()
        t.apply_prescribed_bc(0.0)
        it, res = t.solve_slae(feahip.CG, 1e-12, 20000)
        return t.solution(), np.array([it, res])
    fresh = solver(deck)
    fresh.set_load_factor(0.5)
    for a, b in zip(assemble_and_solve(fresh), assemble_and_solve(s)):
        assert np.array_equal(a, b)
    fresh.close()
    s.close()
    for a, b in zip(_run(deck, ref, m, g, dt, alpha, beta), _run(deck, ref, m, g, dt, alpha, beta)):
        assert np.array_equal(a, b)


def test_refusals_and_stale_state():
    kind = "tet4"
    ref, deck = reference(kind), DECKS[kind]()
    F = tip_load(deck)
    n3 = 3 * len(deck.nodes)
    lam, phi = np.array([9.0, 4.0, 25.0]), ref.Phi[:, :3].T.copy()       # any three columns serve here; lam out of order
    g = np.ones(5)
    s = feahip.FeaSolver(deck)
    lib, ctx = s._lib, s._ctx
    assert "no mass" in _refused(s, feahip.ESTATE, lambda: s.response_base_load((1.0, 0.0, 0.0)))
    s.set_mass(RHO)
    assert "no modes held" in _refused(s, feahip.ESTATE, lambda: s.response_base_load((1.0, 0.0, 0.0)))
    assert "no modes held" in _refused(s, feahip.ESTATE, lambda: s.response_transient(g, 0.1))
    _refused(s, feahip.ESTATE, lambda: s.time_kernel(25, 1, 1))
    s.response_set_basis(lam, phi)
    assert "no load held" in _refused(s, feahip.ESTATE, lambda: s.response_transient(g, 0.1))
    # the base load
    for bad in ((0.0, 0.0, 0.0), (1.0, np.nan, 0.0), (np.inf, 0.0, 0.0)):
        assert "dir" in _refused(s, feahip.EINVAL, lambda: s.response_base_load(bad))
    assert lib.feahip_response_base_load(ctx, None, 0, 0, 1e-12, 100, None, None, None, None, None, None) == feahip.EINVAL
    assert "solver type" in _refused(s, feahip.EINVAL, lambda: s.response_base_load((1.0, 0.0, 0.0), True, 7))
    assert "max_iterations" in _refused(s, feahip.EINVAL, lambda: s.response_base_load((1.0, 0.0, 0.0), True, feahip.CG, 1e-12, 0))
    with pytest.raises(feahip.FeaHipError, match=f"error {feahip.ENOTCONVERGED}"):
        s.response_base_load((1.0, 0.0, 0.0), True, feahip.CG, 1e-14, 2)
    assert "no load held" in _refused(s, feahip.ESTATE, lambda: s.response_transient(g, 0.1))   # a failed solve leaves none
    one = (C.c_double * 3)(1.0, 0.0, 0.0)
    assert lib.feahip_response_base_load(ctx, one, 0, 0, 1e-12, 100, None, None, None, None, None, None) == 0   # every output may be NULL
    q = s.response_base_load((1.0, 0.0, 0.0), False)[0]
    assert q.shape == (3,)
    assert "no transient" in _refused(s, feahip.ESTATE, lambda: s.time_kernel(25, 1, 1))
    # the transient
    ok = s.response_transient(g, 0.1, 0.1, 0.0, None, 0, [0, n3 - 1], [0, 4])
    assert ok[2].shape == (2, 5) and ok[3].shape == (2, n3)
    assert s.time_kernel(25, 1, 2) > 0.0
    assert "no sweep" in _refused(s, feahip.ESTATE, lambda: s.time_kernel(23, 1, 1))        # its table left the buffer
    s.response_sweep([1.0], 0.1)
    assert "no transient" in _refused(s, feahip.ESTATE, lambda: s.time_kernel(25, 1, 1))    # and the other way round
    peak, at = np.zeros(n3), np.zeros(n3, dtype=np.int32)
    gp = g.ctypes.data_as(_dp)
    tail = (0.1, 0.0, None, 0, peak.ctypes.data_as(_dp), at.ctypes.data_as(_ip), 0, None, None, 0, None, None)
    for n in (0, -1, feahip.TRANSIENT_MAX_STEPS + 1):
        assert lib.feahip_response_transient(ctx, n, 0.1, gp, *tail) == feahip.EINVAL
        assert b"n_steps" in lib.feahip_last_error(ctx)
    assert lib.feahip_response_transient(ctx, 4, 0.1, None, *tail) == feahip.EINVAL
    assert lib.feahip_response_transient(ctx, 4, 0.1, gp, 0.1, 0.0, None, 0, None, at.ctypes.data_as(_ip), 0, None, None, 0, None, None) == feahip.EINVAL
    assert lib.feahip_response_transient(ctx, 4, 0.1, gp, 0.1, 0.0, None, 0, peak.ctypes.data_as(_dp), None, 0, None, None, 0, None, None) == feahip.EINVAL
    idx = np.zeros(2, dtype=np.int32)
    assert lib.feahip_response_transient(ctx, 4, 0.1, gp, 0.1, 0.0, None, 0, peak.ctypes.data_as(_dp), at.ctypes.data_as(_ip), 1, idx.ctypes.data_as(_ip), None, 0, None, None) == feahip.EINVAL
    assert lib.feahip_response_transient(ctx, 4, 0.1, gp, 0.1, 0.0, None, 0, peak.ctypes.data_as(_dp), at.ctypes.data_as(_ip), 0, None, None, 1, idx.ctypes.data_as(_ip), None) == feahip.EINVAL
    bad_g = g.copy()
    bad_g[3] = np.nan
    for kw in (dict(dt=0.0), dict(dt=-0.1), dict(dt=np.inf), dict(dt=np.nan), dict(g=bad_g), dict(g=[1.0, np.inf]),
               dict(quantity=-1), dict(quantity=3), dict(alpha=-0.1), dict(alpha=np.nan), dict(beta=-0.1), dict(beta=np.inf),
               dict(zeta=[0.0, -0.1, 0.0]), dict(zeta=np.nan),
               dict(g=np.ones(2001), dt=1.0, lam_negative=True)):           # the last: a coefficient that is not finite
        a = dict(g=g, dt=0.1, alpha=0.0, beta=0.0, zeta=None, quantity=0)
        a.update(kw)
        if a.pop("lam_negative", False):
            s.response_set_basis([-1e6, 4.0, 9.0], phi)
            s.response_load(F, False)
            assert "not finite" in _refused(s, feahip.EINVAL, lambda: s.response_transient(**a))
            s.response_set_basis(lam, phi)
            s.response_load(F, False)
        else:
            _refused(s, feahip.EINVAL, lambda: s.response_transient(**a))
    assert "n_probe" in _refused(s, feahip.EINVAL, lambda: s.response_transient(g, 0.1, probes=np.zeros(65, dtype=np.int32)))
    for bad in (-1, n3):
        assert "probe dof" in _refused(s, feahip.EINVAL, lambda: s.response_transient(g, 0.1, probes=[0, bad]))
    assert "n_snap" in _refused(s, feahip.EINVAL, lambda: s.response_transient(g, 0.1, snapshots=np.zeros(4097, dtype=np.int32)))
    for bad in (-1, 5):
        assert "snapshot step" in _refused(s, feahip.EINVAL, lambda: s.response_transient(g, 0.1, snapshots=[0, bad]))
    out = s.response_transient(g, 0.1, probes=np.arange(64), snapshots=[4, 4, 0])
    assert out[2].shape == (64, 5) and np.array_equal(out[3][0], out[3][1])
    # whatever fills or drops the store invalidates the load
    s.response_set_basis(lam, phi)
    assert "no load held" in _refused(s, feahip.ESTATE, lambda: s.response_transient(g, 0.1))
    s.response_base_load((0.0, 1.0, 0.0), False)
    s.response_transient(g, 0.1)
    s.create_stiffness_and_residual()
    s.modal_deflate(phi, np.zeros((8, n3)))
    assert "no modes held" in _refused(s, feahip.ESTATE, lambda: s.response_transient(g, 0.1))
    assert "no modes held" in _refused(s, feahip.ESTATE, lambda: s.response_base_load((0.0, 1.0, 0.0), False))
    s.solve_modes_locked(2, 0.0, 1e-6, 500)
    assert "no load held" in _refused(s, feahip.ESTATE, lambda: s.response_transient(g, 0.1))
    s.response_base_load((0.0, 1.0, 0.0), True)
    s.response_transient(g, 0.1)
    s.solve_modes_locked(2, 0.0, 1e-6, 500)
    assert "no load held" in _refused(s, feahip.ESTATE, lambda: s.response_transient(g, 0.1))
    # a row shard
    s.set_row_shard(0, 2)
    assert "row-sharded" in _refused(s, feahip.EINVAL, lambda: s.response_base_load((0.0, 1.0, 0.0), False))
    assert "row-sharded" in _refused(s, feahip.EINVAL, lambda: s.response_transient(g, 0.1))
    s.close()
    r = feahip.RankSolver(deck, 0, 2)
    assert "feahip_create_rank" in _refused(r, feahip.EINVAL, lambda: r.response_base_load((0.0, 1.0, 0.0), False))
    assert "feahip_create_rank" in _refused(r, feahip.EINVAL, lambda: r.response_transient(g, 0.1))
    r.close()


def test_feasolver_hip_runs_a_deck_with_a_transient_section(tmp_path):
    """A lateral traction on the bar's end, one load increment, twelve locked modes.  Under a step with zeta = 0.02 the
    largest displacement peaks near half the first period: the log's peak time is within one step of it.  With :base
    (1 0 0) the effective-mass lines are there and their cumulative fraction grows.  Without the section, the old output."""
    def make(**kw):
        d = loaded_bar("tet4", (3, 8, 3), density=RHO, modal_count=12, load_increments_count=1, **kw)
        d.surface_values = np.tile([0.05, 0.015, 0.0], (len(d.surface_kind), 1))
        return d
    plain = make()
    s = feahip.FeaSolver(plain)
    done, _, _ = s.solve()
    assert done == 1
    ref = ModalReference(plain, RHO, x=s.nodes())
    s.close()
    T1 = 2 * np.pi / np.sqrt(ref.lam[0])
    dt, n = T1 / 13, 26                                                 # half the first period lies between steps 6 and 7
    decks = {"plain": plain, "step": make(transient_steps=n, transient_dt=dt, transient_zeta=0.02),
             "base": make(transient_steps=n, transient_dt=dt, transient_zeta=0.02, transient_shape="half-sine",
                          transient_rise=float(f"{0.4 * T1:.3g}"), transient_base=(1.0, 0.0, 0.0))}
    exe = os.path.join(os.path.dirname(feahip.LIB_PATH), "feasolver_hip")
    out = {}
    for name, d in decks.items():
        path = tmp_path / f"{name}.sexp"
        d.save(str(path))
        out[name] = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
        assert out[name].returncode == 0, out[name].stderr
    log = out["step"].stdout
    assert re.search(r"^Transient: 26 steps of \S+, shape step, 12 modes, static correction on$", log, re.M), log
    hit = re.search(r"^Transient peak: \|u\| = (\S+) at t = (\S+), node (\d+) dof ([012])$", log, re.M)
    assert hit, log
    print("peak", hit.group(1), "at", hit.group(2), "; half the first period", T1 / 2, "step", dt)
    assert float(hit.group(1)) > 0 and abs(float(hit.group(2)) - T1 / 2) <= dt
    assert 1 <= int(hit.group(3)) <= len(plain.nodes)
    strip = lambda text: "".join(l for l in text.splitlines(True) if not l.startswith(("Transient", "Effective mass")))
    assert strip(log) == out["plain"].stdout and "Transient" not in out["plain"].stdout
    msh, old = (tmp_path / "step.msh").read_text(), (tmp_path / "plain.msh").read_text()
    assert msh.startswith(old) and "Transient" not in old
    tail = msh[len(old):]
    assert re.findall(r'^"(Transient [^"]+)"$', tail, re.M) == ["Transient peak displacement", "Transient peak time"]
    assert tail.count("$NodeData") == 2 and len(tail.splitlines()) == 2 * (len(plain.nodes) + 10)
    log = out["base"].stdout
    assert "Effective mass" not in out["step"].stdout
    lines = re.findall(r"^Effective mass: mode (\d+), gamma (\S+), m_eff (\S+), cumulative fraction (\S+) of total (\S+)$", log, re.M)
    assert [int(l[0]) for l in lines] == list(range(1, 13)), log
    frac = np.array([float(l[3]) for l in lines])
    assert np.all(np.diff(frac) >= 0) and frac[-1] > frac[0] and 0 < frac[-1] <= 1 + 1e-12
    assert all(abs(float(l[4]) - 3.0) <= 1e-9 for l in lines)
    assert re.search(r"^Transient peak: ", log, re.M) and strip(log) == out["plain"].stdout

"""Frequency response by mode superposition on the MI355X (kernels_response.hip): the projection and sweep kernels alone on
an exact basis against the complex128 restatement of tests/response_reference.py, the static correction against a dense
solve, the whole chain -- modes from feahip_solve_modes_locked -- against the dense direct solve of the damped system,
modal damping, a free body, what the entries leave of the context's state, reproducibility, refusals and stale state, and
feasolver_hip with a (harmonic ...) section."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import feahip
from dynamics_reference import loaded_bar
from modal_reference import ModalReference
from response_reference import EPS, coefficients, direct, response, rounding_bound, static_solve
from test_gpu_modal_locked import DECKS, RHO, reference, solver

pytestmark = pytest.mark.gpu

_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int)


def tip_load(deck, random_part=0.0, seed=11):
    """x = 1, y = 0.3 on the nodes of the far end (largest y), plus a seeded random part on every dof."""
    F = np.zeros((len(deck.nodes), 3))
    tip = np.abs(deck.nodes[:, 1] - deck.nodes[:, 1].max()) < 1e-12
    F[tip, 0], F[tip, 1] = 1.0, 0.3
    if random_part:
        F += random_part * np.random.default_rng(seed).standard_normal(F.shape)
    return F.reshape(-1)


def rayleigh_for(ref, m):
    """2 % at the first and the m-th reference frequency (the second for m = 1)."""
    return feahip.host_rayleigh(np.sqrt(ref.lam[0]), 0.02, np.sqrt(ref.lam[max(m, 2) - 1]), 0.02)


def frequency_lists(ref, m, correction):
    w1, wm = np.sqrt(ref.lam[0]), np.sqrt(ref.lam[m - 1])
    lo = 0.0 if correction else 0.05 * w1
    return [np.array([0.7 * w1]), np.array([lo, 0.98 * w1, 1.7 * w1]), np.linspace(lo, 1.2 * max(wm, 2.0 * w1), 257)]


def decided(mag, bound):
    """(argmax over the frequencies, the dofs whose largest value exceeds their second largest by more than 2 bound)."""
    best = mag.argmax(axis=0)
    if len(mag) == 1:
        return best, np.ones(mag.shape[1], dtype=bool)
    part = np.partition(mag, len(mag) - 2, axis=0)
    return best, part[-1] - part[-2] > 2 * bound


def check_sweep(ref, Phi, coef, u_s, omega_count, peak, at):
    """peak to the rounding bound, peak_at the restatement's argmax where that is decided, an index within the bound of
    the largest elsewhere; at least 95 % of the free dofs decided; zero on the prescribed dofs."""
    u = response(Phi, coef, u_s)
    mag, bound = np.abs(u), rounding_bound(Phi, coef, u_s).max(axis=0)
    assert mag.shape == (omega_count, len(ref.mask))
    print("peak: largest error / bound", (np.abs(peak - mag.max(axis=0))[~ref.mask] / bound[~ref.mask]).max())
    assert np.all(np.abs(peak - mag.max(axis=0)) <= bound)
    best, sure = decided(mag, bound)
    free = ~ref.mask
    print("peak_at: decided", (sure & free).sum(), "of", free.sum(), "free dofs")
    assert (sure & free).sum() >= 0.95 * free.sum()
    assert np.array_equal(at[sure & free], best[sure & free])
    assert np.all(mag[at, np.arange(len(at))] >= mag.max(axis=0) - 2 * bound)
    assert not peak[ref.mask].any() and not at[ref.mask].any()


CASES = [("fan", 1, False), ("tet10", 8, True), ("hex8", 20, True), ("tet4", 24, False), ("tet4", 64, True)]


@pytest.mark.parametrize("kind,m,correction", CASES)
def test_kernels_on_an_exact_basis(kind, m, correction):
    """A single column, a full panel, a partial last panel, three panels and all eight; 143 nodes leave a partial last
    wave.  The restatement takes the GPU's own q and u_s: both are checked on their own (q here, u_s below)."""
    ref, deck = reference(kind), DECKS[kind]()
    lam, Phi = ref.lam[:m], ref.Phi[:, :m]
    F = tip_load(deck, 0.1)
    Fm = np.where(ref.mask, 0.0, F)
    alpha, beta = rayleigh_for(ref, m)
    s = solver(deck)
    s.response_set_basis(lam, Phi.T)
    assert s.locked_count() == m and np.array_equal(s.locked_modes(), Phi.T)
    q, its, res = s.response_load(F, correction, feahip.CG, 1e-14, 20000)
    qb = len(F) * EPS * (np.abs(Phi) * np.abs(Fm)[:, None]).sum(axis=0)
    print(kind, m, "q: largest error / bound", (np.abs(q - Phi.T @ Fm) / qb).max(), "PCG", its, res)
    assert q.shape == (m,) and np.all(np.abs(q - Phi.T @ Fm) <= qb)
    u_s = s.response_static()
    assert not u_s[ref.mask].any() and (u_s.any() == bool(correction)) and (its > 0) == bool(correction)
    probes = np.array([0, 4, len(F) // 2, len(F) - 2, len(F) - 1, int(np.nonzero(ref.mask)[0][0])], dtype=np.int32)
    for omega in frequency_lists(ref, m, correction):
        coef = coefficients(lam, q, omega, alpha, beta, None, correction)
        peak, at, curve = s.response_sweep(omega, alpha, beta, None, probes)
        check_sweep(ref, Phi, coef, u_s, len(omega), peak, at)
        u, bound = response(Phi, coef, u_s), rounding_bound(Phi, coef, u_s)
        assert curve.shape == (len(probes), len(omega))
        assert np.all(np.abs(curve.real - u.real[:, probes].T) <= bound[:, probes].T)
        assert np.all(np.abs(curve.imag - u.imag[:, probes].T) <= bound[:, probes].T)
        if len(omega) == 3:
            for j, w in enumerate(omega):
                field = s.response_field(w, alpha, beta)
                print("field: largest error / bound", (np.abs(field - u[j])[~ref.mask] / bound[j][~ref.mask]).max())
                assert np.all(np.abs(field.real - u[j].real) <= bound[j]) and np.all(np.abs(field.imag - u[j].imag) <= bound[j])
                assert not field[ref.mask].any()
                assert np.array_equal(field[probes], curve[:, j])          # the host sums the probes in the kernel's order
    # the same frequency twice: the lower index on every dof
    w1 = np.sqrt(ref.lam[0])
    peak, at, _ = s.response_sweep([0.98 * w1, 0.5 * w1, 0.98 * w1], alpha, beta)
    assert at.max() <= 1 and (at == 0).any()
    s.close()


@pytest.mark.parametrize("kind", ["tet4", "hex8", "tet10"])
def test_static_vector_against_a_dense_solve(kind):
    """1e-8 of the largest entry with solver tolerance 1e-14: the bound of the PCG against a direct solve elsewhere."""
    ref, deck = reference(kind), DECKS[kind]()
    F = tip_load(deck, 0.1)
    s = solver(deck)
    s.response_set_basis(ref.lam[:3], ref.Phi[:, :3].T)
    s.response_load(F, True, feahip.CG, 1e-14, 20000)
    u, want = s.response_static(), static_solve(ref.K, ref.mask, F)
    s.close()
    print(kind, "u_s: largest error / largest entry", np.abs(u - want).max() / np.abs(want).max())
    assert np.abs(u - want).max() <= 1e-8 * np.abs(want).max()


@pytest.mark.parametrize("kind,m", [("tet4", 24), ("hex8", 20), ("tet10", 16)])
def test_end_to_end_against_the_dense_direct_solve(kind, m):
    """Modes from the locked solve, Rayleigh damping of 2 % at the first and the m-th frequency.  trunc(w) is the error of
    the restatement with the REFERENCE's first m pairs against the direct solve (DESIGN.md 21 tabulates it); the GPU
    field may add 1e-4: the eigenvalue bound 1e-6 times the resonance amplification 1 / (2 zeta) = 25 times four for
    the eigenvectors.  Errors are the largest over the dofs, relative to the largest |u| of the direct solve."""
    ref, deck = reference(kind), DECKS[kind]()
    lam, Phi = ref.lam[:m], ref.Phi[:, :m]
    F = tip_load(deck)
    alpha, beta = rayleigh_for(ref, m)
    w1 = np.sqrt(ref.lam[0])
    omega = np.array([0.0, 0.5 * w1, 0.98 * w1, np.sqrt(0.5 * (ref.lam[3] + ref.lam[4]))])
    exact = [direct(ref.K, ref.M, ref.mask, F, w, alpha, beta) for w in omega]
    q_ref = Phi.T @ np.where(ref.mask, 0.0, F)
    with_c = response(Phi, coefficients(lam, q_ref, omega, alpha, beta, None, True), static_solve(ref.K, ref.mask, F))
    without = response(Phi, coefficients(lam, q_ref, omega, alpha, beta, None, False))
    s = solver(deck)
    lam_gpu, res, steps, sweeps = s.solve_modes_locked(m, 0.0, 1e-8, 2000)
    err = {}
    for correction in (True, False):
        s.response_load(F, correction, feahip.CG, 1e-14, 20000)
        for j, w in enumerate(omega):
            field = s.response_field(w, alpha, beta)
            scale = np.abs(exact[j]).max()
            err[correction, j] = np.abs(field - exact[j]).max() / scale
            if correction:
                trunc = np.abs(with_c[j] - exact[j]).max() / scale
                print(kind, "w / w1", w / w1, "trunc", trunc, "GPU against the direct solve", err[True, j])
                assert err[True, j] <= 2 * trunc + 1e-4
            else:
                gap = np.abs(field - without[j]).max() / scale
                print(kind, "w / w1", w / w1, "uncorrected: GPU against the restatement", gap, "against the direct solve", err[False, j])
                assert gap <= 1e-4
    s.close()
    print(kind, "at 0.5 w1: uncorrected / corrected error", err[False, 1] / err[True, 1])
    assert err[False, 1] >= 10 * err[True, 1]


def test_modal_damping_alone():
    kind, m = "tet4", 24
    ref, deck = reference(kind), DECKS[kind]()
    lam, Phi = ref.lam[:m], ref.Phi[:, :m]
    F = tip_load(deck, 0.1)
    s = solver(deck)
    s.response_set_basis(lam, Phi.T)
    q, _, _ = s.response_load(F, True, feahip.CG, 1e-14, 20000)
    u_s = s.response_static()
    zeta = np.full(m, 0.02)
    omega = frequency_lists(ref, m, True)[2]
    coef = coefficients(lam, q, omega, 0.0, 0.0, zeta, True)
    peak, at, _ = s.response_sweep(omega, zeta=0.02)
    check_sweep(ref, Phi, coef, u_s, len(omega), peak, at)
    peak_b, at_b, _ = s.response_sweep(omega, zeta=zeta)                  # one ratio per mode, the same ones
    assert np.array_equal(peak, peak_b) and np.array_equal(at, at_b)
    for w in (0.98 * np.sqrt(lam[0]), np.sqrt(lam[5])):                   # the second one exactly on a resonance
        field = s.response_field(w, zeta=zeta)
        c1 = coefficients(lam, q, [w], 0.0, 0.0, zeta, True)
        u, bound = response(Phi, c1, u_s)[0], rounding_bound(Phi, c1, u_s)[0]
        assert np.all(np.abs(field.real - u.real) <= bound) and np.all(np.abs(field.imag - u.imag) <= bound)
    s.close()


def _refused(s, code, fn):
    with pytest.raises(feahip.FeaHipError) as e:
        fn()
    prefix = f"libfeahip error {code}: "
    msg = str(e.value)
    assert msg.startswith(prefix) and len(msg) > len(prefix) + 5, msg
    return msg


def test_free_body():
    """The 14 lowest pairs of the free block; eigh returns its six zero eigenvalues as +-1e-13 of either sign, they are
    installed as the zeros they are.  Such a body sweeps at w > 0 without correction; the correction and w = 0 are
    refused, and so is the correction after a solve with a shift."""
    kind, m = "free_tet4", 14
    ref, deck = reference(kind), DECKS[kind]()
    assert np.all(np.abs(ref.lam[:6]) <= 1e-9 * ref.lam[6]) and not ref.mask.any()
    lam, Phi = np.concatenate([np.zeros(6), ref.lam[6:m]]), ref.Phi[:, :m]
    F = tip_load(deck, 0.1)
    s = solver(deck)
    s.response_set_basis(lam, Phi.T)
    assert "no static correction" in _refused(s, feahip.EINVAL, lambda: s.response_load(F, True))
    q, its, _ = s.response_load(F, False)
    assert its == 0 and not s.response_static().any()
    w7 = np.sqrt(ref.lam[6])
    omega = np.array([0.3, 0.9, 1.4]) * w7
    coef = coefficients(lam, q, omega, 0.0, 0.0, np.full(m, 0.02), False)
    peak, at, _ = s.response_sweep(omega, zeta=0.02)
    check_sweep(ref, Phi, coef, None, 3, peak, at)
    u, bound = response(Phi, coef), rounding_bound(Phi, coef)
    for j, w in enumerate(omega):
        field = s.response_field(w, zeta=0.02)
        assert np.all(np.abs(field.real - u[j].real) <= bound[j]) and np.all(np.abs(field.imag - u[j].imag) <= bound[j])
    assert "not finite" in _refused(s, feahip.EINVAL, lambda: s.response_sweep([0.0, w7], zeta=0.02))
    assert "not finite" in _refused(s, feahip.EINVAL, lambda: s.response_field(0.0, zeta=0.02))
    shift = float(f"{ref.lam[6]:.1e}")
    s.solve_modes_locked(m, shift, 1e-8, 2000)
    assert "shift" in _refused(s, feahip.EINVAL, lambda: s.response_load(F, True))
    s.response_load(F, False)
    assert np.isfinite(s.response_sweep(omega, zeta=0.02)[0]).all()
    s.close()


def _run(deck, ref, F, m, omega, alpha, beta):
    s = solver(deck)
    s.response_set_basis(ref.lam[:m], ref.Phi[:, :m].T)
    q, _, _ = s.response_load(F, True, feahip.CG, 1e-14, 20000)
    peak, at, curve = s.response_sweep(omega, alpha, beta, 0.01, [7, 8])
    field = s.response_field(omega[1], alpha, beta, 0.01)
    s.close()
    return q, peak, at, curve, field


def test_state_is_left_alone_and_two_cold_runs_agree():
    kind, m = "tet4", 24
    ref, deck = reference(kind), DECKS[kind]()
    F = tip_load(deck, 0.1)
    alpha, beta = rayleigh_for(ref, m)
    omega = frequency_lists(ref, m, True)[2]
    rng = np.random.default_rng(2)
    s = solver(deck)
    s.set_velocities(rng.standard_normal((s.N, 3)))
    s.set_accelerations(rng.standard_normal((s.N, 3)))
    s.set_time(0.375)
    s.set_load_factor(0.5)
    s.response_set_basis(ref.lam[:m], ref.Phi[:, :m].T)
    state = lambda: (s.nodes(), s.velocities(), s.accelerations(), np.array(s.time()), np.array(s.load_factor()), s.locked_modes())
    before = state()
    s.response_load(F, True, feahip.CG, 1e-14, 20000)
    s.response_sweep(omega, alpha, beta, 0.01, [7, 8])
    s.response_field(omega[1], alpha, beta, 0.01)
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
    for a, b in zip(_run(deck, ref, F, m, omega, alpha, beta), _run(deck, ref, F, m, omega, alpha, beta)):
        assert np.array_equal(a, b)


def test_refusals_and_stale_state():
    kind = "tet4"
    ref, deck = reference(kind), DECKS[kind]()
    F = tip_load(deck)
    n3 = 3 * len(deck.nodes)
    lam, phi = np.array([9.0, 4.0, 25.0]), ref.Phi[:, :3].T.copy()       # any three columns serve here; lam out of order
    s = feahip.FeaSolver(deck)
    lib, ctx = s._lib, s._ctx
    assert "no mass" in _refused(s, feahip.ESTATE, lambda: s.response_set_basis(lam, phi))
    s.set_mass(RHO)
    assert "no modes held" in _refused(s, feahip.ESTATE, lambda: s.response_load(F))
    for call in (s.response_static, lambda: s.response_field(1.0), lambda: s.response_sweep([1.0])):
        assert "no modes held" in _refused(s, feahip.ESTATE, call)
    for what in (23, 24):
        _refused(s, feahip.ESTATE, lambda: s.time_kernel(what, 1, 1))
    # set_basis
    one = (C.c_double * 1)(4.0)
    buf = np.zeros(65 * n3)
    for n in (0, 65):
        assert lib.feahip_response_set_basis(ctx, n, buf.ctypes.data_as(_dp), buf.ctypes.data_as(_dp)) == feahip.EINVAL
        assert b"[1, 64]" in lib.feahip_last_error(ctx)
    assert lib.feahip_response_set_basis(ctx, 1, None, buf.ctypes.data_as(_dp)) == feahip.EINVAL
    assert lib.feahip_response_set_basis(ctx, 1, one, None) == feahip.EINVAL
    for bad in (np.nan, np.inf):
        assert "not finite" in _refused(s, feahip.EINVAL, lambda: s.response_set_basis([4.0, bad, 9.0], phi))
    s.response_set_basis(lam, phi)
    assert np.array_equal(s.locked_modes(), phi[[1, 0, 2]])             # read back ascending in lam
    # load
    assert "no load held" in _refused(s, feahip.ESTATE, lambda: s.response_sweep([1.0]))
    assert "no load held" in _refused(s, feahip.ESTATE, lambda: s.response_static())
    for bad in (np.nan, np.inf):
        G = F.copy()
        G[5] = bad
        assert "not finite" in _refused(s, feahip.EINVAL, lambda: s.response_load(G))
    assert lib.feahip_response_load(ctx, None, 1, 0, 1e-12, 100, None, None, None) == feahip.EINVAL
    assert "solver type" in _refused(s, feahip.EINVAL, lambda: s.response_load(F, True, 7))
    assert "max_iterations" in _refused(s, feahip.EINVAL, lambda: s.response_load(F, True, feahip.CG, 1e-12, 0))
    with pytest.raises(feahip.FeaHipError, match=f"error {feahip.ENOTCONVERGED}"):
        s.response_load(F, True, feahip.CG, 1e-14, 2)
    assert "no load held" in _refused(s, feahip.ESTATE, lambda: s.response_sweep([1.0]))   # a failed solve leaves none
    q, _, _ = s.response_load(F, False)
    assert q.shape == (3,)
    assert "no sweep" in _refused(s, feahip.ESTATE, lambda: s.time_kernel(23, 1, 1))
    # sweep
    ok = s.response_sweep([1.0, 2.5], 0.1, 0.0, None, [0, n3 - 1])
    assert ok[2].shape == (2, 2)
    for what in (23, 24):
        assert s.time_kernel(what, 1, 2) > 0.0
    peak, at = np.zeros(n3), np.zeros(n3, dtype=np.int32)
    om = np.linspace(1.0, 2.0, 4097)
    args = (0.1, 0.0, None, peak.ctypes.data_as(_dp), at.ctypes.data_as(_ip), 0, None, None, None)
    for n in (0, 4097):
        assert lib.feahip_response_sweep(ctx, n, om.ctypes.data_as(_dp), *args) == feahip.EINVAL
        assert b"n_freq" in lib.feahip_last_error(ctx)
    assert lib.feahip_response_sweep(ctx, 1, None, *args) == feahip.EINVAL
    for kw in (dict(omega=[-1.0]), dict(omega=[1.0, np.nan]), dict(omega=[np.inf]), dict(alpha=-0.1), dict(alpha=np.nan),
               dict(beta=-0.1), dict(beta=np.inf), dict(zeta=[0.0, -0.1, 0.0]), dict(zeta=np.nan),
               dict(omega=[2.0]), dict(omega=[5.0], zeta=0.0)):                      # the last two: w^2 = lam_k undamped
        a = dict(omega=[1.0], alpha=0.0, beta=0.0, zeta=None)
        a.update(kw)
        _refused(s, feahip.EINVAL, lambda: s.response_sweep(a["omega"], a["alpha"], a["beta"], a["zeta"]))
        _refused(s, feahip.EINVAL, lambda: s.response_field(a["omega"][-1], a["alpha"], a["beta"], a["zeta"]))
    assert np.isfinite(s.response_sweep([2.0], 0.1)[0]).all()            # the same resonance with damping
    assert "n_probe" in _refused(s, feahip.EINVAL, lambda: s.response_sweep([1.0], 0.1, probes=np.zeros(65, dtype=np.int32)))
    for bad in (-1, n3):
        assert "probe dof" in _refused(s, feahip.EINVAL, lambda: s.response_sweep([1.0], 0.1, probes=[0, bad]))
    assert s.response_sweep([1.0], 0.1, probes=np.arange(64))[2].shape == (64, 1)
    # whatever fills or drops the store invalidates the load
    s.response_set_basis(lam, phi)
    assert "no load held" in _refused(s, feahip.ESTATE, lambda: s.response_sweep([1.0], 0.1))
    s.response_load(F, False)
    s.response_sweep([1.0], 0.1)
    s.create_stiffness_and_residual()
    s.modal_deflate(phi, np.zeros((8, n3)))
    assert "no modes held" in _refused(s, feahip.ESTATE, lambda: s.response_sweep([1.0], 0.1))
    assert "no modes held" in _refused(s, feahip.ESTATE, lambda: s.response_load(F, False))
    s.solve_modes_locked(2, 0.0, 1e-6, 500)
    assert "no load held" in _refused(s, feahip.ESTATE, lambda: s.response_field(1.0, 0.1))
    s.response_load(F, True)
    s.response_field(1.0, 0.1)
    s.solve_modes_locked(2, 0.0, 1e-6, 500)
    assert "no load held" in _refused(s, feahip.ESTATE, lambda: s.response_field(1.0, 0.1))
    # a row shard
    s.set_row_shard(0, 2)
    assert "row-sharded" in _refused(s, feahip.EINVAL, lambda: s.response_load(F, False))
    assert "row-sharded" in _refused(s, feahip.EINVAL, lambda: s.response_set_basis(lam, phi))
    s.close()
    r = feahip.RankSolver(deck, 0, 2)
    assert "feahip_create_rank" in _refused(r, feahip.EINVAL, lambda: r.response_load(np.ones(r.ndof), False))
    r.close()


def test_feasolver_hip_sweeps_a_deck_with_a_harmonic_section(tmp_path):
    """A lateral traction on the bar's end, one load increment, twelve locked modes, 101 frequencies over 0.5 .. 1.5 of
    the first natural frequency with zeta = 0.02: the two log lines, the two sections of the .msh file, the peak within one
    grid step of the first reference frequency at the state reached; without the section, the old output."""
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
    f1 = np.sqrt(ref.lam[0]) / (2 * np.pi)
    f0, f2, n = float(f"{0.5 * f1:.3g}"), float(f"{1.5 * f1:.3g}"), 101
    deck = make(harmonic_count=n, harmonic_from=f0, harmonic_to=f2, harmonic_zeta=0.02)
    exe = os.path.join(os.path.dirname(feahip.LIB_PATH), "feasolver_hip")
    out = {}
    for name, d in (("plain", plain), ("harmonic", deck)):
        path = tmp_path / f"{name}.sexp"
        d.save(str(path))
        out[name] = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
        assert out[name].returncode == 0, out[name].stderr
    log = out["harmonic"].stdout
    assert re.search(r"^Harmonic: 101 frequencies \S+ \.\. \S+ Hz, 12 modes, static correction on$", log, re.M), log
    hit = re.search(r"^Harmonic peak: \|u\| = (\S+) at f = (\S+) Hz, node (\d+) dof ([012])$", log, re.M)
    assert hit, log
    step = (f2 - f0) / (n - 1)
    print("peak", hit.group(1), "at", hit.group(2), "Hz; first reference frequency", f1, "grid step", step)
    assert float(hit.group(1)) > 0 and abs(float(hit.group(2)) - f1) <= step
    assert 1 <= int(hit.group(3)) <= len(deck.nodes)
    strip = lambda text: "".join(l for l in text.splitlines(True) if not l.startswith("Harmonic"))
    assert strip(log) == out["plain"].stdout and "Harmonic" not in out["plain"].stdout
    msh, old = (tmp_path / "harmonic.msh").read_text(), (tmp_path / "plain.msh").read_text()
    assert msh.startswith(old) and "Harmonic" not in old
    tail = msh[len(old):]
    assert re.findall(r'^"(Harmonic [^"]+)"$', tail, re.M) == ["Harmonic peak amplitude", "Harmonic peak frequency"]
    assert tail.count("$NodeData") == 2 and len(tail.splitlines()) == 2 * (len(deck.nodes) + 10)

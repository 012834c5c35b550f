"""Stress peaks over a frequency sweep or a transient on the MI355X (kernels_stress_sweep.hip) against the float64
restatement of tests/stress_sweep_reference.py: the five stores of tests/test_gpu_response.py under its frequency lists and
the histories of tests/test_gpu_transient.py, single rows against feahip_response_stress_field bit for bit, histories that
need a second launch, the selection by material, what the entries leave of the context's state, reproducibility, a permuted
installation, refusals and hooks 29 and 30, and feasolver_hip on a deck with :stress t in (harmonic ...) and (transient ...).

T and T_s come from the library's getters (checked on their own in tests/test_gpu_modal_stress.py), q from the load, the
tables from the library's host entries; tests/test_stress_sweep_reference_cpu.py holds the precondition of the index checks.

Measured on the MI355X (largest error over its bound, every case): see the printed lines; the figures of one run are in
DESIGN.md section 25."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import feahip
import stress_sweep_reference as ssr
from dynamics_reference import loaded_bar
from hetero_reference import MATERIALS, layered_ids, with_materials
from modal_reference import ModalReference
from stress_sweep_cases import (CASES, CHUNK, CHUNK_CASES, chunk_histories, frequency_lists, histories, sweep_table,
                                transient_table)
from test_gpu_modal_locked import DECKS, RHO, reference, solver
from test_gpu_modal_stress import held
from test_gpu_response import _refused, rayleigh_for, tip_load
from test_gpu_transient import half_sine, period

pytestmark = pytest.mark.gpu

_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int)


def probes_of(N):
    return np.array([0, 1, N // 2, N - 1], dtype=np.int32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def rows_of(n):
    return sorted({0, n // 2, n - 1})


def check_sweep(what, s, lam, q, T, Ts, damping, correction, omega, keep=None):
    """One sweep against the restatement; three of its rows against feahip_response_stress_field."""
    N = T.shape[1]
    probes = probes_of(N)
    coef = sweep_table(lam, q, omega, damping, correction)
    peak6, at6, vm, vat, curves = s.response_stress_sweep(omega, *damping, None, probes)
    mag, b6, vmr, bvm = ssr.sweep_values(T, Ts, coef)
    ssr.check_peaks(f"{what} peak6", mag, b6, peak6, at6, None if keep is None else keep[:, None])
    ssr.check_peaks(f"{what} vm", vmr, bvm, vm, vat, keep)
    comp, e = ssr.components(T, Ts, coef), ssr.component_bound(T, Ts, coef)
    assert curves.shape == (len(probes), len(omega), 6)
    assert np.all(np.abs(curves.real - comp.real[:, probes].transpose(1, 0, 2)) <= e[:, probes].transpose(1, 0, 2))
    assert np.all(np.abs(curves.imag - comp.imag[:, probes].transpose(1, 0, 2)) <= e[:, probes].transpose(1, 0, 2))
    for j in rows_of(len(omega)):
        fr, _ = s.response_stress_field(coef[j].real, 1.0)
        fi, _ = s.response_stress_field(coef[j].imag, 0.0)
        assert same_bits(curves[:, j].real, fr[probes]) and same_bits(curves[:, j].imag, fi[probes])
        field = fr + 1j * fi
        hit = at6 == j
        assert np.all(np.abs(np.abs(field) - peak6)[hit] <= b6[j][hit])
        hit = vat == j
        assert np.all(np.abs(ssr.harmonic_peak(field) - vm)[hit] <= bvm[j][hit])
    return peak6, at6, vm, vat, curves


def check_transient(what, s, lam, q, T, Ts, damping, correction, g, dt, rows=None, keep=None):
    """One history against the restatement; some of its rows against feahip_response_stress_field."""
    N = T.shape[1]
    probes = probes_of(N)
    coef = transient_table(lam, q, g, dt, damping, correction)
    peak6, at6, vm, vat, hist = s.response_stress_transient(g, dt, *damping, None, probes)
    mag, b6, vmr, bvm = ssr.transient_values(T, Ts, coef, g)
    ssr.check_peaks(f"{what} peak6", mag, b6, peak6, at6, None if keep is None else keep[:, None])
    ssr.check_peaks(f"{what} vm", vmr, bvm, vm, vat, keep)
    comp, e = ssr.components(T, Ts, coef, g), ssr.component_bound(T, Ts, coef, g)
    assert hist.shape == (len(probes), len(g), 6)
    assert np.all(np.abs(hist - comp[:, probes].transpose(1, 0, 2)) <= e[:, probes].transpose(1, 0, 2))
    for n in rows_of(len(g)) if rows is None else rows:
        f6, fvm = s.response_stress_field(coef[n], g[n])
        assert same_bits(hist[:, n], f6[probes])
        hit = at6 == n
        assert np.all(np.abs(np.abs(f6) - peak6)[hit] <= b6[n][hit])
        hit = vat == n
        assert np.all(np.abs(fvm - vm)[hit] <= bvm[n][hit])
    return peak6, at6, vm, vat, hist


# ---- 1. the kernels on the five stores ----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,m,correction", CASES)
def test_sweep_against_the_restatement(kind, m, correction):
    """A single column, a full panel, a partial last panel, three panels and all eight; the fan's 143 nodes leave a last
    wave with 3 of its 10 nodes.  1, 3 and 257 frequencies."""
    ref, s, lam, q, T, Ts, damping = held(kind, m, correction)
    for omega in frequency_lists(ref, m, correction):
        check_sweep(f"{kind} {m} modes, {len(omega)} frequencies:", s, lam, q, T, Ts, damping, correction, omega)
    # the same frequency twice: the lower index everywhere
    w1 = np.sqrt(lam[0])
    _, at6, _, vat, _ = s.response_stress_sweep([0.98 * w1, 0.5 * w1, 0.98 * w1], *damping)
    assert at6.max() <= 1 and vat.max() <= 1 and (vat == 0).any()
    s.close()


@pytest.mark.parametrize("kind,m,correction", CASES)
def test_transient_against_the_restatement(kind, m, correction):
    """1, 3 and 257 steps of the half-sine of 0.4 T1 and of the step."""
    ref, s, lam, q, T, Ts, damping = held(kind, m, correction)
    for name, g, dt in histories(ref):
        check_transient(f"{kind} {m} modes, {name}:", s, lam, q, T, Ts, damping, correction, g, dt)
    # the same value at every step: the lowest step everywhere
    peak6, at6, vm, vat, _ = s.response_stress_transient(np.zeros(40), histories(ref)[0][2], *damping)
    assert not peak6.any() and not at6.any() and not vm.any() and not vat.any()
    s.close()


@pytest.mark.parametrize("kind,m,correction", CHUNK_CASES)
def test_a_history_that_needs_a_second_launch(kind, m, correction):
    """FEA_TRANSIENT_CHUNK + 3 steps: the second launch takes four rows and continues from the peaks of the first.  The
    early half-sine has every peak in the first chunk; the late one has peaks in the second, and on the TET10 bar some in
    the last rows of the first as well."""
    ref, s, lam, q, T, Ts, damping = held(kind, m, correction)
    for name, g, dt in chunk_histories(ref):
        rows = [0, CHUNK - 1, CHUNK, CHUNK + 3]
        _, at6, _, vat, _ = check_transient(f"{kind} {m} modes, {name}:", s, lam, q, T, Ts, damping, correction, g, dt, rows)
        print(name, "vm_at", vat.min(), "..", vat.max())
        if name.startswith("early"):
            assert vat.max() < CHUNK
        else:
            assert (vat >= CHUNK).any() and (at6 >= CHUNK).any()
    s.close()


# ---- 2. the selection by material -----------------------------------------------------------------------------------------
def test_selection_by_material():
    """Three layers along the bar, the store of material 1 alone: the nodes that touch none of its elements get exactly 0
    and index 0, and are left out of the decided share."""
    base = loaded_bar("tet4", (2, 4, 2))
    ids = layered_ids(base)
    deck = with_materials(base, MATERIALS, ids)
    m = 12
    s = solver(deck)
    lam = s.solve_modes_locked(m, 0.0, 1e-8, 2000)[0]
    q, _, _ = s.response_load(tip_load(deck, 0.1), True, feahip.CG, 1e-14, 20000)
    s.response_stress_basis(1)
    T, Ts = s.modal_stresses(), s.response_static_stress()
    outside = ~np.isin(np.arange(len(deck.nodes)), deck.elements[ids == 1])
    assert outside.any() and not outside.all() and not T[:, outside].any() and not Ts[outside].any()
    damping = feahip.host_rayleigh(np.sqrt(lam[0]), 0.02, np.sqrt(lam[-1]), 0.02)
    omega = np.linspace(0.0, 1.2 * np.sqrt(lam[-1]), 65)
    peak6, at6, vm, vat, _ = check_sweep("material 1, sweep:", s, lam, q, T, Ts, damping, True, omega, ~outside)
    assert not peak6[outside].any() and not at6[outside].any() and not vm[outside].any() and not vat[outside].any()
    assert vm[~outside].all()
    T1 = 2 * np.pi / np.sqrt(lam[0])
    dt = 3 * T1 / 257
    g = half_sine(258, dt, 0.4 * T1)
    peak6, at6, vm, vat, _ = check_transient("material 1, transient:", s, lam, q, T, Ts, damping, True, g, dt, None, ~outside)
    assert not peak6[outside].any() and not at6[outside].any() and not vm[outside].any() and not vat[outside].any()
    s.close()


# ---- 3. state, reproducibility, a permuted installation ------------------------------------------------------------------
def _run(deck, lam, phi, omega, g, dt, alpha, beta):
    s = solver(deck)
    s.response_set_basis(lam, phi)
    s.response_base_load((1.0, 0.5, 0.0), True, feahip.CG, 1e-14, 20000)
    s.response_stress_basis()
    out = (*s.response_stress_sweep(omega, alpha, beta, 0.01, [0, 5]), *s.response_stress_transient(g, dt, alpha, beta, 0.01, [0, 5]))
    s.close()
    return out


def test_state_is_left_alone_and_two_cold_runs_agree():
    kind, m = "tet4", 24
    ref, deck = reference(kind), DECKS[kind]()
    alpha, beta = rayleigh_for(ref, m)
    omega = np.linspace(0.0, 1.2 * np.sqrt(ref.lam[m - 1]), 33)
    T1 = period(ref)
    g, dt = half_sine(41, T1 / 40, 0.4 * T1), T1 / 40
    rng = np.random.default_rng(2)
    s = solver(deck)
    s.set_velocities(rng.standard_normal((s.N, 3)))
    s.set_accelerations(rng.standard_normal((s.N, 3)))
    s.set_time(0.375)
    s.set_load_factor(0.5)
    s.response_set_basis(ref.lam[:m], ref.Phi[:, :m].T)
    s.response_base_load((1.0, 0.5, 0.0), True, feahip.CG, 1e-14, 20000)
    s.response_stress_basis()
    state = lambda: (s.nodes(), s.velocities(), s.accelerations(), np.array(s.time()), np.array(s.load_factor()), s.locked_modes(),
                     s.response_static(), s.forces(), s.solution(), s.matrix_yale()[2], s.modal_stresses(), s.response_static_stress())

    def both_entries():
        s.response_stress_sweep(omega, alpha, beta, 0.01, [3])
        assert s.time_kernel(29, 1, 2) > 0.0                              # (the two share the stress entries' own table)
        s.response_stress_transient(g, dt, alpha, beta, 0.01, [3])
        assert s.time_kernel(30, 1, 2) > 0.0

    # the table of the displacement sweep (hook 23) and the two forms (hooks 26 and 28) stay
    sweep = s.response_sweep(omega[:9], alpha, beta, 0.01)
    combined = s.response_combine(np.eye(m), np.ones(m), 1.0)
    stress_combined = s.response_stress_combine(np.eye(m), np.ones(m), 1.0)
    before = state()
    both_entries()
    assert s.time_kernel(23, 1, 2) > 0.0 and s.time_kernel(26, 1, 2) > 0.0 and s.time_kernel(28, 1, 2) > 0.0
    for a, b in zip(before, state()):
        assert np.array_equal(a, b)
    for a, b in zip(sweep, s.response_sweep(omega[:9], alpha, beta, 0.01)):
        assert np.array_equal(a, b)
    assert np.array_equal(combined, s.response_combine(np.eye(m), np.ones(m), 1.0))
    for a, b in zip(stress_combined, s.response_stress_combine(np.eye(m), np.ones(m), 1.0)):
        assert np.array_equal(a, b)
    # the last chunk of a displacement transient (hook 25): it shares the buffer of the sweep's table, so a phase of its own
    trans = s.response_transient(g, dt, alpha, beta, 0.01)
    both_entries()
    assert s.time_kernel(25, 1, 2) > 0.0 and s.time_kernel(26, 1, 2) > 0.0 and s.time_kernel(28, 1, 2) > 0.0
    for a, b in zip(trans, s.response_transient(g, dt, alpha, beta, 0.01)):
        assert np.array_equal(a, b)
    for a, b in zip(before, state()):
        assert np.array_equal(a, b)
    # the hooks write the peak buffers only: the entries give the same bits after them
    first = s.response_stress_sweep(omega, alpha, beta, 0.01, [3])
    assert s.time_kernel(29, 1, 2) > 0.0
    for a, b in zip(first, s.response_stress_sweep(omega, alpha, beta, 0.01, [3])):
        assert np.array_equal(a, b)
    s.close()
    lam, phi = ref.lam[:m], ref.Phi[:, :m].T
    cold = _run(deck, lam, phi, omega, g, dt, alpha, beta)
    for a, b in zip(cold, _run(deck, lam, phi, omega, g, dt, alpha, beta)):
        assert np.array_equal(a, b)


def test_a_permuted_installation_gives_the_bits_of_the_ascending_one():
    """The same pairs listed in another order: every output of both entries to the bit.  The sums run one fma per store
    column in ascending column order, and feahip_response_set_basis puts the pairs into the store by ascending lam whatever
    order the caller lists them in, so the terms are added in the same order."""
    kind, m = "tet4", 24
    ref, deck = reference(kind), DECKS[kind]()
    alpha, beta = rayleigh_for(ref, m)
    omega = np.linspace(0.0, 1.2 * np.sqrt(ref.lam[m - 1]), 33)
    T1 = period(ref)
    g, dt = half_sine(41, T1 / 40, 0.4 * T1), T1 / 40
    lam, phi = ref.lam[:m], ref.Phi[:, :m].T
    perm = np.random.default_rng(3).permutation(m)
    a, b = _run(deck, lam, phi, omega, g, dt, alpha, beta), _run(deck, lam[perm], phi[perm], omega, g, dt, alpha, beta)
    names = ("sweep peak6", "sweep peak6_at", "sweep vm", "sweep vm_at", "sweep curves", "transient peak6", "transient peak6_at",
             "transient vm", "transient vm_at", "transient histories")
    for name, x, y in zip(names, a, b):
        print(name, "entries that differ", int((x != y).sum()), "of", x.size, "; largest difference / largest entry",
              float(np.abs(x - y).max() / max(np.abs(x).max(), 1e-300)))
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


# ---- 4. refusals and hooks ------------------------------------------------------------------------------------------------
def _raw_sweep(s, omega, n_freq=None, probes=(), n_probe=None):
    """The C entry on arrays filled with a sentinel: (return code, the six output arrays)."""
    N = s.ndof // 3
    omega = np.ascontiguousarray(omega, dtype=np.float64)
    pr = np.ascontiguousarray(probes, dtype=np.int32)
    k = len(pr) if n_probe is None else n_probe
    d = [np.full((N, 6), -7.0), np.full(N, -7.0), np.full((max(k, 1), max(len(omega), 1), 6), -7.0), np.full((max(k, 1), max(len(omega), 1), 6), -7.0)]
    i = [np.full((N, 6), -7, dtype=np.int32), np.full(N, -7, dtype=np.int32)]
    rc = s._lib.feahip_response_stress_sweep(s._ctx, len(omega) if n_freq is None else n_freq, omega.ctypes.data_as(_dp), 0.0, 0.0, None,
                                             d[0].ctypes.data_as(_dp), i[0].ctypes.data_as(_ip), d[1].ctypes.data_as(_dp),
                                             i[1].ctypes.data_as(_ip), k, pr.ctypes.data_as(_ip), d[2].ctypes.data_as(_dp),
                                             d[3].ctypes.data_as(_dp))
    return rc, d + i


def _raw_transient(s, g, dt, n_steps=None, probes=(), n_probe=None):
    N = s.ndof // 3
    g = np.ascontiguousarray(g, dtype=np.float64)
    pr = np.ascontiguousarray(probes, dtype=np.int32)
    k = len(pr) if n_probe is None else n_probe
    d = [np.full((N, 6), -7.0), np.full(N, -7.0), np.full((max(k, 1), len(g), 6), -7.0)]
    i = [np.full((N, 6), -7, dtype=np.int32), np.full(N, -7, dtype=np.int32)]
    rc = s._lib.feahip_response_stress_transient(s._ctx, len(g) - 1 if n_steps is None else n_steps, dt, g.ctypes.data_as(_dp), 0.0, 0.0,
                                                 None, d[0].ctypes.data_as(_dp), i[0].ctypes.data_as(_ip), d[1].ctypes.data_as(_dp),
                                                 i[1].ctypes.data_as(_ip), k, pr.ctypes.data_as(_ip), d[2].ctypes.data_as(_dp))
    return rc, d + i


def _untouched(s, code, part, got):
    rc, arrays = got
    msg = s._lib.feahip_last_error(s._ctx).decode()
    assert rc == code and part in msg and len(msg) > 10, (rc, msg)
    assert all((a == -7).all() for a in arrays)


def test_refusals_and_hooks():
    kind = "tet4"
    ref, deck = reference(kind), DECKS[kind]()
    F = tip_load(deck)
    N = len(deck.nodes)
    lam, phi = np.array([9.0, 4.0, 25.0]), ref.Phi[:, :3].T.copy()
    omega, g, dt = np.array([0.5, 1.0, 1.5]), np.ones(5), 0.1
    s = feahip.FeaSolver(deck)
    s.set_mass(RHO)
    entries = (lambda: s.response_stress_sweep(omega, 0.1), lambda: s.response_stress_transient(g, dt, 0.1))
    hooks = (lambda: s.time_kernel(29, 1, 1), lambda: s.time_kernel(30, 1, 1))
    for call in (*entries, *hooks):
        assert "no modes held" in _refused(s, feahip.ESTATE, call)
    _untouched(s, feahip.ESTATE, "no modes held", _raw_sweep(s, omega))
    _untouched(s, feahip.ESTATE, "no modes held", _raw_transient(s, g, dt))
    s.response_set_basis(lam, phi)
    for call in (*entries, *hooks):
        assert "no load held" in _refused(s, feahip.ESTATE, call)
    s.response_load(F, True)
    for call in (*entries, *hooks):                                      # no basis
        assert "no stress store" in _refused(s, feahip.ESTATE, call)
    _untouched(s, feahip.ESTATE, "no stress store", _raw_sweep(s, omega))
    s.response_stress_basis()
    s.response_load(F, True)                                             # a stale basis after a new load
    for call in (*entries, *hooks):
        assert "a load was made" in _refused(s, feahip.ESTATE, call)
    _untouched(s, feahip.ESTATE, "a load was made", _raw_transient(s, g, dt))
    s.response_stress_basis()
    # hooks 29 and 30 before a sweep or a transient, and after
    assert "no stress sweep" in _refused(s, feahip.ESTATE, hooks[0])
    assert "no stress transient" in _refused(s, feahip.ESTATE, hooks[1])
    # the arguments
    _untouched(s, feahip.EINVAL, "n_freq", _raw_sweep(s, omega, n_freq=0))
    _untouched(s, feahip.EINVAL, "n_freq", _raw_sweep(s, np.ones(4097)))
    _untouched(s, feahip.EINVAL, "omega", _raw_sweep(s, [0.5, -1.0, 1.5]))
    _untouched(s, feahip.EINVAL, "not finite", _raw_sweep(s, [0.5, 2.0, 1.5]))           # w^2 = lam_k = 4, undamped
    _untouched(s, feahip.EINVAL, "probe node", _raw_sweep(s, omega, probes=[0, N]))
    _untouched(s, feahip.EINVAL, "probe node", _raw_sweep(s, omega, probes=[-1]))
    _untouched(s, feahip.EINVAL, "n_probe", _raw_sweep(s, omega, probes=np.zeros(65), n_probe=65))
    _untouched(s, feahip.EINVAL, "n_steps", _raw_transient(s, g, dt, n_steps=0))
    _untouched(s, feahip.EINVAL, "dt", _raw_transient(s, g, 0.0))
    _untouched(s, feahip.EINVAL, "probe node", _raw_transient(s, g, dt, probes=[N]))
    _untouched(s, feahip.EINVAL, "n_probe", _raw_transient(s, g, dt, probes=np.zeros(65), n_probe=65))
    bad = g.copy()
    bad[2] = np.nan
    _untouched(s, feahip.EINVAL, "response_stress_transient", _raw_transient(s, bad, dt))
    assert "no stress sweep" in _refused(s, feahip.ESTATE, hooks[0])     # a refused call leaves no table
    rc, arrays = _raw_sweep(s, omega, probes=[0, N - 1])
    assert rc == 0 and all(np.isfinite(a).all() and (a != -7).all() for a in arrays)
    assert s.time_kernel(29, 1, 2) > 0.0
    assert "no stress transient" in _refused(s, feahip.ESTATE, hooks[1])
    rc, arrays = _raw_transient(s, g, dt, probes=[0, N - 1])
    assert rc == 0 and all(np.isfinite(a).all() and (a != -7).all() for a in arrays)
    assert s.time_kernel(30, 1, 2) > 0.0
    assert "no stress sweep" in _refused(s, feahip.ESTATE, hooks[0])     # the transient's chunk took the table's place
    # a new filling of the locked store drops the table with the stress store
    s.response_stress_sweep(omega, 0.1)
    s.response_set_basis(lam, phi)
    s.response_load(F, True)
    s.response_stress_basis()
    assert "no stress sweep" in _refused(s, feahip.ESTATE, hooks[0])
    # a row shard, a rank context
    s.set_row_shard(0, 2)
    for call in (*entries, *hooks):
        assert "row-sharded" in _refused(s, feahip.EINVAL, call)
    s.close()
    r = feahip.RankSolver(deck, 0, 2)
    assert "feahip_create_rank" in _refused(r, feahip.EINVAL, lambda: r.response_stress_sweep(omega, 0.1))
    assert "feahip_create_rank" in _refused(r, feahip.EINVAL, lambda: r.response_stress_transient(g, dt, 0.1))
    r.close()


# ---- 5. the command line --------------------------------------------------------------------------------------------------
def test_feasolver_hip_runs_a_deck_with_the_stress_key(tmp_path):
    """A (3, 8, 3) TET4 bar under a lateral traction, twelve locked modes, (harmonic ...) and (transient ...) with :stress t:
    the two log lines and the two one-component $NodeData sections behind the old ones, whose largest entry is the logged
    value at the logged node, the values against the Python entries on the same state, and without the key the old output
    byte for byte."""
    def make(**kw):
        d = loaded_bar("tet4", (3, 8, 3), density=RHO, modal_count=12, load_increments_count=1, **kw)
        d.surface_values = np.tile([0.05, 0.015, 0.0], (len(d.surface_kind), 1))
        return d
    plain = make()
    s = feahip.FeaSolver(plain)
    done, _, _ = s.solve()
    assert done == 1
    lam1 = ModalReference(plain, RHO, x=s.nodes()).lam[0]
    s.close()
    f1, T1 = np.sqrt(lam1) / (2 * np.pi), 2 * np.pi / np.sqrt(lam1)
    sections = dict(harmonic_count=33, harmonic_from=float(f"{0.5 * f1:.3g}"), harmonic_to=float(f"{1.5 * f1:.3g}"), harmonic_zeta=0.02,
                    transient_steps=120, transient_dt=float(f"{T1 / 40:.3g}"), transient_shape="half-sine",
                    transient_rise=float(f"{0.4 * T1:.3g}"), transient_zeta=0.02)
    decks = {"old": make(**sections), "stress": make(**sections, harmonic_stress=True, transient_stress=True)}
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
    assert titles[-6:] == ["Harmonic peak amplitude", "Harmonic peak frequency", "Harmonic peak von Mises stress",
                           "Transient peak displacement", "Transient peak time", "Transient peak von Mises stress"]
    lines = out["stress"].stdout.splitlines()
    order = [k for k, l in enumerate(lines) if l.startswith(("Harmonic peak:", "Harmonic peak von Mises:", "Transient peak:", "Transient peak von Mises:"))]
    assert len(order) == 4 and [lines[k].split(":")[0] for k in order] == ["Harmonic peak", "Harmonic peak von Mises", "Transient peak", "Transient peak von Mises"]
    got, where = {}, {}
    for title, pattern in (("Harmonic peak von Mises stress", r"^Harmonic peak von Mises: vm = (\S+), node (\d+), f = (\S+) Hz$"),
                           ("Transient peak von Mises stress", r"^Transient peak von Mises: vm = (\S+), node (\d+), t = (\S+)$")):
        hit = re.search(pattern, out["stress"].stdout, re.M)
        assert hit, out["stress"].stdout
        body = new[new.index(f'"{title}"'):].splitlines()
        assert body[5] == "1" and body[6] == str(n_nodes) and body[7 + n_nodes] == "$EndNodeData"
        rows = np.array([float(l.split()[1]) for l in body[7:7 + n_nodes]])
        vm, node = float(hit.group(1)), int(hit.group(2))
        print(title, vm, "node", node, "at", hit.group(3))
        assert vm > 0 and abs(rows.max() - vm) <= 1e-9 * vm and abs(rows[node - 1] - vm) <= 1e-9 * vm
        got[title], where[title] = rows, (node, float(hit.group(3)))
    # the Python entries on the state the command line reached: the solved nodes, its modes, the surface load
    d = decks["stress"]
    s = feahip.FeaSolver(d)
    s.set_mass(RHO)
    done, _, _ = s.solve(load_increments=1)
    assert done == 1
    s.solve_modes_locked(12, 0.0, d.modal_tolerance, d.modal_max)
    s.response_load(s.surface_forces(), True)
    s.response_stress_basis()
    two_pi = 6.283185307179586
    freq = np.array([d.harmonic_from + (d.harmonic_to - d.harmonic_from) * k / (d.harmonic_count - 1) for k in range(d.harmonic_count)])
    _, _, hvm, hat, _ = s.response_stress_sweep(two_pi * freq, 0.0, 0.0, 0.02)
    t = np.arange(d.transient_steps + 1) * d.transient_dt
    g = np.where(t < d.transient_rise, np.sin(np.pi * t / d.transient_rise), 0.0)
    _, _, tvm, tat, _ = s.response_stress_transient(g, d.transient_dt, 0.0, 0.0, 0.02)
    for title, mine, at, scale in (("Harmonic peak von Mises stress", hvm, freq[hat], 1.0), ("Transient peak von Mises stress", tvm, tat * d.transient_dt, 1.0)):
        want = got[title]
        print(title, "command line against Python", np.abs(mine - want).max() / want.max())
        assert np.all(np.abs(mine - want) <= 1e-9 * want.max())
        node, x = where[title]
        assert abs(at[node - 1] - x) <= 1e-12 * max(abs(x), 1.0)
    s.close()

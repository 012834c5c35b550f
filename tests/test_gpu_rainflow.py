"""Rainflow counting of a transient on the MI355X (kernels_stress_rainflow.hip): the five stores of tests/test_gpu_response.py
under the histories of tests/rainflow_cases.py.  At the probe nodes the device's count must equal feahip.host_rainflow of
the returned history in everything but the rounding of the damage sum; at every node it is held to the count of the float64
restatement's histories wherever the bounds e_c of tests/stress_sweep_reference.py decide the reversals and the closures
(tests/test_rainflow_reference_cpu.py holds the preconditions).  Projections in one and in two passes, histories that need a
second launch, a ring of four points, a depth that grows between calls, the selection by material, reproducibility, what
the entry leaves of the context's state, refusals and hook 33, and feasolver_hip on a deck with the three keys in
(transient ... :stress t).

The damage tolerance at a probe is k (c + b + 4) EPS of the long-double sum over the host's list, c the cycles counted, with
k = 2: the power of the device measured here on the one-step histories, where the damage is a single half cycle, for a whole
exponent (squaring and multiplying) and for b = 3.5 (pow), both within 2 units in the last place (printed by
test_count_on_the_five_stores; DESIGN.md section 27 has the figures of one run)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import feahip
import rainflow_reference as rr
from dynamics_reference import loaded_bar
from hetero_reference import MATERIALS, layered_ids, with_materials
from modal_reference import ModalReference
from rainflow_cases import CASES, CHUNK, CHUNK_CASES, DEPTH, SN, STEP_CASE, chunk_histories, count_all, histories, rows_of, two_tone
from stress_sweep_cases import transient_table
from test_gpu_modal_locked import DECKS, RHO, reference, solver
from test_gpu_modal_stress import held
from test_gpu_response import _refused, rayleigh_for, tip_load
from test_gpu_transient import half_sine, period

pytestmark = pytest.mark.gpu

_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
LD, EPS = rr.LD, rr.EPS
KEYS = ("damage", "cycles", "max_range", "status", "depth_used")
SN_FRACTIONAL = (3.5, 1e3)                              # an exponent that is no whole number: the instance with pow
PLANES = feahip.plane_projections([[1.0, 0.0, 0.0], [1.0, 1.0, 0.0], [0.3, -0.5, 0.8]])


def probes_of(deck):
    """Two nodes at the clamp, the middle one, and the last three (a last wave of the fan holds three nodes)."""
    N = len(deck.nodes)
    clamp = np.flatnonzero(np.abs(deck.nodes[:, 1] - deck.nodes[:, 1].min()) < 1e-12)[:2]
    return np.unique(np.concatenate([clamp, [N // 2, N - 3, N - 2, N - 1]])).astype(np.int32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def check_probes(what, out, probes, depth=DEPTH, sn=SN):
    """Every process of every probe against host_rainflow of its returned history: four numbers exactly, the damage within
    2 (c + b + 4) EPS of the long-double sum over the host's list.  Returns the largest damage error over its tolerance."""
    worst = 0.0
    hist = out["probes"]
    for r, node in enumerate(probes):
        for k in range(hist.shape[2]):
            host = feahip.host_rainflow(hist[r, :, k], *sn, depth)
            got = {key: out[key][node, k] for key in KEYS}
            assert got["cycles"] == host["cycles"] and got["max_range"] == host["max_range"], (what, node, k, got, host)
            assert got["status"] == host["status"] and got["depth_used"] == host["depth_used"], (what, node, k, got, host)
            exact = rr.damage_of(list(zip(host["ranges"], host["means"], host["counts"])), *sn)
            tol = rr.damage_tolerance(len(host["ranges"]), sn[0], 2)
            err = abs(LD(got["damage"]) - exact)
            assert err <= tol * exact, (what, node, k, float(err / exact), tol)
            if exact > 0:
                worst = max(worst, float(err / exact) / tol)
    return worst


def check_every_node(what, out, T, Ts, coef, g, depth=DEPTH, keep=None):
    """cycles and status equal and max_range within 2 e_c on every row the bounds decide; their share at least 0.9."""
    h, e = rows_of(T, Ts, coef, g)
    want = count_all(h, e, depth)
    sure = want["decided"] if keep is None else want["decided"] & np.repeat(keep, 6)
    total = len(sure) if keep is None else 6 * int(keep.sum())
    share = sure.sum() / total
    cyc, st, top = (out[key][:, :6].reshape(-1) for key in ("cycles", "status", "max_range"))
    err = np.abs(top - want["max_range"])[sure] / np.maximum(2 * e.max(axis=0)[sure], 1e-300)
    print(f"{what}: decided {share:.4f} of {total} rows; max_range error / (2 e_c) up to {err.max() if err.size else 0.0:.3f}")
    assert share >= 0.9
    assert np.array_equal(cyc[sure], want["n_cycles"][sure]) and np.array_equal(st[sure], want["status"][sure])
    assert np.all(err <= 1.0)
    assert np.all(np.isfinite(out["damage"])) and np.all(out["damage"] >= 0)


def pow_error_in_ulps(out, sn):
    """On a history whose count is one half cycle the damage is 0.5 (r / 2)^b / A: its error in units in the last place of
    the long-double value, over every row that counted one (the power, and half a unit for the product with 1 / A)."""
    dmg, rng, cyc = (out[key].reshape(-1) for key in ("damage", "max_range", "cycles"))
    one = cyc == 0.5
    exact = LD(0.5) * (rng[one].astype(LD) / 2) ** LD(sn[0]) / LD(sn[1])
    ulp = np.spacing(np.abs(exact.astype(np.float64)))
    return float((np.abs(dmg[one].astype(LD) - exact) / ulp).max()), int(one.sum())


# ---- 1. the kernel on the five stores -------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,m,correction", CASES)
def test_count_on_the_five_stores(kind, m, correction):
    """A single column, a full panel, a partial last panel, three panels and all eight; the fan's 143 nodes leave a last
    wave with 3 of its 10 nodes.  Every history with three planes, the first of them the x axis: one projection pass with
    three live lanes per node."""
    ref, s, lam, q, T, Ts, damping = held(kind, m, correction)
    deck = DECKS[kind]()
    probes = probes_of(deck)
    assert PLANES[0].tolist() == [1.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    for name, g, dt in histories(ref):
        what = f"{kind} {m} modes, {name}"
        out = s.response_stress_rainflow(g, dt, *damping, None, *SN, DEPTH, PLANES, probes)
        assert out["probes"].shape == (len(probes), len(g), 9) and out["damage"].shape == (len(deck.nodes), 9)
        hist = s.response_stress_transient(g, dt, *damping, None, probes)[4]
        assert same_bits(out["probes"][:, :, :6], hist)
        worst = check_probes(what, out, probes)
        for key in KEYS:                                                 # the x axis is component 0
            assert np.array_equal(out[key][:, 6], out[key][:, 0]), (what, key)
        assert np.array_equal(out["probes"][:, :, 6], out["probes"][:, :, 0])
        check_every_node(what, out, T, Ts, transient_table(lam, q, g, dt, damping, correction), g)
        print(f"{what}: probes' damage error / tolerance up to {worst:.3f}; deepest stack {out['depth_used'].max()}")
        assert not (out["status"][:, :6] & feahip.RAINFLOW_OVERFLOW).any()
        if len(g) == 2 or name.endswith("two tones"):
            # a whole exponent runs the instance that squares and multiplies, any other the one with pow: both, on the same
            # history, with the same count
            frac = s.response_stress_rainflow(g, dt, *damping, None, *SN_FRACTIONAL, DEPTH, PLANES, probes)
            for key in ("cycles", "max_range", "status", "depth_used", "probes"):
                assert np.array_equal(frac[key], out[key]), (what, key)
            worst = check_probes(what + f", b = {SN_FRACTIONAL[0]}", frac, probes, sn=SN_FRACTIONAL)
            print(f"{what}, b = {SN_FRACTIONAL[0]}: probes' damage error / tolerance up to {worst:.3f}")
            if len(g) == 2:
                for label, res, sn in (("whole b", out, SN), ("pow", frac, SN_FRACTIONAL)):
                    ulps, rows = pow_error_in_ulps(res, sn)
                    print(f"{what}: damage of one half cycle, b = {sn[0]} ({label}), {rows} rows: error up to {ulps:.3f} ulp")
                    assert rows >= 0.9 * out["damage"].size
                    assert ulps <= 2.0                                   # what k = 2 of the probes' tolerance rests on
    # a constant history: bit 0 and zeros everywhere
    out = s.response_stress_rainflow(np.zeros(40), histories(ref)[0][2], *damping, None, *SN, DEPTH, PLANES)
    assert (out["status"] == feahip.RAINFLOW_CONSTANT).all()
    assert not out["damage"].any() and not out["cycles"].any() and not out["max_range"].any() and not out["depth_used"].any()
    s.close()


def test_seven_projections_take_a_second_pass():
    """Seven planes: the second projection pass runs with one live lane per node.  The first three are those of the other
    tests and must come out to the bit of a call with them alone."""
    kind, m, correction = CASES[3]
    ref, s, lam, q, T, Ts, damping = held(kind, m, correction)
    deck = DECKS[kind]()
    probes = probes_of(deck)
    T1 = period(ref)
    dt = 3 * T1 / 257
    g = two_tone(258, dt, T1)
    seven = np.vstack([PLANES, feahip.plane_projections(np.random.default_rng(7).standard_normal((4, 3)))])
    out7 = s.response_stress_rainflow(g, dt, *damping, None, *SN, DEPTH, seven, probes)
    out3 = s.response_stress_rainflow(g, dt, *damping, None, *SN, DEPTH, PLANES, probes)
    out0 = s.response_stress_rainflow(g, dt, *damping, None, *SN, DEPTH, None, probes)
    assert out7["damage"].shape == (len(deck.nodes), 13) and out7["probes"].shape == (len(probes), 258, 13)
    for key in KEYS + ("probes",):
        assert np.array_equal(out7[key][..., :9], out3[key]) and np.array_equal(out3[key][..., :6], out0[key]), key
    print("seven projections: probes' damage error / tolerance up to", check_probes("seven projections", out7, probes))
    # the seventh is a pass of its own: live, and not a copy of another column
    assert out7["cycles"][:, 12].all() and not (out7["status"][:, 12] & feahip.RAINFLOW_CONSTANT).any()
    assert not np.array_equal(out7["damage"][:, 12], out7["damage"][:, 6])
    # a plane's normal stress is the projection of the components: the probe column against the six it is made of
    mix = out7["probes"][:, :, :6] @ seven[6]
    assert np.all(np.abs(out7["probes"][:, :, 12] - mix) <= 64 * EPS * (np.abs(out7["probes"][:, :, :6]) @ np.abs(seven[6])) + 1e-300)
    s.close()


# ---- 2. two launches, a small ring, a growing ring ------------------------------------------------------------------------
@pytest.mark.parametrize("kind,m,correction", CHUNK_CASES)
def test_a_history_that_needs_a_second_launch(kind, m, correction):
    """FEA_TRANSIENT_CHUNK + 3 steps: the second launch takes four rows and continues from the state of the first -- the last
    kept sample, whose reversal its first row confirms, and the ring, which under the step has dropped points by then.  The
    history in one piece through host_rainflow is the check."""
    ref, s, lam, q, T, Ts, damping = held(kind, m, correction)
    deck = DECKS[kind]()
    probes = probes_of(deck)
    for name, g, dt in chunk_histories(ref):
        assert len(g) == CHUNK + 4
        out = s.response_stress_rainflow(g, dt, *damping, None, *SN, DEPTH, PLANES, probes)
        worst = check_probes(f"{kind} {m} modes, {name}", out, probes)
        at = [np.isin([CHUNK - 1, CHUNK], rr.reversal_indices(out["probes"][r, :, k])).any() for r in range(len(probes)) for k in range(9)]
        over = (out["status"][probes] & feahip.RAINFLOW_OVERFLOW) != 0
        print(f"{kind} {m} modes, {name}: probes' damage error / tolerance up to {worst:.3f}; {sum(at)} of {len(at)} probe rows turn "
              f"at the boundary, {over.sum()} overflowed; cycles up to {out['cycles'].max()}")
        assert any(at) if name == "two tones" else over[:, :6].all()
    s.close()


def test_a_ring_of_four_points_on_the_step_history():
    """Depth 4 under the step: 64 probes spread over the bar, overflow bits where the host's ring count has them, every
    number of the host's ring count; some rows overflow and some do not."""
    kind, m, correction = STEP_CASE
    ref, s, lam, q, T, Ts, damping = held(kind, m, correction)
    N = len(DECKS[kind]().nodes)
    probes = np.unique(np.linspace(0, N - 1, 64).astype(np.int32))
    name, g, dt = [x for x in histories(ref) if x[0] == "257 steps, step"][0]
    out = s.response_stress_rainflow(g, dt, *damping, None, *SN, 4, PLANES, probes)
    worst = check_probes("depth 4", out, probes, depth=4)
    over = (out["status"] & feahip.RAINFLOW_OVERFLOW) != 0
    print(f"depth 4, {name}: overflowed {over.mean():.3f} of the rows, {over[probes].mean():.3f} of the probes' rows; damage "
          f"error / tolerance up to {worst:.3f}")
    assert over[probes].any() and not over[probes].all() and out["depth_used"].max() == 4
    check_every_node("depth 4", out, T, Ts, transient_table(lam, q, g, dt, damping, correction), g, depth=4)
    s.close()


def _cold(kind, m, g, dt, alpha, beta, depths, probes):
    ref, deck = reference(kind), DECKS[kind]()
    s = solver(deck)
    s.response_set_basis(ref.lam[:m], ref.Phi[:, :m].T)
    s.response_base_load((1.0, 0.5, 0.0), True, feahip.CG, 1e-14, 20000)
    s.response_stress_basis()
    outs = [s.response_stress_rainflow(g, dt, alpha, beta, 0.01, *SN, d, PLANES, probes) for d in depths]
    s.close()
    return outs


def test_a_depth_that_grows_and_two_cold_runs():
    """Depth 4, then 64 on the same context (the stack is allocated again): the second call has the bits of a cold run at
    depth 64, and two cold runs agree to the bit."""
    kind, m = "tet4", 24
    ref = reference(kind)
    alpha, beta = rayleigh_for(ref, m)
    T1 = period(ref)
    dt = 3 * T1 / 257
    g = np.ones(258)
    grown = _cold(kind, m, g, dt, alpha, beta, (4, 64), [0, 5])
    cold = _cold(kind, m, g, dt, alpha, beta, (64,), [0, 5])
    again = _cold(kind, m, g, dt, alpha, beta, (64,), [0, 5])
    for key in KEYS + ("probes",):
        assert np.array_equal(grown[1][key], cold[0][key]) and np.array_equal(cold[0][key], again[0][key]), key
    assert same_bits(cold[0]["damage"], again[0]["damage"])
    assert (grown[0]["status"] & feahip.RAINFLOW_OVERFLOW).any() and not (grown[1]["status"] & feahip.RAINFLOW_OVERFLOW).any()
    assert grown[0]["depth_used"].max() == 4 and 4 < grown[1]["depth_used"].max() <= 64


# ---- 3. the selection by material ------------------------------------------------------------------------------------------
def test_selection_by_material():
    """Three layers along the bar, the store of material 1 alone: the nodes that touch none of its elements have status bit
    0 and exact zeros in every process, projections included."""
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
    assert outside.any() and not outside.all()
    damping = feahip.host_rayleigh(np.sqrt(lam[0]), 0.02, np.sqrt(lam[-1]), 0.02)
    T1 = 2 * np.pi / np.sqrt(lam[0])
    dt = 3 * T1 / 257
    g = two_tone(258, dt, T1)
    probes = np.array([np.flatnonzero(outside)[0], np.flatnonzero(~outside)[0]], dtype=np.int32)
    out = s.response_stress_rainflow(g, dt, *damping, None, *SN, DEPTH, PLANES, probes)
    assert (out["status"][outside] == feahip.RAINFLOW_CONSTANT).all()
    for key in ("damage", "cycles", "max_range", "depth_used"):
        assert not out[key][outside].any(), key
    assert not out["probes"][0].any()
    assert (out["status"][~outside] == 0).all() and out["damage"][~outside].all()
    check_probes("material 1", out, probes)
    check_every_node("material 1", out, T, Ts, transient_table(lam, q, g, dt, damping, True), g, keep=~outside)
    s.close()


# ---- 4. state ----------------------------------------------------------------------------------------------------------------
def test_state_is_left_alone():
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
    sweep = s.response_sweep(omega[:9], alpha, beta, 0.01)
    combined = s.response_combine(np.eye(m), np.ones(m), 1.0)
    stress_combined = s.response_stress_combine(np.eye(m), np.ones(m), 1.0)
    stress_sweep = s.response_stress_sweep(omega, alpha, beta, 0.01, [3])
    before = state()
    first = s.response_stress_rainflow(g, dt, alpha, beta, 0.01, *SN, DEPTH, PLANES, [3])
    assert s.time_kernel(33, 1, 2) > 0.0
    for hook in (23, 26, 28, 29):                                        # their tables and forms are still there
        assert s.time_kernel(hook, 1, 2) > 0.0
    for a, b in zip(before, state()):
        assert np.array_equal(a, b)
    for a, b in zip(sweep, s.response_sweep(omega[:9], alpha, beta, 0.01)):
        assert np.array_equal(a, b)
    assert np.array_equal(combined, s.response_combine(np.eye(m), np.ones(m), 1.0))
    for a, b in zip(stress_combined, s.response_stress_combine(np.eye(m), np.ones(m), 1.0)):
        assert np.array_equal(a, b)
    for a, b in zip(stress_sweep, s.response_stress_sweep(omega, alpha, beta, 0.01, [3])):
        assert np.array_equal(a, b)
    # the last chunks of the displacement and of the stress transient (hooks 25 and 30) stay as well
    trans = s.response_transient(g, dt, alpha, beta, 0.01)
    stress_trans = s.response_stress_transient(g, dt, alpha, beta, 0.01, [3])
    s.response_stress_rainflow(g[:20], dt, alpha, beta, 0.01, *SN, DEPTH, None, [3])
    assert s.time_kernel(25, 1, 2) > 0.0 and s.time_kernel(30, 1, 2) > 0.0 and s.time_kernel(33, 1, 2) > 0.0
    for a, b in zip(trans, s.response_transient(g, dt, alpha, beta, 0.01)):
        assert np.array_equal(a, b)
    for a, b in zip(stress_trans, s.response_stress_transient(g, dt, alpha, beta, 0.01, [3])):
        assert np.array_equal(a, b)
    for a, b in zip(before, state()):
        assert np.array_equal(a, b)
    # the hook writes the entry's own buffers only: the same bits after it
    again = s.response_stress_rainflow(g, dt, alpha, beta, 0.01, *SN, DEPTH, PLANES, [3])
    for key in KEYS + ("probes",):
        assert np.array_equal(first[key], again[key]), key
    s.close()


# ---- 5. refusals and the hook -----------------------------------------------------------------------------------------------
def _raw(s, g, dt, n_steps=None, probes=(), n_probe=None, b=3.0, A=1e3, depth=32, proj=None, n_proj=None):
    """The C entry on arrays filled with a sentinel: (return code, the output arrays)."""
    N = s.ndof // 3
    g = np.ascontiguousarray(g, dtype=np.float64)
    pr = np.ascontiguousarray(probes, dtype=np.int32)
    pj = None if proj is None else np.ascontiguousarray(proj, dtype=np.float64)
    k = len(pr) if n_probe is None else n_probe
    npj = (0 if pj is None else len(pj)) if n_proj is None else n_proj
    W = 6 + max(min(npj, 64), 0)
    d = [np.full((N, W), -7.0) for _ in range(3)] + [np.full((max(k, 1), len(g), W), -7.0)]
    i = [np.full((N, W), -7, dtype=np.int32) for _ in range(2)]
    rc = s._lib.feahip_response_stress_rainflow(s._ctx, len(g) - 1 if n_steps is None else n_steps, dt, g.ctypes.data_as(_dp), 0.0, 0.0,
                                                None, b, A, depth, npj, None if pj is None else pj.ctypes.data_as(_dp),
                                                d[0].ctypes.data_as(_dp), d[1].ctypes.data_as(_dp), d[2].ctypes.data_as(_dp),
                                                i[0].ctypes.data_as(_ip), i[1].ctypes.data_as(_ip), k, pr.ctypes.data_as(_ip),
                                                d[3].ctypes.data_as(_dp))
    return rc, d + i


def _untouched(s, code, part, got):
    rc, arrays = got
    msg = s._lib.feahip_last_error(s._ctx).decode()
    assert rc == code and part in msg and len(msg) > 10, (rc, msg)
    assert all((a == -7).all() for a in arrays)


def test_refusals_and_the_hook():
    kind = "tet4"
    ref, deck = reference(kind), DECKS[kind]()
    F = tip_load(deck)
    N = len(deck.nodes)
    lam, phi = np.array([9.0, 4.0, 25.0]), ref.Phi[:, :3].T.copy()
    g, dt = np.array([0.0, 1.0, -1.0, 2.0, 0.5]), 0.1
    s = feahip.FeaSolver(deck)
    s.set_mass(RHO)
    entry = lambda: s.response_stress_rainflow(g, dt, 0.1, sn_exponent=3.0, sn_coefficient=1e3)
    hook = lambda: s.time_kernel(33, 1, 1)
    for call in (entry, hook):
        assert "no modes held" in _refused(s, feahip.ESTATE, call)
    _untouched(s, feahip.ESTATE, "no modes held", _raw(s, g, dt))
    s.response_set_basis(lam, phi)
    for call in (entry, hook):
        assert "no load held" in _refused(s, feahip.ESTATE, call)
    s.response_load(F, True)
    for call in (entry, hook):
        assert "no stress store" in _refused(s, feahip.ESTATE, call)
    _untouched(s, feahip.ESTATE, "no stress store", _raw(s, g, dt))
    s.response_stress_basis()
    s.response_load(F, True)                                             # a stale basis after a new load
    for call in (entry, hook):
        assert "a load was made" in _refused(s, feahip.ESTATE, call)
    _untouched(s, feahip.ESTATE, "a load was made", _raw(s, g, dt))
    s.response_stress_basis()
    assert "no stress rainflow" in _refused(s, feahip.ESTATE, hook)      # before the entry
    # the arguments of the transient
    _untouched(s, feahip.EINVAL, "n_steps", _raw(s, g, dt, n_steps=0))
    _untouched(s, feahip.EINVAL, "dt", _raw(s, g, 0.0))
    _untouched(s, feahip.EINVAL, "probe node", _raw(s, g, dt, probes=[N]))
    _untouched(s, feahip.EINVAL, "probe node", _raw(s, g, dt, probes=[-1]))
    _untouched(s, feahip.EINVAL, "n_probe", _raw(s, g, dt, probes=np.zeros(65), n_probe=65))
    bad = g.copy()
    bad[2] = np.nan
    _untouched(s, feahip.EINVAL, "response_stress_rainflow", _raw(s, bad, dt))
    # the curve, the ring, the projections
    for kw in (dict(b=0.5), dict(b=65.0), dict(b=np.nan), dict(A=0.0), dict(A=-2.0), dict(A=np.inf), dict(depth=3), dict(depth=1025)):
        _untouched(s, feahip.EINVAL, "S-N curve", _raw(s, g, dt, **kw))
    _untouched(s, feahip.EINVAL, "n_proj", _raw(s, g, dt, proj=np.ones((49, 6))))
    _untouched(s, feahip.EINVAL, "n_proj", _raw(s, g, dt, n_proj=-1))
    _untouched(s, feahip.EINVAL, "null proj", _raw(s, g, dt, n_proj=2))
    for v in (np.nan, np.inf):
        pj = PLANES.copy()
        pj[1, 4] = v
        _untouched(s, feahip.EINVAL, "proj is not finite", _raw(s, g, dt, proj=pj))
    assert "no stress rainflow" in _refused(s, feahip.ESTATE, hook)      # a refused call leaves nothing to time
    rc, arrays = _raw(s, g, dt, probes=[0, N - 1], proj=PLANES)
    assert rc == 0 and all(np.isfinite(a).all() and (a != -7).all() for a in arrays)
    assert s.time_kernel(33, 1, 2) > 0.0
    # any output may be NULL
    null = C.cast(None, _dp)
    rc = s._lib.feahip_response_stress_rainflow(s._ctx, len(g) - 1, dt, g.ctypes.data_as(_dp), 0.0, 0.0, None, 3.0, 1e3, 32, 0, None,
                                                null, null, null, C.cast(None, _ip), C.cast(None, _ip), 0, C.cast(None, _ip), null)
    assert rc == 0
    # a new filling of the locked store drops the chunk with the stress store
    s.response_set_basis(lam, phi)
    s.response_load(F, True)
    s.response_stress_basis()
    assert "no stress rainflow" in _refused(s, feahip.ESTATE, hook)
    # a row shard, a rank context
    s.set_row_shard(0, 2)
    for call in (entry, hook):
        assert "row-sharded" in _refused(s, feahip.EINVAL, call)
    s.close()
    r = feahip.RankSolver(deck, 0, 2)
    assert "feahip_create_rank" in _refused(r, feahip.EINVAL, lambda: r.response_stress_rainflow(g, dt, 0.1))
    r.close()


# ---- 6. the command line --------------------------------------------------------------------------------------------------
def test_feasolver_hip_runs_a_deck_with_the_rainflow_keys(tmp_path):
    """A (3, 8, 3) TET4 bar under a lateral traction, twelve locked modes, (transient ... :stress t) with and without the
    three keys: the log line, the section "Fatigue damage (rainflow)" behind the old ones, the largest of the six component
    damages of the Python entry on the same state within the digits of the file, and without the keys the old output byte
    for byte."""
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
    T1 = 2 * np.pi / np.sqrt(lam1)
    section = dict(transient_steps=240, transient_dt=float(f"{T1 / 40:.3g}"), transient_shape="half-sine",
                   transient_rise=float(f"{0.4 * T1:.3g}"), transient_zeta=0.02, transient_stress=True)
    keys = dict(transient_sn_exponent=3.0, transient_sn_coefficient=1e-3, transient_rainflow_depth=16)
    decks = {"old": make(**section), "rainflow": make(**section, **keys)}
    exe = os.path.join(os.path.dirname(feahip.LIB_PATH), "feasolver_hip")
    out = {}
    for name, d in decks.items():
        path = tmp_path / f"{name}.sexp"
        d.save(str(path))
        out[name] = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
        assert out[name].returncode == 0, out[name].stderr
    old, new = (tmp_path / "old.msh").read_text(), (tmp_path / "rainflow.msh").read_text()
    assert "fatigue" not in out["old"].stdout and "rainflow" not in old
    keep = "".join(l for l in out["rainflow"].stdout.splitlines(True) if not l.startswith("Transient fatigue:"))
    assert keep == out["old"].stdout
    assert new.startswith(old) and re.findall(r'^"([^"]+)"$', new[len(old):], re.M) == ["Fatigue damage (rainflow)"]
    hit = re.search(r"^Transient fatigue: damage = (\S+) \(rainflow\), node (\d+), component (\d), cycles = (\S+)$", out["rainflow"].stdout, re.M)
    assert hit, out["rainflow"].stdout
    lines = out["rainflow"].stdout.splitlines()
    assert lines.index(hit.group(0)) == [k for k, l in enumerate(lines) if l.startswith("Transient peak von Mises:")][0] + 1
    n_nodes = len(decks["old"].nodes)
    body = new[new.index('"Fatigue damage (rainflow)"'):].splitlines()
    assert body[5] == "1" and body[6] == str(n_nodes) and body[7 + n_nodes] == "$EndNodeData"
    rows = np.array([float(l.split()[1]) for l in body[7:7 + n_nodes]])
    best, node, comp, cycles = float(hit.group(1)), int(hit.group(2)), int(hit.group(3)), float(hit.group(4))
    assert best > 0 and abs(rows.max() - best) <= 1e-9 * best and abs(rows[node - 1] - best) <= 1e-9 * best
    # the Python entry on the state the command line reached: the solved nodes, its modes, the surface load
    d = decks["rainflow"]
    s = feahip.FeaSolver(d)
    s.set_mass(RHO)
    done, _, _ = s.solve(load_increments=1)
    assert done == 1
    s.solve_modes_locked(12, 0.0, d.modal_tolerance, d.modal_max)
    s.response_load(s.surface_forces(), True)
    s.response_stress_basis()
    t = np.arange(d.transient_steps + 1) * d.transient_dt
    g = np.where(t < d.transient_rise, np.sin(np.pi * t / d.transient_rise), 0.0)
    mine = s.response_stress_rainflow(g, d.transient_dt, 0.0, 0.0, 0.02, 3.0, 1e-3, 16)
    want = mine["damage"].max(axis=1)
    print("command line against Python", np.abs(want - rows).max() / want.max(), "; damage", best, "node", node, "component", comp,
          "cycles", cycles, "; overflowed rows", int(((mine["status"] & feahip.RAINFLOW_OVERFLOW) != 0).sum()))
    assert np.all(np.abs(want - rows) <= 1e-9 * want.max())
    assert mine["damage"][node - 1, comp] == mine["damage"].max() and mine["cycles"][node - 1, comp] == cycles
    over = int(((mine["status"] & feahip.RAINFLOW_OVERFLOW) != 0).sum())
    said = re.search(r"^Transient fatigue: (\d+) of (\d+) stress rows overflowed the stack of 16 points$", out["rainflow"].stdout, re.M)
    assert (said is None) == (over == 0) and (over == 0 or (int(said.group(1)), int(said.group(2))) == (over, 6 * n_nodes))
    s.close()

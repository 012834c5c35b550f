"""tests/stress_sweep_reference.py without a GPU: the closed form of the cycle peak of the von Mises stress against brute
force over 4096 phases, its special states, the nearly hydrostatic state that the expanded form loses, the library's host
helper, the :stress key of (harmonic ...) and (transient ...) through the deck reader and writer, and the precondition of the
index checks of tests/test_gpu_stress_sweep.py: on its cases the bounds decide at least 95 % of the peak indices."""
import numpy as np
import pytest

import feahip
import stress_sweep_reference as ssr
from results_reference import von_mises
from stress_sweep_cases import (CASES, CHUNK, CHUNK_CASES, LATE, chunk_histories, frequency_lists, histories, reference,
                                reference_inputs, sweep_table, transient_table)
from test_stress_reference_cpu import RANDOM, SPECTRUM, _deck

EPS = ssr.EPS


def random_states(n, seed=31):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, 6)) + 1j * rng.standard_normal((n, 6))


def test_closed_form_against_4096_phases():
    """The sampled maximum misses the true one by at most the curvature over half a sample: vm^2(t) = h + R cos(2wt + p),
    R <= h, so sampled^2 >= peak^2 - R (1 - cos(delta)) >= peak^2 (1 - delta^2 / 2), delta = 2 pi / 4096 in the phase of
    sigma, and it never exceeds the peak beyond rounding."""
    s = random_states(10000)
    peak, sampled = ssr.harmonic_peak(s), ssr.harmonic_sampled(s)
    delta = 2 * np.pi / ssr.PHASES
    print("sampled^2 / peak^2: smallest", (sampled ** 2 / peak ** 2).min(), "largest", (sampled ** 2 / peak ** 2).max())
    assert np.all(sampled ** 2 >= peak ** 2 * (1 - delta ** 2 / 2))
    assert np.all(sampled ** 2 <= peak ** 2 * (1 + 16 * EPS))


def test_special_states():
    rng = np.random.default_rng(32)
    re = rng.standard_normal((50, 6))
    vm = von_mises(re)
    assert np.all(np.abs(ssr.harmonic_peak(re + 0j) - vm) <= 8 * EPS * vm)                       # purely real
    assert np.all(np.abs(ssr.harmonic_peak(1j * re) - vm) <= 8 * EPS * vm)                       # purely imaginary
    assert np.all(np.abs(ssr.harmonic_peak((1 + 1j) * re) - np.sqrt(2.0) * vm) <= 16 * EPS * vm)   # in phase: one line
    # a state whose imaginary part is the real one turned by 90 degrees in the von Mises form: A = B, C = 0, so the von
    # Mises stress is the same at every phase.  Deviatoric shear xy and yz of equal size are such a pair
    turn = np.zeros((1, 6), dtype=np.complex128)
    turn[0, 3], turn[0, 4] = 2.0, 2.0j
    peak = ssr.harmonic_peak(turn)
    th = np.linspace(0, 2 * np.pi, 97)[:, None]
    over_the_cycle = von_mises(turn.real * np.cos(th) - turn.imag * np.sin(th))
    assert np.all(np.abs(over_the_cycle - peak) <= 8 * EPS * peak) and abs(peak[0] - np.sqrt(12.0)) <= 8 * EPS * peak[0]
    assert ssr.harmonic_peak(np.zeros((3, 6), dtype=np.complex128)).tolist() == [0.0, 0.0, 0.0]
    assert feahip.host_harmonic_von_mises(np.zeros(6)).tolist() == 0.0


def hydrostatic_states():
    """A hydrostatic part of 1e8 on a deviator of unit size, real and imaginary part each."""
    rng = np.random.default_rng(33)
    dev = ssr.deviator(rng.standard_normal((200, 6))) + 1j * ssr.deviator(rng.standard_normal((200, 6)))
    dev /= np.sqrt((np.abs(dev) ** 2).sum(axis=-1))[:, None]
    s = dev.copy()
    s[:, :3] += 1e8 * (1.0 + 0.5j)
    return s


def test_nearly_hydrostatic_state():
    """Within 64 EPS |s| of the long-double value for the restatement and for the library's helper (the mean carries an
    error of EPS |s|, and that is all the deviator sees); the expanded form is off by far more."""
    s = hydrostatic_states()
    exact = ssr.harmonic_peak_longdouble(s)
    norm = np.sqrt((np.abs(s) ** 2).sum(axis=-1))
    for name, got in (("restatement", ssr.harmonic_peak(s)), ("host helper", feahip.host_harmonic_von_mises(s))):
        print(name, "largest error / (EPS |s|)", (np.abs(got - exact) / (EPS * norm)).max())
        assert np.all(np.abs(got - exact) <= 64 * EPS * norm)
    bad = np.abs(ssr.harmonic_peak_expanded(s) - exact)
    print("expanded form: largest error / (EPS |s|)", (bad / (EPS * norm)).max())
    assert (bad > 64 * EPS * norm).any()


def test_host_helper_matches_the_restatement():
    """Exported, vectorised over the leading axes, and within the arithmetic term of the sweep's bound of the
    restatement."""
    assert "feahip_host_harmonic_von_mises" in feahip.ABI
    s = random_states(2000, 34).reshape(40, 50, 6)
    got, want = feahip.host_harmonic_von_mises(s), ssr.harmonic_peak(s)
    norm = np.sqrt(3.0 * (np.abs(s) ** 2).sum(axis=-1))
    assert got.shape == (40, 50)
    print("helper against the restatement: largest error / (EPS sqrt(3) |s|)", (np.abs(got - want) / (EPS * norm)).max())
    assert np.all(np.abs(got - want) <= ssr.K_SWEEP * EPS * norm)
    one = feahip.host_harmonic_von_mises(s[3, 4])
    assert one.shape == () and one == got[3, 4]


HARMONIC = dict(harmonic_count=5, harmonic_from=0.5, harmonic_to=4.0, harmonic_zeta=0.02)
TRANSIENT = dict(transient_steps=20, transient_dt=0.01, transient_shape="half-sine", transient_rise=0.05, transient_base=(1.0, 0.0, 0.0))


def test_deck_round_trip_of_the_two_new_keys(tmp_path):
    """:stress t is read, written and read again in (harmonic ...) and in (transient ...); a deck without it is written byte
    for byte as before; (modal ...) and (slae-solver ...) still refuse it."""
    p = tmp_path / "stress.sexp"
    for kw, fields in ((dict(HARMONIC, harmonic_stress=True), (1, 0)), (dict(TRANSIENT, transient_stress=True), (0, 1)),
                       (dict(HARMONIC, **TRANSIENT, harmonic_stress=True, transient_stress=True), (1, 1))):
        _deck(**kw).save(str(p))
        text = p.read_text()
        assert text.count(":stress t") == sum(fields)
        back = feahip.Deck.load(str(p))
        fd = back.to_struct()
        assert (fd.harmonic_stress, fd.transient_stress) == fields
        assert (back.harmonic_stress, back.transient_stress) == tuple(map(bool, fields))
        back.save(str(p))
        assert p.read_text() == text
        plain = {k: v for k, v in kw.items() if not k.endswith("_stress")}
        _deck(**plain).save(str(p))
        assert p.read_text() == text.replace(" :stress t", "") and ":stress" not in p.read_text()
        again = feahip.Deck.load(str(p))
        assert not again.harmonic_stress and not again.transient_stress
    # the four sections side by side keep their own flags
    _deck(**HARMONIC, **TRANSIENT, **SPECTRUM, **RANDOM, harmonic_stress=True, random_stress=True).save(str(p))
    back = feahip.Deck.load(str(p))
    assert (back.harmonic_stress, back.transient_stress, back.spectrum_stress, back.random_stress) == (True, False, False, True)
    _deck(**HARMONIC, **TRANSIENT, harmonic_stress=True).save(str(p))
    text = p.read_text()
    for old, new in ((":stress t", ":stress maybe"), ("(modal ", "(modal :stress t "), ("(slae-solver ", "(slae-solver :stress t ")):
        assert text.count(old) == 1
        p.write_text(text.replace(old, new))
        with pytest.raises(feahip.FeaHipError):
            feahip.Deck.load(str(p))
    p.write_text(text.replace(":stress t", ":stress nil"))
    assert not feahip.Deck.load(str(p)).harmonic_stress
    with pytest.raises(ValueError, match="harmonic_stress"):
        _deck(harmonic_stress=True)
    with pytest.raises(ValueError, match="transient_stress"):
        _deck(transient_stress=True)


def _shares(what, mag, b6, vm, bvm):
    rows, nodes = ssr.decided_share(mag, b6), ssr.decided_share(vm, bvm)
    print(what, "decided: peak6_at", rows, "vm_at", nodes)
    return rows, nodes


@pytest.mark.parametrize("kind,m,correction", CASES)
def test_the_bounds_decide_the_indices_of_the_gpu_cases(kind, m, correction):
    """The precondition of the index checks on the GPU, from the reference modes alone: with T of the restatement and the
    library's host tables for the lists and histories used there, at least 95 % of the nodes (vm_at) and of the rows
    (peak6_at) have a largest value that exceeds the runner-up by more than both their bounds."""
    ref = reference(kind)
    lam, q, T, Ts, damping = reference_inputs(kind, m, correction)
    for omega in frequency_lists(ref, m, correction):
        coef = sweep_table(lam, q, omega, damping, correction)
        rows, nodes = _shares(f"{kind} {m} sweep of {len(omega)}", *ssr.sweep_values(T, Ts, coef))
        assert rows >= 0.95 and nodes >= 0.95
    for name, g, dt in histories(ref):
        coef = transient_table(lam, q, g, dt, damping, correction)
        rows, nodes = _shares(f"{kind} {m} {name}", *ssr.transient_values(T, Ts, coef, g))
        assert rows >= 0.95 and nodes >= 0.95


@pytest.mark.parametrize("kind,m,correction", CHUNK_CASES)
def test_the_bounds_decide_the_indices_of_the_two_launch_histories(kind, m, correction):
    """The same for the histories of FEA_TRANSIENT_CHUNK + 3 steps; the early half-sine has every von Mises peak in the
    first chunk, the late one most of them in the second (on the TET10 bar a fifth of the nodes, those near the clamp, peak
    in the last rows of the first chunk: the second launch has to keep what the first one found)."""
    ref = reference(kind)
    lam, q, T, Ts, damping = reference_inputs(kind, m, correction)
    for name, g, dt in chunk_histories(ref):
        assert len(g) == CHUNK + 4
        coef = transient_table(lam, q, g, dt, damping, correction)
        mag, b6, vm, bvm = ssr.transient_values(T, Ts, coef, g)
        rows, nodes = _shares(f"{kind} {m} {name}", mag, b6, vm, bvm)
        assert rows >= 0.95 and nodes >= 0.95
        best = vm.argmax(axis=0)
        print(name, "von Mises peaks at rows", best.min(), "..", best.max())
        if name.startswith("early"):
            assert best.max() < CHUNK
        else:
            assert best.min() >= CHUNK - LATE and (best >= CHUNK).mean() >= 0.5

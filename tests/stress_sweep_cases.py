"""The cases tests/test_gpu_stress_sweep.py runs and tests/test_stress_sweep_reference_cpu.py checks the precondition of: the
five stores of tests/test_gpu_response.py, its frequency lists, the histories of tests/test_gpu_transient.py and two
histories that need a second launch; and the same inputs from the reference modes alone, without the library's device side."""
import functools

import numpy as np

import feahip
import stress_reference as sr
from response_reference import static_solve
from test_gpu_modal_locked import DECKS, reference
from test_gpu_response import CASES, frequency_lists, rayleigh_for, tip_load
from test_gpu_transient import half_sine, period

CHUNK = feahip.TRANSIENT_CHUNK
CHUNK_CASES = [CASES[0], CASES[1]]                      # the fan with one mode, TET10 with eight and the correction
LATE = 20                                               # the late half-sine begins this many rows before the second launch


def histories(ref):
    """[(name, g, dt)]: 1, 3 and 257 steps of the half-sine of 0.4 T1 and of the step."""
    T1 = period(ref)
    dt = 3 * T1 / 257
    return [(f"{n} steps, {name}", g, dt) for n in (1, 3, 257)
            for name, g in (("half-sine", half_sine(n + 1, dt, 0.4 * T1)), ("step", np.ones(n + 1)))]


def chunk_histories(ref):
    """[(name, g, dt)] of FEA_TRANSIENT_CHUNK + 3 steps, two launches (the second of four rows): a half-sine at the start,
    whose peaks lie in the first chunk, and one that begins LATE rows before the second chunk and is still rising at the
    last row, so most peaks lie in the second (on the TET10 bar the nodes near the clamp peak in the last rows of the first)."""
    T1 = period(ref)
    dt = 3 * T1 / 257
    points = CHUNK + 4
    return [("early half-sine", half_sine(points, dt, 0.4 * T1), dt),
            ("late half-sine", half_sine(points, dt, 0.4 * T1, CHUNK - LATE), dt)]


@functools.lru_cache(maxsize=None)
def reference_inputs(kind, m, correction):
    """(lam, q, T[m][N][6], Ts[N][6] or None, (alpha, beta)) from the reference's first m pairs: q = Phi' F on the free
    dofs, T and T_s the restatement's nodal stresses of the modes and of the dense static solve."""
    ref, deck = reference(kind), DECKS[kind]()
    lam, Phi = ref.lam[:m], ref.Phi[:, :m]
    F = tip_load(deck, 0.1)
    q = Phi.T @ np.where(ref.mask, 0.0, F)
    cols = [Phi.T] + ([static_solve(ref.K, ref.mask, F)[None, :]] if correction else [])
    r = sr.StressRestatement(deck)
    try:
        T, _ = r.nodal(deck.nodes, np.vstack(cols))
    finally:
        r.close()
    return lam, q, T[:m], (T[m] if correction else None), rayleigh_for(ref, m)


def sweep_table(lam, q, omega, damping, correction):
    """The library's host table of a sweep, complex [n_freq][m]."""
    return feahip.host_response_coefficients(lam, q, omega, *damping, None, correction)[:, :len(lam)]


def transient_table(lam, q, g, dt, damping, correction):
    """The library's host table of a transient, [n_steps + 1][m]."""
    return feahip.host_transient_coefficients(lam, q, g, dt, *damping, None, correction)[:, :len(lam)]

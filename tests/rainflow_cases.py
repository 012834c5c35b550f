"""The cases tests/test_gpu_rainflow.py runs and tests/test_rainflow_reference_cpu.py checks the preconditions of: the five
stores of tests/test_gpu_response.py under 1, 2, 3 and 257 steps of the half-sine and of the step and under a two-tone
history with nested cycles, two histories that need a second launch, and the count of every stress row of a case from the
float64 restatement's histories with the bounds that decide it."""
import numpy as np

import rainflow_reference as rr
import stress_sweep_reference as ssr
from stress_sweep_cases import CASES, CHUNK, CHUNK_CASES, reference, reference_inputs, transient_table  # noqa: F401 (re-exported)
from test_gpu_transient import half_sine, period

SN = (3.0, 1e3)                                         # the S-N curve of the tests: b, A
DEPTH = 32
STEP_CASE = CASES[3]                                    # the damped TET4 bar with 24 modes: the case of the depth-4 test


def two_tone(points, dt, T1):
    """A slow tone of period 1.5 T1 carrying a fast one of a seventh of that period and 0.45 of its size: small cycles nested
    inside large ones, so that the stack holds more than three points."""
    t = np.arange(points) * dt
    return np.sin(2 * np.pi * t / (1.5 * T1)) + 0.45 * np.sin(2 * np.pi * 7 * t / (1.5 * T1))


def histories(ref):
    """[(name, g, dt)]: 1, 2, 3 and 257 steps of the half-sine of 0.4 T1 and of the step, and 257 steps of the two tones."""
    T1 = period(ref)
    dt = 3 * T1 / 257
    out = [(f"{n} steps, {name}", g, dt) for n in (1, 2, 3, 257)
           for name, g in (("half-sine", half_sine(n + 1, dt, 0.4 * T1)), ("step", np.ones(n + 1)))]
    return out + [("257 steps, two tones", two_tone(258, dt, T1), dt)]


def chunk_histories(ref):
    """[(name, g, dt)] of FEA_TRANSIENT_CHUNK + 3 steps, two launches (the second of four rows): the two tones, whose fast one
    turns every nine rows, so that rows turn at the launch boundary, and a step, whose ring-down fills a ring of 32 points
    long before the second launch, so that a ring with its base off slot 0 crosses the boundary."""
    T1 = period(ref)
    dt = 3 * T1 / 257
    return [("two tones", two_tone(CHUNK + 4, dt, T1), dt), ("step", np.ones(CHUNK + 4), dt)]


def rows_of(T, Ts, coef, g):
    """(h[n][6N], e[n][6N]): the restatement's histories of every stress row and the bound e_c on each sample."""
    h, e = ssr.components(T, Ts, coef, g), ssr.component_bound(T, Ts, coef, g)
    return h.reshape(len(h), -1), e.reshape(len(e), -1)


def reference_rows(kind, m, correction, g, dt):
    """rows_of from the reference modes alone."""
    lam, q, T, Ts, damping = reference_inputs(kind, m, correction)
    return rows_of(T, Ts, transient_table(lam, q, g, dt, damping, correction), g)


def count_all(h, e, depth=None):
    """rainflow_reference.count_rows over every row."""
    return rr.count_rows(h, e, depth)

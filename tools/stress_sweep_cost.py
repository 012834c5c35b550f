"""Cost of the stress sweep kernels on the bench's block: k_stress_sweep over a table of frequencies (what = 29) and one
launch of k_stress_transient over a full chunk of rows (what = 30), next to k_response_sweep (what = 23) and
k_transient_sweep (what = 25) on the same context, the same synthetic modes and the same tables.  The stress kernels own 6N
rows where the displacement kernels own 3N dofs, so the yardstick is the time per row and table row.  With --field-calls the
only other route to a sweep's peaks is timed as well: calls of response_stress_field through Python, two per frequency.  The
basis is random: the kernels do the same work on any numbers.  Warm-up, then single launches timed one by one with device
events: min / median / max, and the process's own streaming-copy rate beside them.  Run every library in a process of its
own and alternate them when two are compared (FEAHIP_LIB picks a variant build).  Run by hand, under a time limit; no test
and no benchmark calls it.

    python tools/stress_sweep_cost.py [--n 66] [--modes 8,24,64] [--freq 1024] [--launches 10] [--field-calls 16] [--out result.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fea-large_amd"))

import numpy as np  # noqa: E402

import feahip  # noqa: E402
import mesh  # noqa: E402

FP64_VECTOR_PEAK = 78.6e12
MOVES_SWEEP, MOVES_TRANSIENT = 23, 9                    # DPP moves of a double per table row: 2 means of 4 and 3 sums of 5; 1 and 1


def stats(s, what, warmup, launches):
    s.time_kernel(what, warmup, 1)
    t = np.array([s.time_kernel(what, 0, 1) for _ in range(launches)])
    return {"min_ms": float(t.min()), "median_ms": float(np.median(t)), "max_ms": float(t.max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=66, help="block of n x 6n x n cubes (66 = 10M tets, 5.3M dofs)")
    ap.add_argument("--modes", default="8,24,64")
    ap.add_argument("--freq", type=int, default=1024)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--field-calls", type=int, default=0, help="calls of response_stress_field to time at the last mode count")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    deck = mesh.bar_deck(n=a.n, recipe="clamped")
    s = feahip.FeaSolver(deck)
    s.set_mass(1.0)
    ndof, N = s.ndof, s.ndof // 3
    rng = np.random.default_rng(1)
    F = rng.standard_normal(ndof)
    rows = feahip.TRANSIENT_CHUNK
    g = np.sin(0.01 * np.arange(rows))
    omega = np.linspace(0.5, 450.0, a.freq)
    out = {"elements": int(len(deck.elements)), "nodes": N, "launches": a.launches, "library": feahip.LIB_PATH, "n_freq": a.freq,
           "rows": rows, "copy_gb_per_s": s.copy_bandwidth(1 << 30)}
    modes = [int(v) for v in a.modes.split(",")]
    for m in modes:
        block = rng.standard_normal((min(m, 8), ndof)) / np.sqrt(ndof)
        phi = np.concatenate([block * (1.0 + 0.01 * p) for p in range((m + 7) // 8)])[:m]
        s.response_set_basis(np.linspace(1.0, 400.0, m) ** 2, phi)
        del phi
        s.response_load(F, False)
        s.response_stress_basis()
        panels = (m + 7) // 8
        res = {}
        # the frequency sweeps: 2 x 8 P fused multiply-adds per row (dof) and frequency
        s.response_sweep(omega, 0.1, 1e-5)
        k23 = stats(s, 23, a.warmup, a.launches)
        t0 = time.perf_counter()
        s.response_stress_sweep(omega, 0.1, 1e-5)
        call_ms = 1e3 * (time.perf_counter() - t0)
        k29 = stats(s, 29, a.warmup, a.launches)
        flop = 2.0 * 2 * 8 * panels
        sec23, sec29 = k23["median_ms"] * 1e-3, k29["median_ms"] * 1e-3
        res["sweep"] = dict(k23, tflop_per_s=flop * ndof * a.freq / sec23 / 1e12, ps_per_row_and_frequency=sec23 / (ndof * a.freq) * 1e12)
        res["stress_sweep"] = dict(k29, call_ms=call_ms, tflop_per_s=flop * 6 * N * a.freq / sec29 / 1e12,
                                   fp64_vector_peak_fraction=flop * 6 * N * a.freq / sec29 / FP64_VECTOR_PEAK,
                                   ps_per_row_and_frequency=sec29 / (6 * N * a.freq) * 1e12, moves_per_table_row=MOVES_SWEEP)
        res["stress_sweep_over_sweep_per_row"] = (sec29 / (6 * N)) / (sec23 / ndof)
        # the transients: 8 P fused multiply-adds per row (dof) and step
        s.response_transient(g, 1e-3, 0.1, 1e-5)
        k25 = stats(s, 25, a.warmup, a.launches)
        t0 = time.perf_counter()
        s.response_stress_transient(g, 1e-3, 0.1, 1e-5)
        call_ms = 1e3 * (time.perf_counter() - t0)
        k30 = stats(s, 30, a.warmup, a.launches)
        flop = 2.0 * 8 * panels
        sec25, sec30 = k25["median_ms"] * 1e-3, k30["median_ms"] * 1e-3
        res["transient"] = dict(k25, tflop_per_s=flop * ndof * rows / sec25 / 1e12, ps_per_row_and_step=sec25 / (ndof * rows) * 1e12)
        res["stress_transient"] = dict(k30, call_ms=call_ms, tflop_per_s=flop * 6 * N * rows / sec30 / 1e12,
                                       fp64_vector_peak_fraction=flop * 6 * N * rows / sec30 / FP64_VECTOR_PEAK,
                                       ps_per_row_and_step=sec30 / (6 * N * rows) * 1e12, moves_per_table_row=MOVES_TRANSIENT)
        res["stress_transient_over_transient_per_row"] = (sec30 / (6 * N)) / (sec25 / ndof)
        if a.field_calls and m == modes[-1]:
            # the route without the sweep entry: response_stress_field of the real and of the imaginary part of every frequency
            coef = feahip.host_response_coefficients(np.linspace(1.0, 400.0, m) ** 2, np.ones(m), omega[:a.field_calls], 0.1, 1e-5, None, False)
            s.response_stress_field(coef[0, :m].real, 1.0)
            t0 = time.perf_counter()
            for j in range(a.field_calls):
                s.response_stress_field(coef[j, :m].real if j % 2 == 0 else coef[j, :m].imag, 1.0 if j % 2 == 0 else 0.0)
            per_call = (time.perf_counter() - t0) / a.field_calls
            res["field_route"] = {"calls_timed": a.field_calls, "ms_per_call": per_call * 1e3, "calls_needed": 2 * a.freq,
                                  "seconds_for_the_sweep": per_call * 2 * a.freq,
                                  "one_sweep_call_seconds": res["stress_sweep"]["call_ms"] * 1e-3}
        out[f"modes_{m}"] = res
        print(f"modes_{m}", json.dumps(res), flush=True)
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    s.close()


if __name__ == "__main__":
    main()

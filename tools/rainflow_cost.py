"""Cost of the rainflow kernel on the bench's block: one launch of k_stress_rainflow over a full chunk of rows (what = 33, the
component pass as a first and last launch) next to one launch of k_stress_transient over the same rows (what = 30), on the
same context, the same synthetic modes and the same table, under a half-sine and under a noisy history: the FMA chain is
the same in both kernels and the counter's work depends on the data, since a lane works on its stack only at a reversal and
lanes of a wave turn at different rows.  One Python call of response_stress_rainflow is timed against the route without the
entry: calls of response_stress_transient with 64 probe nodes each, N / 64 of them for the histories of every node, timed on
a few calls and scaled (the count on the host comes on top and is not timed).  The basis is random: the kernels do the same
work on any numbers.  Warm-up, then single launches timed one by one with device events: min / median / max, and the
process's own streaming-copy rate beside them.  Run by hand, under a time limit; no test and no benchmark calls it.

    python tools/rainflow_cost.py [--n 66] [--modes 8,24,64] [--depth 32] [--launches 5] [--probe-calls 3] [--out result.json]
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


def stats(s, what, warmup, launches):
    s.time_kernel(what, warmup, 1)
    t = np.array([s.time_kernel(what, 0, 1) for _ in range(launches)])
    return {"min_ms": float(t.min()), "median_ms": float(np.median(t)), "max_ms": float(t.max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=66, help="block of n x 6n x n cubes (66 = 10M tets, 5.3M dofs)")
    ap.add_argument("--modes", default="8,24,64")
    ap.add_argument("--depth", type=int, default=32)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--probe-calls", type=int, default=3, help="calls of response_stress_transient with 64 probes to time at the last mode count")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    deck = mesh.bar_deck(n=a.n, recipe="clamped")
    s = feahip.FeaSolver(deck)
    s.set_mass(1.0)
    ndof, N = s.ndof, s.ndof // 3
    rng = np.random.default_rng(1)
    F = rng.standard_normal(ndof)
    rows = feahip.TRANSIENT_CHUNK
    t = np.arange(rows) * 1e-3
    loads = {"half-sine": np.where(t < 2.0, np.sin(np.pi * t / 2.0), 0.0), "noise": rng.standard_normal(rows)}
    out = {"elements": int(len(deck.elements)), "nodes": N, "launches": a.launches, "library": feahip.LIB_PATH, "rows": rows,
           "depth": a.depth, "stack_gb": a.depth * 6 * N * 8 / 1e9, "copy_gb_per_s": s.copy_bandwidth(1 << 30)}
    modes = [int(v) for v in a.modes.split(",")]
    for m in modes:
        block = rng.standard_normal((min(m, 8), ndof)) / np.sqrt(ndof)
        phi = np.concatenate([block * (1.0 + 0.01 * p) for p in range((m + 7) // 8)])[:m]
        s.response_set_basis(np.linspace(1.0, 400.0, m) ** 2, phi)
        del phi
        s.response_load(F, False)
        s.response_stress_basis()
        res = {}
        for name, g in loads.items():
            s.response_stress_transient(g, 1e-3, 0.1, 1e-5)
            k30 = stats(s, 30, a.warmup, a.launches)
            t0 = time.perf_counter()
            got = s.response_stress_rainflow(g, 1e-3, 0.1, 1e-5, None, 3.0, 1e3, a.depth)
            call_ms = 1e3 * (time.perf_counter() - t0)
            k33 = stats(s, 33, a.warmup, a.launches)
            res[name] = {"stress_transient": k30, "stress_rainflow": dict(k33, call_ms=call_ms),
                         "rainflow_over_transient": k33["median_ms"] / k30["median_ms"],
                         "ps_per_row_and_step": k33["median_ms"] * 1e-3 / (6 * N * rows) * 1e12,
                         "cycles_mean": float(got["cycles"].mean()), "depth_used_max": int(got["depth_used"].max()),
                         "rows_overflowed": float(((got["status"] & feahip.RAINFLOW_OVERFLOW) != 0).mean())}
            del got
        if a.probe_calls and m == modes[-1]:
            g = loads["noise"]
            probes = np.arange(64, dtype=np.int32)
            s.response_stress_transient(g, 1e-3, 0.1, 1e-5, None, probes)
            t0 = time.perf_counter()
            for j in range(a.probe_calls):
                s.response_stress_transient(g, 1e-3, 0.1, 1e-5, None, probes + 64 * (j + 1))
            per_call = (time.perf_counter() - t0) / a.probe_calls
            res["probe_route"] = {"calls_timed": a.probe_calls, "ms_per_call": per_call * 1e3, "calls_needed": (N + 63) // 64,
                                  "seconds_for_every_node": per_call * ((N + 63) // 64),
                                  "one_rainflow_call_seconds": res["noise"]["stress_rainflow"]["call_ms"] * 1e-3}
        out[f"modes_{m}"] = res
        print(f"modes_{m}", json.dumps(res), flush=True)
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    s.close()


if __name__ == "__main__":
    main()

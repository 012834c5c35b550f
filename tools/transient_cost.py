"""Cost of the transient sweep on the bench's block: k_transient_sweep (what = 25) over 8, 24 and 64 synthetic modes, one
launch over a full chunk of FEA_TRANSIENT_CHUNK rows, as time per step, next to k_response_sweep (what = 23) over 1024
frequencies on the same basis in the same process, as time per frequency -- per frequency and dof that kernel does twice
the FMAs and reads twice the coefficient bytes, so the transient step is expected at half its time -- and next to the
whole call response_transient as the caller sees it, the host's table and the copies included.  The basis is random:
the kernels do the same work on any numbers.  Warm-up, then single launches timed one by one with device events: min /
median / max.  Run every library in a process of its own and alternate them when two are compared (FEAHIP_LIB picks a
variant build).  Run by hand, under a time limit; no test and no benchmark calls it.

    python tools/transient_cost.py [--n 66] [--modes 8,24,64] [--launches 10] [--out result.json]
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


def stats(s, what, warmup, launches):
    s.time_kernel(what, warmup, 1)
    t = np.array([s.time_kernel(what, 0, 1) for _ in range(launches)])
    return {"min_ms": float(t.min()), "median_ms": float(np.median(t)), "max_ms": float(t.max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=66, help="block of n x 6n x n cubes (66 = 10M tets, 5.3M dofs)")
    ap.add_argument("--modes", default="8,24,64")
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--freq", type=int, default=1024, help="frequencies of the sweep timed beside it")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    deck = mesh.bar_deck(n=a.n, recipe="clamped")
    s = feahip.FeaSolver(deck)
    s.set_mass(1.0)
    ndof = s.ndof
    rng = np.random.default_rng(1)
    F = rng.standard_normal(ndof)
    out = {"elements": int(len(deck.elements)), "dofs": ndof, "launches": a.launches, "library": feahip.LIB_PATH,
           "chunk": feahip.TRANSIENT_CHUNK}
    rows = feahip.TRANSIENT_CHUNK
    g = np.sin(0.01 * np.arange(rows))
    for m in [int(v) for v in a.modes.split(",")]:
        block = rng.standard_normal((min(m, 8), ndof)) / np.sqrt(ndof)
        phi = np.concatenate([block * (1.0 + 0.01 * p) for p in range((m + 7) // 8)])[:m]
        s.response_set_basis(np.linspace(1.0, 400.0, m) ** 2, phi)
        del phi
        s.response_load(F, False)
        panels = (m + 7) // 8
        t0 = time.perf_counter()
        s.response_transient(g, 1e-3, 0.1, 1e-5)
        call_ms = 1e3 * (time.perf_counter() - t0)
        k = stats(s, 25, a.warmup, a.launches)
        per_step = k["median_ms"] * 1e-3 / rows
        flop = 2.0 * 8 * panels * ndof
        res = dict(k, rows=rows, call_ms=call_ms, us_per_step=per_step * 1e6, tflop_per_s=flop / per_step / 1e12,
                   fp64_vector_peak_fraction=flop / per_step / FP64_VECTOR_PEAK, coefficient_bytes_per_step=64.0 * panels + 8.0)
        s.response_sweep(np.linspace(0.5, 450.0, a.freq), 0.1, 1e-5)
        k23 = stats(s, 23, a.warmup, a.launches)
        per_freq = k23["median_ms"] * 1e-3 / a.freq
        res["sweep"] = dict(k23, n_freq=a.freq, us_per_frequency=per_freq * 1e6, tflop_per_s=2 * flop / per_freq / 1e12)
        res["step_over_frequency"] = per_step / per_freq
        out[f"modes_{m}"] = res
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    s.close()


if __name__ == "__main__":
    main()

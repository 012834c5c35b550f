"""Cost of the combine kernel on the bench's block: k_response_combine (what = 26) over 8, 16, ... 64 synthetic modes -- one
launch evaluates the quadratic form of every dof -- with the mode values as they are and with their magnitudes (the ABS
rule), next to k_response_sweep (what = 23) over 1024 frequencies on the same basis in the same process: the ratio is the
number of frequencies at which the sweep costs what one combination costs, whatever the number of frequencies behind the
form.  Also the copy bandwidth of the box, to hold the time against the one read of the panels, and the host time of
feahip_host_random_form at FEA_RANDOM_MAX_FREQ frequencies.  The basis is random: the kernels do the same work on any
numbers.  Warm-up, then single launches timed one by one with device events: min / median / max.  Run every library in a
process of its own and alternate them when two are compared (FEAHIP_LIB picks a variant build).  Run by hand, under a time
limit; no test and no benchmark calls it.

    python tools/combine_cost.py [--n 66] [--modes 8,16,24,32,40,48,56,64] [--launches 10] [--out result.json]
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
    ap.add_argument("--modes", default="8,16,24,32,40,48,56,64")
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--freq", type=int, default=1024, help="frequencies of the sweep timed beside it")
    ap.add_argument("--host-freq", type=int, default=feahip.RANDOM_MAX_FREQ, help="frequencies of the host builder timed (0: skip)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    deck = mesh.bar_deck(n=a.n, recipe="clamped")
    s = feahip.FeaSolver(deck)
    s.set_mass(1.0)
    ndof = s.ndof
    rng = np.random.default_rng(1)
    F = rng.standard_normal(ndof)
    out = {"elements": int(len(deck.elements)), "dofs": ndof, "launches": a.launches, "library": feahip.LIB_PATH,
           "copy_gb_per_s": s.copy_bandwidth(1 << 30)}
    for m in [int(v) for v in a.modes.split(",")]:
        block = rng.standard_normal((min(m, 8), ndof)) / np.sqrt(ndof)
        phi = np.concatenate([block * (1.0 + 0.01 * p) for p in range((m + 7) // 8)])[:m]
        lam = np.linspace(1.0, 400.0, m) ** 2
        s.response_set_basis(lam, phi)
        del phi
        s.response_load(F, False)
        panels = (m + 7) // 8
        G = rng.standard_normal((m, m))
        Cm = G @ G.T
        res = {}
        for name, absolute in (("combine", False), ("combine_abs", True)):
            t0 = time.perf_counter()
            s.response_combine(Cm, None, 0.0, absolute)
            call_ms = 1e3 * (time.perf_counter() - t0)
            k = stats(s, 26, a.warmup, a.launches)
            sec = k["median_ms"] * 1e-3
            w = 8 * panels
            flop = 2.0 * (w * (w + 1) / 2 + 2 * w) * ndof
            read = (64.0 * panels + 8.0 + 8.0) * ndof                  # the panels, u_s and the output
            res[name] = dict(k, call_ms=call_ms, tflop_per_s=flop / sec / 1e12, fp64_vector_peak_fraction=flop / sec / FP64_VECTOR_PEAK,
                             gb_per_s=read / sec / 1e9)
        s.response_sweep(np.linspace(0.5, 450.0, a.freq), 0.1, 1e-5)
        k23 = stats(s, 23, a.warmup, a.launches)
        per_freq = k23["median_ms"] / a.freq
        res["sweep"] = dict(k23, n_freq=a.freq, us_per_frequency=per_freq * 1e3)
        res["frequencies_of_equal_cost"] = res["combine"]["median_ms"] / per_freq
        res["frequencies_of_equal_cost_abs"] = res["combine_abs"]["median_ms"] / per_freq
        out[f"modes_{m}"] = res
        print(f"modes_{m}", json.dumps(res), flush=True)
        if a.host_freq and m == 64:
            w = np.linspace(0.0, 450.0, a.host_freq)
            t0 = time.perf_counter()
            feahip.host_random_form(lam, np.ones(m), w, np.ones_like(w), 0.1, 1e-5, None, True, 0)
            out["host_random_form"] = {"n_freq": a.host_freq, "modes": m, "seconds": time.perf_counter() - t0}
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    s.close()


if __name__ == "__main__":
    main()

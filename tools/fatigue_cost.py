"""Cost of the fatigue kernels on the bench's block: k_stress_moments, four forms on the nine combinations of every node in
one launch (what = 31), next to k_stress_combine, one form (what = 28), on the same context, the same synthetic modes and
the same store -- four launches of it are what the one launch replaces -- and k_fatigue_rates, the pointwise statistics of
the 7 N pairs (what = 32).  The basis is random: the kernels do the same work on any numbers.  Warm-up, then single
launches timed one by one with device events: min / median / max.  Run every library in a process of its own and
alternate them when two are compared (FEAHIP_LIB picks a variant build: k_stress_moments with the four forms resident at
every panel count, or at none, is
`make -C fea-large_amd/csrc variant NAME=momres8 VSRC=kernels_stress_fatigue VFLAGS=-DFEA_MOMENTS_RESIDENT_MAX=8`, or `=0`).
Run by hand, under a time limit; no test and no benchmark calls it.

    python tools/fatigue_cost.py [--n 66] [--modes 8,24,64] [--launches 10] [--out result.json]
"""
import argparse
import json
import os
import sys

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
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    deck = mesh.bar_deck(n=a.n, recipe="clamped")
    s = feahip.FeaSolver(deck)
    s.set_mass(1.0)
    ndof, N, E = s.ndof, s.ndof // 3, len(deck.elements)
    rng = np.random.default_rng(1)
    F = rng.standard_normal(ndof)
    out = {"elements": int(E), "nodes": N, "launches": a.launches, "library": feahip.LIB_PATH, "copy_gb_per_s": s.copy_bandwidth(1 << 30)}
    for m in [int(v) for v in a.modes.split(",")]:
        block = rng.standard_normal((min(m, 8), ndof)) / np.sqrt(ndof)
        phi = np.concatenate([block * (1.0 + 0.01 * p) for p in range((m + 7) // 8)])[:m]
        lam = np.linspace(1.0, 400.0, m) ** 2
        s.response_set_basis(lam, phi)
        del phi
        s.response_load(F, False)
        s.response_stress_basis()
        panels, w = (m + 7) // 8, 8 * ((m + 7) // 8)
        G = rng.standard_normal((m, m))
        Cm = G @ G.T
        s.response_stress_combine(Cm)
        # a PSD over the band of the modes on a coarse grid: the kernels' work does not depend on the grid
        omega = np.linspace(0.0, 480.0, 257)
        s.response_stress_fatigue(omega, 1.0 / (1.0 + omega), 0.0, 0.0, 0.02, 3.0, 1e3)
        res = {}
        for name, what in (("stress_combine", 28), ("stress_moments", 31), ("stress_combine_again", 28), ("fatigue_rates", 32)):
            res[name] = stats(s, what, a.warmup, a.launches)
        form_flop = 2.0 * 9 * (w * (w + 1) / 2 + 2 * w) * N
        read = (12 * 64.0 * panels + 6 * 8.0 + 7 * 8.0) * N           # k_stress_combine: twelve row loads per node, T_s, the outputs
        sec = res["stress_moments"]["median_ms"] * 1e-3
        res["stress_moments"].update(tflop_per_s=4 * form_flop / sec / 1e12, fp64_vector_peak_fraction=4 * form_flop / sec / FP64_VECTOR_PEAK,
                                     store_once_gb_per_s=read / sec / 1e9, store_four_times_gb_per_s=4 * read / sec / 1e9)
        sec = res["fatigue_rates"]["median_ms"] * 1e-3
        res["fatigue_rates"]["gb_per_s"] = 7.0 * N * (4 * 8 + 2 * 8 + 3 * 8 + 4) / sec / 1e9
        res["moments_over_four_combines"] = res["stress_moments"]["median_ms"] / (2.0 * (res["stress_combine"]["median_ms"] + res["stress_combine_again"]["median_ms"]))
        out[f"modes_{m}"] = res
        print(f"modes_{m}", json.dumps(res), flush=True)
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    s.close()


if __name__ == "__main__":
    main()

"""Cost of the stress kernels on the bench's block: the element and node passes of the stress store over every panel in use
(what = 27) and k_stress_combine, the nine forms of every node (what = 28), next to k_response_combine (what = 26) on the
same context, the same synthetic modes and the same form.  The basis is random: the kernels do the same work on any
numbers.  Warm-up, then single launches timed one by one with device events: min / median / max.  Run every library in a
process of its own and alternate them when two are compared (FEAHIP_LIB picks a variant build).  Run by hand, under a time
limit; no test and no benchmark calls it.

    python tools/stress_cost.py [--n 66] [--modes 8,64] [--launches 10] [--out result.json]
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
    ap.add_argument("--modes", default="8,64")
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
        s.response_set_basis(np.linspace(1.0, 400.0, m) ** 2, phi)
        del phi
        s.response_load(F, False)
        panels, w = (m + 7) // 8, 8 * ((m + 7) // 8)
        G = rng.standard_normal((m, m))
        Cm = G @ G.T
        t0 = time.perf_counter()
        s.response_stress_basis()
        res = {"basis_call_ms": 1e3 * (time.perf_counter() - t0)}
        k27 = stats(s, 27, a.warmup, a.launches)
        # bytes requested per panel (the caches serve part of them): the element pass reads npe nodes of 192 bytes and the
        # coordinates and writes a record of 384 bytes, the node pass reads a record per visit (npe E of them) and writes
        # 384 bytes per node
        npe = deck.nodes_per_element
        moved = panels * (E * (npe * 192.0 + npe * 64.0 + 384.0) + npe * E * 392.0 + N * 384.0)
        res["store"] = dict(k27, requested_gb_per_s=moved / (k27["median_ms"] * 1e-3) / 1e9)
        s.response_stress_combine(Cm)
        k28 = stats(s, 28, a.warmup, a.launches)
        flop = 2.0 * 9 * (w * (w + 1) / 2 + 2 * w) * N
        read = (12 * 64.0 * panels + 6 * 8.0 + 7 * 8.0) * N           # twelve row loads per node (six differences re-read), T_s, the outputs
        sec = k28["median_ms"] * 1e-3
        res["stress_combine"] = dict(k28, tflop_per_s=flop / sec / 1e12, fp64_vector_peak_fraction=flop / sec / FP64_VECTOR_PEAK,
                                     gb_per_s=read / sec / 1e9)
        s.response_combine(Cm)
        res["combine"] = stats(s, 26, a.warmup, a.launches)
        res["stress_combine_over_combine"] = k28["median_ms"] / res["combine"]["median_ms"]
        out[f"modes_{m}"] = res
        print(f"modes_{m}", json.dumps(res), flush=True)
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    s.close()


if __name__ == "__main__":
    main()

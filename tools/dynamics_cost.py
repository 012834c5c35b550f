"""Cost of the two mass kernels on the path of a dynamic Newton iteration: k_mass_add (K += c M, what = 8) and
k_mass_residual (f -= a0 M (x - xt), what = 9), next to the stiffness+residual assembly (what = 0) and the copy
bandwidth of the box.  Warm-up, then single launches timed one by one with device events: min / median / max.  Run
every configuration in a process of its own.

    python tools/dynamics_cost.py [--n 66] [--quadratic] [--launches 40] [--out result.json]
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


def stats(s, what, warmup, launches):
    s.time_kernel(what, warmup, 1)
    t = np.array([s.time_kernel(what, 0, 1) for _ in range(launches)])
    return {"min_ms": float(t.min()), "median_ms": float(np.median(t)), "max_ms": float(t.max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=66)
    ap.add_argument("--quadratic", action="store_true")
    ap.add_argument("--launches", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    deck = mesh.bar_deck(n=a.n, quadratic=a.quadratic, recipe="clamped")
    s = feahip.FeaSolver(deck)
    s.set_nodes(mesh.deformed_state(deck.nodes))
    asm = stats(s, 0, a.warmup, a.launches)
    s.set_mass(1.0)
    nnzb, rows = int(s.sizes()[4]), len(deck.nodes)
    add, res = stats(s, 8, a.warmup, a.launches), stats(s, 9, a.warmup, a.launches)
    model_add = 152.0 * nnzb                                           # 8 B of m + read and write of the 72-byte block
    model_res = (8.0 + 4.0) * nnzb + 2 * 32.0 * nnzb + 2 * 24.0 * rows  # m, colidx, two gathered node records; f read and written
    out = {"elements": int(len(deck.elements)), "nodes": rows, "blocks": nnzb, "launches": a.launches,
           "assembly_what0": asm, "mass_add_what8": add, "mass_residual_what9": res,
           "copy_gbytes_per_s": s.copy_bandwidth(),
           "mass_add_model_bytes": model_add, "mass_add_gbytes_per_s": model_add / (add["median_ms"] * 1e-3) / 1e9,
           "mass_residual_model_bytes": model_res, "mass_residual_gbytes_per_s": model_res / (res["median_ms"] * 1e-3) / 1e9}
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    s.close()


if __name__ == "__main__":
    main()

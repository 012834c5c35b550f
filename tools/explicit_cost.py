"""Cost of an explicit step: the two pointwise kernels together (k_explicit_kick + k_explicit_finish, what = 10) and
k_gershgorin (what = 11) next to the residual-only assembly (what = 2) and, for one Newmark Newton iteration from the
same process, the stiffness+residual assembly (what = 0), K += a0 M (what = 8), the inertia term (what = 9) and one PCG
iteration (what = 4).  A full explicit step is what = 2 plus what = 10 plus the node update x += u (a 56-byte-per-node
pass, not timed on its own).  Warm-up, then single launches timed one by one with device events: min / median / max, and
the achieved bytes per second of the byte models against the copy bandwidth of the box.  Run every configuration in a
process of its own.

    python tools/explicit_cost.py [--n 66] [--quadratic] [--launches 40] [--out result.json]
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
    s.set_mass(1.0)
    nnzb, rows = s.sizes()["nnzb"], len(deck.nodes)
    res = stats(s, 2, a.warmup, a.launches)
    asm = stats(s, 0, a.warmup, a.launches)                            # (K of the deformed state: what = 11 reads it)
    ger = stats(s, 11, a.warmup, a.launches)
    add, ine, pcg = stats(s, 8, a.warmup, a.launches), stats(s, 9, a.warmup, a.launches), stats(s, 4, a.warmup, a.launches)
    pw = stats(s, 10, a.warmup, a.launches)                            # last: it advances v and a
    # kick: v, a read (64 B), mask (3 B), vh (32 B) and u (24 B) written; finish: f (24 B), ml (8 B), mask (3 B) and vh (32 B)
    # read, v and a written (64 B)
    model_pw = 254.0 * rows
    model_ger = 72.0 * nnzb + 8.0 * rows
    copy = s.copy_bandwidth()
    out = {"elements": int(len(deck.elements)), "nodes": rows, "blocks": nnzb, "launches": a.launches,
           "residual_what2": res, "pointwise_what10": pw, "gershgorin_what11": ger,
           "assembly_what0": asm, "mass_add_what8": add, "mass_residual_what9": ine, "pcg_iteration_what4": pcg,
           "explicit_step_median_ms": res["median_ms"] + pw["median_ms"],
           "newmark_iteration_without_solve_median_ms": asm["median_ms"] + add["median_ms"] + ine["median_ms"],
           "copy_gbytes_per_s": copy, "node_arrays_bytes": 200.0 * rows,
           "pointwise_model_bytes": model_pw, "pointwise_gbytes_per_s": model_pw / (pw["median_ms"] * 1e-3) / 1e9,
           "gershgorin_model_bytes": model_ger, "gershgorin_gbytes_per_s": model_ger / (ger["median_ms"] * 1e-3) / 1e9}
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    s.close()


if __name__ == "__main__":
    main()

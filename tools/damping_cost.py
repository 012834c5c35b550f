"""Cost of the kernels of Rayleigh damping on the path of a damped Newton iteration: k_damp_residual<KD> (what = 22)
against the unfused pair it stands for, SpMV (what = 3) plus k_mass_residual (what = 9), and k_damp_add (what = 21) against
k_mass_add (what = 8), next to the stiffness+residual assembly (what = 0) and the copy bandwidth of the box.  Warm-up,
then single launches timed one by one with device events: min / median / max.  Run every configuration in a process of
its own, and alternate the libraries when two are compared; a library without feahip_set_damping gives the first four
timings alone.

    python tools/damping_cost.py [--n 40] [--quadratic] [--launches 40] [--alpha 0.5] [--beta 0.01] [--out result.json]
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
    ap.add_argument("--n", type=int, default=40)
    ap.add_argument("--quadratic", action="store_true")
    ap.add_argument("--launches", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--alpha", type=float, default=0.5)
    ap.add_argument("--beta", type=float, default=0.01)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    deck = mesh.bar_deck(n=a.n, quadratic=a.quadratic, recipe="clamped")
    s = feahip.FeaSolver(deck)
    s.set_nodes(mesh.deformed_state(deck.nodes))
    out = {"elements": int(len(deck.elements)), "nodes": len(deck.nodes), "launches": a.launches,
           "assembly_what0": stats(s, 0, a.warmup, a.launches)}
    s.set_mass(1.0)
    nnzb, rows = int(s.sizes()["nnzb"]), len(deck.nodes)
    out["blocks"] = nnzb
    out["spmv_what3"] = stats(s, 3, a.warmup, a.launches)
    out["mass_residual_what9"] = stats(s, 9, a.warmup, a.launches)
    out["mass_add_what8"] = stats(s, 8, a.warmup, a.launches)
    out["copy_gbytes_per_s"] = s.copy_bandwidth()
    if hasattr(s, "set_damping"):
        s.set_damping(a.alpha, a.beta)
        res = stats(s, 22, a.warmup, a.launches)
        out["damp_residual_what22"] = res
        kd = a.beta > 0.0
        # per block: the 72-byte block of K_d (KD), m, colidx, three gathered node records; f read and written per row
        model_res = ((72.0 if kd else 0.0) + 8.0 + 4.0 + 3 * 32.0) * nnzb + 2 * 24.0 * rows
        out["damp_residual_model_bytes"] = model_res
        out["damp_residual_gbytes_per_s"] = model_res / (res["median_ms"] * 1e-3) / 1e9
        out["unfused_pair_ms"] = out["spmv_what3"]["median_ms"] + out["mass_residual_what9"]["median_ms"]
        if kd:
            add = stats(s, 21, a.warmup, a.launches)
            out["damp_add_what21"] = add
            model_add = 224.0 * nnzb                                   # K read and written, K_d read, m
            out["damp_add_model_bytes"] = model_add
            out["damp_add_gbytes_per_s"] = model_add / (add["median_ms"] * 1e-3) / 1e9
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    s.close()


if __name__ == "__main__":
    main()

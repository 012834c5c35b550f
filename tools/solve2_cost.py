"""The two-vector product and the two-column PCG iteration against two of the single ones, on the flagship block
(n = 66: 10M linear tetrahedra, bench.py's workload): feahip_time_kernel 6 against twice 3, 7 against twice 4, all
four in the same process, the median of --runs timings of each, interleaved so that drift hits all alike.

    python tools/solve2_cost.py [--n 66] [--runs 7] [--iters 20] [--out result.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=66)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    deck = mesh.bar_deck(n=a.n, recipe="clamped")
    s = feahip.FeaSolver(deck)
    s.set_pcg_variant(0)
    s.set_nodes(mesh.deformed_state(deck.nodes))
    s.update_nodes_with_bc(1.0)
    s.create_stiffness_and_residual()
    s.apply_prescribed_bc(0.0)
    t = {w: [] for w in (3, 6, 4, 7)}
    for _ in range(a.runs):
        for w in t:
            t[w].append(s.time_kernel(w, a.warmup, a.iters))
    med = {w: float(np.median(v)) for w, v in t.items()}
    sizes = s.sizes()
    nnzb, n = sizes["nnzb"], sizes["N"]
    # bytes of a product: 76 per block (72 of values, 4 of column index) and the gathered x, 24 or 48 per block row
    model = (76.0 * nnzb + 48.0 * n) / (2.0 * (76.0 * nnzb + 24.0 * n))
    res = {"n": a.n, "elements": int(len(deck.elements)), "runs": a.runs,
           "spmv_ms": med[3], "spmv2_ms": med[6], "spmv2_over_two_spmv": med[6] / (2 * med[3]),
           "pcg_iteration_ms": med[4], "pcg2_iteration_ms": med[7], "pcg2_over_two_pcg": med[7] / (2 * med[4]),
           "byte_model_ratio": model, "all_ms": {str(w): v for w, v in t.items()}}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    s.close()


if __name__ == "__main__":
    main()

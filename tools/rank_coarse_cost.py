"""Cost of the coarse level across the ranks (preconditioner 2) on ONE GPU: one PCG iteration (time_kernel(4)) on the
n x 6n x n Kuhn block (n = 66: 10M linear tetrahedra, bench.py's workload) with preconditioner 1 and 2 alternately in
one process, and the host + device time of one numeric setup of the coarse level.  On one GPU the coarse space is the
context's own 16 aggregates and nothing is all-reduced: this is the cost of the added kernels and the second stream, not
of the communication, and how much of the all-reduce hides under the cycle needs an 8-GPU node.  For the kernel times
run it under `rocprofv3 --kernel-trace --stats -d <dir> -- python tools/rank_coarse_cost.py` (k_coarse_*).

    python tools/rank_coarse_cost.py [--n 66] [--iters 20] [--repeats 3] [--out result.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fea-large_amd"))

import feahip  # noqa: E402
import mesh  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=66)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    deck = mesh.bar_deck(n=a.n, recipe="clamped")
    s = feahip.FeaSolver(deck)
    s.update_nodes_with_bc(1.0); s.create_stiffness_and_residual(); s.apply_prescribed_bc(0.0)
    ms = {1: [], 2: []}
    for _ in range(a.repeats):
        for kind in (1, 2):
            s.set_preconditioner(kind)
            ms[kind].append(s.time_kernel(4, a.warmup, a.iters))
    # one numeric setup of the coarse level alone (the multigrid's own is current): K re-assembled, same values
    s.set_preconditioner(2)
    s.coarse_info()
    setup = []
    for _ in range(a.repeats):
        s.set_preconditioner(1); s.create_stiffness_and_residual(); s.apply_prescribed_bc(0.0)
        s.amg_info(); s.sync()                                        # the multigrid's numeric part, outside the clock
        s.set_preconditioner(2)
        t0 = time.time()
        info = s.coarse_info()                                        # topology + numeric setup + inverse
        setup.append(time.time() - t0)
    its = {}
    for kind in (1, 2):
        s.set_preconditioner(kind)
        its[kind] = s.solve_slae(feahip.PCG_ILU, 1e-12, 20000)[0]
    res = {"elements": int(len(deck.elements)), "iters": a.iters, "pcg_iteration_ms_kind1": ms[1], "pcg_iteration_ms_kind2": ms[2],
           "kind2_over_kind1": min(ms[2]) / min(ms[1]), "aggregates": info["aggregates"], "coarse_unknowns": info["unknowns"],
           "coarse_topology_and_setup_s": setup, "pcg_iterations_to_1e-12": its}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    s.close()


if __name__ == "__main__":
    main()

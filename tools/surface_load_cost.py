"""Cost of the surface-load kernels on the flagship deck: a follower pressure on the WHOLE outer boundary of the
n x 6n x n Kuhn block (n = 66: 10M linear tetrahedra, bench.py's workload), timed with device events next to the
stiffness+residual assembly with and without the loads.  For the kernel times themselves run it under
`rocprofv3 --kernel-trace --stats -d <dir> -- python tools/surface_load_cost.py` (k_surface_faces, k_surface_nodes).

    python tools/surface_load_cost.py [--n 66] [--iters 50] [--out result.json]
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


def outer_faces(nodes, elements):
    """The element faces lying on the block's six sides (a convex block: those are exactly its boundary faces), in
    the element's face order."""
    lo, hi = nodes.min(axis=0), nodes.max(axis=0)
    tol = 1e-9 * (hi - lo).max()
    out = []
    for lf in mesh.TET4_FACES:
        f = elements[:, lf]
        c = nodes[f]                                                  # [E][3][3]
        on = np.zeros(len(f), dtype=bool)
        for ax in range(3):
            for v in (lo[ax], hi[ax]):
                on |= np.all(np.abs(c[:, :, ax] - v) < tol, axis=1)
        out.append(f[on])
    return np.ascontiguousarray(np.concatenate(out).astype(np.int32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=66)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    deck = mesh.bar_deck(n=a.n, recipe="clamped")
    t0 = time.time()
    faces = outer_faces(deck.nodes, deck.elements)
    nx, ny, nz = mesh.block_dims(a.n)
    assert len(faces) == 4 * (nx * ny + ny * nz + nz * nx), len(faces)
    s = feahip.FeaSolver(deck)
    s.set_nodes(mesh.deformed_state(deck.nodes))
    s.update_nodes_with_bc(1.0)                                       # load factor 1
    asm_plain = s.time_kernel(0, a.warmup, a.iters)
    s.set_surface_loads(faces, np.zeros(len(faces), np.int32), np.tile([0.5, 0.0, 0.0], (len(faces), 1)))
    setup_s = time.time() - t0
    asm_loaded = s.time_kernel(0, a.warmup, a.iters)
    surf = s.time_kernel(5, a.warmup, a.iters)
    s.set_surface_loads([], [], [])
    asm_plain2 = s.time_kernel(0, a.warmup, a.iters)
    res = {"elements": int(len(deck.elements)), "loaded_faces": int(len(faces)), "iters": a.iters,
           "assembly_ms_without_loads": [asm_plain, asm_plain2], "assembly_ms_with_loads": asm_loaded,
           "surface_kernels_ms": surf, "surface_over_assembly": surf / min(asm_plain, asm_plain2),
           "host_setup_s": setup_s}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    s.close()


if __name__ == "__main__":
    main()

"""What it costs to make ONE rank's context of an 8-rank run, two ways, on the n x 6n x n bar block:

  (a) mesh.bar_deck (the whole block) + feahip.RankSolver        -- feahip_create_rank cuts the slab out of the whole mesh
  (b) mesh.bar_slab (the rank's slab) + feahip.LocalRankSolver   -- feahip_create_rank_local is handed the slab

Each variant runs in a fresh child process, one after the other (never two with the GPU open), each under
`timeout -k 10`; a child prints the seconds from its start to a ready context and its peak resident set
(resource.getrusage).  --host-only stops before the context and needs no GPU: the generator plus the host half of the
constructor (feahip_host_rank_mesh for (a), feahip_host_slab_order + feahip_host_rank_local_plan for (b)).
If a variant fails or runs out of time nothing further is started.

    python tools/rank_setup_cost.py [--n 24] [--tet4] [--rank 3] [--nranks 8] [--host-only] [--limit 420] [--out r.json]
"""
import argparse
import json
import os
import resource
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(a):
    t0 = time.time()
    sys.path.insert(0, os.path.join(ROOT, "fea-large_amd"))
    import feahip
    import mesh
    feahip.load_library(); feahip.load_host_library()
    t_import = time.time() - t0
    quadratic = not a.tet4

    def say(what):                                                  # progress on stderr: a long variant is not silent
        print(f"({a.child}) {time.time() - t0:7.1f} s  {what}", file=sys.stderr, flush=True)
    out = {"variant": a.child, "n": a.n, "quadratic": quadratic, "rank": a.rank, "nranks": a.nranks, "host_only": a.host_only}
    if a.child == "a":
        deck = mesh.bar_deck(n=a.n, quadratic=quadratic)
        out["mesh_s"] = time.time() - t0 - t_import
        out["whole_nodes"], out["whole_elements"] = len(deck.nodes), len(deck.elements)
        say(f"whole deck built: {len(deck.nodes)} nodes, {len(deck.elements)} elements")
        if a.host_only:
            m = feahip.host_rank_mesh(deck, a.rank, a.nranks)
            out["local_nodes"], out["owned_nodes"], out["local_elements"] = m["local_nodes"], m["owned_nodes"], m["local_elements"]
        else:
            s = feahip.RankSolver(deck, a.rank, a.nranks)
    else:
        slab = mesh.bar_slab(a.rank, a.nranks, n=a.n, quadratic=quadratic)
        out["mesh_s"] = time.time() - t0 - t_import
        if not a.keep_order:
            slab = slab.reordered()                                 # the order RankSolver's slab has: the library's numbering
            out["reorder_s"] = time.time() - t0 - t_import - out["mesh_s"]
        out["whole_nodes"] = slab.n_global_nodes
        say(f"slab built: {len(slab.nodes)} nodes, {len(slab.elements)} elements")
        if a.host_only:
            feahip.host_rank_local_plan(slab, a.rank, a.nranks)
            out["local_nodes"], out["owned_nodes"], out["local_elements"] = len(slab.nodes), slab.n_own, len(slab.elements)
        else:
            s = feahip.LocalRankSolver(slab, a.rank, a.nranks)
    if not a.host_only:
        s.sync()
        out["local_nodes"], out["owned_nodes"], out["local_elements"] = s.N, s.n_own, s.E
    out["ready_s"] = time.time() - t0
    out["import_s"] = t_import
    out["peak_rss_mb"] = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1024.0
    print("RESULT " + json.dumps(out), flush=True)
    if not a.host_only:
        s.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=24)
    ap.add_argument("--tet4", action="store_true", help="linear tetrahedra instead of the 10-node ones")
    ap.add_argument("--rank", type=int, default=3)
    ap.add_argument("--nranks", type=int, default=8)
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--keep-order", action="store_true", help="(b) without Slab.reordered()")
    ap.add_argument("--limit", type=int, default=420, help="seconds a variant may take")
    ap.add_argument("--box", default="", help="a name for the machine, copied into the result")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", choices=["a", "b"], default=None)
    a = ap.parse_args()
    if a.child:
        return child(a)
    res = {"n": a.n, "quadratic": not a.tet4, "rank": a.rank, "nranks": a.nranks, "host_only": a.host_only, "box": a.box,
           "cpus": len(os.sched_getaffinity(0)), "variants": {}}
    rc = 0
    for v in ("a", "b"):
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", v, "--n", str(a.n),
               "--rank", str(a.rank), "--nranks", str(a.nranks)]
        cmd += (["--tet4"] if a.tet4 else []) + (["--host-only"] if a.host_only else []) + (["--keep-order"] if a.keep_order else [])
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            res["variants"][v] = {"failed": p.returncode, "output": p.stdout[-1500:]}
            print(f"variant ({v}) ended with status {p.returncode}; nothing further is started", file=sys.stderr)
            rc = 1
            break
        res["variants"][v] = json.loads(line[0][len("RESULT "):])
        print(f"({v}) ready in {res['variants'][v]['ready_s']:.2f} s, peak RSS {res['variants'][v]['peak_rss_mb']:.0f} MB", flush=True)
    if rc == 0:
        va, vb = res["variants"]["a"], res["variants"]["b"]
        res["seconds_b_over_a"] = vb["ready_s"] / va["ready_s"]
        res["rss_b_over_a"] = vb["peak_rss_mb"] / va["peak_rss_mb"]
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return rc


if __name__ == "__main__":
    sys.exit(main())

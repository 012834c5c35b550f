#!/usr/bin/env python3
"""gather_run_costs.py -- what the runs of the linear-tet gather kernel cost, from the in-kernel stamps.

The diagnostic build (make debug with -DFEAHIP_NOABL added to the Makefile's CXXFLAGS) stores one line per run and wave when
FEAHIP_GATHER_STAMPS=1;
with FEAHIP_GATHER_STAMPS_FILE=path the lines of the 50th launch are written to `path`.  This script sets the runs'
shader cycles (wave 0) against what the host knows about the chunks of every run (the same maps, rebuilt here on the
host under the same FEAHIP_GATHER_* settings, for the same number of compute units and by the same build: the cut
follows the cost model's coefficients):

  * the slowest run against the mean run, per set of stamps;
  * a least-squares fit (no intercept: runs of one launch hold nearly the same number of chunks) of the run totals of all
    sets together to the sums of the quantities of the cost model (gather.cpp, gather_chunk_cost) -- the coefficients
    the model carries;
  * a second fit by kind of chunk: interior (full rows, the most elements), partial (fewer rows), face (the rest), and
    what requesting the successor's map words adds.  Two sets with different walks (row order and grouped) separate the
    words from the face bricks that mostly request them in row order.

  python tools/gather_run_costs.py --stamps a.bin,order=0,balance=0 b.bin [--n 66 | --mesh tetgen] [--ncu 256] [--json out.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "fea-large_amd"), os.path.join(ROOT, "tests"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

HEADER = ("r0", "r1", "b0", "nb", "nnode", "nelem", "noffd", "depth", "nvthr", "vdepth", "ddepth", "wd0", "wd1", "wd2", "flags", "pad")


def headers(walk):
    """The 64-byte headers of the records, as a dict of int arrays in walk order."""
    rec = walk["blob"].reshape(walk["chunks"], walk["stride"])[:, :64]
    h = np.ascontiguousarray(rec).view(np.int32).reshape(walk["chunks"], 16)
    return {k: h[:, i].astype(np.int64) for i, k in enumerate(HEADER)}


def model_terms(h):
    """The quantities gather_chunk_cost multiplies its coefficients with, per record."""
    simd = np.zeros((len(h["nelem"]), 4), dtype=np.int64)
    for w in range(12):
        simd[:, w & 3] += (h[f"wd{w >> 2}"] >> (8 * (w & 3))) & 255
    return {"chunk": np.ones_like(h["nelem"]), "elem_wave": (h["nelem"] + 63) // 64, "list_word": simd.max(axis=1) + h["ddepth"],
            "block": h["nb"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stamps", required=True, nargs="+", help="file[,order=0][,balance=0][,run=n]: stamps and the settings they were taken under")
    ap.add_argument("--n", type=int, default=66)
    ap.add_argument("--mesh", default="block", choices=["block", "tetgen"])
    ap.add_argument("--ncu", type=int, default=256)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import feahip
    import mesh

    if args.mesh == "tetgen":
        import bench
        deck = bench.tetgen_corner_tets(feahip, mesh)
    else:
        deck = mesh.bar_deck(n=args.n, recipe="clamped")
    ids, _ = feahip.host_numbering(deck.elements, deck.nodes)
    el = ids[deck.elements]
    out = {"sets": {}}
    As, Bs, cs = [], [], []
    for spec in args.stamps:
        path, *settings = spec.split(",")
        for k in ("ORDER", "BALANCE", "RUN", "NRUNS"):
            os.environ.pop("FEAHIP_GATHER_" + k, None)
        for kv in settings:
            k, v = kv.split("=")
            os.environ["FEAHIP_GATHER_" + k.upper()] = v
        raw = np.fromfile(path, dtype=np.uint64)
        nruns, nw = int(raw[0]), int(raw[1])
        st = raw[2:].reshape(nruns, nw, 8).astype(np.float64)
        cyc = st[:, 0, 6]
        w = feahip.host_gather_walk(el, len(deck.nodes), ncu=args.ncu)
        if w["runs"] != nruns:
            sys.exit(f"{path} holds {nruns} runs, the host builds {w['runs']}: other settings or another --ncu")
        h = headers(w)
        rs = w["run_start"]
        last = np.zeros(w["chunks"], dtype=bool)
        last[rs[1:] - 1] = True
        loads = ((h["flags"] & 1) == 0) & ~last           # record i requests its successor's words unless flagged or the last of its run
        terms = model_terms(h)
        terms["words"] = loads.astype(np.int64)
        rows = h["r1"] - h["r0"]
        interior = (rows == rows.max()) & (h["nelem"] == h["nelem"].max())
        partial = rows < rows.max()
        kinds = {"interior": interior, "face": ~interior & ~partial, "partial": partial, "words": loads}
        A = np.stack([np.add.reduceat(v, rs[:-1]) for v in terms.values()], axis=1).astype(np.float64)
        B = np.stack([np.add.reduceat(v.astype(np.int64), rs[:-1]) for v in kinds.values()], axis=1).astype(np.float64)
        mod = np.add.reduceat(w["cost"].astype(np.int64), rs[:-1]).astype(np.float64)
        full = cyc > 0.8 * np.median(cyc)                  # the short last run of an equal-count cut says nothing about the rest
        out["sets"][spec] = {"runs": nruns, "chunks": w["chunks"], "clock_MHz": 100.0 * st[:, 0, 6].sum() / max(st[:, 0, 7].sum(), 1.0),
                             "chunks_per_run": [int(np.diff(rs).min()), int(np.diff(rs).max())],
                             "run_cycles": {"mean": cyc.mean(), "mean_of_full_runs": cyc[full].mean(), "max": cyc.max(), "min": cyc.min(),
                                            "max_over_mean": cyc.max() / cyc.mean(), "max_over_mean_of_full_runs": cyc.max() / cyc[full].mean()},
                             "modelled_run_cost": {"mean": mod.mean(), "max": mod.max(), "max_over_mean": mod.max() / mod.mean(),
                                                   "measured_over_modelled": cyc.sum() / mod.sum()},
                             "kind_counts": {k: int(v.sum()) for k, v in kinds.items()}}
        As.append(A[full]); Bs.append(B[full]); cs.append(cyc[full])
    A, B, c = np.vstack(As), np.vstack(Bs), np.concatenate(cs)
    coef, *_ = np.linalg.lstsq(A, c, rcond=None)
    out["model_fit"] = {k: float(v) for k, v in zip(list(terms), coef)}
    out["model_fit_rms_residual"] = float(np.sqrt(((c - A @ coef) ** 2).mean()))
    kc, *_ = np.linalg.lstsq(B, c, rcond=None)
    out["kind_fit"] = {k: float(v) for k, v in zip(list(kinds), kc)}
    out["kind_fit_rms_residual"] = float(np.sqrt(((c - B @ kc) ** 2).mean()))
    for k, v in out.items():
        print(k, json.dumps(v) if isinstance(v, dict) else v)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

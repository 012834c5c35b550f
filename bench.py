#!/usr/bin/env python3
"""bench.py -- element-stiffness assemblies/s on the BASELINE.json block.

A step = one pass of the hot path over the mesh: stiffness + residual
assembly of every element (state evaluation at the Gauss points included,
one-time pattern build excluded), inputs resident in HBM.  Default workload:
BASELINE.json configs[2], the 10M linear-tet Neo-Hookean block
(66 x 396 x 66 Kuhn cubes on the reference's 1 x 6 x 1 bar).

  python bench.py --gpus N --steps K --warmup W          (any N: with N > 1 and no WORLD_SIZE in the environment
                                                          this process starts the N ranks itself, as children)
  python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N ...

With N > 1 the block rows (hence the elements that touch them) are sharded
over the ranks as slabs across the long axis; assembly needs no collective,
so the data path has none -- torch.distributed (RCCL) only carries the
barrier and the max-over-ranks of the wall time.  Rank 0 prints ONE JSON line.

A plain run does only what the headline needs: set up, ramp the clocks, warm
up, time the K steps, write --dump-outputs if asked, print the line.  Everything
else the benchmark measures or checks runs with --full, after the timed steps:
per-kernel timings and the roofline, the cross-check of the timed K, the copy
bandwidth, the TET10, HEX8 and off-lattice legs, the PCG / Newton solve legs
(with N > 1: the RCCL communicator they need) and the CPU baselines (the
all-cores ones before the GPU is touched).  The --cpu-sample, --no-newton,
--cpu-single-only, --no-tet10 and --no-off-lattice switches choose among those.
"""
import argparse
import json
import os
import sys
import threading
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.join(ROOT, "fea-large_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

HBM_PEAK_GBS = 8000.0       # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec


def algorithmic_bytes(npe, E, N, nnz):
    """every input read once, every output written once --
    int32 connectivity, X0 and x, FP64 CSR values, residual."""
    return 4 * npe * E + 48 * N + 8 * nnz + 24 * N


def spmv_bytes(nnz, N):
    return 8 * nnz + 4 * nnz // 9 + 4 * (N + 1) + 48 * N


def pmc_traffic(args, world, kernel):
    """HBM bytes per assembly launch from rocprofv3 PMC counters (FETCH_SIZE + WRITE_SIZE, separate passes,
    tools/pmc_profile.sh, corrected as MI355X_MICROARCH.md prescribes).  bench.py cannot collect PMC itself: the
    number is the one measured for THIS kernel and configuration (profiles/pmc_traffic.json carries the kernel, the
    numbering and the commit it was measured at), and null for anything else.  Returns (bytes, provenance)."""
    path = os.path.join(ROOT, "profiles", "pmc_traffic.json")
    if world != 1 or args.n != 66 or args.quadratic or args.model != "neohookean" or args.mesh != "block" or not os.path.exists(path):
        return None, None
    try:
        rec = json.load(open(path))
        # the library numbers the nodes itself now: every numbering of the caller ends in the same bricks
        if rec.get("kernel") != kernel or rec.get("code_sha256") != kernel_code_hash():
            return None, None                       # measured for other code: a stale constant is dropped, not printed
        return rec["assembly_bytes_per_launch"], {k: rec.get(k) for k in ("commit", "source", "fetch_correction", "code_sha256")}
    except Exception:                               # noqa: BLE001
        return None, None


def tetgen_corner_tets(feahip, mesh, copies=(8, 8, 7)):
    """The unstructured linear-tet mesh of the off-lattice legs: the tetrahedra on the corner nodes of the reference's
    TetGen deck brick_fine.sexp (deck order kept, sexp_loader.c:170-215), `copies` translated copies side by side."""
    import gzip
    import shutil
    import tempfile
    src = os.path.join(ROOT, "tests", "golden", "decks", "brick_fine.sexp.gz")
    with tempfile.TemporaryDirectory() as td:
        pth = os.path.join(td, "brick_fine.sexp")
        with gzip.open(src, "rb") as fi, open(pth, "wb") as fo:
            shutil.copyfileobj(fi, fo)
        bf = feahip.Deck.load(pth)
    bf.presc_node = (bf.presc_node - 1).astype(np.int32)         # the deck's boundary ids are 1-based
    return mesh.tiled(mesh.corner_tets(bf), copies)


def kernel_code_hash():
    """sha256 over the sources the dominant assembly kernel and its maps are built from: profiles/pmc_traffic.json
    carries the hash its PMC passes were measured at."""
    import hashlib
    h = hashlib.sha256()
    for f in ("kernels_gather.hip", "gather_device.h", "gather.cpp", "fem_device.h", "renumber.cpp", "feahip_internal.h", "pattern.cpp",
              "kernels_assemble.hip", "dpp_device.h"):
        with open(os.path.join(ROOT, "fea-large_amd", "csrc", f), "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()


DUMP_BYTES = 64 * 10 ** 6       # --dump-outputs: everything written, .npy headers included, stays under this
DUMP_SEED = 20261015


def dump_outputs(solver, out_dir):
    """What the timed path hands its caller after a step -- the global stiffness matrix (scalar CSR in the caller's dof
    ids, feahip_get_matrix_yale64) and the residual forces -- as float64 .npy files in out_dir.  Rows are taken in a
    fixed seeded order until the files would pass DUMP_BYTES (all rows when they fit), then written in ascending order:
      rows                   the dof ids of the rows written
      stiffness_row_offsets  offsets of those rows into the next two arrays (len(rows) + 1)
      stiffness_columns      the column (dof) ids of their non-zeros
      stiffness_values       their values
      residual               the residual forces at those dofs
    Ids are stored as float64 (exact below 2^53).  Returns a short description for the JSON line."""
    off, idx, val = solver.matrix_yale64()
    f = solver.forces()
    ndof = len(off) - 1
    rowlen = np.diff(off)
    order = np.random.default_rng(DUMP_SEED).permutation(ndof)
    # bytes after taking the first r rows of `order`: rows + residual + offsets (8 B each per row, +8) + 16 B per non-zero
    cost = 8 * (3 * np.arange(1, ndof + 1) + 1) + 16 * np.cumsum(rowlen[order]) + 5 * 128
    r = int(np.searchsorted(cost, DUMP_BYTES, side="right"))
    rows = np.sort(order[:r])
    lens = rowlen[rows]
    sub_off = np.zeros(r + 1, dtype=np.int64)
    np.cumsum(lens, out=sub_off[1:])
    take = np.repeat(off[rows] - sub_off[:-1], lens) + np.arange(sub_off[-1])
    os.makedirs(out_dir, exist_ok=True)
    arrays = {"rows": rows, "stiffness_row_offsets": sub_off, "stiffness_columns": idx[take], "stiffness_values": val[take],
              "residual": f[rows]}
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), np.ascontiguousarray(a, dtype=np.float64))
    return {"dir": os.path.abspath(out_dir), "rows": r, "of_rows": ndof, "nonzeros": int(sub_off[-1]), "of_nonzeros": int(off[-1]),
            "seed": DUMP_SEED}


def cpu_baseline(n_sample, quadratic=False, model=None):
    """The oracle (CPU restatement of the reference loops, 1 thread) timed on
    a bounded sample of the same workload: a smaller Kuhn block of the same
    bar in the same deformed state."""
    import mesh
    from oracle_binding import OracleSolver
    kw = {} if model is None else {"model": model}
    deck = mesh.bar_deck(n=n_sample, quadratic=quadratic, **kw)
    o = OracleSolver(deck)
    o.set_nodes(mesh.deformed_state(deck.nodes))
    t0 = time.perf_counter()
    o.update_state()
    o.create_stiffness()
    o.create_residual_forces()
    dt = time.perf_counter() - t0
    E = len(deck.elements)
    return {"value": E / dt, "unit": "elements/s", "cores": 1, "kind": "port",
            "sample": f"{E} {'TET10/5GP' if quadratic else 'TET4'} of the same bar ({n_sample}x{6 * n_sample}x{n_sample} cubes), "
                      f"state+stiffness+residual, {dt:.1f} s, oracle/fea_oracle.c -O2 -ffp-contract=off"}


_WORKER = r"""
import json, sys, time
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import mesh
from oracle_binding import OracleSolver
n, quadratic, model, t_go = int(sys.argv[3]), sys.argv[4] == "1", int(sys.argv[5]), float(sys.argv[6])
deck = mesh.bar_deck(n=n, quadratic=quadratic, model=model)
o = OracleSolver(deck)
o.set_nodes(mesh.deformed_state(deck.nodes))
while time.time() < t_go:            # all copies start their timed region together
    time.sleep(0.01)
t0 = time.perf_counter()
o.update_state(); o.create_stiffness(); o.create_residual_forces()
print(json.dumps({"E": len(deck.elements), "dt": time.perf_counter() - t0, "late": time.time() - t_go}))
"""


_WORKER_OMP = r"""
import json, sys, time
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import mesh
from oracle_binding import OracleSolver
n, quadratic, model, threads = int(sys.argv[3]), sys.argv[4] == "1", int(sys.argv[5]), int(sys.argv[6])
deck = mesh.bar_deck(n=n, quadratic=quadratic, model=model)
o = OracleSolver(deck)
o.set_nodes(mesh.deformed_state(deck.nodes))
o.assemble_coloured(threads)                      # threads started, pages touched
t0 = time.perf_counter()
ncol = o.assemble_coloured(threads)
print(json.dumps({"E": len(deck.elements), "dt": time.perf_counter() - t0, "colours": ncol}))
"""


def cpu_baseline_openmp(n_sample, quadratic, model, cores):
    """ONE problem on all host cores: the oracle's loops with the elements coloured (no two elements of a colour share
    a node) and every colour an OpenMP parallel loop -- SURVEY.md 8(d)(ii).  A child process, started before the GPU is
    touched (OMP_NUM_THREADS set for it alone)."""
    import subprocess
    args = [sys.executable, "-c", _WORKER_OMP, os.path.join(ROOT, "fea-large_amd"), os.path.join(ROOT, "tests"),
            str(n_sample), "1" if quadratic else "0", str(model), str(cores)]
    env = dict(os.environ, OMP_NUM_THREADS=str(cores), OMP_PROC_BIND="false")
    pr = subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True, timeout=600, env=env)
    r = json.loads(pr.stdout.strip().splitlines()[-1])
    return {"value": r["E"] / r["dt"], "unit": "elements/s", "cores": cores, "kind": "port",
            "sample": f"{r['E']} elements of the same bar in ONE oracle context, {r['colours']} colours, every colour an OpenMP parallel loop "
                      f"over {cores} threads (oracle/fea_oracle.c orc_assemble_coloured), state+stiffness+residual, {r['dt']:.1f} s"}


def cpu_baseline_all_cores(n_sample, quadratic, model, cores):
    """The same single-threaded oracle, one independent copy of the sample block per host core, all timed
    together: the reference is single-threaded by construction, so this is what the box's cores
    can do with it -- independent problems side by side.  Separate processes, started before the GPU is touched."""
    import subprocess
    t_go = time.time() + (14.0 if not quadratic else 8.0) + 0.12 * n_sample
    args = [sys.executable, "-c", _WORKER, os.path.join(ROOT, "fea-large_amd"), os.path.join(ROOT, "tests"),
            str(n_sample), "1" if quadratic else "0", str(model), repr(t_go)]
    procs = [subprocess.Popen(args, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True) for _ in range(cores)]
    outs = []
    for pr in procs:
        try:
            o, _ = pr.communicate(timeout=300)
            outs.append(json.loads(o.strip().splitlines()[-1]))
        except Exception:                           # noqa: BLE001
            pr.kill()
    if not outs or max(r["late"] - r["dt"] for r in outs) > 0.5:       # a copy missed the common start
        return None
    E = outs[0]["E"]
    return {"value": sum(r["E"] / r["dt"] for r in outs), "cores": len(outs),
            "slowest_copy_s": max(r["dt"] for r in outs), "elements_per_copy": E}


def self_launch(n, argv):
    """`python3 bench.py --gpus N` started by hand (no torch.distributed.run around it): this process touches neither
    the GPU nor torch; it starts the N ranks as child processes (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* as
    torch.distributed.run would set them), lets rank 0's stdout through (the ONE JSON line), and leaves with the
    worst return code.  One command drives all ranks, as one solve() call does in the reference (fea_solver.c:130-242).
    Never os.exec*: a process that replaces itself after the GPU was initialised takes the box down."""
    import socket
    import subprocess
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), FEAHIP_BENCH_SELF_LAUNCHED="1")
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + argv, env=env,
                                      stdout=None if r == 0 else subprocess.DEVNULL))
    # a rank that dies leaves the others in a barrier: once one has failed the rest get a grace period, then SIGTERM
    # by PID (never by pattern); the whole launch is bounded as well
    deadline = time.time() + float(os.environ.get("FEAHIP_BENCH_LAUNCH_TIMEOUT", "1500"))
    failed_at = None
    while any(p.poll() is None for p in procs):
        time.sleep(0.2)
        if failed_at is None and any(p.poll() not in (None, 0) for p in procs):
            failed_at = time.time()
        if (failed_at is not None and time.time() - failed_at > 60) or time.time() > deadline:
            for p in procs:
                if p.poll() is None:
                    p.terminate()
            time.sleep(5)
            for p in procs:
                if p.poll() is None:
                    p.kill()
            break
    rcs = [p.wait() for p in procs]
    bad = [(r, rc) for r, rc in enumerate(rcs) if rc != 0]
    if bad:
        print("bench.py: ranks with a non-zero exit code: " + ", ".join(f"rank {r}: {rc}" for r, rc in bad), file=sys.stderr)
    return next((min(abs(rc), 255) for rc in rcs if rc != 0), 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--n", "--cubes", dest="n", type=int, default=66, help="block of n x 6n x n cubes (66 = 10M tets, 31 = 1M)")
    ap.add_argument("--quadratic", action="store_true", help="TET10 / 5 Gauss points instead of TET4 / 1")
    ap.add_argument("--hex", action="store_true", help="HEXAHEDRA8 / 8 Gauss points: one trilinear brick per cube (n x 6n x n bricks)")
    ap.add_argument("--model", default="neohookean", choices=["neohookean", "a5"])
    ap.add_argument("--cpu-sample", type=int, default=None,
                    help="--full: n of the CPU-baseline sample block (0 = skip; default: ~10 s of single-core work, 48 for TET4, 14 for TET10)")
    ap.add_argument("--no-newton", action="store_true", help="--full: skip the single full Newton iteration")
    ap.add_argument("--assembly", default="auto", help="assembly strategy: auto | gather | staged | ... (fea_hip.h)")
    ap.add_argument("--numbering", default="lex", help="node numbering the CALLER hands in: 'lex' = x fastest, z, y slowest (default; the "
                    "library numbers the nodes itself, csrc/renumber.cpp), 'brick' = bricks of 4x4x4 nodes (3x4x4 half-grid nodes with "
                    "--quadratic), or bx,by,bz")
    ap.add_argument("--cpu-single-only", action="store_true", help="--full: skip the one-oracle-copy-per-core CPU baseline")
    ap.add_argument("--no-tet10", action="store_true", help="--full: skip the small TET10 and HEX8 legs of extras")
    ap.add_argument("--mesh", default="block", choices=["block", "tetgen"],
                    help="tetgen: the unstructured linear-tet mesh of the third off-lattice leg (corner tetrahedra of the reference's "
                         "TetGen deck, 8 x 8 x 7 copies) as THE workload, assembly only -- for rocprofv3 / PMC passes of that case")
    ap.add_argument("--no-off-lattice", action="store_true", help="--full: skip the off-lattice legs of extras (jittered + permuted block, tiled TetGen deck)")
    ap.add_argument("--pcg-variant", type=int, default=-1, help="-1: the context's default; 0: two-reduction PCG; 1: single-reduction PCG")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one computed (stiffness matrix rows and residual, a fixed "
                         "seeded sample of at most 64 MB in all) to DIR/<name>.npy, float64 (one GPU only)")
    ap.add_argument("--full", action="store_true",
                    help="also run what the headline does not need: kernel timings and roofline, the check of the timed K, "
                         "copy bandwidth, the TET10 / HEX8 / off-lattice legs, the solve legs and the CPU baselines")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.warmup < 0:
        ap.error("--warmup must not be negative")
    if args.dump_outputs is not None and args.gpus != 1:
        ap.error("--dump-outputs needs --gpus 1")
    if args.mesh == "tetgen":                       # assembly of that mesh only: no solve, no other element, no CPU leg
        args.no_newton = args.no_tet10 = args.no_off_lattice = True
        args.cpu_sample = 0
    if args.cpu_sample is None:
        args.cpu_sample = 0 if args.hex else 14 if args.quadratic else 48     # (the CPU legs are wired for the tet blocks)

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # started like `--gpus 1` is started: become the launcher (before feahip / torch / any GPU call)
        sys.exit(self_launch(args.gpus, sys.argv[1:]))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    import feahip
    import mesh
    model = feahip.MODEL_COMPRESSIBLE_NEOHOOKEAN if args.model == "neohookean" else feahip.MODEL_A5
    cpu_all = cpu_omp = None
    if args.full and world == 1 and args.cpu_sample > 0 and not args.cpu_single_only:
        # before anything touches the GPU: child processes, one oracle copy per host core (at most 16)
        try:
            cpu_all = cpu_baseline_all_cores(args.cpu_sample, args.quadratic, model, min(16, os.cpu_count() or 1))
        except Exception as e:                      # noqa: BLE001
            print(f"all-cores CPU baseline skipped: {e}", file=sys.stderr)
        try:
            cpu_omp = cpu_baseline_openmp(args.cpu_sample, args.quadratic, model, min(16, os.cpu_count() or 1))
        except Exception as e:                      # noqa: BLE001
            print(f"OpenMP CPU baseline skipped: {e}", file=sys.stderr)
    import torch
    if world != args.gpus:
        if rank == 0:
            print(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}; launch with torch.distributed.run", file=sys.stderr)
        sys.exit(2)
    if not torch.cuda.is_available():
        print("bench.py needs an MI355X: the hot path has no CPU mode", file=sys.stderr)
        sys.exit(2)
    # rehearsal of the multi-rank code path on a box with fewer GPUs than ranks (FEAHIP_BENCH_BACKEND=gloo): ranks
    # share devices and torch.distributed runs over gloo; the driver's runs use one GPU per rank over nccl (= RCCL)
    backend = os.environ.get("FEAHIP_BENCH_BACKEND", "nccl")
    if backend != "nccl":
        local = local % torch.cuda.device_count()
    torch.cuda.set_device(local)
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(backend)

    def barrier():
        if world > 1:
            dist.barrier()

    t_setup = time.perf_counter()
    # 'brick': 4x4x4 nodes for linear tetrahedra, 3x4x4 nodes of the half-spacing grid for 10-node tetrahedra (48 rows: one
    # gather chunk of kernels_gather10.hip), 4x4x4 nodes for 8-node bricks
    brick = (None if args.numbering == "lex" else ((3, 4, 4) if args.quadratic else (4, 4, 4)) if args.numbering == "brick"
             else tuple(int(v) for v in args.numbering.split(",")))
    if args.mesh == "tetgen":
        if world > 1 or args.quadratic or args.hex:
            print("bench.py: --mesh tetgen is a one-GPU linear-tet workload", file=sys.stderr)
            sys.exit(2)
        deck = tetgen_corner_tets(feahip, mesh)
    else:
        deck = mesh.bar_deck(n=args.n, quadratic=args.quadratic, hexa=args.hex, recipe="clamped", model=model, brick=brick,
                             solver_type=feahip.PCG_ILU, solver_tolerance=1e-14, solver_max_iter=20000)
    free0 = torch.cuda.mem_get_info(local)[0]
    comm_ok = False
    if world > 1:
        # a rank holds only its slab (feahip_create_rank): the nodes it owns, the elements around them, their halo --
        # locally indexed; the timed assembly needs no collective; the RCCL communicator of the sharded solve is built
        # afterwards, under the watchdog, so a wedged rendezvous cannot cost the line
        solver = feahip.RankSolver(deck, rank, world, device=local)
        local_nodes = solver.node_global.astype(np.int64)
    else:
        solver = feahip.FeaSolver(deck, device=local)
        local_nodes = slice(None)
    solver.set_assembly(getattr(feahip, "ASM_" + args.assembly.upper()))
    if args.pcg_variant >= 0:
        solver.set_pcg_variant(args.pcg_variant)
    solver.set_nodes(mesh.deformed_state(deck.nodes)[local_nodes])
    solver.create_stiffness_and_residual()              # builds the assembly maps of the rows this rank owns
    solver.sync()
    sz = solver.sizes()
    t_setup = time.perf_counter() - t_setup
    dev_bytes = free0 - torch.cuda.mem_get_info(local)[0]
    in_use = solver.assembly_in_use()
    kernel = {feahip.ASM_GATHER: "k_assemble_gather10" if (args.quadratic or args.hex) else "k_assemble_gather", feahip.ASM_STAGED: "k_assemble_visit", feahip.ASM_PIPELINED: "k_assemble_run",
              feahip.ASM_SHARED: "k_assemble_quad", feahip.ASM_PATCH: "k_assemble_patch", feahip.ASM_PAIRED: "k_assemble_pair",
              feahip.ASM_ATOMIC: "k_assemble_atomic"}.get(in_use, "k_assemble_rowowner")

    E_total, N = len(deck.elements), len(deck.nodes)
    if world > 1:
        # the whole matrix's non-zeros = the sum of the ranks' owned rows
        nn = torch.tensor([solver.nnzb_owned * 9], dtype=torch.int64, device="cuda" if backend == "nccl" else "cpu")
        dist.all_reduce(nn)
        nnz = int(nn.item())
    else:
        nnz = sz["nnzb"] * 9
    # The device needs ~25 back-to-back launches (~30 ms of load) to reach its sustained clocks: the rocprofv3 trace
    # of this program shows the same kernel on the same data going from 1.25 to 1.01 ms over its first 25 launches
    # (profiles/r01_l_*).  A Newton loop keeps the device busy for seconds, so the sustained rate is the
    # one to report: a fixed, untimed ramp precedes the contract's W warm-up steps and K timed steps.
    RAMP = 0
    t_ramp = time.perf_counter()
    while RAMP < 30 or time.perf_counter() - t_ramp < 0.05:      # >= 30 launches and >= 50 ms of load (a shard's launch is short)
        for _ in range(10):
            solver.create_stiffness_and_residual()
        solver.sync()
        RAMP += 10
    for _ in range(args.warmup):
        solver.create_stiffness_and_residual()
    solver.sync(); torch.cuda.synchronize(); barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        solver.create_stiffness_and_residual()
    solver.sync(); torch.cuda.synchronize(); barrier()
    dt = time.perf_counter() - t0
    if world > 1:
        tt = torch.tensor([dt], dtype=torch.float64, device="cuda" if backend == "nccl" else "cpu")
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        dt = float(tt.item())
    ms_per_step = 1e3 * dt / args.steps
    value = E_total * args.steps / dt
    dumped = None
    if args.dump_outputs is not None:
        # before anything below assembles again: the matrix and residual of the last timed step (the headline is
        # measured; the kernel timings of extras below then follow seconds of host work instead of the timed steps)
        dumped = dump_outputs(solver, args.dump_outputs)

    measured = {}
    if args.full:
        share = 1.0 / world
        # dominant kernel, HIP events on the library's own stream (local, no collective), right behind the timed steps: the
        # device is at the clocks it held there
        k_ms = solver.time_kernel(0, warmup=5, iters=max(5, args.steps))
        # ---- one untimed cross-check of the K the timed launches assemble: its product with a random vector against the
        # product of the K a second, independent kernel assembles from the same state (staged visits / the generic
        # row-owner kernel), K . translation = 0, and symmetry by <a, K b> = <b, K a>
        verified = None
        if world == 1:
            try:
                rng = np.random.default_rng(66)
                va, vb = rng.normal(size=3 * N), rng.normal(size=3 * N)
                ya, yb = solver.spmv(va), solver.spmv(vb)
                tr = np.zeros(3 * N); tr[1::3] = 1.0
                ok = bool(np.abs(solver.spmv(tr)).max() < 1e-10 * np.abs(ya).max() and abs(vb @ ya - va @ yb) < 1e-10 * abs(vb @ ya))
                other = feahip.ASM_ROWOWNER if (args.quadratic or args.hex) else feahip.ASM_STAGED
                if in_use != other:
                    solver.set_assembly(other)
                    solver.create_stiffness_and_residual()
                    ok = ok and bool(np.abs(solver.spmv(va) - ya).max() < 1e-11 * np.abs(ya).max())
                    solver.set_assembly(getattr(feahip, "ASM_" + args.assembly.upper()))
                    solver.create_stiffness_and_residual()
                    solver.sync()
                verified = ok
            except Exception as e:                      # noqa: BLE001
                verified = f"check failed to run: {e}"
        copy_gbps = copy3 = None
        try:
            copy3 = solver.copy_bandwidth_detail(1 << 30)
            copy_gbps = max(copy3)
        except Exception as e:                          # noqa: BLE001
            print(f"copy bandwidth not measured: {e}", file=sys.stderr)
        B = algorithmic_bytes(sz["npe"], E_total, N, nnz) * share
        achieved = B / (k_ms * 1e-3) / 1e9
        spmv_ms = solver.time_kernel(3, warmup=2, iters=10)
        measured = {
            "assembly_kernel_ms": k_ms,
            "residual_only_ms": solver.time_kernel(2, warmup=2, iters=10),
            "spmv_ms": spmv_ms,
            "spmv_GBps": spmv_bytes(nnz, N) * share / (spmv_ms * 1e-3) / 1e9,
            "verified": verified,
            "copy_bandwidth_GBps": copy_gbps,
            "copy_bandwidth_GBps_by_method": (dict(zip(("one_16B_load_per_lane", "four_16B_loads_in_flight", "hipMemcpyDtoDAsync", "four_16B_nontemporal"), copy3))
                                              if copy3 else None),
            "assembly_frac_of_copy_bandwidth": achieved / copy_gbps if copy_gbps else None,
        }
    renumbered = True if world > 1 else not np.array_equal(solver.node_numbering(), np.arange(N))
    extras = {
        "setup_s": t_setup,
        "aux_map_bytes_per_element": sz["aux_bytes"] / E_total,
        "rccl_sharded_solve": comm_ok if world > 1 and args.full else None,
        "device_bytes_this_rank": int(dev_bytes),
        "node_numbering": ("caller: " + ("deck order (TetGen), copy by copy" if args.mesh == "tetgen" else "lexicographic (x fastest, z, y slowest)" if brick is None else "bricks of %dx%dx%d nodes" % brick) +
                           "; library: " + (("renumbered by recursive coordinate bisection (csrc/renumber.cpp)" if args.mesh == "tetgen" else
                                             "renumbered to compact cells (csrc/renumber.cpp)") if renumbered else "the caller's ids kept")),
        "gather_maps": solver.assembly_stats(),
        "device_addresses_mod_2MiB": {k: v % (1 << 21) for k, v in solver.device_layout().items()},
        "rank0_holds": ({"nodes": solver.N, "owned_nodes": solver.n_own, "elements": solver.E, "rows_sent_per_exchange": solver.rows_sent}
                        if world > 1 else None),
    }
    extras.update(measured)

    # ---- the reference's own element next to the headline: 10-node tetrahedra / 5 Gauss points on a small block
    # (24 x 144 x 24 cubes, 497 664 elements, a few ms), same deformed state, what AUTO runs
    tet10 = None
    if args.full and world == 1 and not args.quadratic and not args.hex and not args.no_tet10:
        try:
            d10 = mesh.bar_deck(n=24, quadratic=True, recipe="clamped", model=model)
            s10 = feahip.FeaSolver(d10, device=local)
            s10.set_nodes(mesh.deformed_state(d10.nodes))
            s10.create_stiffness_and_residual(); s10.sync()
            z10 = s10.sizes()
            for _ in range(50):                     # the clock ramp (~30 ms of load) after the host-side deck build, as for the headline
                s10.create_stiffness_and_residual()
            s10.sync()
            ms10 = s10.time_kernel(0, warmup=10, iters=20)
            B10 = algorithmic_bytes(10, z10["E"], z10["N"], z10["nnzb"] * 9)
            tet10 = {"workload": f"{z10['E']} TET10/5GP {args.model} block (24x144x24 Kuhn cubes), stiffness+residual, caller numbering lexicographic",
                     "assembly_ms": ms10, "elements_per_s": z10["E"] / (ms10 * 1e-3), "algorithmic_GBps": B10 / (ms10 * 1e-3) / 1e9,
                     "hbm_frac": B10 / (ms10 * 1e-3) / 1e9 / HBM_PEAK_GBS, "fp64_vector_frac": 27e3 * z10["E"] / (ms10 * 1e-3) / 78.6e12,
                     "kernel": "k_state10 + k_assemble_gather10" if s10.assembly_in_use() == feahip.ASM_GATHER else str(s10.assembly_in_use()),
                     "residual_only_ms": s10.time_kernel(2, warmup=5, iters=10)}
            s10.close()
        except Exception as e:                      # noqa: BLE001
            tet10 = {"failed": str(e)}
    # ---- the extension element that rides the same templates: 8-node bricks / 8 Gauss points (40 x 240 x 40 bricks,
    # 384 000 elements), measured the same way
    hex8 = None
    if args.full and world == 1 and not args.quadratic and not args.hex and not args.no_tet10:
        try:
            d8 = mesh.bar_deck(n=40, hexa=True, recipe="clamped", model=model)
            s8 = feahip.FeaSolver(d8, device=local)
            s8.set_nodes(mesh.deformed_state(d8.nodes))
            s8.create_stiffness_and_residual(); s8.sync()
            z8 = s8.sizes()
            for _ in range(50):
                s8.create_stiffness_and_residual()
            s8.sync()
            ms8 = s8.time_kernel(0, warmup=10, iters=20)
            B8 = algorithmic_bytes(8, z8["E"], z8["N"], z8["nnzb"] * 9)
            hex8 = {"workload": f"{z8['E']} HEX8/8GP {args.model} block (40x240x40 bricks), stiffness+residual, caller numbering lexicographic",
                    "assembly_ms": ms8, "elements_per_s": z8["E"] / (ms8 * 1e-3), "algorithmic_GBps": B8 / (ms8 * 1e-3) / 1e9,
                    "hbm_frac": B8 / (ms8 * 1e-3) / 1e9 / HBM_PEAK_GBS,
                    "kernel": "k_state10<8> + k_assemble_gather10<8>" if s8.assembly_in_use() == feahip.ASM_GATHER else str(s8.assembly_in_use())}
            s8.close()
        except Exception as e:                      # noqa: BLE001
            hex8 = {"failed": str(e)}
    # ---- off the lattice: (i) the SAME block with every node displaced by a deterministic
    # pseudo-random +-0.2 spacings (0.3 inverts Kuhn tetrahedra) and the caller's ids randomly permuted; (ii) the
    # reference's TetGen deck brick_fine.sexp (22 934 TET10, deck order kept as sexp_loader.c:170-215 does), 48 copies
    # side by side = 1.1 M TET10 / 5 GP.  Which kernel AUTO takes, element evaluations per element, time, roofline fraction.
    off = None
    if args.full and world == 1 and not args.quadratic and not args.hex and not args.no_off_lattice:
        off = {}

        def leg(name, d, what):
            try:
                t0 = time.perf_counter()
                s2 = feahip.FeaSolver(d, device=local)
                s2.set_nodes(mesh.deformed_state(d.nodes))
                s2.create_stiffness_and_residual(); s2.sync()
                bad = s2.update_state()
                t_set = time.perf_counter() - t0
                z2 = s2.sizes()
                for _ in range(30):
                    s2.create_stiffness_and_residual()
                s2.sync()
                ms = s2.time_kernel(0, warmup=5, iters=20)
                B2 = algorithmic_bytes(z2["npe"], z2["E"], z2["N"], z2["nnzb"] * 9)
                iu = s2.assembly_in_use()
                off[name] = {"workload": what, "elements": z2["E"], "nodes": z2["N"], "scalar_nnz": z2["nnzb"] * 9,
                             "assembly_in_use": {feahip.ASM_GATHER: "GATHER", feahip.ASM_STAGED: "STAGED", feahip.ASM_SHARED: "SHARED",
                                                 feahip.ASM_ROWOWNER: "ROWOWNER"}.get(iu, str(iu)),
                             "gather_maps": s2.assembly_stats(), "inverted_gauss_points": bad,
                             "assembly_ms": ms, "elements_per_s": z2["E"] / (ms * 1e-3), "algorithmic_GBps": B2 / (ms * 1e-3) / 1e9,
                             "hbm_frac": B2 / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, "setup_s": t_set,
                             "renumbered_by_library": not np.array_equal(s2.node_numbering(), np.arange(z2["N"]))}
                s2.close()
            except Exception as e:                  # noqa: BLE001
                off[name] = {"failed": str(e)}

        leg("jittered_permuted_block", mesh.jitter_permute(deck, amp=0.2, seed=4),
            f"the timed block ({E_total} TET4), nodes displaced by +-0.2 spacings (seeded), caller ids randomly permuted")
        try:
            import gzip
            import shutil
            import tempfile
            src = os.path.join(ROOT, "tests", "golden", "decks", "brick_fine.sexp.gz")
            with tempfile.TemporaryDirectory() as td:
                pth = os.path.join(td, "brick_fine.sexp")
                with gzip.open(src, "rb") as fi, open(pth, "wb") as fo:
                    shutil.copyfileobj(fi, fo)
                bf = feahip.Deck.load(pth)
            bf.presc_node = (bf.presc_node - 1).astype(np.int32)     # the deck's boundary ids are 1-based
            leg("brick_fine_tiled", mesh.tiled(bf, (4, 4, 3)),
                "the reference's TetGen deck brick_fine.sexp (22 934 TET10 / 5 GP, 34 070 nodes, deck order), 4 x 4 x 3 copies side by side")
            leg("brick_fine_corner_tets_tiled", mesh.tiled(mesh.corner_tets(bf), (8, 8, 7)),
                "the linear tetrahedra on the corner nodes of the same TetGen deck (22 934 TET4 / 1 GP), 8 x 8 x 7 copies side by side: "
                "an unstructured linear-tet mesh for the headline kernel (library numbering: recursive coordinate bisection, csrc/renumber.cpp)")
        except Exception as e:                      # noqa: BLE001
            off["brick_fine_tiled"] = {"failed": str(e)}
    if off is not None:
        extras["off_lattice"] = off
    if tet10 is not None:
        extras["tet10"] = tet10
    if hex8 is not None:
        extras["hex8"] = hex8
    if dumped is not None:
        extras["dumped_outputs"] = dumped
    out = {
        "metric": "element-stiffness assemblies/sec", "value": value, "unit": "elements/s",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": ms_per_step,
        "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "f64",
        "data": "synthetic",
        "config": {"workload": (f"{E_total} TET4/1GP unstructured mesh (corner tetrahedra of the reference's TetGen deck brick_fine.sexp, "
                                f"8 x 8 x 7 copies, deck order), stiffness+residual assembly, deformed state k1=1.1" if args.mesh == "tetgen" else
                                f"{E_total} {'HEX8/8GP' if args.hex else 'TET10/5GP' if args.quadratic else 'TET4/1GP'} {args.model} block "
                                f"({args.n}x{6 * args.n}x{args.n} {'bricks' if args.hex else 'Kuhn cubes'} on the 1x6x1 bar), "
                                f"stiffness+residual assembly, deformed state k1=1.1"),
                   "elements": E_total, "nodes": N, "scalar_nnz": nnz, "clock_ramp_launches_before_warmup": RAMP,
                   "sharding": f"{world} slab(s) across y; a rank holds only its slab (owned nodes, the elements around them, their halo, "
                               f"locally indexed); ghost elements recomputed, no collective in assembly"},
        "extras": extras,
    }
    if args.full:
        traffic, traffic_src = pmc_traffic(args, world, kernel)
        out["roofline"] = {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                           "frac": achieved / HBM_PEAK_GBS, "traffic": traffic, "traffic_source": traffic_src,
                           "kernel": kernel, "algorithmic_bytes_per_launch": B}

    printed = threading.Event()

    def emit():
        if rank == 0 and not printed.is_set():
            printed.set()
            print(json.dumps(out), flush=True)

    # The sharded solve is a bonus leg: a watchdog prints the line and leaves if a collective wedges.
    def bail():
        extras["solve_leg"] = "timed out (a collective or the solve wedged): the assembly figures above stand, the solve leg does not"
        emit()
        print(f"[rank {rank}] solve leg timed out under the watchdog", file=sys.stderr, flush=True)
        # like a failed solve leg below: the assembly figures are complete and in the line, the exit code carries the
        # wedge only on request (every rank has this timer, so they all leave; os._exit: a wedged collective cannot be joined)
        os._exit(3 if os.environ.get("FEAHIP_BENCH_STRICT", "0") == "1" else 0)

    watchdog = threading.Timer(240.0, bail)
    watchdog.daemon = True
    watchdog.start()
    rc_exit = 0
    if args.full and world > 1:
        # RCCL communicator for the sharded linear solve (halo rows + scalar all-reduces).  RCCL refuses ranks that
        # share a device, so the gloo rehearsal (several ranks on one GPU) does not attempt it.
        why = None
        if backend != "nccl":
            why = "not attempted: ranks share a device in the %s rehearsal" % backend
        else:
            try:
                uid = [feahip.comm_unique_id() if rank == 0 else None]
                dist.broadcast_object_list(uid, src=0)
                solver.comm_init(rank, world, uid[0])
                comm_ok = True
            except Exception as e:                  # noqa: BLE001
                why = f"rccl init failed on rank {rank}: {e}"
                print(f"[rank {rank}] {why}", file=sys.stderr)
        flags = [None] * world
        dist.all_gather_object(flags, (comm_ok, why))
        comm_ok = all(f[0] for f in flags)
        extras["rccl_sharded_solve"] = comm_ok
        if not comm_ok:
            extras["solve_leg"] = next(f[1] for f in flags if not f[0])
            if backend == "nccl":
                rc_exit = 4                         # the line is printed, but a dead solve path is a failed run
    if args.full and (world == 1 or comm_ok):
        try:
            extras["pcg_iteration_ms"] = solver.time_kernel(4, warmup=2, iters=10)      # collective when sharded
            if not args.no_newton:
                # one full Newton iteration of the first load increment: bump, assemble, BC, PCG to 1e-14, update
                def newton_iteration():
                    solver.set_nodes(deck.nodes[local_nodes])
                    solver.sync(); barrier()
                    t0 = time.perf_counter()
                    solver.update_nodes_with_bc(1.0)
                    solver.create_stiffness_and_residual()
                    solver.apply_prescribed_bc(0.0)
                    its, res = solver.solve_slae(feahip.PCG_ILU, 1e-14, 20000)
                    en = solver.energy()
                    solver.update_nodes_with_solution()
                    solver.sync(); barrier()
                    return time.perf_counter() - t0, its, res, en

                tn, its, res, en = newton_iteration()
                extras.update({"newton_iters_per_s": 1.0 / tn, "newton_iteration_s": tn, "cg_iterations": its,
                               "cg_relative_residual": res, "energy_u_f": en,
                               "newton_preconditioner": "3x3 block-Jacobi",
                               "newton_iters_per_s_block_jacobi": 1.0 / tn})
                if True:
                    # same iteration with the aggregation-multigrid preconditioner: sharded, every rank runs the
                    # W-cycle on its own diagonal block (block-Jacobi over the ranks, no collective inside it)
                    extras["block_jacobi"] = {"newton_iteration_s": tn, "cg_iterations": its}
                    t_amg = time.perf_counter()
                    solver.set_preconditioner(1)          # builds the aggregates and coarse patterns on the host, once
                    t_amg = time.perf_counter() - t_amg
                    newton_iteration()
                    tn, its, res, en2 = newton_iteration()
                    extras.update({"newton_iters_per_s": 1.0 / tn, "newton_iteration_s": tn, "cg_iterations": its,
                                   "cg_relative_residual": res, "energy_u_f": en2,
                                   "newton_preconditioner": "aggregation multigrid (rigid-body modes), W-cycle",
                                   "newton_iters_per_s_multigrid": 1.0 / tn,
                                   "amg_setup_s": t_amg,
                                   "energy_u_f_block_jacobi": en})
                    solver.set_preconditioner(0)
        except Exception as e:                      # noqa: BLE001
            extras["solve_leg"] = f"failed: {e}"
            rc_exit = 5
    if world == 1:
        watchdog.cancel()                           # (with several ranks it also covers the closing barrier below)
    if args.full and rank == 0 and args.cpu_sample > 0 and world == 1:
        out["cpu_baseline"] = cpu_baseline(args.cpu_sample, args.quadratic, model)
        if cpu_all is not None:
            cpu_all["unit"] = "elements/s"
            cpu_all["note"] = "independent copies of the same sample, one single-threaded oracle per core, timed together"
            out["cpu_baseline"]["all_cores"] = cpu_all
        if cpu_omp is not None:
            out["cpu_baseline"]["all_cores_one_problem_openmp"] = cpu_omp
    emit()
    solver.close()
    if world > 1:
        try:
            dist.barrier()
            dist.destroy_process_group()
        except Exception:                           # noqa: BLE001
            pass
        watchdog.cancel()
    # The assembly line above is complete and measured even when the solve leg behind it failed: the failure is in the
    # line (extras.rccl_sharded_solve / extras.solve_leg) and on stderr; it becomes the exit code only on request, so that
    # a scaling run keeps its assembly numbers.
    if rc_exit:
        print(f"[rank {rank}] solve leg failed (code {rc_exit}): {extras.get('solve_leg')}", file=sys.stderr)
        if os.environ.get("FEAHIP_BENCH_STRICT", "0") == "1":
            sys.exit(rc_exit)


if __name__ == "__main__":
    main()

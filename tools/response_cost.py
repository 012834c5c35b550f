"""Cost of the two kernels of the frequency response on the bench's block: k_response_sweep (what = 23) over 64 synthetic
modes at 1, 64 and 1024 frequencies, and k_response_project (what = 24), next to the whole calls response_sweep and
response_load (without correction) as the caller sees them, copies included.  The basis is random: the kernels do the
same work on any numbers.  Warm-up, then single launches timed one by one with device events: min / median / max.  The
flop rate 4 x 64 x n_freq x 3N / time stands against the FP64 vector peak of the data sheet (78.6 TFLOP/s, half the FP32
vector rate), the bytes of one read of the panels (plus u_s and the two outputs) against the 8 TB/s of the data sheet and
the copy bandwidth measured on the box.  Run every library in a process of its own and alternate them when two are
compared (FEAHIP_LIB picks a variant build).  Run by hand, under a time limit; no test and no benchmark calls it.

    python tools/response_cost.py [--n 66] [--modes 64] [--launches 10] [--out result.json]
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
HBM_PEAK = 8.0e12


def stats(s, what, warmup, launches):
    s.time_kernel(what, warmup, 1)
    t = np.array([s.time_kernel(what, 0, 1) for _ in range(launches)])
    return {"min_ms": float(t.min()), "median_ms": float(np.median(t)), "max_ms": float(t.max())}


def wall_ms(fn):
    t0 = time.perf_counter()
    fn()
    return 1e3 * (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=66, help="block of n x 6n x n cubes (66 = 10M tets, 5.3M dofs)")
    ap.add_argument("--modes", type=int, default=64)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    deck = mesh.bar_deck(n=a.n, recipe="clamped")
    s = feahip.FeaSolver(deck)
    s.set_mass(1.0)
    ndof, m = s.ndof, a.modes
    rng = np.random.default_rng(1)
    block = rng.standard_normal((min(m, 8), ndof)) / np.sqrt(ndof)
    phi = np.concatenate([block * (1.0 + 0.01 * p) for p in range((m + 7) // 8)])[:m]
    lam = np.linspace(1.0, 400.0, m) ** 2
    s.response_set_basis(lam, phi)
    del phi
    F = rng.standard_normal(ndof)
    out = {"elements": int(len(deck.elements)), "dofs": ndof, "modes": m, "launches": a.launches, "library": feahip.LIB_PATH,
           "copy_gbytes_per_s": s.copy_bandwidth()}
    out["response_load_call_ms"] = wall_ms(lambda: s.response_load(F, False))
    out["response_load_call_again_ms"] = wall_ms(lambda: s.response_load(F, False))
    panels = (m + 7) // 8
    for n_freq in (1, 64, 1024):
        omega = np.linspace(0.5, 450.0, n_freq)
        call = wall_ms(lambda: s.response_sweep(omega, 0.1, 1e-5))
        call = min(call, wall_ms(lambda: s.response_sweep(omega, 0.1, 1e-5)))
        k = stats(s, 23, a.warmup, a.launches)
        flop = 4.0 * 8 * panels * n_freq * ndof
        nbytes = (64.0 * panels + 8.0 + 12.0) * ndof + 1024.0 * n_freq
        t = k["median_ms"] * 1e-3
        out[f"sweep_{n_freq}"] = dict(k, call_ms=call, flop=flop, tflop_per_s=flop / t / 1e12, fp64_vector_peak_fraction=flop / t / FP64_VECTOR_PEAK,
                                      bytes=nbytes, gbytes_per_s=nbytes / t / 1e9, hbm_peak_fraction=nbytes / t / HBM_PEAK)
    k = stats(s, 24, a.warmup, a.launches)
    nbytes = (64.0 * panels + 8.0) * ndof
    out["project"] = dict(k, bytes=nbytes, gbytes_per_s=nbytes / (k["median_ms"] * 1e-3) / 1e9,
                          hbm_peak_fraction=nbytes / (k["median_ms"] * 1e-3) / HBM_PEAK)
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    s.close()


if __name__ == "__main__":
    main()

"""fp64 PPA accumulation A/B: the staged branch of
hip_backend.kmn_knm_and_kmny(precision="fp64") (fp32 chunk, .double() copy,
two torch products) against the fused f64 matrix-core kernel
(fused_fp64=True, ppa_fp64.hip), same process, same inputs, alternating.

Usage (GPU box):  python scripts/bench_ppa_fp64.py ROWS M D [--reps R]
                      [--family rbf|m32|m52] [--out FILE]

Per variant: the time of the whole accumulation stage (host clock around a
device synchronise), min / median / max over R alternating repetitions after
one warm-up of each, the peak allocated device memory of one run, and for
the fused variant the share of the 78 TF fp64 matrix peak, counting the
flops the algorithm needs: 2 n m (m + 1) / 2 for the lower triangle of KK
plus 2 n m for Ky (not the padding of partial tiles, nor the generation).
Also the largest relative difference between the two results, which differ
only in the order of fp64 additions.  One JSON line; --out appends it.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

import numpy as np
import torch

from spark_gp_amd import _hip_ext  # noqa: F401  fail loudly if missing
from spark_gp_amd import kernels as ks
from spark_gp_amd.ops import hip_backend
from spark_gp_amd.ops.ppa_plan import ppa_fp64_plan

FP64_MATRIX_PEAK = 78e12

ap = argparse.ArgumentParser()
ap.add_argument("rows", type=int)
ap.add_argument("m", type=int)
ap.add_argument("d", type=int)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--family", default="rbf", choices=["rbf", "m32", "m52"])
ap.add_argument("--out")
args = ap.parse_args()
n, m, d = args.rows, args.m, args.d

if not torch.cuda.is_available():
    sys.exit("bench_ppa_fp64 needs a GPU: a CPU timing says nothing here")
dev = torch.device("cuda:0")
torch.manual_seed(0)
X = torch.rand(n, d, device=dev)
y = torch.sin(X.sum(-1))
A = torch.rand(m, d, device=dev)
cls = {"rbf": ks.ARDRBFKernel, "m32": ks.ARDMatern32Kernel,
       "m52": ks.ARDMatern52Kernel}[args.family]
kernel = 1 * cls(d) + ks.Scalar(1e-3).const * ks.EyeKernel()
kernel.set_hyperparameters(np.concatenate(
    [[1.2], np.random.default_rng(8).uniform(0.5, 2, d) / np.sqrt(d)]))


def run(fused):
    return hip_backend.kmn_knm_and_kmny(kernel, A, X, y, precision="fp64",
                                        fused_fp64=fused)


def timed(fused):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run(fused)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def peak_mb(fused):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    run(fused)
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


# warm-up of both, and the results' agreement at the size that is timed
KK0, Ky0 = run(False)
KK1, Ky1 = run(True)
diff = max(float((KK1 - KK0).abs().max() / KK0.abs().max()),
           float((Ky1 - Ky0).abs().max() / Ky0.abs().max()))
del KK0, Ky0, KK1, Ky1
mem = {"staged": peak_mb(False), "fused": peak_mb(True)}
times = {"staged": [], "fused": []}
for _ in range(args.reps):                      # alternate
    times["staged"].append(timed(False))
    times["fused"].append(timed(True))

plan = ppa_fp64_plan(m, d, torch.float32, 262144)
flops = 2.0 * n * m * (m + 1) / 2 + 2.0 * n * m
res = {"rows": n, "m": m, "d": d, "family": args.family,
       "feeder": plan.feeder, "split_k": plan.split_k, "reps": args.reps,
       "max_rel_diff": diff}
for name, ts in times.items():
    res[name] = {"min_ms": min(ts) * 1e3,
                 "median_ms": statistics.median(ts) * 1e3,
                 "max_ms": max(ts) * 1e3,
                 "spread_ms": (max(ts) - min(ts)) * 1e3,
                 "rows_per_s": n / statistics.median(ts),
                 "peak_alloc_mb": mem[name]}
res["fused"]["share_of_fp64_matrix_peak"] = \
    flops / statistics.median(times["fused"]) / FP64_MATRIX_PEAK
res["speedup_median"] = (statistics.median(times["staged"])
                         / statistics.median(times["fused"]))
line = json.dumps(res)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")

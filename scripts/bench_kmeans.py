"""K-means Lloyd step benchmark: the torch step (the arithmetic of
``KMeansActiveSetProvider``'s loop body: a [2^18, m] score matrix, argmin,
two index_add scatters) against the fused step of kmeans.hip, on one GPU.

Usage (GPU box):  python scripts/bench_kmeans.py [--shapes 1000000x32x100,...]
                      [--warmup W] [--repeats R] [--paths torch,fused]
                      [--out FILE]

Data: N x D uniform fp32 rows generated on the device from a seed; the
centres are M of the rows, as the provider's seeded start.  Times are host
clocks around one step that ends in a device synchronise; the two paths
alternate inside the repeat loop, after WARMUP untimed steps of each, and the
record carries median, min and max over the repeats.  Peak memory is
``torch.cuda.max_memory_allocated`` over a path's timed steps less what was
allocated before them (X and the centres).  ``gflops`` is the two n m d
products of a step (scores and sums, 4 n m d flops) over the median: a
whole-step figure, not a kernel's.  For per-kernel times run the script under
a kernel trace with ``--paths fused``.  One JSON line per (shape, path).
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

import torch

from spark_gp_amd import _hip_ext as ext  # noqa: F401  fail loudly if missing
from spark_gp_amd.ops import hip_backend, torch_backend

SHAPES = "1000000x32x100,1000000x32x1000,11769x784x1000"


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=SHAPES, help="NxDxM, comma-separated")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--paths", default="torch,fused")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_kmeans needs a GPU"
    dev = torch.device("cuda:0")
    out = open(args.out, "w") if args.out else None
    paths = [p for p in args.paths.split(",") if p]

    for shape in args.shapes.split(","):
        n, d, m = (int(v) for v in shape.split("x"))
        g = torch.Generator(device=dev).manual_seed(13)
        X = torch.rand(n, d, generator=g, device=dev)
        centers = X[torch.randperm(n, generator=g, device=dev)[:m]].clone()
        assert hip_backend.supports_kmeans(X, centers)
        work = {}
        steps = {"torch": lambda: torch_backend.kmeans_step(X, centers),
                 "fused": lambda: hip_backend.kmeans_step(X, centers, work)}
        secs = {p: [] for p in paths}
        peak = {}
        last = {}
        for p in paths:
            for _ in range(args.warmup):
                timed(steps[p])
            base = torch.cuda.memory_allocated(dev)
            if p == "fused":        # the buffers of the loop belong to the step
                base -= sum(t.numel() * t.element_size()
                            for t in work.values() if torch.is_tensor(t))
            torch.cuda.reset_peak_memory_stats(dev)
            _, last[p] = timed(steps[p])
            peak[p] = torch.cuda.max_memory_allocated(dev) - base
        for _ in range(args.repeats):
            for p in paths:
                secs[p].append(timed(steps[p])[0])
        agree = None
        if len(last) == 2:
            st, ct, at = last["torch"]
            sf, cf, af = last["fused"]
            agree = {"assign_equal_fraction":
                     float((at == af.long()).double().mean()),
                     "counts_max_abs_diff": float((ct - cf).abs().max()),
                     "sums_max_abs_diff": float((st - sf).abs().max())}
        for p in paths:
            med = statistics.median(secs[p])
            rec = {"path": p, "n": n, "d": d, "m": m, "repeats": args.repeats,
                   "median_ms": med * 1e3, "min_ms": min(secs[p]) * 1e3,
                   "max_ms": max(secs[p]) * 1e3,
                   "gflops": 4.0 * n * m * d / med / 1e9,
                   "peak_mb": peak[p] / 2 ** 20}
            if p == "fused" and agree:
                rec.update(agree)
            line = json.dumps(rec)
            print(line, flush=True)
            if out:
                out.write(line + "\n")
                out.flush()
        del X, centers, work, last, steps


if __name__ == "__main__":
    main()

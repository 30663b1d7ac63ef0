"""Objective evaluation in fp64 on experts of up to 128 rows: the batched
torch objective on fp64 device tensors (what ``setDtype(torch.float64)`` runs
by default) against the fused fp64 kernel of expert_nll_f64.hip
(``fused_fp64=True``), with the fp32 fused kernel for context, on one GPU.

Usage (GPU box):  python scripts/bench_nll_f64.py [--shapes 100x32,...]
                      [--experts 20000] [--warmup W] [--repeats R] [--out FILE]

Data: E experts of k x d uniform rows generated on the device from a seed,
y = sin(2 sum x) + 0.1 noise, an ARD-RBF kernel at amplitude 1, noise 0.05,
scales near 1 / sqrt(d).  Paths: ``torch64``, ``f64`` (fp64 rows), ``f64_x32``
(fp32 rows, widened in the kernel) and ``fp32`` are one
``ops.nll_grad_compiled`` call each (launch, reductions, the host read);
``kernel64`` and ``kernel32`` are the bindings alone.  Times are host clocks
around a call that ends in a device synchronise; the paths alternate inside
the repeat loop, after WARMUP untimed calls of each, and a record carries
median, min and max over the repeats.  ``gflops`` counts k^3 flops per expert
over the median: a whole-call figure.  One JSON line per (shape, path).
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

from spark_gp_amd import _hip_ext as ext
from spark_gp_amd import ops
from spark_gp_amd.kernels import (ARDRBFKernel, EyeKernel, Scalar,
                                  compile_kernel)
from spark_gp_amd.ops import hip_backend

SHAPES = "32x8,100x32,100x128,128x32"


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=SHAPES, help="KxD, comma-separated")
    ap.add_argument("--experts", type=int, default=20000)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--paths",
                    default="torch64,f64,f64_x32,kernel64,fp32,kernel32")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_nll_f64 needs a GPU"
    dev = torch.device("cuda:0")
    out = open(args.out, "w") if args.out else None
    paths = [p for p in args.paths.split(",") if p]

    for shape in args.shapes.split(","):
        k, d = (int(v) for v in shape.split("x"))
        E = args.experts
        g = torch.Generator(device=dev).manual_seed(13)
        X = torch.rand(E, k, d, generator=g, device=dev)
        y = (torch.sin(2.0 * X.sum(-1))
             + 0.1 * torch.randn(E, k, generator=g, device=dev))
        X64, y64 = X.double(), y.double()
        cs = compile_kernel(1 * ARDRBFKernel(d)
                            + Scalar(0.05).const * EyeKernel())
        theta = np.concatenate([[1.0], np.random.default_rng(d).uniform(
            0.8, 1.25, d) / np.sqrt(d)])
        if not hip_backend.supports_nll_f64(cs, X64):
            print(json.dumps({"k": k, "d": d, "skipped": "gate refuses"}))
            continue
        s32 = torch.as_tensor(theta[1:], dtype=torch.float32, device=dev)
        s64 = s32.double()
        calls = {
            "torch64": lambda: ops.nll_grad_compiled(cs, theta, X64, y64),
            "f64": lambda: ops.nll_grad_compiled(cs, theta, X64, y64,
                                                 fused_fp64=True),
            "f64_x32": lambda: ops.nll_grad_compiled(cs, theta, X, y,
                                                     fused_fp64=True),
            "kernel64": lambda: ext.fused_expert_nll_f64(X64, y64, s64, 1.0,
                                                         0.05),
            "fp32": lambda: ops.nll_grad_compiled(cs, theta, X, y),
            "kernel32": lambda: ext.fused_expert_nll(X, y, s32, 1.0, 0.05)}
        secs = {p: [] for p in paths}
        last = {}
        for p in paths:
            for _ in range(args.warmup):
                last[p] = timed(calls[p])[1]
        for _ in range(args.repeats):
            for p in paths:
                secs[p].append(timed(calls[p])[0])
        for p in paths:
            med = statistics.median(secs[p])
            rec = {"path": p, "E": E, "k": k, "d": d, "repeats": args.repeats,
                   "median_ms": med * 1e3, "min_ms": min(secs[p]) * 1e3,
                   "max_ms": max(secs[p]) * 1e3,
                   "gflops": float(E) * k ** 3 / med / 1e9}
            if p.startswith("kernel"):
                rec["bad"] = int((last[p][4] != 0).sum())
            elif p != "torch64" and "torch64" in last:
                (n0, g0), (n1, g1) = last["torch64"], last[p]
                rec["nll_rel_diff"] = abs(n1 - n0) / abs(n0)
                rec["grad_max_diff_over_max"] = float(
                    np.abs(g1 - g0).max() / np.abs(g0).max())
            line = json.dumps(rec)
            print(line, flush=True)
            if out:
                out.write(line + "\n")
                out.flush()
        del X, y, X64, y64, last, calls
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

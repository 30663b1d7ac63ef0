"""Objective evaluation on experts of more than 128 rows: the batched torch
path (what ``ops.nll_grad_compiled`` runs for them by default) against the
fused panel kernel of expert_nll_panel.hip (``panel=True``), on one GPU.

Usage (GPU box):  python scripts/bench_nll_panel.py [--shapes 256x32,...]
                      [--rows 1000000] [--warmup W] [--repeats R] [--out FILE]

Data: E = rows // k experts of k x d uniform fp32 rows generated on the device
from a seed, y = sin(2 sum x) + 0.1 noise, an ARD-RBF kernel at amplitude 1,
noise 0.05, scales near 1 / sqrt(d).  Paths: ``torch`` and ``panel`` are one
``ops.nll_grad_compiled`` call each (launch, reductions, the host read);
``sb64`` and ``sb128`` are the binding alone at either super-block.  Times
are host clocks around a call that ends in a device synchronise; the paths
alternate inside the repeat loop, after WARMUP untimed calls of each, and a
record carries median, min and max over the repeats.  ``gflops`` counts the
k^3 flops of an expert (Cholesky, inverse and K^-1 at k^3 / 3 each) over the
median: a whole-call figure, not a kernel's.  One JSON line per (shape, path).
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

SHAPES = "256x32,512x32,1000x32"


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=SHAPES, help="KxD, comma-separated")
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--paths", default="torch,panel,sb64,sb128")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_nll_panel needs a GPU"
    dev = torch.device("cuda:0")
    out = open(args.out, "w") if args.out else None
    paths = [p for p in args.paths.split(",") if p]

    for shape in args.shapes.split(","):
        k, d = (int(v) for v in shape.split("x"))
        E = max(1, args.rows // k)
        g = torch.Generator(device=dev).manual_seed(13)
        X = torch.rand(E, k, d, generator=g, device=dev)
        y = (torch.sin(2.0 * X.sum(-1))
             + 0.1 * torch.randn(E, k, generator=g, device=dev))
        cs = compile_kernel(1 * ARDRBFKernel(d)
                            + Scalar(0.05).const * EyeKernel())
        theta = np.concatenate([[1.0], np.random.default_rng(d).uniform(
            0.8, 1.25, d) / np.sqrt(d)])
        assert hip_backend.supports_nll_panel(cs, X)
        scale = torch.as_tensor(theta[1:], dtype=torch.float32, device=dev)
        calls = {
            "torch": lambda: ops.nll_grad_compiled(cs, theta, X, y),
            "panel": lambda: ops.nll_grad_compiled(cs, theta, X, y,
                                                   panel=True),
            "sb64": lambda: ext.fused_expert_nll_panel(
                X, y, scale, 1.0, 0.05, sb=64),
            "sb128": lambda: ext.fused_expert_nll_panel(
                X, y, scale, 1.0, 0.05, sb=128)}
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
            if p in ("sb64", "sb128"):
                # a launch takes min(E, resident, scratch bound) workgroups;
                # the bound alone is reported, the launch never exceeds it
                sb = int(p[2:])
                rec["slab_bytes"] = ext.fused_expert_nll_panel_scratch_bytes(
                    1, k, sb)
                rec["bad"] = int((last[p][4] != 0).sum())
            if p == "panel" and "torch" in last:
                (n0, g0), (n1, g1) = last["torch"], last["panel"]
                rec["nll_rel_diff"] = abs(n1 - n0) / abs(n0)
                rec["grad_max_diff_over_max"] = float(
                    np.abs(g1 - g0).max() / np.abs(g0).max())
            line = json.dumps(rec)
            print(line, flush=True)
            if out:
                out.write(line + "\n")
                out.flush()
        del X, y, last, calls


if __name__ == "__main__":
    main()

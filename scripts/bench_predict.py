"""Prediction microbenchmark: the staged path against the fused kernel.

Usage (GPU box):  python scripts/bench_predict.py [--shapes T,M,D ...]
                      [--rounds R] [--budget-gb G] [--out FILE]

For every shape, family (RBF, Matern 5/2) and mode (mean only, mean and
variance) it times, alternating and after a warm-up of each,

  staged  the default ``predict`` computation (cross_kernel_tile, fp64 GEMV,
          fp64 GEMM, rowwise product), over row chunks sized so that one
          chunk's [rows, m] intermediates (about 32 B per cross value) stay
          under --budget-gb;
  fused   ``hip_backend.predict`` (predict.hip), one launch for all rows;

and reports per path the best and worst wall time of the rounds (host clock
around a device synchronise), the peak device memory above the inputs, the
row-tile height the gate chose, and the largest difference between the two
results.  One JSON line per (shape, family, mode).
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

import numpy as np
import torch

from spark_gp_amd import _hip_ext as ext  # fail loudly if missing
from spark_gp_amd.kernels import (ARDRBFKernel, EyeKernel, Matern52Kernel,
                                  Scalar)
from spark_gp_amd.models.predictor import GaussianProjectedProcessRawPredictor
from spark_gp_amd.ops import hip_backend

DEFAULT_SHAPES = ["2000000,1000,32", "2000000,100,16", "2000000,256,32"]


def make_kernel(family, d):
    if family == "rbf":
        kernel = 1 * ARDRBFKernel(d) + Scalar(1e-3).const * EyeKernel()
        scales = np.random.default_rng(4).uniform(0.5, 2.0, d) / np.sqrt(d)
    else:
        kernel = 1 * Matern52Kernel(1.0) + Scalar(1e-3).const * EyeKernel()
        scales = [np.sqrt(d)]
    kernel.set_hyperparameters(np.concatenate([[1.7], scales]))
    return kernel


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def peak_above(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - before, out


def bench(t, m, d, family, with_var, rounds, budget_gb, dev):
    g = torch.Generator().manual_seed(t + m + d)
    X = torch.rand(t, d, generator=g).to(dev)
    A = torch.rand(m, d, generator=g).to(dev)
    M = torch.randn(m, m, generator=g, dtype=torch.float64)
    M = (0.5 * (M + M.T) / m).to(dev)
    mv = torch.randn(m, generator=g, dtype=torch.float64).to(dev)
    kernel = make_kernel(family, d)
    raw = GaussianProjectedProcessRawPredictor(mv, M, kernel, A)
    chunk = int(min(t, max(1, budget_gb * 1e9 // (32 * m))))

    def staged():
        mean = torch.empty(t, dtype=torch.float64, device=dev)
        var = torch.empty_like(mean) if with_var else None
        for s in range(0, t, chunk):
            mc, vc = raw.predict(X[s:s + chunk], with_var=with_var)
            mean[s:s + chunk] = mc
            if with_var:
                var[s:s + chunk] = vc
            del mc, vc
        return mean, var

    def fused():
        return hip_backend.predict(kernel, X, A, mv, M, with_var)

    if not hip_backend.supports_predict(kernel, X, m):
        raise SystemExit(f"the gate refuses (m, d) = ({m}, {d})")
    peak_s, (mean_s, var_s) = peak_above(staged)      # also the warm-up
    peak_f, (mean_f, var_f) = peak_above(fused)
    diff = {"mean": float((mean_f - mean_s).abs().max())}
    if with_var:
        diff["var"] = float((var_f - var_s).abs().max())
        diff["var_scale"] = float(var_s.abs().max())
    del mean_s, var_s, mean_f, var_f
    ts, tf = [], []
    for _ in range(rounds):                           # alternate
        ts.append(timed(staged)[0])
        tf.append(timed(fused)[0])
    return {
        "t": t, "m": m, "d": d, "family": family, "with_var": with_var,
        "tile_rows": int(ext.ppa_predict_tile_rows(m)),
        "staged_chunk_rows": chunk,
        "staged_ms": [min(ts), max(ts)], "fused_ms": [min(tf), max(tf)],
        "speedup_best": min(ts) / min(tf),
        "staged_peak_bytes": peak_s, "fused_peak_bytes": peak_f,
        "max_abs_diff": diff,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=DEFAULT_SHAPES)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--budget-gb", type=float, default=8.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_predict.py needs a GPU"
    dev = torch.device("cuda:0")
    lines = []
    for shape in args.shapes:
        t, m, d = (int(v) for v in shape.split(","))
        for family in ("rbf", "m52"):
            for with_var in (False, True):
                res = bench(t, m, d, family, with_var, args.rounds,
                            args.budget_gb, dev)
                lines.append(json.dumps(res))
                print(lines[-1], flush=True)
                if args.out:
                    with open(args.out, "w") as f:
                        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

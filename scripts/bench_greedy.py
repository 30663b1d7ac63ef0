"""Greedy active-set selection benchmark: the recomputing provider against
the incremental one (greedy.hip) on one GPU.

Usage (GPU box):  python scripts/bench_greedy.py [--n N] [--d D]
                      [--parent-m 64,128] [--m 64,128,1000] [--out FILE]

Data: N x D uniform fp32 rows generated on the device from a seed,
y = sin(3 sum x / sqrt(D)) + 0.1 noise, 1.7 * ARD RBF + 1e-2 noise.

Times are host clocks around work that ends in a device synchronise.  Every
selection is timed after a warm-up selection of 8 points at the same (N, D).
For the incremental path the largest m is driven round by round, and each
round (host step, both passes, the allreduce-sized copies, the argmax
readback) is timed on its own; "GB/s" of a round is the bytes the two passes
must move, counted from shapes,

    n_pad mc (4 + 8 + 8)  +  n d 4  +  n_pad (4 + 4 + 6 * 8 + 4 * 8 + 4)

(U once and V twice; X; c written and read, y twice, p, q, mu read and
written, delta written), over that round's wall time: a whole-round figure,
host step included, not a kernel's.  One JSON line per measurement.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

import numpy as np
import torch

from spark_gp_amd import GreedilyOptimizingActiveSetProvider, ops
from spark_gp_amd import _hip_ext as ext  # fail loudly if missing
from spark_gp_amd.kernels import ARDRBFKernel, EyeKernel, Scalar
from spark_gp_amd.ops import hip_backend
from spark_gp_amd.parallel.dist import Comm

SEED = 5


def round_bytes(n, d, mc):
    npad = ext.greedy_npad(n)
    return npad * mc * 20 + n * d * 4 + npad * (4 + 4 + 6 * 8 + 4 * 8 + 4)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def rounds_timed(kernel, X, y, m):
    """The incremental provider's loop with a clock on every round; returns
    (active, seconds of the round that appended point mc, for mc >= 1)."""
    comm = Comm()
    active = comm.sample_rows(X, 1, SEED)
    state = ops.greedy_state(kernel, X, y, m - 1)
    assert isinstance(state, hip_backend.GreedyState)
    state.append(active[0], comm)
    secs = []
    while True:
        row = X[state.best()[0]][None]
        active = torch.cat([active, row])
        if active.shape[0] >= m:
            return active, secs
        t, _ = timed(lambda: (state.append(row[0], comm), state.best()))
        secs.append(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--d", type=int, default=32)
    ap.add_argument("--parent-m", default="64,128")
    ap.add_argument("--m", default="64,128,1000")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_greedy needs a GPU"
    dev = torch.device("cuda:0")
    n, d = args.n, args.d
    g = torch.Generator(device=dev).manual_seed(13)
    X = torch.rand(n, d, generator=g, device=dev)
    y = (torch.sin(3.0 * X.sum(-1) / d ** 0.5)
         + 0.1 * torch.randn(n, generator=g, device=dev))
    kernel = 1 * ARDRBFKernel(d) + Scalar(1e-2).const * EyeKernel()
    scales = np.random.default_rng(4).uniform(0.5, 2.0, d) / np.sqrt(d)
    kernel.set_hyperparameters(np.concatenate([[1.7], scales]))
    theta = kernel.get_hyperparameters()
    out = open(args.out, "w") if args.out else None

    def emit(rec):
        line = json.dumps(dict(rec, n=n, d=d))
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    def select(incremental, m):
        prov = GreedilyOptimizingActiveSetProvider(incremental=incremental)
        return timed(lambda: prov(m, X, y, kernel, theta, SEED, Comm()))

    picks = {}
    ms = [int(v) for v in args.m.split(",") if v]
    select(True, 8)
    for m in ms[:-1]:
        t, picks[m] = select(True, m)
        emit({"path": "incremental", "m": m, "seconds": t})
    m = ms[-1]
    t, (picks[m], secs) = timed(lambda: rounds_timed(kernel, X, y, m))
    emit({"path": "incremental", "m": m, "seconds": t,
          "state_gb": ext.greedy_state_bytes(n, m - 1) / 1e9})
    for mc in sorted({v for v in (16, 64, 128, 256, 512, 768, m - 2)
                      if 1 <= v <= len(secs)}):
        s = secs[mc - 1]
        emit({"path": "incremental", "m": m, "round_mc": mc,
              "round_ms": s * 1e3,
              "round_gbps": round_bytes(n, d, mc) / s / 1e9})

    select(False, 8)
    for m in [int(v) for v in args.parent_m.split(",") if v]:
        t, ref = select(False, m)
        same = (int((ref == picks[m]).all(-1).sum()) if m in picks else None)
        emit({"path": "recompute", "m": m, "seconds": t,
              "rows_equal_to_incremental": same})


if __name__ == "__main__":
    main()

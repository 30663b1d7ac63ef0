"""One Laplace evidence evaluation on wide-feature experts (d > k): the
streamed-feature HIP kernels (``fused_wide=True``, laplace_wide.hip) against
the batched torch Laplace these shapes take without the option.  Both start
from the same warm latent (a converged f at the evaluation point), as the
evaluations of a fit after the first do, and run at the same tol.  The two are
timed alternately in one process; each figure is a median over ``--reps``
calls with the min..max range, every call ended by a device synchronise.
"""

import argparse
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from spark_gp_amd import _hip_ext, ops
from spark_gp_amd.kernels import ARDRBFKernel, EyeKernel, RBFKernel, Scalar

SHAPES = [(118, 100, 784), (2000, 100, 784), (2000, 100, 256),
          (2000, 128, 1024)]


def tree(base, d):
    # mean scaled squared distance of U[0, 1) rows about 1
    b = math.sqrt(6.0 / d)
    base_k = (ARDRBFKernel(d, b) if base == "ard"
              else RBFKernel(1.0 / (math.sqrt(2.0) * b)))
    return 1 * base_k + Scalar(1e-2).const * EyeKernel()


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--tol", type=float, default=1e-5)
    p.add_argument("--experts", type=int, default=0,
                   help="override E of every shape (rehearsals)")
    p.add_argument("--skip", type=int, default=0,
                   help="leave out the first SKIP shapes")
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_laplace_wide needs a GPU")
    dev = torch.device("cuda:0")
    for E, k, d in SHAPES[args.skip:]:
        E = args.experts or E
        g = torch.Generator().manual_seed(E + k + d)
        X = torch.rand(E, k, d, generator=g).to(dev)
        y = (X.sum(-1) > d / 2).to(torch.float32)
        occ = _hip_ext.fused_laplace_wide_occupancy(k, d)
        for base in ("ard", "rbf"):
            kernel = tree(base, d)
            theta = kernel.get_hyperparameters()
            warm = torch.zeros(E, k, device=dev)
            ops.laplace_nll_grad(kernel, theta, X, y, warm, args.tol,
                                 fused_wide=True)
            times = {True: [], False: []}
            out = {}
            for rep in range(args.reps + 1):        # rep 0 warms both up
                for wide in (True, False):
                    if wide in out and out[wide] is None:
                        continue
                    f = warm.clone()
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    try:
                        out[wide] = ops.laplace_nll_grad(
                            kernel, theta, X, y, f, args.tol, fused_wide=wide)
                    except torch.OutOfMemoryError:
                        # the torch path's [E, p, k, k] derivative tensor
                        out[wide] = None
                        torch.cuda.empty_cache()
                        continue
                    torch.cuda.synchronize()
                    if rep:
                        times[wide].append(time.perf_counter() - t0)
            rel = (abs(out[True][0] - out[False][0]) / abs(out[False][0])
                   if out[False] else float("nan"))
            line = (f"E={E} k={k} d={d} base={base} tol={args.tol} "
                    f"resident_wgs_per_cu={occ} nll_rel_diff={rel:.1e}")
            for wide, name in ((True, "wide_hip"), (False, "torch")):
                if out[wide] is None:
                    line += f"  {name}: out of memory"
                    continue
                t = [1e3 * v for v in times[wide]]
                line += (f"  {name}: {statistics.median(t):.2f} ms "
                         f"({min(t):.2f}..{max(t):.2f})")
            print(line, flush=True)


if __name__ == "__main__":
    main()

"""One Laplace evidence evaluation under the probit link: the probit
instantiations of the fused HIP kernels (``fused_probit=True``; resident for
d <= k, streamed with ``fused_wide=True`` for d > k) against the batched torch
Laplace that a ProbitLikelihood takes without the option, and against the
logistic link on the same kernels, which shows what the fp64 link evaluation
costs per launch.  All start from the same warm latent (a converged probit f
at the evaluation point; the logistic call from its own) and run at the same
tol.  The three are timed alternately in one process; each figure is a median
over ``--reps`` calls with the min..max range, every call ended by a device
synchronise.
"""

import argparse
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from spark_gp_amd import ops
from spark_gp_amd.kernels import ARDRBFKernel, EyeKernel, RBFKernel, Scalar
from spark_gp_amd.likelihoods import ProbitLikelihood

CASES = [(2000, 100, 32, "rbf"), (2000, 100, 32, "ard"),
         (118, 100, 784, "rbf"), (118, 100, 784, "ard"),
         (2000, 100, 784, "ard")]


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
                   help="override E of every case (rehearsals)")
    p.add_argument("--skip", type=int, default=0,
                   help="leave out the first SKIP cases")
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_laplace_probit needs a GPU")
    dev = torch.device("cuda:0")
    lik = ProbitLikelihood()
    # name -> keywords of ops.laplace_nll_grad (fused_wide is added per shape)
    variants = {"probit_hip": dict(likelihood=lik, fused_probit=True),
                "probit_torch": dict(likelihood=lik),
                "logistic_hip": dict()}
    for E, k, d, base in CASES[args.skip:]:
        E = args.experts or E
        g = torch.Generator().manual_seed(E + k + d)
        X = torch.rand(E, k, d, generator=g).to(dev)
        y = (X.sum(-1) > d / 2).to(torch.float32)
        kernel = tree(base, d)
        theta = kernel.get_hyperparameters()
        wide = dict(fused_wide=True) if d > k else {}
        warm = {}
        for name, kw in variants.items():
            if name == "probit_torch":
                continue
            warm[name] = torch.zeros(E, k, device=dev)
            ops.laplace_nll_grad(kernel, theta, X, y, warm[name], args.tol,
                                 **kw, **wide)
        warm["probit_torch"] = warm["probit_hip"]
        times = {name: [] for name in variants}
        out = {}
        for rep in range(args.reps + 1):        # rep 0 warms all three up
            for name, kw in variants.items():
                if name in out and out[name] is None:
                    continue
                f = warm[name].clone()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                try:
                    out[name] = ops.laplace_nll_grad(
                        kernel, theta, X, y, f, args.tol, **kw, **wide)
                except torch.OutOfMemoryError:
                    # the torch path's [E, p, k, k] derivative tensor
                    out[name] = None
                    torch.cuda.empty_cache()
                    continue
                torch.cuda.synchronize()
                if rep:
                    times[name].append(time.perf_counter() - t0)
        ref = out["probit_torch"]
        rel = (abs(out["probit_hip"][0] - ref[0]) / abs(ref[0])
               if ref else float("nan"))
        line = (f"E={E} k={k} d={d} base={base} tol={args.tol} "
                f"probit_nll_rel_diff={rel:.1e}")
        for name in variants:
            if out[name] is None:
                line += f"  {name}: out of memory"
                continue
            t = [1e3 * v for v in times[name]]
            line += (f"  {name}: {statistics.median(t):.2f} ms "
                     f"({min(t):.2f}..{max(t):.2f})")
        print(line, flush=True)


if __name__ == "__main__":
    main()

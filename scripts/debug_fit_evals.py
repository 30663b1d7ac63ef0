import sys, time, subprocess
sys.path.insert(0, "/root/repo")
import numpy as np, torch
from spark_gp_amd.ops import hip_backend, torch_backend
from spark_gp_amd import GaussianProcessRegression
from spark_gp_amd.kernels import ARDRBFKernel
from spark_gp_amd.data import shard_performance_benchmark_data

orig = hip_backend.nll_grad_compiled
log = []
def wrapped(cs, theta, X, y):
    t0 = time.perf_counter()
    # peek bad count by calling ext directly? just time orig and record theta
    out = orig(cs, theta, X, y)
    torch.cuda.synchronize()
    log.append((time.perf_counter()-t0, float(theta[0]), float(theta[1:].max())))
    return out
hip_backend.nll_grad_compiled = wrapped
# also count fallback entries
orig_tb = torch_backend.nll_grad_compiled
tb_calls = []
def wrapped_tb(cs, theta, X, y):
    t0 = time.perf_counter()
    out = orig_tb(cs, theta, X, y)
    tb_calls.append((time.perf_counter()-t0, tuple(X.shape)))
    return out
torch_backend.nll_grad_compiled = wrapped_tb

X, y = shard_performance_benchmark_data(10_000_000, 32, 0, 1, seed=13)
gp = (GaussianProcessRegression().setKernel(lambda: 1*ARDRBFKernel(32))
      .setDatasetSizeForExpert(100).setActiveSetSize(1000).setSigma2(1e-3)
      .setMaxIter(15).setSeed(13).setPpaPrecision("mixed")
      .setOptimizerRestart(False).setDevice("cuda"))
for rep in range(3):
    log.clear(); tb_calls.clear()
    t0 = time.perf_counter()
    gp = (GaussianProcessRegression().setKernel(lambda: 1*ARDRBFKernel(32))
          .setDatasetSizeForExpert(100).setActiveSetSize(1000).setSigma2(1e-3)
          .setMaxIter(15).setSeed(13).setPpaPrecision("mixed")
          .setOptimizerRestart(False).setDevice("cuda"))
    m = gp.fit(X, y)
    med = sorted(d for d, _, _ in log)[len(log)//2]
    print(f"fit {rep}: {round(time.perf_counter()-t0, 2)} s; evals {len(log)}; "
          f"median eval {med*1e3:.1f} ms; objective_time "
          f"{m._instr.timings.get('objective_time'):.2f}", flush=True)
print("fallbacks last fit:", len(tb_calls))
for i, (dt, amp, bmax) in enumerate(log):
    print(f"  eval {i}: {dt*1e3:7.1f} ms  amp={amp:9.3e} betamax={bmax:9.3e}")
print("fallback calls:", len(tb_calls),
      [(round(d,3), s) for d, s in tb_calls[:5]])

"""The incremental greedy selection state on the kernels of greedy.hip against
the fp64 torch state (``torch_backend.GreedyState`` on CPU), with the oracle's
own selection sequence forced into both.

Tolerance.  The kernels compute in fp64 from a cross-kernel column c rounded
to fp32, so their scores may be no worse than those of the recomputing
provider's GPU path (fp32 ``ops.cross_kernel`` and fp32 scoring GEMMs), whose
error against the same oracle on these inputs, as max |delta - oracle| /
(1 + |oracle|) over rows and checked rounds, was measured on an MI355X:

    case                  recompute path   greedy.hip
    ard-63x3-m10          9.8e+00          2.0e-06
    ard_m52-63x3-m10      2.9e+01          4.8e-06
    ard-1x3-m3            7.4e-02          7.7e-06
    ard-1037x3-m10        5.9e+01          3.9e-06
    ard-63x1-m10          3.4e-02          1.1e-05
    ard-63x32-m10         6.7e-01          3.5e-05
    ard-1037x3-m70        inf              4.0e-06
    ard_m52-1037x32-m70   inf              4.1e-06

(inf: that path's fp32 quadratic forms leave the domain of the score's
logarithms.)  No bound was derived from c's rounding alone: the scores pass
through PD^-1, whose conditioning a worst-case bound overstates by orders of
magnitude.  TOL is therefore the smallest of the recompute path's figures,
3.4e-2, for every case: none is held to less than that path delivers on any
of them.  A wrong column, tail or index moves a score by the order of the
score itself, and the argmax checks and the end-to-end selection below do not
depend on TOL at all.
"""

import numpy as np
import pytest
import torch

from spark_gp_amd import (GaussianProcessRegression,
                          GreedilyOptimizingActiveSetProvider)
from spark_gp_amd.kernels import (ARDMatern52Kernel, ARDRBFKernel, EyeKernel,
                                  Scalar)
from spark_gp_amd.ops import torch_backend
from spark_gp_amd.parallel.dist import Comm

TOL = 3.4e-2
SIGMA2 = 1e-3         # the oracle has no -inf / NaN score on these inputs
EVERY = 4             # rounds between checks (the last is always checked)

# (base, n, d, m): one sweep per axis from (ard, 63, 3, 10).  n: one row, less
# than a wave, and two 512-row blocks with a ragged tail; d: around the
# 16-wide staging pass; m = 70 takes mc across the 8-column tile, the 64
# boundary and several tails of both, on more than one block.
CASES = [("ard", 63, 3, 10), ("ard_m52", 63, 3, 10), ("ard", 1, 3, 3),
         ("ard", 1037, 3, 10), ("ard", 63, 1, 10), ("ard", 63, 32, 10),
         ("ard", 1037, 3, 70), ("ard_m52", 1037, 32, 70)]
IDS = [f"{b}-{n}x{d}-m{m}" for b, n, d, m in CASES]


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def make_kernel(base, d, sigma2=SIGMA2):
    cls = {"ard": ARDRBFKernel, "ard_m52": ARDMatern52Kernel}[base]
    return 1 * cls(d) + Scalar(sigma2).const * EyeKernel()


def make_problem(n, d):
    X = np.random.default_rng(11).random((n, d)).astype(np.float32)
    y = np.sin(X.astype(np.float64).sum(-1) * 3.0).astype(np.float32)
    return torch.tensor(X), torch.tensor(y)


def score_error(got, oracle):
    return float(((got - oracle).abs() / (1.0 + oracle.abs())).max())


def forced_rounds(base, n, d, m, dev):
    """Drive the oracle and the HIP state with the oracle's selection and
    yield (mc, oracle, hip) after every EVERY-th append and the last."""
    from spark_gp_amd.ops import hip_backend
    X, y = make_problem(n, d)
    kernel = make_kernel(base, d)
    oracle = torch_backend.GreedyState(kernel, X.double(), y.double(), m)
    assert hip_backend.supports_greedy(kernel, X.to(dev), m)
    hip = hip_backend.GreedyState(kernel, X.to(dev), y.to(dev), m)
    row = X[0]
    for mc in range(1, m + 1):
        oracle.append(row.double(), Comm())
        hip.append(row.to(dev), Comm())
        if mc % EVERY == 0 or mc == m:
            yield mc, oracle, hip
        row = X[oracle.best()[0]]


@pytest.mark.gpu
@pytest.mark.parametrize("base,n,d,m", CASES, ids=IDS)
def test_scores_and_argmax_vs_fp64_state(base, n, d, m, dev):
    for mc, oracle, hip in forced_rounds(base, n, d, m, dev):
        so, sh = oracle.scores(), hip.scores().cpu()
        assert sh.shape == (n,) and sh.dtype == torch.float64
        finite = torch.isfinite(so)
        assert bool(finite.all()), f"mc={mc}: oracle has non-finite scores"
        assert bool((sh[~finite] == -np.inf).all())
        err = score_error(sh, so)
        print(f"{base} n={n} d={d} mc={mc}: score error {err:.3e}")
        assert err <= TOL, f"mc={mc}: score error {err:.3e} > {TOL:.1e}"
        idx, val = hip.best()
        assert idx == int(sh.argmax()) and val == float(sh[idx])
        top = float(so.max())
        assert float(so[idx]) >= top - TOL * (1.0 + abs(top)), (mc, idx)


@pytest.mark.gpu
def test_two_runs_are_bit_identical(dev):
    runs = [[hip.scores().clone() for _, _, hip in
             forced_rounds("ard", 1037, 3, 70, dev)] for _ in range(2)]
    for s0, s1 in zip(*runs):
        assert torch.equal(s0, s1)


@pytest.mark.gpu
def test_regression_fit_selects_the_cpu_oracles_rows(dev):
    from spark_gp_amd import ops
    from spark_gp_amd.ops import hip_backend
    n, d, m = 2000, 4, 48
    X, y = make_problem(n, d)
    assert isinstance(ops.greedy_state(make_kernel("ard", d), X.to(dev),
                                       y.to(dev), m), hip_backend.GreedyState)
    model = (GaussianProcessRegression()
             .setKernel(lambda: 1 * ARDRBFKernel(d))
             .setDatasetSizeForExpert(100).setActiveSetSize(m)
             .setActiveSetProvider(
                 GreedilyOptimizingActiveSetProvider(incremental=True))
             .setSigma2(SIGMA2).setMaxIter(5).setSeed(5).setDevice("cuda:0")
             .fit(X.numpy(), y.numpy()))
    kernel = model.raw.kernel
    ref = GreedilyOptimizingActiveSetProvider(incremental=True)(
        m, X.double(), y.double(), kernel, kernel.get_hyperparameters(), 5,
        Comm())
    got = model.raw.active_set.cpu().double()
    assert got.shape == (m, d)
    assert torch.equal(got, ref)

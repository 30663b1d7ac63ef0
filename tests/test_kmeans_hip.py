"""The fused Lloyd step of kmeans.hip (``ops.kmeans_step`` on the GPU) against
fp64, and ``KMeansActiveSetProvider(fused=True)`` on top of it.

Assignment slack.  The kernel scores s_j = ||c_j||^2 - 2 x.c_j in fp32 with
u = 2^-24.  With X and C the largest row and centre norms, the d-term norm is
off by at most d u C^2, the d-term dot by at most d u X C (any summation
order), and the combine rounds once, u |s_j| <= u (C^2 + 2 X C).  One score is
therefore within (d + 1) u (C^2 + 2 X C) of its fp64 value to first order;
(d + 3) covers the higher-order terms, and the difference of two scores is
within slack = 2 (d + 3) u (C^2 + 2 X C).  So the fp64 score of the kernel's
choice is at most the fp64 minimum plus slack, and a row whose fp64 runner-up
lies more than 2 slack above its minimum ("decisive") must get the fp64 argmin.

Sums.  One-hot times x is exact, so only the fp32 accumulation of at most
L = min(n, slice rows) terms rounds: |sums - exact| <= L u sum |x| over the
centroid's rows, whatever the order inside an MFMA, plus 1e-12 relative for
the fp64 adds of the slices' partials.
"""

import functools

import numpy as np
import pytest
import torch

from spark_gp_amd import GaussianProcessRegression, KMeansActiveSetProvider
from spark_gp_amd import ops
from spark_gp_amd.kernels import ARDRBFKernel
from spark_gp_amd.parallel.dist import Comm

U = 2.0 ** -24
# (n, d, m), one sweep per axis from (63, 3, 10); n = None: 37 rows past a
# row slice of the accumulate kernel.  n: one row, a ragged row tile on more
# than one block, and past the 65536 rows up to which the assign kernel tiles
# by 64 rows, not 256; d: 1, the staged chunk of 32 and one past it, past one
# dims panel; m: one centroid, across the 16- and 64-column boundaries, past
# one 128-centroid slab.
CASES = [(63, 3, 10), (1, 3, 3), (1037, 3, 70), (63, 1, 10), (1037, 32, 70),
         (300, 33, 17), (1037, 3, 1), (2100, 130, 200), (None, 3, 10),
         (66037, 3, 70), (66037, 70, 10)]
IDS = ["slice+37" if n is None else f"{n}x{d}-m{m}" for n, d, m in CASES]


def make_inputs(n, d, m):
    X = np.random.default_rng(11).random((n, d)).astype(np.float32)
    rng = np.random.default_rng(5)
    C = (X[rng.choice(n, m, replace=False)] if m <= n
         else rng.random((m, d)).astype(np.float32))
    return torch.tensor(X), torch.tensor(C)


def step(X, C):
    dev = torch.device("cuda:0")
    return tuple(t.cpu() for t in ops.kmeans_step(X.to(dev), C.to(dev)))


@functools.lru_cache(maxsize=None)
def case(n, d, m):
    from spark_gp_amd import _hip_ext as ext
    X, C = make_inputs(ext.kmeans_slice_rows() + 37 if n is None else n, d, m)
    return (X, C) + step(X, C)


def check_assign(X, C, assign, rows=None):
    """Check 1 of the module docstring; ``rows`` restricts the decisive part."""
    n, d = X.shape
    Xd, Cd = X.double(), C.double()
    S = (Cd * Cd).sum(-1) - 2.0 * (Xd @ Cd.T)
    cn, xn = float(Cd.norm(dim=1).max()), float(Xd.norm(dim=1).max())
    slack = 2.0 * (d + 3) * U * (cn * cn + 2.0 * xn * cn)
    assert assign.shape == (n,) and assign.dtype == torch.int32
    a = assign.long()
    assert bool(((a >= 0) & (a < C.shape[0])).all())
    excess = float((S.gather(1, a[:, None])[:, 0] - S.min(1).values).max())
    low2 = S.topk(min(2, C.shape[0]), dim=1, largest=False).values
    decisive = (low2[:, -1] - low2[:, 0] > 2.0 * slack) | (C.shape[0] == 1)
    if rows is not None:
        decisive, n = decisive & rows, int(rows.sum())
    frac = float(decisive.sum()) / n
    print(f"n={X.shape[0]} d={d} m={C.shape[0]}: excess {excess:.3e} "
          f"slack {slack:.3e} decisive {frac:.4f}")
    assert excess <= slack
    assert frac >= 0.99
    assert torch.equal(a[decisive], S.argmin(1)[decisive])


@pytest.mark.gpu
@pytest.mark.parametrize("n,d,m", CASES, ids=IDS)
def test_assign_vs_fp64(n, d, m):
    X, C, _, _, assign = case(n, d, m)
    check_assign(X, C, assign)


@pytest.mark.gpu
@pytest.mark.parametrize("n,d,m", CASES, ids=IDS)
def test_sums_and_counts_given_assign(n, d, m):
    from spark_gp_amd import _hip_ext as ext
    X, C, sums, counts, assign = case(n, d, m)
    a, Xd = assign.long(), X.double()
    assert sums.dtype == counts.dtype == torch.float64
    assert torch.equal(counts, torch.bincount(a, minlength=m).double())
    ref = torch.zeros(m, d, dtype=torch.float64).index_add_(0, a, Xd)
    mag = torch.zeros(m, d, dtype=torch.float64).index_add_(0, a, Xd.abs())
    L = min(X.shape[0], ext.kmeans_slice_rows())
    ratio = float(((sums - ref).abs() / (L * U * mag + 1e-12 * mag
                                         + 1e-300)).max())
    print(f"n={X.shape[0]} d={d} m={m}: |sums - ref| / bound = {ratio:.3e}")
    assert ratio <= 1.0


@pytest.mark.gpu
def test_equal_centres_go_to_the_lower_index():
    X, C = make_inputs(1037, 3, 70)
    C[40] = C[7]
    _, _, assign = step(X, C)
    assert not bool((assign == 40).any())
    S = (C.double() ** 2).sum(-1) - 2.0 * (X.double() @ C.double().T)
    check_assign(X, C, assign, rows=S.argmin(1) != 7)


@pytest.mark.gpu
def test_two_runs_are_bit_identical():
    X, C = make_inputs(1037, 32, 70)
    for r0, r1 in zip(step(X, C), step(X, C)):
        assert torch.equal(r0, r1)


@pytest.mark.gpu
def test_provider_and_fit_run_the_hip_step(monkeypatch):
    from spark_gp_amd.ops import hip_backend
    calls, hip_step = [], hip_backend.kmeans_step
    monkeypatch.setattr(hip_backend, "kmeans_step",
                        lambda *a, **k: calls.append(1) or hip_step(*a, **k))
    n, d, m = 2000, 4, 48
    X, _ = make_inputs(n, d, m)
    y = torch.sin(X.double().sum(-1) * 3.0).float()
    Xg = X.to("cuda:0")
    prov = KMeansActiveSetProvider(max_iter=3, fused=True)
    got = prov(m, Xg, None, None, None, 5, Comm())
    assert len(calls) == 3

    centers = Comm().sample_rows(Xg, m, 5)
    for _ in range(3):
        sums, counts, _ = ops.kmeans_step(Xg, centers)
        centers = centers.clone()
        centers[counts > 0] = (sums[counts > 0]
                               / counts[counts > 0].unsqueeze(-1)).float()
    assert torch.equal(got, centers)

    model = (GaussianProcessRegression()
             .setKernel(lambda: 1 * ARDRBFKernel(d))
             .setDatasetSizeForExpert(100).setActiveSetSize(m)
             .setActiveSetProvider(prov).setSigma2(1e-3).setMaxIter(5)
             .setSeed(5).setDevice("cuda:0").fit(X.numpy(), y.numpy()))
    assert torch.equal(model.raw.active_set.cpu(), got.cpu())

"""fused_expert_nll_kernel with the scaled features staged in LDS for the
kernel build: phase B stages X' in the front of the working buffer (in column
slabs when d exceeds the buffer's row stride) and holds its tiles in registers
across the barrier before the epilogue overwrites the staging area.  Parity
with the fp64 oracle at the shapes that take each path of B and of the
gradient contraction H, bitwise repeatability at the shapes where a missing
barrier would show, and the degenerate-expert early return."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ext():
    from spark_gp_amd import _hip_ext
    return _hip_ext


def _experts(E, k, d, seed, dev):
    g = torch.Generator().manual_seed(seed)
    X = torch.rand(E, k, d, generator=g).to(dev)
    y = torch.sin(3.0 * X.sum(-1)).to(dev)
    return X, y


# (k, d, E):
#   (100, 32)  the headline: one B slab of 32 columns
#   (40, 17)   one B slab, zero-filled from column 17 to 32; the second
#              16-column group of H holds a single column
#   (33, 33)   B in two slabs (32 + 1 columns); three column groups in H
#              with the last one partial; partial 32-block
#   (100, 128) B in two slabs (96 + 32), accumulators carried across the
#              slab barrier; 8 column tiles in H
#   (32, 128)  d far above the working buffer's row stride: four B slabs
#   (48, 32)   one B slab, one tile on each of waves 0-5, none on 6-7
#   (7, 3)     no 16-column slab fits: B on the global path
#   (128, 128) largest everything: five tiles per wave on waves 0-3
@pytest.mark.parametrize("k,d,E", [(100, 32, 6), (40, 17, 6), (33, 33, 6),
                                   (100, 128, 6), (32, 128, 6), (48, 32, 6),
                                   (7, 3, 6), (128, 128, 4)])
def test_parity_with_fp64_oracle(dev, ext, k, d, E):
    from spark_gp_amd.kernels import (ARDRBFKernel, EyeKernel, Scalar,
                                      compile_kernel)
    from spark_gp_amd.ops import hip_backend, torch_backend
    X, y = _experts(E, k, d, seed=21, dev=dev)
    cs = compile_kernel(1 * ARDRBFKernel(d) + Scalar(1e-3).const * EyeKernel())
    rng = np.random.default_rng(5)
    # inverse length scales shrink with d past 32, so that the squared
    # distances, and with them the gradient that phase H contracts, stay
    # of the size they have at the headline shape
    beta = rng.uniform(0.5, 2.0, d) * min(1.0, (32.0 / d) ** 0.5)
    theta = np.concatenate([[1.1], beta])
    scale = torch.as_tensor(theta[1:], dtype=torch.float32, device=dev)
    *_, bad = ext.fused_expert_nll(X, y, scale, float(theta[0]), 1e-3)
    assert int(bad.sum()) == 0, "experts fell back: kernel not exercised"
    nll_h, grad_h = hip_backend.nll_grad_compiled(cs, theta, X, y)
    nll_o, grad_o = torch_backend.nll_grad_compiled(
        cs, theta, X.double().cpu(), y.double().cpu())
    assert nll_h == pytest.approx(nll_o, rel=2e-4)
    np.testing.assert_allclose(grad_h, grad_o, rtol=3e-3,
                               atol=2e-3 * np.abs(grad_o).max())


# E: two rounds of three experts on each of the 256 CUs at (100, 32); one
# round at (100, 128), whose B phase crosses a slab barrier
@pytest.mark.parametrize("k,d,E", [(100, 32, 1536), (100, 128, 768)])
def test_staging_is_race_free(dev, ext, k, d, E):
    """A missing barrier between the last fragment read of the staging area
    and the next write into it (the next slab of B, or B's epilogue) shows
    as a bitwise difference between two launches, or between the
    batch and its first 64 experts launched alone."""
    X, y = _experts(E, k, d, seed=22, dev=dev)
    scale = torch.linspace(0.6, 1.8, d, device=dev) * (32.0 / d) ** 0.5
    first = ext.fused_expert_nll(X, y, scale, 1.2, 1e-3)
    again = ext.fused_expert_nll(X, y, scale, 1.2, 1e-3)
    alone = ext.fused_expert_nll(X[:64], y[:64], scale, 1.2, 1e-3)
    assert len(first) == 5
    assert int(first[4].sum()) == 0
    for a, b, c in zip(first, again, alone):
        assert torch.equal(a, b)
        assert torch.equal(a[:64], c)


def test_degenerate_expert_still_falls_back(dev, ext):
    """One expert with a duplicated row among good ones.  The two rows are
    0.25 in every coordinate and the scale is 1, so that every product and
    sum of the kernel build is exact in fp32: K[0, 0] = K[1, 0] = K[1, 1] =
    amp, and with zero noise the second pivot is exactly 0.  The early return
    must flag that expert and zero its outputs whatever phase B staged, and
    the experts around it must come out as they do without it."""
    k, d, E, dup = 100, 32, 6, 3
    X, y = _experts(E, k, d, seed=23, dev=dev)
    scale = torch.ones(d, device=dev)
    good = ext.fused_expert_nll(X, y, scale, 1.0, 0.0)
    assert int(good[4].sum()) == 0
    Xd, yd = X.clone(), y.clone()
    Xd[dup, 0] = 0.25
    Xd[dup, 1] = 0.25
    yd[dup, 1] = yd[dup, 0]
    nll, sw, trg, contr, bad = ext.fused_expert_nll(Xd, yd, scale, 1.0, 0.0)
    assert int(bad[dup]) == 1
    assert int(bad.sum()) == 1
    assert float(nll[dup]) == 0.0 and float(sw[dup]) == 0.0
    assert float(trg[dup]) == 0.0
    assert int(torch.count_nonzero(contr[dup])) == 0
    keep = [i for i in range(E) if i != dup]
    for a, b in zip(good[:4], (nll, sw, trg, contr)):
        assert torch.equal(a[keep], b[keep])

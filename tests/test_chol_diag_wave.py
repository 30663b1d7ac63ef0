"""chol_invert_lower with the sub-block loop of each 32x32 diagonal block run
by wave 0 alone (no workgroup barrier inside it; waves 1-7 apply the
previous panel's update meanwhile; one barrier behind it on every path).

Parity with the fp64 oracle on strongly coupled kernel matrices at the
block and sub-block edges, breakdown at a chosen pivot in exact arithmetic
(a missed update leaves the pivot at 1 and the flag down; a wave that left
the barrier sequence would hang), and bitwise repeatability, where a
missing wave-scope wait between a dependent LDS write and read shows."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

AMP, NOISE = 1.1, 1e-2


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ext():
    from spark_gp_amd import _hip_ext
    return _hip_ext


def _coupled(E, k, d, seed, dev):
    """Experts whose kernel matrix has a median off-diagonal of 0.74-0.85
    of the diagonal (fp64 condition number 2.5e2-4.4e3): the inverse
    length scales are small enough that every point sees every other."""
    g = torch.Generator().manual_seed(seed)
    X = torch.rand(E, k, d, generator=g).to(dev)
    y = torch.sin(3.0 * X.sum(-1)).to(dev)
    rng = np.random.default_rng(seed)
    beta = rng.uniform(0.1, 0.4, d) * (32.0 / d) ** 0.5
    return X, y, beta


# (k, d): a single sub-block, a partial second sub-block, a block one
# column short, one full block; then last blocks of 1 and 8 columns after
# one full block, two full blocks, 1 column after two and after three,
# 4 columns after three (the headline k), and four full blocks
@pytest.mark.parametrize("k,d", [(8, 8), (9, 8), (31, 8), (32, 8),
                                 (33, 32), (40, 32), (64, 32), (65, 32),
                                 (97, 32), (100, 32), (128, 32)])
def test_parity_with_fp64_oracle_coupled(dev, ext, k, d):
    from spark_gp_amd.kernels import (ARDRBFKernel, EyeKernel, Scalar,
                                      compile_kernel)
    from spark_gp_amd.ops import hip_backend, torch_backend
    E = 6
    X, y, beta = _coupled(E, k, d, seed=31, dev=dev)
    cs = compile_kernel(1 * ARDRBFKernel(d) + Scalar(NOISE).const * EyeKernel())
    theta = np.concatenate([[AMP], beta])
    scale = torch.as_tensor(beta, dtype=torch.float32, device=dev)
    *_, bad = ext.fused_expert_nll(X, y, scale, AMP, NOISE)
    assert int(bad.sum()) == 0, "experts fell back: kernel not exercised"
    nll_h, grad_h = hip_backend.nll_grad_compiled(cs, theta, X, y)
    nll_o, grad_o = torch_backend.nll_grad_compiled(
        cs, theta, X.double().cpu(), y.double().cpu())
    gmax = np.abs(grad_o).max()
    print(f"\n(k={k}, d={d}): nll rel err "
          f"{abs(nll_h - nll_o) / abs(nll_o):.3e}, grad max abs err / "
          f"max|grad| {np.abs(grad_h - grad_o).max() / gmax:.3e}")
    assert nll_h == pytest.approx(nll_o, rel=2e-4)
    np.testing.assert_allclose(grad_h, grad_o, rtol=3e-3, atol=2e-3 * gmax)


def test_breakdown_at_chosen_pivot(dev, ext):
    """K is exactly I plus one 2x2 block of ones at rows (r, r+1): points sit
    at 20*a on the first axis, so every squared distance is an integer
    multiple of 400 (exact in fp32) and the base kernel is exactly the
    identity; expert e repeats row r as row r+1.  Every pivot before r+1 is
    exactly 1 and pivot r+1 exactly 0 — if the update that carries the
    coupling is missed, the pivot stays 1 and the flag stays down.  r = 6:
    inside the register 8x8; 7, 63, 70: the intra-block panel and trailing
    update across a sub-block edge; 31, 63: phase1, C2 and the waves 1-7
    update across a block edge; 98: the short last block."""
    k, d = 100, 4
    rs = [6, 7, 31, 45, 63, 70, 98]
    E = len(rs) + 1
    X = torch.zeros(E, k, d)
    X[:, :, 0] = 20.0 * torch.arange(k, dtype=torch.float32)
    g = torch.Generator().manual_seed(33)
    y = torch.randn(E, k, generator=g)
    for e, r in enumerate(rs):
        X[e, r + 1] = X[e, r]
        y[e, r + 1] = y[e, r]
    X, y = X.to(dev), y.to(dev)
    scale = torch.ones(d, device=dev)
    nll, sw, trg, contr, bad = ext.fused_expert_nll(X, y, scale, 1.0, 0.0)
    ctl = E - 1
    assert bad.tolist() == [1] * len(rs) + [0]
    for e in range(len(rs)):
        assert float(nll[e]) == 0.0 and float(sw[e]) == 0.0
        assert float(trg[e]) == 0.0
        assert int(torch.count_nonzero(contr[e])) == 0
    alone = ext.fused_expert_nll(X[ctl:], y[ctl:], scale, 1.0, 0.0)
    assert int(alone[4][0]) == 0
    for a, b in zip((nll, sw, trg, contr), alone[:4]):
        assert torch.equal(a[ctl:], b)


# (100, 32): two rounds of three experts on each of the 256 CUs, the inputs
# of the parity test; (32, 8): one block per expert, one round
@pytest.mark.parametrize("k,d,E", [(100, 32, 1536), (32, 8, 768)])
def test_diag_block_is_race_free(dev, ext, k, d, E):
    """A missing wave-scope wait between a dependent LDS write and read of
    wave 0's diagonal-block section, or a missing block barrier, shows as a
    bitwise difference between two launches, or between the batch and its
    first 64 experts launched alone."""
    X, y, beta = _coupled(E, k, d, seed=32, dev=dev)
    scale = torch.as_tensor(beta, dtype=torch.float32, device=dev)
    first = ext.fused_expert_nll(X, y, scale, AMP, NOISE)
    again = ext.fused_expert_nll(X, y, scale, AMP, NOISE)
    alone = ext.fused_expert_nll(X[:64], y[:64], scale, AMP, NOISE)
    assert len(first) == 5
    assert int(first[4].sum()) == 0
    for a, b, c in zip(first, again, alone):
        assert torch.equal(a, b)
        assert torch.equal(a[:64], c)

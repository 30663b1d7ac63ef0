"""fused_expert_nll_kernel with three experts resident per CU: parity with
the fp64 oracle at the shapes where the X fragment chunks, the 32-blocks and
the 16x16 tiles are partial, determinism under co-residency, and the
residency the runtime reports."""

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


# (k, d, E): partial second / third 16-column feature group with partial
# 32-blocks; the headline geometry; exactly one 16-column group; largest k
@pytest.mark.parametrize("k,d,E", [(40, 17, 6), (33, 33, 6), (100, 32, 8),
                                   (20, 16, 6), (128, 48, 6)])
def test_parity_with_fp64_oracle(dev, ext, k, d, E):
    from spark_gp_amd.kernels import (ARDRBFKernel, EyeKernel, Scalar,
                                      compile_kernel)
    from spark_gp_amd.ops import hip_backend, torch_backend
    X, y = _experts(E, k, d, seed=11, dev=dev)
    cs = compile_kernel(1 * ARDRBFKernel(d) + Scalar(1e-3).const * EyeKernel())
    rng = np.random.default_rng(3)
    theta = np.concatenate([[1.1], rng.uniform(0.5, 2.0, d)])
    scale = torch.as_tensor(theta[1:], dtype=torch.float32, device=dev)
    *_, bad = ext.fused_expert_nll(X, y, scale, float(theta[0]), 1e-3)
    assert int(bad.sum()) == 0, "experts fell back: kernel not exercised"
    nll_h, grad_h = hip_backend.nll_grad_compiled(cs, theta, X, y)
    nll_o, grad_o = torch_backend.nll_grad_compiled(
        cs, theta, X.double().cpu(), y.double().cpu())
    assert nll_h == pytest.approx(nll_o, rel=2e-4)
    np.testing.assert_allclose(grad_h, grad_o, rtol=3e-3,
                               atol=2e-3 * np.abs(grad_o).max())


def test_coresident_experts_are_deterministic(dev, ext):
    """E = 1536 is two rounds of three experts on each of the 256 CUs.  A
    race inside a workgroup, or any dependence on which experts share the CU,
    shows as a bitwise difference between two runs or between the batch and
    its first 64 experts run alone."""
    X, y = _experts(1536, 100, 32, seed=12, dev=dev)
    scale = torch.linspace(0.6, 1.8, 32, device=dev)
    first = ext.fused_expert_nll(X, y, scale, 1.2, 1e-3)
    again = ext.fused_expert_nll(X, y, scale, 1.2, 1e-3)
    alone = ext.fused_expert_nll(X[:64], y[:64], scale, 1.2, 1e-3)
    assert int(first[4].sum()) == 0
    for a, b, c in zip(first, again, alone):
        assert torch.equal(a, b)
        assert torch.equal(a[:64], c)


def test_reported_residency(dev, ext):
    assert ext.fused_expert_nll_occupancy(100, 32) >= 3
    assert ext.fused_expert_nll_occupancy(128, 128) >= 1
    assert ext.fused_expert_nll_supported(128, 128) is True
    assert ext.fused_expert_nll_supported(129, 4) is False

"""Host side of the panel expert kernel option: routing, the setter, the
gate and the binding's argument checks (no GPU)."""

import numpy as np
import pytest
import torch


def test_panel_is_ignored_on_cpu():
    from spark_gp_amd import ops
    from spark_gp_amd.kernels import (ARDRBFKernel, EyeKernel, Scalar,
                                      compile_kernel)
    g = torch.Generator().manual_seed(0)
    X = torch.rand(2, 160, 3, generator=g)
    y = torch.sin(2.0 * X.sum(-1))
    cs = compile_kernel(1 * ARDRBFKernel(3) + Scalar(0.05).const * EyeKernel())
    theta = np.array([1.0, 0.6, 0.5, 0.7])
    nll0, grad0 = ops.nll_grad_compiled(cs, theta, X, y)
    nll1, grad1 = ops.nll_grad_compiled(cs, theta, X, y, panel=True)
    assert nll1 == nll0 and np.array_equal(grad1, grad0)


def test_set_fused_large_experts_round_trip():
    from spark_gp_amd import GaussianProcessRegression
    gp = GaussianProcessRegression()
    assert gp.get_params()["fused_large_experts"] is False
    assert gp.setFusedLargeExperts(True) is gp
    assert gp.get_params()["fused_large_experts"] is True
    gp2 = GaussianProcessRegression(**gp.get_params())
    assert gp2.get_params()["fused_large_experts"] is True


@pytest.fixture(scope="module")
def ext():
    return pytest.importorskip("spark_gp_amd._hip_ext")


@pytest.mark.parametrize("k,d,ok", [(129, 1, True), (1024, 128, True),
                                    (128, 4, False), (1025, 4, False),
                                    (200, 129, False), (200, 0, False)])
def test_panel_gate(ext, k, d, ok):
    assert ext.fused_expert_nll_panel_supported(k, d) is ok
    assert ext.fused_expert_nll_supported(129, 4) is False


@pytest.mark.parametrize("what,name", [
    ("strided", "X must be contiguous"), ("scale", "scale must have 4"),
    ("family", "family must be")])
def test_panel_binding_rejects(ext, what, name):
    X = torch.zeros(2, 160, 4)
    y, scale, family = torch.zeros(2, 160), torch.ones(4), 0
    if what == "strided":
        X = torch.zeros(2, 160, 8)[:, :, ::2]
    elif what == "scale":
        scale = torch.ones(5)
    else:
        family = 3
    with pytest.raises(RuntimeError, match=name):
        ext.fused_expert_nll_panel(X, y, scale, 1.0, 0.05, family=family)

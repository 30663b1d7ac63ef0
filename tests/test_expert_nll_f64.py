"""Host side of the fp64 expert kernel option: routing, the setter and the
gate (no GPU)."""

import numpy as np
import pytest
import torch


def test_fused_fp64_is_ignored_on_cpu():
    from spark_gp_amd import ops
    from spark_gp_amd.kernels import (ARDRBFKernel, EyeKernel, Scalar,
                                      compile_kernel)
    g = torch.Generator().manual_seed(0)
    X = torch.rand(2, 60, 3, generator=g)
    y = torch.sin(2.0 * X.sum(-1))
    cs = compile_kernel(1 * ARDRBFKernel(3) + Scalar(0.05).const * EyeKernel())
    theta = np.array([1.0, 0.6, 0.5, 0.7])
    nll0, grad0 = ops.nll_grad_compiled(cs, theta, X, y)
    nll1, grad1 = ops.nll_grad_compiled(cs, theta, X, y, fused_fp64=True)
    assert nll1 == nll0 and np.array_equal(grad1, grad0)


def test_set_fused_fp64_experts_round_trip():
    from spark_gp_amd import GaussianProcessRegression
    gp = GaussianProcessRegression()
    assert gp.get_params()["fused_fp64_experts"] is False
    assert gp.setFusedFp64Experts(True) is gp
    assert gp.get_params()["fused_fp64_experts"] is True
    gp2 = GaussianProcessRegression(**gp.get_params())
    assert gp2.get_params()["fused_fp64_experts"] is True


@pytest.mark.parametrize("k,d,ok", [(1, 1, True), (100, 128, True),
                                    (128, 32, True), (129, 4, False),
                                    (100, 129, False), (100, 0, False)])
def test_f64_gate(k, d, ok):
    ext = pytest.importorskip("spark_gp_amd._hip_ext")
    assert ext.fused_expert_nll_f64_supported(k, d) is ok

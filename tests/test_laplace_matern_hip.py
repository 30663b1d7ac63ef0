"""The Matern instantiations of the fused Laplace kernels (laplace.hip)
against the fp64 torch oracles on the CPU, and their opt-in.  Tolerances are
test_hip_kernels.py::test_fused_laplace_evidence_vs_torch's, per expert.  X, y
and f are the fp32 values the kernel sees, widened; the oracle's scale is the
fp64 value whose fp32 rounding the kernel gets (6e-8 relative)."""

import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from spark_gp_amd.kernels import (ARDMatern32Kernel, ARDMatern52Kernel,
                                  ARDRBFKernel, EyeKernel, Matern32Kernel,
                                  Matern52Kernel, RBFKernel, Scalar,
                                  compile_kernel)
from spark_gp_amd.kernels.compiled import FAM_M32, FAM_M52, base_scale
from spark_gp_amd.ops import torch_backend as tb

NOISE = float(np.float32(1e-2))
ARD = {FAM_M32: (ARDMatern32Kernel, 3.0), FAM_M52: (ARDMatern52Kernel, 5.0)}
TREES = {"rbf": lambda d: RBFKernel(0.8), "ard": ARDRBFKernel,
         "m32": lambda d: Matern32Kernel(0.8),
         "m52": lambda d: Matern52Kernel(0.8),
         "ard_m32": lambda d: ARDMatern32Kernel(np.full(d, 0.8)),
         "ard_m52": lambda d: ARDMatern52Kernel(np.full(d, 0.8))}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ext():
    from spark_gp_amd import _hip_ext
    return _hip_ext


def make(fam, k, d, E=4):
    """amplitude 1, noise 1e-2, scales about 0.8; expert 1 has row 1 copied
    onto row 0 (t = 0 off the diagonal)"""
    g = torch.Generator().manual_seed(1000 * fam + k + d)
    X = torch.rand(E, k, d, generator=g)
    X[1, 0] = X[1, 1]
    y = (X.sum(-1) > d / 2).to(torch.float32)
    cls, nup = ARD[fam]
    s = 0.8 * (0.75 + 0.5 * torch.rand(d, generator=g)).double().numpy()
    kernel = 1 * cls(s / math.sqrt(nup)) + Scalar(NOISE).const * EyeKernel()
    cs, theta = compile_kernel(kernel), kernel.get_hyperparameters()
    scale = torch.as_tensor(base_scale(cs.base, theta[cs.base_idx], d),
                            dtype=torch.float32)
    return SimpleNamespace(X=X, y=y, scale=scale, kernel=kernel, cs=cs,
                           theta=theta, amp=float(cs.amp(theta)))


def launch(entry, c, f, dev, max_newton, **kw):
    return entry(c.X.to(dev), c.y.to(dev), f, c.scale.to(dev), c.amp, NOISE,
                 1e-6, max_newton, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("k,d", [(33, 7), (100, 32), (128, 1)])
@pytest.mark.parametrize("fam", [FAM_M32, FAM_M52])
def test_evidence_tail_vs_fp64(dev, ext, fam, k, d):
    c = make(fam, k, d)
    f = 0.5 * (2.0 * c.y - 1.0)
    fd = f.to(dev)
    logz, grad, iters, bad = launch(ext.fused_laplace_evidence, c, fd, dev, 0,
                                    family=fam)
    assert not bad.any() and not iters.any()
    assert torch.equal(fd.cpu(), f)
    lz_ref, g_ref = tb.laplace_evidence_experts(
        c.cs, c.theta, c.X.double(), c.y.double(), f.double())
    np.testing.assert_allclose(logz.cpu(), lz_ref, rtol=1e-3)
    for ge, gr in zip(grad.cpu().numpy(), g_ref.numpy()):
        np.testing.assert_allclose(ge, gr, rtol=2e-2,
                                   atol=1e-3 * np.abs(gr).max())


@pytest.mark.gpu
@pytest.mark.parametrize("k,d", [(33, 7), (100, 32)])
@pytest.mark.parametrize("fam", [FAM_M32, FAM_M52])
def test_newton_loop_vs_fp64_mode(dev, ext, fam, k, d):
    c = make(fam, k, d)
    f = torch.zeros_like(c.y, device=dev)
    psi, sll, iters, bad = launch(ext.fused_laplace_newton, c, f, dev, 40,
                                  family=fam)
    f_ref = torch.zeros_like(c.y, dtype=torch.float64)
    tb.laplace_nll_grad(c.kernel, c.theta, c.X.double(), c.y.double(), f_ref,
                        1e-12)
    assert not bad.any() and (iters > 0).all()
    np.testing.assert_allclose(f.cpu().numpy(), f_ref.numpy(), rtol=2e-3,
                               atol=2e-3)


@pytest.mark.gpu
@pytest.mark.parametrize("base", ["m32", "ard_m32", "m52", "ard_m52"])
def test_public_path_opt_in(dev, base, monkeypatch):
    from spark_gp_amd import ops
    from spark_gp_amd.ops import hip_backend
    E, k, d, tol = 4, 100, 8, 1e-5
    X = torch.rand(E, k, d, generator=torch.Generator().manual_seed(11))
    y = (X.sum(-1) > d / 2).to(torch.float32)
    kernel = 1 * TREES[base](d) + Scalar(1e-2).const * EyeKernel()
    theta = kernel.get_hyperparameters()
    calls = []
    inner = hip_backend.laplace_evidence
    monkeypatch.setattr(hip_backend, "laplace_evidence",
                        lambda *a: calls.append(1) or inner(*a))
    f0 = torch.zeros(E, k, device=dev)
    ops.laplace_nll_grad(kernel, theta, X.to(dev), y.to(dev), f0, tol)
    assert not calls
    f = torch.zeros(E, k, device=dev)
    nll, grad = ops.laplace_nll_grad(kernel, theta, X.to(dev), y.to(dev), f,
                                     tol, fused_matern=True)
    assert len(calls) == 1
    f_ref = torch.zeros(E, k, dtype=torch.float64)
    nll_ref, grad_ref = tb.laplace_nll_grad(kernel, theta, X.double(),
                                            y.double(), f_ref, tol)
    assert nll == pytest.approx(nll_ref, rel=1e-3)
    np.testing.assert_allclose(grad, grad_ref, rtol=2e-2,
                               atol=1e-3 * np.abs(grad_ref).max())
    np.testing.assert_allclose(f.cpu().numpy(), f_ref.numpy(), rtol=2e-3,
                               atol=2e-3)


@pytest.mark.gpu
def test_guards(dev, ext):
    c = make(FAM_M52, 33, 7)
    f0 = 0.5 * (2.0 * c.y - 1.0)
    fa, fb = f0.to(dev), f0.to(dev)
    lza, ga, ita, bada = launch(ext.fused_laplace_evidence, c, fa, dev, 40,
                                family=FAM_M52)
    c.X[2, 5, 3] = float("inf")
    lzb, gb, itb, badb = launch(ext.fused_laplace_evidence, c, fb, dev, 40,
                                family=FAM_M52)
    assert bada.tolist() == [0, 0, 0, 0] and badb.tolist() == [0, 0, 2, 0]
    assert torch.equal(fb[2].cpu(), f0[2]) and not gb[2].any()
    ok = [0, 1, 3]
    # no atomics in the Newton loop; the tail's diagKRK sums fp32 terms by
    # LDS atomics in an order that varies run to run (1e-6 relative)
    assert torch.equal(fb[ok], fa[ok]) and torch.equal(itb[ok], ita[ok])
    np.testing.assert_allclose(lzb[ok].cpu(), lza[ok].cpu(), rtol=1e-5)
    np.testing.assert_allclose(gb[ok].cpu(), ga[ok].cpu(), rtol=1e-5,
                               atol=1e-5 * float(ga.abs().max()))
    with pytest.raises(RuntimeError, match="family"):
        launch(ext.fused_laplace_newton, c, fa, dev, 1, family=3)
    c = make(FAM_M32, 33, 7)
    f1, f2 = torch.zeros(4, 33, device=dev), torch.zeros(4, 33, device=dev)
    out1 = launch(ext.fused_laplace_newton, c, f1, dev, 40)
    out2 = launch(ext.fused_laplace_newton, c, f2, dev, 40, family=0)
    assert torch.equal(f1, f2)
    assert all(torch.equal(a, b) for a, b in zip(out1, out2))


@pytest.mark.parametrize("base", list(TREES))
def test_gates_and_setter(base, monkeypatch):
    from spark_gp_amd import GaussianProcessClassifier
    from spark_gp_amd.ops import hip_backend
    monkeypatch.setattr(hip_backend, "ext", SimpleNamespace(
        fused_laplace_newton_supported=lambda k, d: True,
        fused_laplace_evidence_supported=lambda k, d: True))
    cs = compile_kernel(1 * TREES[base](4) + Scalar(1e-2).const * EyeKernel())
    assert cs.base == base
    X = torch.rand(3, 16, 4)
    rbf = base in ("rbf", "ard")
    for gate in (hip_backend.supports_laplace,
                 hip_backend.supports_laplace_evidence):
        assert gate(cs, X, matern=True)
        assert gate(cs, X) == rbf
    gpc = GaussianProcessClassifier()
    assert gpc._fused_matern is False
    assert gpc.setFusedMatern(True) is gpc and gpc._fused_matern is True

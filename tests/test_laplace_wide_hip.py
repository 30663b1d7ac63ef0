"""The streamed-feature fused Laplace kernels (laplace_wide.hip: d > k, up to
1024 dimensions) against the fp64 torch oracles on the CPU, against the
resident kernels where both apply, and their opt-in.  Tolerances are
test_hip_kernels.py::test_fused_laplace_evidence_vs_torch's, per expert.  X, y
and f are the fp32 values the kernel sees, widened; the oracle's scale is the
fp64 value whose fp32 rounding the kernel gets."""

import functools
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from spark_gp_amd.kernels import (ARDRBFKernel, EyeKernel, Matern52Kernel,
                                  Scalar, compile_kernel)
from spark_gp_amd.kernels.compiled import base_scale
from spark_gp_amd.ops import torch_backend as tb

NOISE = float(np.float32(1e-2))
# k below one tile; k no multiple of 16; d one past a slab and one past a
# multiple of 4; the workload's d at the k limit; the d limit
SHAPES = [(16, 17), (33, 40), (100, 131), (128, 784), (20, 1024)]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ext():
    from spark_gp_amd import _hip_ext
    return _hip_ext


@functools.lru_cache(maxsize=None)
def make(k, d, E=4):
    """ARD-RBF, amplitude 1, noise 1e-2, scales about sqrt(6 / d): U[0, 1)
    rows then have a mean scaled squared distance near 1, so Kb is neither 1
    nor 0 at any d.  Expert 1 has row 1 copied onto row 0 (q = 0 off the
    diagonal, where the Gram form cancels completely)."""
    g = torch.Generator().manual_seed(7000 + k + d)
    X = torch.rand(E, k, d, generator=g)
    X[1, 0] = X[1, 1]
    y = (X.sum(-1) > d / 2).to(torch.float32)
    s = math.sqrt(6.0 / d) * (0.75 + 0.5 * torch.rand(d, generator=g))
    kernel = 1 * ARDRBFKernel(s.double().numpy()) \
        + Scalar(NOISE).const * EyeKernel()
    cs, theta = compile_kernel(kernel), kernel.get_hyperparameters()
    scale = torch.as_tensor(base_scale(cs.base, theta[cs.base_idx], d),
                            dtype=torch.float32)
    q = torch.cdist(X[0].double() * scale.double(),
                    X[0].double() * scale.double()) ** 2
    assert 0.5 < float(q.sum() / (k * (k - 1))) < 2.0
    return SimpleNamespace(X=X, y=y, scale=scale, kernel=kernel, cs=cs,
                           theta=theta, amp=float(cs.amp(theta)))


def launch(entry, c, f, dev, max_newton, X=None):
    return entry((c.X if X is None else X).to(dev), c.y.to(dev), f,
                 c.scale.to(dev), c.amp, NOISE, 1e-6, max_newton)


@pytest.mark.gpu
@pytest.mark.parametrize("k,d", SHAPES)
def test_evidence_tail_vs_fp64(dev, ext, k, d):
    c = make(k, d)
    f = 0.5 * (2.0 * c.y - 1.0)
    fd = f.to(dev)
    logz, grad, iters, bad = launch(ext.fused_laplace_evidence_wide, c, fd,
                                    dev, 0)
    assert not bad.any() and not iters.any()
    assert torch.equal(fd.cpu(), f)
    lz_ref, g_ref = tb.laplace_evidence_experts(
        c.cs, c.theta, c.X.double(), c.y.double(), f.double())
    np.testing.assert_allclose(logz.cpu(), lz_ref, rtol=1e-3)
    for ge, gr in zip(grad.cpu().numpy(), g_ref.numpy()):
        np.testing.assert_allclose(ge, gr, rtol=2e-2,
                                   atol=1e-3 * np.abs(gr).max())


@pytest.mark.gpu
@pytest.mark.parametrize("k,d", SHAPES[:3])
def test_newton_loop_vs_fp64(dev, ext, k, d):
    c = make(k, d)
    f = torch.zeros_like(c.y, device=dev)
    psi, sll, iters, bad = launch(ext.fused_laplace_newton_wide, c, f, dev,
                                  40)
    f_ref = torch.zeros_like(c.y, dtype=torch.float64)
    tb.laplace_nll_grad(c.kernel, c.theta, c.X.double(), c.y.double(), f_ref,
                        1e-12)
    assert not bad.any() and (iters > 0).all()
    np.testing.assert_allclose(f.cpu().numpy(), f_ref.numpy(), rtol=2e-3,
                               atol=2e-3)


@pytest.mark.gpu
@pytest.mark.parametrize("k,d", [(33, 7), (100, 32)])
def test_agrees_with_resident_kernel(dev, ext, k, d):
    c = make(k, d)
    f0 = 0.5 * (2.0 * c.y - 1.0)
    lzr, gr, _, badr = launch(ext.fused_laplace_evidence, c, f0.to(dev), dev,
                              0)
    lzw, gw, _, badw = launch(ext.fused_laplace_evidence_wide, c, f0.to(dev),
                              dev, 0)
    assert not badr.any() and not badw.any()
    np.testing.assert_allclose(lzw.cpu(), lzr.cpu(), rtol=1e-4)
    np.testing.assert_allclose(gw.cpu(), gr.cpu(), rtol=1e-4,
                               atol=1e-4 * float(gr.abs().max()))


@pytest.mark.gpu
def test_guards(dev, ext):
    c = make(33, 40)
    f0 = 0.5 * (2.0 * c.y - 1.0)
    fa, fb = f0.to(dev), f0.to(dev)
    lza, ga, ita, bada = launch(ext.fused_laplace_evidence_wide, c, fa, dev,
                                40)
    Xb = c.X.clone()
    Xb[2, 5, 37] = float("inf")
    lzb, gb, itb, badb = launch(ext.fused_laplace_evidence_wide, c, fb, dev,
                                40, X=Xb)
    assert bada.tolist() == [0, 0, 0, 0] and badb.tolist() == [0, 0, 2, 0]
    assert torch.equal(fb[2].cpu(), f0[2])
    assert not gb[2].any() and float(lzb[2]) == 0.0
    ok = [0, 1, 3]
    # no atomics in the Newton loop; the tail's diagKRK sums fp32 terms by
    # LDS atomics in an order that varies run to run (1e-6 relative)
    assert torch.equal(fb[ok], fa[ok]) and torch.equal(itb[ok], ita[ok])
    np.testing.assert_allclose(lzb[ok].cpu(), lza[ok].cpu(), rtol=1e-5)
    np.testing.assert_allclose(gb[ok].cpu(), ga[ok].cpu(), rtol=1e-5,
                               atol=1e-5 * float(ga.abs().max()))
    for k, d in [(129, 8), (8, 1025)]:
        with pytest.raises(RuntimeError, match="1<=k<=128"):
            ext.fused_laplace_newton_wide(
                torch.zeros(1, k, d, device=dev), torch.zeros(1, k, device=dev),
                torch.zeros(1, k, device=dev), torch.ones(d, device=dev),
                1.0, NOISE, 1e-6, 1)


@pytest.mark.gpu
def test_public_path_opt_in(dev, monkeypatch):
    from spark_gp_amd import GaussianProcessClassifier, ops
    from spark_gp_amd.ops import hip_backend
    E, k, d, tol = 4, 50, 200, 1e-5
    X = torch.rand(E, k, d, generator=torch.Generator().manual_seed(11))
    y = (X.sum(-1) > d / 2).to(torch.float32)

    def tree():
        return 1 * ARDRBFKernel(d, math.sqrt(6.0 / d)) \
            + Scalar(1e-2).const * EyeKernel()

    kernel = tree()
    theta = kernel.get_hyperparameters()
    calls = []
    inner = hip_backend.ext.fused_laplace_evidence_wide
    monkeypatch.setattr(hip_backend.ext, "fused_laplace_evidence_wide",
                        lambda *a: calls.append(1) or inner(*a))
    f_ref = torch.zeros(E, k, dtype=torch.float64)
    nll_ref, grad_ref = tb.laplace_nll_grad(kernel, theta, X.double(),
                                            y.double(), f_ref, tol)
    f0 = torch.zeros(E, k, device=dev)
    ops.laplace_nll_grad(kernel, theta, X.to(dev), y.to(dev), f0, tol)
    assert not calls
    f = torch.zeros(E, k, device=dev)
    nll, grad = ops.laplace_nll_grad(kernel, theta, X.to(dev), y.to(dev), f,
                                     tol, fused_wide=True)
    assert len(calls) == 1
    assert nll == pytest.approx(nll_ref, rel=1e-3)
    np.testing.assert_allclose(grad, grad_ref, rtol=2e-2,
                               atol=1e-3 * np.abs(grad_ref).max())
    np.testing.assert_allclose(f.cpu().numpy(), f_ref.numpy(), rtol=2e-3,
                               atol=2e-3)
    # the classifier hands the option down: a two-iteration fit on the same
    # rows goes through the wide entry at every objective evaluation
    gpc = (GaussianProcessClassifier().setKernel(tree)
           .setDatasetSizeForExpert(k).setActiveSetSize(40).setMaxIter(2)
           .setTol(tol).setSeed(3).setDevice("cuda:0")
           .setFusedWideFeatures(True))
    model = gpc.fit(X.reshape(-1, d).numpy(), y.reshape(-1).numpy())
    assert len(calls) > 2
    assert np.isfinite(model.predict_proba(X[0].numpy())).all()


def test_gates_and_setter(monkeypatch):
    from spark_gp_amd import GaussianProcessClassifier, ops
    from spark_gp_amd.ops import hip_backend
    monkeypatch.setattr(hip_backend, "ext", SimpleNamespace(
        fused_laplace_newton_supported=lambda k, d: k <= 128 and d <= k,
        fused_laplace_evidence_supported=lambda k, d: k <= 128 and d <= k,
        fused_laplace_wide_supported=lambda k, d: k <= 128 and d <= 1024))
    ard = 1 * ARDRBFKernel(4) + Scalar(1e-2).const * EyeKernel()
    cs = compile_kernel(ard)
    m52 = compile_kernel(1 * Matern52Kernel(0.8)
                         + Scalar(1e-2).const * EyeKernel())
    X = torch.rand(3, 16, 40)
    assert hip_backend.supports_laplace_wide(cs, X)
    assert not hip_backend.supports_laplace_wide(m52, X)
    assert not hip_backend.supports_laplace_wide(cs, X.double())
    assert not hip_backend.supports_laplace_wide(cs, X.transpose(1, 2))
    assert not hip_backend.supports_laplace_wide(cs, torch.rand(1, 16, 1025))
    assert not hip_backend.supports_laplace_wide(cs, torch.rand(1, 129, 40))

    # routing: the wide branch is taken only when asked for
    seen = []
    monkeypatch.setattr(hip_backend, "laplace_evidence",
                        lambda *a, wide=False: seen.append(wide) or (1.5, 0))
    monkeypatch.setattr(ops, "_backend_for", lambda name, X: hip_backend)
    monkeypatch.setattr(ops.torch_backend, "laplace_nll_grad",
                        lambda *a, **kw: "torch")
    Xg = SimpleNamespace(is_cuda=True, dtype=torch.float32, shape=X.shape,
                         dim=X.dim, is_contiguous=X.is_contiguous)
    args = (ard, ard.get_hyperparameters(), Xg, None, None, 1e-5)
    assert ops.laplace_nll_grad(*args) == "torch" and not seen
    assert ops.laplace_nll_grad(*args, fused_wide=True) == (1.5, 0)
    assert seen == [True]

    gpc = GaussianProcessClassifier()
    assert gpc._fused_wide_features is False
    assert gpc.setFusedWideFeatures(True) is gpc
    assert gpc._fused_wide_features is True
    assert GaussianProcessClassifier._PARAMS["fused_wide_features"] \
        == "_fused_wide_features"
    assert GaussianProcessClassifier(
        fused_wide_features=True)._fused_wide_features is True

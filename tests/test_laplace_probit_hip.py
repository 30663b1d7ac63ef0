"""The probit fused Laplace kernels against the fp64 torch oracles on the CPU,
and their opt-in: tolerances and inputs as in test_laplace_wide_hip.py."""

import functools
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from spark_gp_amd.kernels import (ARDRBFKernel, EyeKernel, Matern52Kernel,
                                  Scalar, compile_kernel)
from spark_gp_amd.kernels.compiled import base_scale
from spark_gp_amd.likelihoods import ProbitLikelihood
from spark_gp_amd.ops import torch_backend as tb

NOISE = float(np.float32(1e-2))
dev = "cuda:0"
LIK = ProbitLikelihood()
# k: under a tile, odd, the workload's, the limit; wide d: slab + 1, not 4n
CASES = [("", 16, 5), ("", 33, 7), ("", 100, 32), ("", 128, 16),
         ("_wide", 16, 17), ("_wide", 33, 40), ("_wide", 100, 131)]


@pytest.fixture(scope="module")
def ext():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from spark_gp_amd import _hip_ext
    return _hip_ext


@functools.lru_cache(maxsize=None)
def make(k, d, E=4):
    """test_laplace_wide_hip.py's case; expert 1 has row 1 copied onto row 0"""
    g = torch.Generator().manual_seed(9000 + k + d)
    X = torch.rand(E, k, d, generator=g)
    X[1, 0] = X[1, 1]
    y = (X.sum(-1) > d / 2).to(torch.float32)
    s = math.sqrt(6.0 / d) * (0.75 + 0.5 * torch.rand(d, generator=g))
    kernel = 1 * ARDRBFKernel(s.double().numpy()) \
        + Scalar(NOISE).const * EyeKernel()
    cs, theta = compile_kernel(kernel), kernel.get_hyperparameters()
    scale = torch.as_tensor(base_scale(cs.base, theta[cs.base_idx], d),
                            dtype=torch.float32)
    return SimpleNamespace(X=X, y=y, scale=scale, kernel=kernel, cs=cs,
                           theta=theta, amp=float(cs.amp(theta)),
                           Xd=X.double(), yd=y.double())


def latent(c, amp):
    f = amp * (2.0 * c.y - 1.0)
    f[:, ::5] *= -1.0 if amp > 0.5 else 1.0
    return f


def launch(entry, c, f, max_newton, **kw):
    return entry(c.X.to(dev), c.y.to(dev), f, c.scale.to(dev), c.amp, NOISE,
                 1e-6, max_newton, **kw)


def assert_grad_close(grad, grad_ref, rtol=2e-2, atol=1e-3):
    np.testing.assert_allclose(grad, grad_ref, rtol=rtol,
                               atol=atol * np.abs(grad_ref).max())


@pytest.mark.gpu
@pytest.mark.parametrize("amp", [0.5, 4.0])
@pytest.mark.parametrize("wide,k,d", CASES)
def test_evidence_tail_vs_fp64(ext, wide, k, d, amp):
    """f = amp t, at amp = 4 with every fifth row flipped to z = -4 (W = 0.95,
    h = 4.2; W = 5e-4 at +4).  Kept at 4: the fp32 oracle on the CPU holds
    these tolerances against the fp64 one at every shape (logZ to 2.5e-5)."""
    c = make(k, d)
    f = latent(c, amp)
    fd = f.to(dev)
    logz, grad, iters, bad = launch(
        getattr(ext, "fused_laplace_evidence" + wide), c, fd, 0, link=1)
    assert not bad.any() and not iters.any() and torch.equal(fd.cpu(), f)
    lz_ref, g_ref = tb.laplace_evidence_experts(c.cs, c.theta, c.Xd, c.yd,
                                                f.double(), likelihood=LIK)
    np.testing.assert_allclose(logz.cpu(), lz_ref, rtol=1e-3)
    for ge, gr in zip(grad.cpu().numpy(), g_ref.numpy()):
        assert_grad_close(ge, gr)


@pytest.mark.gpu
@pytest.mark.parametrize("wide,k,d", [CASES[1], CASES[2], CASES[5]])
def test_newton_loop_vs_fp64(ext, wide, k, d):
    c = make(k, d)
    f = torch.zeros_like(c.y, device=dev)
    _, _, iters, bad = launch(getattr(ext, "fused_laplace_newton" + wide), c,
                              f, 40, link=1)
    f_ref = torch.zeros_like(c.yd)
    tb.laplace_nll_grad(c.kernel, c.theta, c.Xd, c.yd, f_ref, 1e-12,
                        likelihood=LIK)
    assert not bad.any() and (iters > 0).all()
    np.testing.assert_allclose(f.cpu().numpy(), f_ref.numpy(), rtol=2e-3,
                               atol=2e-3)


@pytest.mark.gpu
@pytest.mark.parametrize("wide,k,d", [CASES[1], CASES[5]])
def test_links_differ_and_default_is_logistic(ext, wide, k, d):
    c = make(k, d)
    f0 = latent(c, 0.5)
    entry = getattr(ext, "fused_laplace_evidence" + wide)
    lz, g, _, _ = launch(entry, c, f0.to(dev), 0)
    lz0, g0, _, _ = launch(entry, c, f0.to(dev), 0, link=0)
    lz1, _, _, bad1 = launch(entry, c, f0.to(dev), 0, link=1)
    np.testing.assert_allclose(lz0.cpu(), lz.cpu(), rtol=1e-5)  # atomics
    assert_grad_close(g0.cpu().numpy(), g.cpu().numpy(), 1e-5, 1e-5)
    assert not bad1.any()
    # ten times the tolerance (the fp64 oracles are 0.58 and 1.65 apart)
    assert float((lz1 - lz).abs().max()) > 10 * 1e-3 * float(lz.abs().max())
    with pytest.raises(RuntimeError, match="link must be"):
        launch(entry, c, f0.to(dev), 1, link=2)


@pytest.mark.gpu
def test_routing(ext, monkeypatch):
    from spark_gp_amd import ops
    from spark_gp_amd.ops import hip_backend
    seen, inner, tol = [], hip_backend.laplace_evidence, 1e-5
    monkeypatch.setattr(hip_backend, "laplace_evidence",
                        lambda *a, **kw: seen.append(kw) or inner(*a, **kw))

    def run(kernel, c, **flags):
        del seen[:]
        return ops.laplace_nll_grad(
            kernel, kernel.get_hyperparameters(), c.X.to(dev), c.y.to(dev),
            torch.zeros_like(c.y, device=dev), tol, likelihood=LIK, **flags)

    for (k, d), flags, want in [((100, 32), {}, {"link": "probit"}),
                                ((33, 40), {"fused_wide": True},
                                 {"wide": True, "link": "probit"})]:
        c = make(k, d)
        nll_ref, grad_ref = tb.laplace_nll_grad(
            c.kernel, c.theta, c.Xd, c.yd, torch.zeros_like(c.yd), tol,
            likelihood=LIK)
        run(c.kernel, c, **flags)
        assert not seen
        nll, grad = run(c.kernel, c, fused_probit=True, **flags)
        assert seen == [want]
        assert nll == pytest.approx(nll_ref, rel=1e-3)
        assert_grad_close(grad, grad_ref)
    # Matern x probit is not built: the flags send it to torch
    m52 = 1 * Matern52Kernel(0.8) + Scalar(NOISE).const * EyeKernel()
    nll, _ = run(m52, make(33, 7), fused_probit=True, fused_matern=True)
    assert not seen and np.isfinite(nll)


@pytest.mark.gpu
def test_probit_fit_takes_the_fused_kernels(ext, monkeypatch):
    """test_hip_kernels.py::test_probit_classifier_gpu with the options on"""
    from spark_gp_amd import (GaussianProcessClassifier, RBFKernel,
                              StandardScaler)
    from spark_gp_amd.data import mnist_like_binary
    links, inner = [], ext.fused_laplace_evidence_wide
    monkeypatch.setattr(
        ext, "fused_laplace_evidence_wide",
        lambda *a, **kw: links.append(kw.get("link")) or inner(*a, **kw))
    X, y = mnist_like_binary(2400, seed=13)
    Xs = StandardScaler().fit_transform(X)
    model = (GaussianProcessClassifier()
             .setKernel(lambda: 1 * RBFKernel(10.0))
             .setLink("probit").setFusedProbit(True)
             .setFusedWideFeatures(True).setDatasetSizeForExpert(100)
             .setActiveSetSize(300).setSigma2(1e-3).setTol(1e-3)
             .setMaxIter(30).setSeed(13).setDevice("cuda").fit(Xs, y))
    assert float((model.predict(Xs) == y).mean()) > 0.97
    assert links and set(links) == {1}


def test_evidence_experts_vs_generic_path():
    """against the generic path, which builds the derivative tensor, in fp64"""
    c = make(33, 7)
    f = latent(c, 4.0).double()
    nll, grad = tb.laplace_evidence_compiled(c.cs, c.theta, c.Xd, c.yd, f,
                                             likelihood=LIK)
    nll_ref, grad_ref = tb.laplace_nll_grad(
        c.kernel, c.theta, c.Xd, c.yd, f.clone(), 1e-12, newton=False,
        likelihood=LIK)
    assert nll == pytest.approx(nll_ref, rel=1e-8)
    np.testing.assert_allclose(grad, grad_ref, rtol=1e-8)

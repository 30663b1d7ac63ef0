"""Bounded-memory prediction (``stream=True``) on the CPU: the chunked staged
path against the default path through every public predict method, and
``hip_backend.predict`` / the ``ops.predict_stream`` gate against a fake
extension that computes the fused kernel's contract in fp64 torch.
(The real kernel runs under @gpu in test_predict_hip.py.)"""

import numpy as np
import pytest
import torch

from spark_gp_amd import (GaussianProcessClassifier,
                          GaussianProcessPoissonRegression,
                          GaussianProcessRegression, ops)
from spark_gp_amd.kernels import (ARDMatern32Kernel, ARDMatern52Kernel,
                                  ARDRBFKernel, EyeKernel, Matern32Kernel,
                                  Matern52Kernel, RBFKernel, Scalar,
                                  WhiteNoiseKernel, compile_kernel)
from spark_gp_amd.kernels.compiled import BASES, base_family, base_scale
from spark_gp_amd.models.predictor import GaussianProjectedProcessRawPredictor
from spark_gp_amd.ops import hip_backend

T, CHUNK = 37, 8          # chunk_rows smaller than and not dividing t
RTOL = 1e-12


def _data(kind, n=240, d=2, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.uniform(size=(n, d))
    f = np.sin(3.0 * X.sum(-1))
    if kind == "regression":
        return X, f + 0.05 * rng.standard_normal(n)
    if kind == "classification":
        return X, (f > 0.2).astype(np.float64)
    return X, rng.poisson(np.exp(1.0 + f)).astype(np.float64)


def _fit(est, kernel, kind):
    X, y = _data(kind)
    model = (est.setKernel(kernel).setDatasetSizeForExpert(40)
             .setActiveSetSize(30).setSigma2(1e-2).setMaxIter(8).setSeed(0)
             .setDevice("cpu").fit(X, y))
    Xq = np.random.default_rng(5).uniform(size=(T, X.shape[1]))
    return model, Xq


KERNELS = {
    "canonical": lambda: 1 * ARDRBFKernel(2),
    # two stationary bases: compile_kernel gives None
    "sum-of-rbf": lambda: 1 * RBFKernel(0.3) + 1 * RBFKernel(1.5),
}


@pytest.fixture(scope="module", params=list(KERNELS))
def regression(request):
    return _fit(GaussianProcessRegression(), KERNELS[request.param],
                "regression")


@pytest.fixture(scope="module", params=list(KERNELS))
def classifier(request):
    return _fit(GaussianProcessClassifier(), KERNELS[request.param],
                "classification")


@pytest.fixture(scope="module", params=list(KERNELS))
def poisson(request):
    return _fit(GaussianProcessPoissonRegression(), KERNELS[request.param],
                "poisson")


def test_sum_of_rbf_is_not_canonical():
    assert compile_kernel(KERNELS["sum-of-rbf"]()) is None
    assert compile_kernel(KERNELS["canonical"]()) is not None


def test_regression_stream_equals_default(regression):
    model, Xq = regression
    mean, std = model.predict(Xq, return_std=True)
    mean_s, std_s = model.predict(Xq, return_std=True, stream=True,
                                  chunk_rows=CHUNK)
    assert mean_s.dtype == np.float64 and mean_s.shape == (T,)
    np.testing.assert_allclose(mean_s, mean, rtol=RTOL)
    np.testing.assert_allclose(std_s, std, rtol=RTOL)
    np.testing.assert_allclose(
        model.predict(Xq, stream=True, chunk_rows=CHUNK), mean, rtol=RTOL)
    np.testing.assert_allclose(
        model.transform(Xq, stream=True, chunk_rows=CHUNK), mean, rtol=RTOL)


def test_classifier_stream_equals_default(classifier):
    model, Xq = classifier
    kw = dict(stream=True, chunk_rows=CHUNK)
    np.testing.assert_allclose(model.predict_raw(Xq, **kw),
                               model.predict_raw(Xq), rtol=RTOL)
    np.testing.assert_allclose(model.predict_proba(Xq, **kw),
                               model.predict_proba(Xq), rtol=RTOL)
    np.testing.assert_allclose(model.predict_proba(Xq, averaged=True, **kw),
                               model.predict_proba(Xq, averaged=True),
                               rtol=RTOL)
    np.testing.assert_array_equal(model.predict(Xq, **kw), model.predict(Xq))


def test_poisson_stream_equals_default(poisson):
    model, Xq = poisson
    kw = dict(stream=True, chunk_rows=CHUNK)
    for got, want in zip(model.predict_latent(Xq, **kw),
                         model.predict_latent(Xq)):
        np.testing.assert_allclose(got, want, rtol=RTOL)
    for got, want in zip(model.predict(Xq, return_std=True, **kw),
                         model.predict(Xq, return_std=True)):
        np.testing.assert_allclose(got, want, rtol=RTOL)


def test_raw_predictor_stream_mean_only_and_empty(regression):
    raw = regression[0].raw
    Xq = torch.as_tensor(regression[1])
    mean, var = raw.predict(Xq, with_var=False, stream=True, chunk_rows=CHUNK)
    assert var is None
    np.testing.assert_allclose(mean.numpy(),
                               raw.predict(Xq, with_var=False)[0].numpy(),
                               rtol=RTOL)
    mean, var = raw.predict(Xq[:0], stream=True)
    assert mean.shape == (0,) and var.shape == (0,)
    with pytest.raises(ValueError, match="chunk_rows"):
        raw.predict(Xq, stream=True, chunk_rows=0)


# ---------------------------------------------------------------------------
# host logic of hip_backend.predict against a fake extension
# ---------------------------------------------------------------------------

def _kb(family, q):
    if family == 0:
        return torch.exp(-q)
    s = torch.sqrt(q)
    if family == 1:
        return (1.0 + s) * torch.exp(-s)
    return (1.0 + s + s * s / 3.0) * torch.exp(-s)


class _FakeExt:
    """predict.hip's contract in fp64 torch; records what it was given."""

    def __init__(self, supported=True):
        self.supported = supported
        self.gate_calls, self.calls = [], []

    def ppa_predict_supported(self, m, d):
        self.gate_calls.append((m, d))
        return self.supported

    def ppa_predict(self, X, A, s2, amp, mv, M, kxx, want_var, family=0):
        assert X.dtype == A.dtype == s2.dtype == torch.float32
        assert mv.dtype == M.dtype == torch.float64
        self.calls.append(dict(s2=s2.clone(), amp=amp, kxx=kxx,
                               family=family, want_var=want_var))
        df = X.double()[:, None, :] - A.double()[None, :, :]
        c = amp * _kb(family, (df * df * s2.double()).sum(-1))
        mean = c @ mv
        return mean, (kxx + ((c @ M) * c).sum(-1)) if want_var else None


D = 3
_BASE_KERNEL = {
    "rbf": lambda: RBFKernel(0.8), "ard": lambda: ARDRBFKernel(D),
    "m32": lambda: Matern32Kernel(0.9), "ard_m32": lambda: ARDMatern32Kernel(D),
    "m52": lambda: Matern52Kernel(1.1), "ard_m52": lambda: ARDMatern52Kernel(D),
}


def _predictor(base, m=11, seed=2):
    """A predictor with a canonical tree of the base, trained amplitude 1.7,
    trainable + constant noise, random magic quantities."""
    kernel = (1 * _BASE_KERNEL[base]() + WhiteNoiseKernel(0.1, 0, 1)
              + Scalar(1e-3).const * EyeKernel())
    cs = compile_kernel(kernel)
    assert cs is not None and cs.base == base
    rng = np.random.default_rng(seed)
    theta = kernel.get_hyperparameters()
    theta[cs.amp_idx] = 1.7
    nb = cs.base_idx.stop - cs.base_idx.start
    theta[cs.base_idx] = rng.uniform(0.5, 2.0, nb)
    theta[cs.noise_idx[0]] = 0.12
    kernel.set_hyperparameters(theta)
    g = torch.Generator().manual_seed(seed)
    A = torch.rand(m, D, generator=g)
    M = torch.randn(m, m, generator=g, dtype=torch.float64)
    mv = torch.randn(m, generator=g, dtype=torch.float64)
    X = torch.rand(T, D, generator=g)
    return (GaussianProjectedProcessRawPredictor(mv, M + M.T, kernel, A),
            cs, theta, X)


def test_bases_cover_the_table():
    assert set(_BASE_KERNEL) == set(BASES)


@pytest.mark.parametrize("base", list(_BASE_KERNEL))
@pytest.mark.parametrize("with_var", [True, False])
def test_host_predict_arguments_and_result(base, with_var, monkeypatch):
    raw, cs, theta, X = _predictor(base)
    fake = _FakeExt()
    monkeypatch.setattr(hip_backend, "ext", fake)
    assert hip_backend.supports_predict(raw.kernel, X, raw.active_set.shape[0])
    assert not hip_backend.supports_predict(raw.kernel, X.double(), 11)
    mean, var = hip_backend.predict(raw.kernel, X, raw.active_set,
                                    raw.magic_vector, raw.magic_matrix,
                                    with_var)
    (call,) = fake.calls
    s = base_scale(cs.base, theta[cs.base_idx], D)
    np.testing.assert_allclose(call["s2"].numpy(), s * s, rtol=1e-6)
    assert call["amp"] == 1.7
    assert call["family"] == base_family(base)
    assert call["kxx"] == pytest.approx(1.7 + 0.12 + 1e-3, rel=1e-14)
    assert call["want_var"] is with_var
    # the fake sees fp32 s2 (1e-7 relative); a wrong scale, family or kxx
    # would be off by orders of magnitude more
    want_mean, want_var = raw.predict(X.double(), with_var=with_var)
    np.testing.assert_allclose(mean.numpy(), want_mean.numpy(), rtol=1e-5,
                               atol=1e-5)
    if with_var:
        np.testing.assert_allclose(var.numpy(), want_var.numpy(), rtol=1e-5,
                                   atol=1e-4)
    else:
        assert var is None


@pytest.mark.parametrize("supported", [True, False])
def test_gate_selects_fused_or_chunked(supported, monkeypatch):
    raw, cs, theta, X = _predictor("ard_m52")
    fake = _FakeExt(supported)
    monkeypatch.setattr(hip_backend, "ext", fake)
    real = ops._backend_for

    def backend_for(what, t, required=True):
        return hip_backend if what == "predict_stream" else real(
            what, t, required)

    monkeypatch.setattr(ops, "_backend_for", backend_for)
    mean, var = raw.predict(X, stream=True, chunk_rows=CHUNK)
    assert fake.gate_calls == [(11, D)]
    assert len(fake.calls) == (1 if supported else 0)
    want_mean, want_var = raw.predict(X)
    # X is fp32 here (the gate asks for it), so the default path's cross
    # values carry fp32 rounding (~1e-6, and by a shape-dependent GEMM in the
    # chunked case) that the 11 x 11 O(1) magic matrix sums up
    tol = dict(rtol=1e-5, atol=1e-4)
    np.testing.assert_allclose(mean.numpy(), want_mean.numpy(), **tol)
    np.testing.assert_allclose(var.numpy(), want_var.numpy(), **tol)


def test_non_canonical_tree_never_asks_the_backend(monkeypatch):
    kernel = KERNELS["sum-of-rbf"]() + Scalar(1e-3).const * EyeKernel()
    g = torch.Generator().manual_seed(1)
    A, X = torch.rand(7, 2, generator=g), torch.rand(T, 2, generator=g)
    raw = GaussianProjectedProcessRawPredictor(
        torch.randn(7, generator=g), torch.eye(7), kernel, A)

    def no_backend(*a, **k):
        raise AssertionError("backend consulted for a non-canonical tree")

    monkeypatch.setattr(ops, "_backend_for", no_backend)
    # (ops.cross_kernel consults it too, so call predict_stream's own check)
    assert compile_kernel(kernel) is None
    monkeypatch.setattr(ops, "cross_kernel",
                        lambda k, Xt, Xa: k.cross_kernel(Xt, Xa))
    mean, _ = raw.predict(X, stream=True, chunk_rows=CHUNK)
    monkeypatch.undo()
    np.testing.assert_allclose(mean.numpy(), raw.predict(X)[0].numpy(),
                               rtol=1e-6)

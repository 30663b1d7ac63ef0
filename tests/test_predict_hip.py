"""GPU tests of the fused predict kernel (predict.hip) and of the
``stream=True`` prediction path built on it.

The oracle is the fp64 CPU cross kernel c, then ``c @ mv`` and
``kxx + ((c @ M) * c).sum(-1)``.  The tolerance is the project's cross-kernel
tolerance (test_cross_kernel_tile_vs_torch: rtol 1e-4, atol 1e-5 on c)
propagated exactly through both formulas: with d_rj = 1e-4 |c_rj| + 1e-5,

    |mean_r - oracle| <= sum_j d_rj |mv_j|
    |var_r  - oracle| <= 2 sum_ij d_ri |M_ij| |c_rj| + sum_ij d_ri |M_ij| d_rj

A wrong MFMA fragment or D map gives errors of the order of the value itself.
"""

import numpy as np
import pytest
import torch

from spark_gp_amd.kernels import (ARDMatern32Kernel, ARDMatern52Kernel,
                                  ARDRBFKernel, EyeKernel, Matern32Kernel,
                                  Matern52Kernel, RBFKernel, Scalar)

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


def _bounds(c, mv, M):
    """Per-row (mean, var) error bounds from the oracle's c (docstring)."""
    dl = 1e-4 * c.abs() + 1e-5
    dM = dl @ M.abs()
    return dl @ mv.abs(), 2.0 * (dM * c.abs()).sum(-1) + (dM * dl).sum(-1)


def _oracle(kernel, X, A, mv, M):
    c = kernel.cross_kernel(X.double().cpu(), A.double().cpu())
    mv, M = mv.double().cpu(), M.double().cpu()
    kxx = kernel.self_kernel(X.double().cpu())
    return c, c @ mv, kxx + ((c @ M) * c).sum(-1)


def _check(name, got, want, bound):
    err = (got.cpu() - want).abs()
    worst = float((err / bound).max())
    print(f"{name}: max err {float(err.max()):.3e}, max err/bound {worst:.3e}")
    assert bool((err <= bound).all()), (name, worst)


_BASE = {
    "rbf": lambda d: RBFKernel(1.0), "ard": ARDRBFKernel,
    "m32": lambda d: Matern32Kernel(1.0), "ard_m32": ARDMatern32Kernel,
    "m52": lambda d: Matern52Kernel(1.0), "ard_m52": ARDMatern52Kernel,
}


def _kernel(base, d, seed=4):
    """amp 1.7 and scales in [0.5, 2], as test_cross_kernel_tile_vs_torch."""
    kernel = 1 * _BASE[base](d) + Scalar(1e-3).const * EyeKernel()
    nb = kernel.num_hyperparameters - 1
    theta = np.concatenate(
        [[1.7], np.random.default_rng(seed).uniform(0.5, 2, nb)])
    kernel.set_hyperparameters(theta)
    return kernel


# (t, m, d).  The row tile is 64 up to m = 512, 32 up to 1088, 16 up to 2240.
# t: a partial tile, an exact multiple, exact plus one; m: partial 16-column
# MFMA tiles and partial 4-deep k-steps; d: around the 32-wide d-chunk.
SMALL = [(1, 1, 1), (63, 5, 3), (65, 16, 32), (130, 37, 33), (64, 100, 32),
         (130, 333, 33), (65, 100, 128)]
# every tile height, at both ends of its m range and at the gate's edge
LARGE = [(130, 512, 1), (31, 513, 33), (65, 600, 3), (17, 1088, 3),
         (16, 1089, 3), (33, 1100, 32), (17, 2240, 1)]
CASES = ([(b, s) for b in _BASE for s in SMALL]
         + [(b, s) for b in ("ard", "m52") for s in LARGE])


@pytest.mark.parametrize(
    "base,shape", CASES, ids=[f"{b}-{'x'.join(map(str, s))}" for b, s in CASES])
def test_kernel_vs_fp64_oracle(base, shape, dev, ext):
    from spark_gp_amd.ops import hip_backend
    t, m, d = shape
    assert ext.ppa_predict_supported(m, d)
    g = torch.Generator().manual_seed(1000 * t + m + d)
    X = torch.rand(t, d, generator=g)
    A = torch.rand(m, d, generator=g)
    M = torch.randn(m, m, generator=g, dtype=torch.float64)
    M = 0.5 * (M + M.T)
    mv = torch.randn(m, generator=g, dtype=torch.float64)
    kernel = _kernel(base, d)
    c, mean_o, var_o = _oracle(kernel, X, A, mv, M)
    bm, bv = _bounds(c, mv, M)

    Xg, Ag, mvg, Mg = X.to(dev), A.to(dev), mv.to(dev), M.to(dev)
    assert hip_backend.supports_predict(kernel, Xg, m)
    mean, var = hip_backend.predict(kernel, Xg, Ag, mvg, Mg, True)
    assert mean.dtype == var.dtype == torch.float64
    assert mean.shape == var.shape == (t,)
    _check("mean", mean, mean_o, bm)
    _check("var", var, var_o, bv)
    mean1, none = hip_backend.predict(kernel, Xg, Ag, mvg, Mg, False)
    assert none is None
    _check("mean (mean-only)", mean1, mean_o, bm)


@pytest.fixture
def counted_predict(monkeypatch):
    """Call counter on ext.ppa_predict as hip_backend sees it."""
    from spark_gp_amd.ops import hip_backend
    calls = []
    real = hip_backend.ext.ppa_predict

    def wrapper(*a, **kw):
        calls.append(a[0].shape[0])
        return real(*a, **kw)

    monkeypatch.setattr(hip_backend.ext, "ppa_predict", wrapper)
    return calls


@pytest.mark.parametrize("name,make", [
    ("matern52", lambda: 1 * Matern52Kernel(1.0)),
    ("ard-rbf", lambda: 1 * ARDRBFKernel(4)),
])
def test_fitted_model_stream_vs_oracle(name, make, dev, ext, counted_predict):
    """Realistic conditioning: the model's own magic vector and matrix."""
    from spark_gp_amd import GaussianProcessRegression
    rng = np.random.default_rng(11)
    X = rng.random((2000, 4)).astype(np.float32)
    y = (np.sin(4.0 * X[:, 0]) + X[:, 1] * X[:, 2]
         + 0.05 * rng.standard_normal(2000)).astype(np.float32)
    model = (GaussianProcessRegression().setKernel(make)
             .setDatasetSizeForExpert(100).setActiveSetSize(64)
             .setSigma2(1e-3).setMaxIter(10).setSeed(3)
             .setDevice("cuda:0").fit(X, y))
    raw = model.raw
    Xq = rng.random((500, 4)).astype(np.float32)
    c, mean_o, var_o = _oracle(raw.kernel, torch.as_tensor(Xq),
                               raw.active_set, raw.magic_vector,
                               raw.magic_matrix)
    bm, bv = _bounds(c, raw.magic_vector.cpu(), raw.magic_matrix.cpu())
    var_o = var_o.clamp_min(0.0)     # predict returns sqrt(max(var, 0))

    # the inputs are within reach: the default staged path meets the bound
    mean_d, std_d = model.predict(Xq, return_std=True)
    assert counted_predict == []
    _check("staged mean", torch.as_tensor(mean_d), mean_o, bm)
    _check("staged var", torch.as_tensor(std_d) ** 2, var_o, bv)

    mean_s, std_s = model.predict(Xq, return_std=True, stream=True)
    assert counted_predict == [500]       # the fused kernel ran, once
    _check("fused mean", torch.as_tensor(mean_s), mean_o, bm)
    _check("fused var", torch.as_tensor(std_s) ** 2, var_o, bv)
    print(f"{name}: max |fused - staged| mean "
          f"{np.abs(mean_s - mean_d).max():.3e}, var "
          f"{np.abs(std_s ** 2 - std_d ** 2).max():.3e}")


def _random_predictor(m, d, dev, seed=7):
    from spark_gp_amd.models.predictor import (
        GaussianProjectedProcessRawPredictor)
    g = torch.Generator().manual_seed(seed)
    A = torch.rand(m, d, generator=g).to(dev)
    M = torch.randn(m, m, generator=g, dtype=torch.float64)
    mv = torch.randn(m, generator=g, dtype=torch.float64)
    return GaussianProjectedProcessRawPredictor(
        mv.to(dev), (0.5 * (M + M.T)).to(dev), _kernel("ard", d), A)


def test_no_t_by_m_buffer(dev, ext, counted_predict):
    """Peak memory across the call rises by less than the fp32 cross matrix
    alone; the staged path allocates that and three fp64 ones."""
    from spark_gp_amd import ops
    t, m, d = 200_000, 256, 16
    raw = _random_predictor(m, d, dev)
    X = torch.rand(t, d, generator=torch.Generator().manual_seed(2)).to(dev)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    mean, var = ops.predict_stream(raw.kernel, X, raw.active_set,
                                   raw.magic_vector, raw.magic_matrix,
                                   with_var=True)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print(f"peak rise {rise} B against t*m*4 = {t * m * 4} B")
    assert counted_predict == [t]
    assert rise < t * m * 4
    assert bool(torch.isfinite(mean).all()) and bool(torch.isfinite(var).all())


def test_gate_refusal_takes_the_chunked_path(dev, ext, counted_predict):
    m, d, t = 2300, 4, 50
    assert not ext.ppa_predict_supported(m, d)
    raw = _random_predictor(m, d, dev)
    X = torch.rand(t, d, generator=torch.Generator().manual_seed(3)).to(dev)
    mean, var = raw.predict(X, stream=True, chunk_rows=16)
    assert counted_predict == []
    mean_d, var_d = raw.predict(X)
    # the same fp32 cross values from the elementwise kernel, then fp64 GEMMs
    # of another shape: rounding of 2300^2-term sums of O(1) products
    torch.testing.assert_close(mean, mean_d, rtol=1e-9, atol=1e-9)
    torch.testing.assert_close(var, var_d, rtol=1e-9, atol=1e-7)

"""The panel expert kernel (expert_nll_panel.hip, 128 < k <= 1024) against
the fp64 torch objective on CPU copies of the same inputs."""

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


def _inputs(E, k, d, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    X = torch.rand(E, k, d, generator=g)
    y = torch.sin(2.0 * X.sum(-1)) + 0.1 * torch.randn(E, k, generator=g)
    return X.to(dev), y.to(dev)


def _case(base, d):
    """(compiled kernel, theta) of a base at amplitude 1, noise 0.05 and a
    coordinate scale of 1 / sqrt(d)."""
    from spark_gp_amd import kernels as K
    noise = K.Scalar(0.05).const * K.EyeKernel()
    r = 1.0 / np.sqrt(d)
    if base == "ard":
        rng = np.random.default_rng(d)
        return (K.compile_kernel(1 * K.ARDRBFKernel(d) + noise),
                np.concatenate([[1.0], r * rng.uniform(0.8, 1.25, d)]))
    if base == "rbf":          # s = 1 / (sqrt(2) length)
        return (K.compile_kernel(1 * K.RBFKernel(1.0) + noise),
                np.array([1.0, np.sqrt(d / 2.0)]))
    if base == "m32":          # s = sqrt(3) / length
        return (K.compile_kernel(1 * K.Matern32Kernel(1.0) + noise),
                np.array([1.0, np.sqrt(3.0 * d)]))
    return (K.compile_kernel(1 * K.ARDMatern52Kernel(d) + noise),   # sqrt(5) b
            np.concatenate([[1.0], np.full(d, r / np.sqrt(5.0))]))


CASES = [("ard", 3, 129, 4), ("ard", 2, 160, 5), ("ard", 2, 256, 8),
         ("ard", 2, 257, 3), ("ard", 2, 300, 33), ("ard", 2, 1000, 8),
         ("ard", 2, 1024, 4), ("rbf", 2, 257, 5), ("m32", 2, 257, 5),
         ("ard_m52", 2, 257, 5)]


@pytest.mark.parametrize("base,E,k,d", CASES)
def test_panel_vs_fp64_oracle(dev, ext, base, E, k, d):
    from spark_gp_amd.kernels.compiled import base_family, base_scale
    from spark_gp_amd.ops import hip_backend, torch_backend
    X, y = _inputs(E, k, d, dev)
    cs, theta = _case(base, d)
    assert cs is not None and cs.base == base
    assert hip_backend.supports_nll_panel(cs, X)
    assert not hip_backend.supports_nll(cs, X)
    scale = torch.as_tensor(base_scale(base, theta[cs.base_idx], d),
                            dtype=torch.float32, device=dev)
    *_, bad = ext.fused_expert_nll_panel(X, y, scale, 1.0, 0.05,
                                         family=base_family(base))
    assert int(bad.abs().sum()) == 0, "experts fell back: kernel not exercised"
    nll_h, grad_h = hip_backend.nll_grad_compiled(cs, theta, X, y, panel=True)
    nll_o, grad_o = torch_backend.nll_grad_compiled(
        cs, theta, X.double().cpu(), y.double().cpu())
    print(f"{base} {(E, k, d)}: nll rel {abs(nll_h - nll_o) / abs(nll_o):.2e}"
          f" grad max|d|/max|g| "
          f"{np.abs(grad_h - grad_o).max() / np.abs(grad_o).max():.2e}")
    assert nll_h == pytest.approx(nll_o, rel=2e-4)
    np.testing.assert_allclose(grad_h, grad_o, rtol=3e-3,
                               atol=2e-3 * np.abs(grad_o).max())


def test_panel_slab_reuse_is_bitwise(dev, ext):
    """Two workgroups walking five experts reuse their slabs; every output
    must equal the one-expert-per-workgroup launch bit for bit."""
    X, y = _inputs(5, 160, 4, dev, seed=3)
    scale = torch.full((4,), 0.5, device=dev)
    free = ext.fused_expert_nll_panel(X, y, scale, 1.0, 0.05, max_blocks=0)
    two = ext.fused_expert_nll_panel(X, y, scale, 1.0, 0.05, max_blocks=2)
    assert int(free[4].abs().sum()) == 0
    for a, b in zip(free, two):
        assert torch.equal(a, b)


@pytest.mark.parametrize("row", [10, 196])
def test_panel_flags_breakdown(dev, ext, row):
    """Expert 1 holds two identical rows at noise 0: its matrix is exactly
    singular and the second of the two pivots is exactly 0 in fp32, in the
    first super-block (row 10) or in the last one, after earlier blocks went
    through (row 196).  The pair sits at the origin, so that its q is 0
    without rounding, and the length scale is short: at the 1 / sqrt(d) of
    the other tests a noise-free 200-point matrix is singular in fp32 for
    EVERY expert, and the flag of expert 1 would show nothing.  The
    neighbours must come through untouched.  (The fp64 objective of a
    singular expert is not finite, so no total over all three is compared.)"""
    from spark_gp_amd import kernels as K
    from spark_gp_amd.ops import torch_backend
    E, k, d = 3, 200, 4
    X, y = _inputs(E, k, d, dev, seed=7)
    X[1, row:row + 2] = 0.0
    y[1, row + 1] = y[1, row]
    scale = torch.full((d,), 40.0, device=dev)
    nll, sumW0, trG, contr, bad = ext.fused_expert_nll_panel(
        X, y, scale, 1.0, 0.0)
    assert bad.tolist() == [0, 1, 0]
    assert float(nll[1]) == 0.0 and float(contr[1].abs().sum()) == 0.0
    cs = K.compile_kernel(1 * K.ARDRBFKernel(d))
    theta = np.concatenate([[1.0], np.full(d, 40.0)])
    for e in (0, 2):
        Xe, ye = X[e:e + 1], y[e:e + 1]
        nll_o, grad_o = torch_backend.nll_grad_compiled(
            cs, theta, Xe.double().cpu(), ye.double().cpu())
        assert float(nll[e]) == pytest.approx(nll_o, rel=2e-4)
        assert -0.5 * float(sumW0[e]) == pytest.approx(grad_o[0], rel=3e-3)


def test_panel_fit_end_to_end(dev, ext, monkeypatch):
    from spark_gp_amd import GaussianProcessRegression, rmse
    from spark_gp_amd.kernels import ARDRBFKernel
    calls = [0]
    entry = ext.fused_expert_nll_panel

    def counted(*a, **kw):
        calls[0] += 1
        return entry(*a, **kw)

    monkeypatch.setattr(ext, "fused_expert_nll_panel", counted)
    rng = np.random.default_rng(0)
    X = rng.random((1600, 4)).astype(np.float32)
    y = (np.sin(2.0 * X.sum(-1)) + 0.1 * rng.standard_normal(1600)
         ).astype(np.float32)
    errs = []
    for on in (False, True):
        gp = (GaussianProcessRegression()
              .setKernel(lambda: 1 * ARDRBFKernel(4))
              .setDatasetSizeForExpert(200).setActiveSetSize(100)
              .setSigma2(0.05).setMaxIter(10).setSeed(3).setDevice("cuda:0")
              .setFusedLargeExperts(on))
        errs.append(rmse(y, gp.fit(X, y).predict(X)))
        assert (calls[0] > 0) == on
    print(f"rmse default {errs[0]:.4f}, fused large experts {errs[1]:.4f}")
    assert abs(errs[1] - errs[0]) <= 0.05 * errs[0]

"""The full-fp64 expert kernel (expert_nll_f64.hip, k <= 128) against the
fp64 torch objective on CPU copies of the same inputs."""

import numpy as np
import pytest
import torch

from test_expert_nll_panel_hip import _case, _inputs

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


def _check(nll_h, grad_h, nll_o, grad_o, tol, what):
    scale = np.abs(grad_o).max()
    print(f"{what}: nll rel {abs(nll_h - nll_o) / abs(nll_o):.2e} "
          f"grad max|d|/max|g| {np.abs(grad_h - grad_o).max() / scale:.2e}")
    assert nll_h == pytest.approx(nll_o, rel=tol)
    np.testing.assert_allclose(grad_h, grad_o, rtol=0, atol=tol * scale)


# k: under one block, one block, a block plus a row, 33, the default, the
# largest; d: 1, the tail of the 4-deep MFMA step, 4, 33, 128; every base at
# one mid shape; fp32 rows at two cases
F32, F64 = torch.float32, torch.float64
CASES = [("ard", 3, 5, 1, F64), ("ard", 3, 16, 4, F64), ("ard", 3, 17, 3, F32),
         ("ard", 3, 33, 33, F64), ("ard", 2, 100, 128, F64),
         ("ard", 2, 100, 32, F32), ("ard", 2, 128, 32, F64),
         ("ard", 2, 97, 5, F64), ("rbf", 2, 97, 5, F64),
         ("m32", 2, 97, 5, F64), ("ard_m52", 2, 97, 5, F64)]


@pytest.mark.parametrize("base,E,k,d,xdt", CASES)
def test_f64_vs_fp64_oracle(dev, ext, base, E, k, d, xdt):
    """Tolerance 1e-10: two fp64 factorizations of the oracle disagree by at
    most 1.4e-14 at these shapes and fp32 arithmetic is off by 1e-6."""
    from spark_gp_amd.kernels.compiled import base_family, base_scale
    from spark_gp_amd.ops import hip_backend, torch_backend
    X, y = _inputs(E, k, d, dev)
    X, y = X.to(xdt), y.double()
    cs, theta = _case(base, d)
    assert cs is not None and cs.base == base
    assert hip_backend.supports_nll_f64(cs, X)
    scale = torch.as_tensor(base_scale(base, theta[cs.base_idx], d),
                            dtype=torch.float64, device=dev)
    first = ext.fused_expert_nll_f64(X, y, scale, 1.0, 0.05,
                                     family=base_family(base))
    again = ext.fused_expert_nll_f64(X, y, scale, 1.0, 0.05,
                                     family=base_family(base))
    assert int(first[4].abs().sum()) == 0, "experts fell back"
    for a, b in zip(first, again):
        assert torch.equal(a, b)
    nll_h, grad_h = hip_backend.nll_grad_compiled(cs, theta, X, y, f64=True)
    nll_o, grad_o = torch_backend.nll_grad_compiled(
        cs, theta, X.double().cpu(), y.cpu())
    _check(nll_h, grad_h, nll_o, grad_o, 1e-10, f"{base} {(E, k, d)}")


@pytest.mark.parametrize("base", ["ard", "rbf"])
def test_f64_ill_conditioned(dev, ext, base):
    """Noise 1e-6, where fp32 arithmetic is off by 4e-2 to 1e-1 and the
    oracle's own Cholesky-vs-LU spread is 2e-10: 1e-6 is four orders from
    each."""
    from spark_gp_amd import kernels as K
    from spark_gp_amd.kernels.compiled import base_family, base_scale
    from spark_gp_amd.ops import hip_backend, torch_backend
    E, k, d = 2, 100, 4
    X, y = _inputs(E, k, d, dev)
    _, theta = _case(base, d)
    noise = K.Scalar(1e-6).const * K.EyeKernel()
    cs = K.compile_kernel((1 * K.ARDRBFKernel(d) if base == "ard"
                           else 1 * K.RBFKernel(1.0)) + noise)
    scale = torch.as_tensor(base_scale(base, theta[cs.base_idx], d),
                            dtype=torch.float64, device=dev)
    *_, bad = ext.fused_expert_nll_f64(X, y.double(), scale, 1.0, 1e-6,
                                       family=base_family(base))
    assert int(bad.abs().sum()) == 0
    nll_h, grad_h = hip_backend.nll_grad_compiled(cs, theta, X, y, f64=True)
    nll_o, grad_o = torch_backend.nll_grad_compiled(
        cs, theta, X.double().cpu(), y.double().cpu())
    _check(nll_h, grad_h, nll_o, grad_o, 1e-6, f"{base} noise 1e-6")


@pytest.mark.parametrize("spoil", ["equal_rows", "nan"])
def test_f64_flags_breakdown(dev, ext, spoil):
    """Expert 1 of 3 at noise 0 and a short length scale: rows 0 and 1 at the
    origin with equal y (the second pivot is 1 - 1 * 1, exactly 0 in any
    precision), or a NaN feature in the last row.  Its outputs are zeroed and
    the neighbours come through untouched."""
    from spark_gp_amd import kernels as K
    from spark_gp_amd.ops import torch_backend
    E, k, d = 3, 40, 4
    X, y = _inputs(E, k, d, dev, seed=7)
    X, y = X.double(), y.double()
    if spoil == "equal_rows":
        X[1, 0:2] = 0.0
        y[1, 1] = y[1, 0]
    else:
        X[1, k - 1, 2] = float("nan")
    scale = torch.full((d,), 40.0, dtype=torch.float64, device=dev)
    nll, sumW0, trG, contr, bad = ext.fused_expert_nll_f64(X, y, scale,
                                                           1.0, 0.0)
    assert int(bad[1]) != 0 and int(bad[0]) == 0 and int(bad[2]) == 0
    assert float(nll[1]) == 0.0 and float(sumW0[1]) == 0.0
    assert float(trG[1]) == 0.0 and float(contr[1].abs().sum()) == 0.0
    cs = K.compile_kernel(1 * K.ARDRBFKernel(d))
    theta = np.concatenate([[1.0], np.full(d, 40.0)])
    for e in (0, 2):
        nll_o, grad_o = torch_backend.nll_grad_compiled(
            cs, theta, X[e:e + 1].cpu(), y[e:e + 1].cpu())
        grad_h = cs.assemble_grad(
            theta, g_scale=40.0 * contr[e].cpu().numpy(),
            g_amp=-0.5 * float(sumW0[e]), g_noise=-0.5 * float(trG[e]))
        _check(float(nll[e]), grad_h, nll_o, grad_o, 1e-10, f"expert {e}")


def test_f64_fit_end_to_end(dev, ext, monkeypatch):
    from spark_gp_amd import GaussianProcessRegression, rmse
    from spark_gp_amd.kernels import ARDRBFKernel
    calls = [0]
    entry = ext.fused_expert_nll_f64

    def counted(*a, **kw):
        calls[0] += 1
        return entry(*a, **kw)

    monkeypatch.setattr(ext, "fused_expert_nll_f64", counted)
    rng = np.random.default_rng(0)
    X = rng.random((1600, 4)).astype(np.float32)
    y = (np.sin(2.0 * X.sum(-1)) + 0.1 * rng.standard_normal(1600)
         ).astype(np.float32)
    errs = []
    for on in (False, True):
        gp = (GaussianProcessRegression()
              .setKernel(lambda: 1 * ARDRBFKernel(4))
              .setDatasetSizeForExpert(100).setActiveSetSize(100)
              .setSigma2(0.05).setMaxIter(10).setSeed(3).setDevice("cuda:0")
              .setFusedFp64Experts(on))
        errs.append(rmse(y, gp.fit(X, y).predict(X)))
        assert (calls[0] > 0) == on
    print(f"rmse default {errs[0]:.4f}, fused fp64 experts {errs[1]:.4f}")
    assert abs(errs[1] - errs[0]) <= 0.05 * errs[0]

"""GPU tests of every path hip_backend.kmn_knm_and_kmny (mixed precision)
can take: the three K_nm generators and both SYRK kernels, end to end
against the fp64 CPU torch_backend, with a spy on the extension asserting
which entry points ran.  Tolerance: the one of
test_ppa_stats_fused_vs_two_kernel (rtol 2e-2, atol 2e-2 max|ref|)."""

import collections

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

_SWITCHES = ("SPARK_GP_AMD_PPA_FUSED", "SPARK_GP_AMD_CROSS_MFMA",
             "SPARK_GP_AMD_SYRK_SYNC", "SPARK_GP_AMD_SYRK_PATCH")
_ENTRY_POINTS = ("ppa_fused_acc", "cross_mfma_ppa", "cross_kernel_tile_ppa",
                 "syrk_bf16_acc", "syrk_bf16_sync_acc")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


_PROBLEMS = {}


def _problem(n, m, d):
    """Inputs and the fp64 CPU reference of one shape, built once."""
    if (n, m, d) not in _PROBLEMS:
        from spark_gp_amd.kernels import ARDRBFKernel, EyeKernel, Scalar
        from spark_gp_amd.ops import torch_backend
        g = torch.Generator().manual_seed(100 * n + 10 * m + d)
        X = torch.rand(n, d, generator=g)
        y = torch.sin(X.sum(-1))
        active = torch.rand(m, d, generator=g)
        kernel = 1 * ARDRBFKernel(d) + Scalar(1e-3).const * EyeKernel()
        kernel.set_hyperparameters(np.concatenate(
            [[1.2], np.random.default_rng(8).uniform(0.5, 2, d)]))
        KK, Ky = torch_backend.kmn_knm_and_kmny(kernel, active.double(),
                                                X.double(), y.double())
        _PROBLEMS[(n, m, d)] = (kernel, active, X, y, KK, Ky)
    return _PROBLEMS[(n, m, d)]


def _run_and_compare(dev, monkeypatch, n, m, d, env, **kw):
    """Run the mixed-precision HIP path under ``env``; returns the number of
    calls per extension entry point."""
    from spark_gp_amd import _hip_ext as ext
    from spark_gp_amd.ops import hip_backend
    kernel, active, X, y, KK_ref, Ky_ref = _problem(n, m, d)
    for name in _SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    calls = collections.Counter()

    class _Spy:
        def __getattr__(self, name):
            attr = getattr(ext, name)
            if name not in _ENTRY_POINTS:
                return attr

            def counted(*a, **kw):
                calls[name] += 1
                return attr(*a, **kw)
            return counted

    monkeypatch.setattr(hip_backend, "ext", _Spy())
    KK, Ky = hip_backend.kmn_knm_and_kmny(kernel, active.to(dev), X.to(dev),
                                          y.to(dev), precision="mixed", **kw)
    KK, Ky = KK.cpu(), Ky.cpu()
    print(f"(n, m, d)={(n, m, d)} env={env}: max|dKK| "
          f"{float((KK - KK_ref).abs().max()):.3e} (scale "
          f"{float(KK_ref.abs().max()):.3e}), max|dKy| "
          f"{float((Ky - Ky_ref).abs().max()):.3e}")
    np.testing.assert_allclose(KK.numpy(), KK_ref.numpy(), rtol=2e-2,
                               atol=2e-2 * float(KK_ref.abs().max()))
    np.testing.assert_allclose(Ky.numpy(), Ky_ref.numpy(), rtol=2e-2,
                               atol=2e-2 * float(Ky_ref.abs().max()))
    return dict(calls)


@pytest.mark.parametrize("env,expected", [
    # one fused launch over the doubled chunk (1000 rows: no multiple of 32)
    ({}, {"ppa_fused_acc": 1}),
    # chunks of 512 and 488 rows
    ({"SPARK_GP_AMD_PPA_FUSED": "0"},
     {"cross_mfma_ppa": 2, "syrk_bf16_acc": 2}),
    ({"SPARK_GP_AMD_CROSS_MFMA": "0"},
     {"cross_kernel_tile_ppa": 2, "syrk_bf16_acc": 2}),
], ids=["fused", "mfma", "elementwise"])
def test_small_shape_under_each_generator(dev, monkeypatch, env, expected):
    """m = 300: three tiles (one off-diagonal), the second window partly
    filled."""
    calls = _run_and_compare(dev, monkeypatch, 1000, 300, 8, env,
                             chunk_rows=512)
    assert calls == expected


def test_large_m_takes_the_sync_syrk(dev, monkeypatch):
    """m = 5888: 276 tiles, above the split-k family's 256, so the staged
    MFMA generator feeds the k-synchronized SYRK in two launches (224 + 52
    tiles)."""
    calls = _run_and_compare(dev, monkeypatch, 64, 5888, 4, {})
    assert calls == {"cross_mfma_ppa": 1, "syrk_bf16_sync_acc": 2}

"""GPU tests of the Matérn 3/2 and 5/2 instances of the HIP kernels: the
fused per-expert NLL against the fp64 oracle, the ``family`` argument of the
bindings, the cross kernel and both PPA generators against fp64 Matérn
references, and regression / classification fits end to end."""

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


def _classes():
    from spark_gp_amd.kernels import (ARDMatern32Kernel, ARDMatern52Kernel,
                                      Matern32Kernel, Matern52Kernel)
    return {"m32": Matern32Kernel, "m52": Matern52Kernel,
            "ard_m32": ARDMatern32Kernel, "ard_m52": ARDMatern52Kernel}


def _ard_class(family):
    return _classes()["ard_m32" if family == 1 else "ard_m52"]


def _expert_data(E, k, d, seed, dev):
    """Inputs of test_hip_kernels.py::_ard_setup."""
    g = torch.Generator().manual_seed(seed)
    X = torch.rand(E, k, d, generator=g).to(dev)
    y = torch.sin(3.0 * X.sum(-1)).to(dev)
    return X, y


# (E, k, d): every tail path of the blocked factorization; k across a
# 32-block; nll_bslab == 0 (the global-form B epilogue); the staged epilogue
# with three experts resident per CU
NLL_SHAPES = [(6, 7, 3), (6, 13, 5), (6, 31, 4), (6, 33, 4), (6, 32, 8),
              (16, 100, 32)]


@pytest.mark.parametrize("E,k,d", NLL_SHAPES)
@pytest.mark.parametrize("base", ["ard_m32", "ard_m52", "m52"])
def test_fused_expert_nll_matern_vs_oracle(dev, ext, base, E, k, d):
    from spark_gp_amd.kernels import EyeKernel, Scalar, compile_kernel
    from spark_gp_amd.kernels.compiled import (base_family, base_is_ard,
                                               base_scale)
    from spark_gp_amd.ops import hip_backend, torch_backend
    X, y = _expert_data(E, k, d, 0 if k == 100 else 5, dev)
    cls = _classes()[base]
    ard = base_is_ard(base)
    cs = compile_kernel(1 * (cls(d) if ard else cls(1.0))
                        + Scalar(1e-3).const * EyeKernel())
    assert cs is not None and cs.base == base
    fam = base_family(base)
    assert fam in (ext.FAM_M32, ext.FAM_M52)
    rng = np.random.default_rng(1 if k == 100 else 2)
    amp = 1.3 if k == 100 else 0.9
    theta = np.concatenate([[amp], rng.uniform(0.5, 2.0, d) if ard
                            else [0.8]])

    # the HIP kernel itself must handle every expert (a silent fallback to
    # the torch path would make this test vacuous)
    scale = torch.as_tensor(base_scale(base, theta[cs.base_idx], d),
                            dtype=torch.float32, device=dev)
    nll_e, sumW0, trG, contr, bad = ext.fused_expert_nll(
        X, y, scale, float(theta[0]), 1e-3, family=fam)
    assert int(bad.sum()) == 0, "experts fell back: kernel not exercised"

    Xc, yc = X.double().cpu(), y.double().cpu()
    nll_h, grad_h = hip_backend.nll_grad_compiled(cs, theta, X, y)
    nll_o, grad_o = torch_backend.nll_grad_compiled(cs, theta, Xc, yc)

    # raw sumW0 is sum(G o Kb), not sum(G o Kd)
    Kb, Kd, _ = torch_backend._base_matrices(cs, theta, Xc)
    K = theta[0] * Kb + 1e-3 * torch.eye(k, dtype=torch.float64)
    Kinv = torch.linalg.inv(K)
    alpha = (Kinv @ yc.unsqueeze(-1)).squeeze(-1)
    G = alpha.unsqueeze(-1) * alpha.unsqueeze(-2) - Kinv
    sum_gkb = (G * Kb).sum((-1, -2)).numpy()                   # [E]
    sum_gkd = (G * Kd).sum((-1, -2))
    got = sumW0.cpu().numpy()
    print(f"{base} {(E, k, d)}: nll rel {abs(nll_h - nll_o) / abs(nll_o):.2e}"
          f" grad max|d|/max|g| "
          f"{np.abs(grad_h - grad_o).max() / np.abs(grad_o).max():.2e}"
          f" sumW0 max|d| {np.abs(got - sum_gkb).max():.3e} at max|.| "
          f"{np.abs(sum_gkb).max():.3e} (sum G o Kd is off by "
          f"{np.abs(sum_gkd.numpy() - sum_gkb).max():.3e})")
    np.testing.assert_allclose(got, sum_gkb, rtol=2e-4, atol=2e-4 * k)

    assert nll_h == pytest.approx(nll_o, rel=2e-4)
    np.testing.assert_allclose(grad_h, grad_o, rtol=3e-3,
                               atol=2e-3 * np.abs(grad_o).max())


def test_family_zero_is_the_default(dev, ext):
    """family=0 returns bitwise what the call without the argument does."""
    X, y = _expert_data(6, 33, 4, 5, dev)
    scale = torch.rand(4, device=dev) + 0.5
    a = ext.fused_expert_nll(X, y, scale, 0.9, 1e-3)
    b = ext.fused_expert_nll(X, y, scale, 0.9, 1e-3, family=0)
    c = ext.fused_expert_nll(X, y, scale, 0.9, 1e-3, ext.FAM_RBF)
    for ta, tb, tc in zip(a, b, c):
        assert torch.equal(ta, tb) and torch.equal(ta, tc)
    # ... and a Matérn family does not
    m = ext.fused_expert_nll(X, y, scale, 0.9, 1e-3, family=ext.FAM_M52)
    assert not torch.equal(a[0], m[0])

    g = torch.Generator().manual_seed(3)
    Xc = torch.rand(300, 8, generator=g).to(dev)
    A = torch.rand(130, 8, generator=g).to(dev)
    s2 = torch.rand(8, generator=g).to(dev) + 0.3
    ta = ext.cross_kernel_tile(Xc, A, s2, 1.7, False, False)[0]
    tb = ext.cross_kernel_tile(Xc, A, s2, 1.7, False, False, family=0)[0]
    assert torch.equal(ta, tb)


def test_unknown_family_raises(dev, ext):
    X, y = _expert_data(2, 8, 3, 5, dev)
    scale = torch.ones(3, device=dev)
    for fam in (3, -1):
        with pytest.raises(RuntimeError, match="family"):
            ext.fused_expert_nll(X, y, scale, 1.0, 1e-3, family=fam)
        with pytest.raises(RuntimeError, match="family"):
            ext.fused_expert_nll_occupancy(100, 32, fam)
        with pytest.raises(RuntimeError, match="family"):
            ext.cross_kernel_tile(X[0], X[1], scale, 1.0, False, False,
                                  family=fam)


def test_occupancy_equals_rbf(dev, ext):
    rbf = ext.fused_expert_nll_occupancy(100, 32)
    assert ext.fused_expert_nll_occupancy(100, 32, ext.FAM_RBF) == rbf
    for fam in (ext.FAM_M32, ext.FAM_M52):
        assert ext.fused_expert_nll_occupancy(100, 32, fam) == rbf


@pytest.mark.parametrize("base", ["m32", "m52", "ard_m32", "ard_m52"])
def test_cross_kernel_tile_matern_vs_torch(dev, ext, base):
    """Shapes and tolerance of test_cross_kernel_tile_vs_torch."""
    from spark_gp_amd.kernels import EyeKernel, Scalar
    from spark_gp_amd.ops import hip_backend
    g = torch.Generator().manual_seed(3)
    X = torch.rand(1000, 32, generator=g).to(dev)       # c not mult of 128
    A = torch.rand(333, 32, generator=g).to(dev)        # m not mult of 128
    cls = _classes()[base]
    ard = base.startswith("ard")
    kernel = 1 * (cls(32) if ard else cls(1.0)) \
        + Scalar(1e-3).const * EyeKernel()
    hp = (np.random.default_rng(4).uniform(0.5, 2, 32) if ard else [1.1])
    kernel.set_hyperparameters(np.concatenate([[1.7], hp]))
    assert hip_backend.supports_ppa(kernel, X)
    got = hip_backend.cross_kernel(kernel, X, A)
    ref = kernel.cross_kernel(X.double(), A.double())
    print(f"{base}: max abs err "
          f"{float((got.double() - ref).abs().max()):.3e}")
    np.testing.assert_allclose(got.cpu().numpy(), ref.cpu().numpy(),
                               rtol=1e-4, atol=1e-5)


_PPA = {}


def _ppa_setup(c, m, d, family, dev):
    """Pre-scaled inputs and the fp64 CPU reference of one (shape, family),
    as in test_ppa_fused.py::_setup with the family's Kb for exp(-q);
    built once, shared, never modified."""
    key = (c, m, d, family)
    if key not in _PPA:
        g = torch.Generator().manual_seed(1000 * c + 10 * m + d)
        X = torch.rand(c, d, generator=g)
        A = torch.rand(m, d, generator=g)
        y = torch.rand(c, generator=g)
        beta = torch.rand(d, generator=g) + 0.5
        amp = 1.3
        kernel = amp * _ard_class(family)(beta.numpy())
        K = kernel.cross_kernel(X.double(), A.double())       # [c, m] fp64
        s = beta * (3.0 if family == 1 else 5.0) ** 0.5
        Xs = (X * s).to(dev).contiguous()
        As = (A * s).to(dev).contiguous()
        _PPA[key] = dict(Xs=Xs, As=As, nx=(Xs * Xs).sum(-1).contiguous(),
                         na=(As * As).sum(-1).contiguous(), y=y.to(dev),
                         amp=amp, K=K, KK_ref=K.T @ K,
                         Ky_ref=K.T @ y.double())
    return _PPA[key]


@pytest.mark.parametrize("family", [1, 2])
@pytest.mark.parametrize("c,m,d", [(1000, 300, 8), (513, 130, 5)])
def test_cross_mfma_ppa_matern_vs_oracle(dev, ext, family, c, m, d):
    """Tolerances of test_cross_mfma_ppa_vs_oracle."""
    s = _ppa_setup(c, m, d, family, dev)
    Ky = torch.zeros(m, dtype=torch.float64, device=dev)
    KcT, KlT = ext.cross_mfma_ppa(s["Xs"], s["As"], s["nx"], s["na"],
                                  s["amp"], s["y"], Ky, family=family)
    V = (KcT.float() + KlT.float()).cpu().double()        # [m, c]
    ref = s["K"].T
    err = (V - ref).abs().max().item()
    print(f"family {family} {(c, m, d)}: err {err:.3e} "
          f"(bound {5e-5 * float(ref.abs().max()):.3e})")
    assert err < 5e-5 * float(ref.abs().max()), (c, m, d, err)
    torch.testing.assert_close(Ky.cpu(), s["Ky_ref"], rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("family", [1, 2])
@pytest.mark.parametrize("c,m,d,split_k", [(1000, 300, 8, 1),
                                           (513, 130, 5, 3),
                                           (31, 257, 32, 4)])
def test_ppa_fused_acc_matern_vs_oracle(dev, ext, family, c, m, d, split_k):
    """Tolerances of test_ppa_fused.py::test_fused_vs_oracle_and_pair."""
    s = _ppa_setup(c, m, d, family, dev)
    args = (s["Xs"], s["As"], s["nx"], s["na"], s["amp"], s["y"])
    KK_f = torch.zeros(m, m, dtype=torch.float32, device=dev)
    Ky_f = torch.zeros(m, dtype=torch.float64, device=dev)
    ext.ppa_fused_acc(*args, Ky_f, KK_f, split_k, family=family)
    KK_p = torch.zeros(m, m, dtype=torch.float32, device=dev)
    Ky_p = torch.zeros(m, dtype=torch.float64, device=dev)
    KcT, KlT = ext.cross_mfma_ppa(*args, Ky_p, family=family)
    ext.syrk_bf16_acc(KcT, KlT, KK_p, split_k)
    torch.cuda.synchronize()
    scale = float(s["KK_ref"].abs().max())
    err_f = float((KK_f.cpu().double() - s["KK_ref"]).abs().max())
    err_p = float((KK_p.cpu().double() - s["KK_ref"]).abs().max())
    print(f"family {family} (c,m,d,split_k)={(c, m, d, split_k)} "
          f"scale={scale:.4e} err_fused={err_f:.4e} err_pair={err_p:.4e}")
    assert err_f < 1e-4 * scale, (err_f, scale)
    # same products, different summation order
    assert err_f < 4 * max(err_p, 1e-30), (err_f, err_p)
    torch.testing.assert_close(Ky_f.cpu(), s["Ky_ref"], rtol=1e-4, atol=1e-4)


# ---- end to end ------------------------------------------------------------

def _fit_data():
    """Data of test_matern.py::test_matern_fit_end_to_end."""
    rng = np.random.default_rng(0)
    X = rng.uniform(size=(400, 2))
    y = np.sin(3 * X.sum(-1)) + 0.05 * rng.normal(size=400)
    return X, y


def _fit(kernel_factory, X, y):
    from spark_gp_amd import GaussianProcessRegression
    return (GaussianProcessRegression()
            .setKernel(kernel_factory)
            .setDatasetSizeForExpert(50).setActiveSetSize(80)
            .setSigma2(1e-2).setMaxIter(30).setSeed(0).setDevice("cuda")
            .fit(X, y))


def test_matern_fit_end_to_end_on_gpu(dev, ext, monkeypatch):
    from spark_gp_amd.kernels import ARDMatern52Kernel, Matern52Kernel
    from spark_gp_amd.ops import hip_backend, torch_backend
    from spark_gp_amd.utils import rmse
    calls = {"generic": 0, "fused": 0, "cross": 0}

    def counted(name, fn):
        def wrapper(*a, **kw):
            calls[name] += 1
            return fn(*a, **kw)
        return wrapper

    monkeypatch.setattr(torch_backend, "nll_grad_generic",
                        counted("generic", torch_backend.nll_grad_generic))
    monkeypatch.setattr(hip_backend, "nll_grad_compiled",
                        counted("fused", hip_backend.nll_grad_compiled))
    monkeypatch.setattr(hip_backend, "cross_kernel",
                        counted("cross", hip_backend.cross_kernel))
    X, y = _fit_data()
    model = _fit(lambda: 1 * Matern52Kernel(1.0), X, y)
    err = rmse(y, model.predict(X))
    print(f"Matern52 GPU fit rmse {err:.4f}, calls {calls}")
    assert err < 0.15
    assert calls["generic"] == 0
    assert calls["fused"] > 0 and calls["cross"] > 0

    model = _fit(lambda: 1 * ARDMatern52Kernel(2), X, y)
    err = rmse(y, model.predict(X))
    print(f"ARDMatern52 GPU fit rmse {err:.4f}, calls {calls}")
    assert err < 0.15
    assert calls["generic"] == 0


def test_matern_classifier_on_gpu(dev, ext):
    """A Matérn classifier keeps the torch Laplace path (laplace.hip is
    exp(-q) only) on top of the HIP cross kernel and PPA."""
    from spark_gp_amd import GaussianProcessClassifier, accuracy
    from spark_gp_amd.kernels import Matern52Kernel
    rng = np.random.default_rng(0)
    n = 200
    X = np.concatenate([rng.normal(-1.5, 0.7, (n // 2, 2)),
                        rng.normal(1.5, 0.7, (n // 2, 2))]).astype(np.float32)
    y = np.concatenate([np.zeros(n // 2), np.ones(n // 2)]).astype(np.float32)
    model = (GaussianProcessClassifier()
             .setKernel(lambda: 1 * Matern52Kernel(1.0, 1e-3, 10))
             .setDatasetSizeForExpert(50)
             .setActiveSetSize(40)
             .setSigma2(1e-3)
             .setMaxIter(10)
             .setSeed(7)
             .setDevice("cuda:0")).fit(X, y)
    acc = accuracy(y, model.predict(X))
    print(f"Matern52 GPU classifier accuracy {acc:.3f}")
    assert acc > 0.95

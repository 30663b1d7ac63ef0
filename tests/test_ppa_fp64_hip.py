"""GPU tests of the fused fp64 PPA accumulation (ppa_fp64.hip): both feeders
of ``ext.ppa_fp64_acc`` against fp64 CPU references, bitwise repeatability,
the routing of ``hip_backend.kmn_knm_and_kmny(fused_fp64=True)`` and one
estimator fit.

Shapes: m in {1, 128, 129, 300} is a lone partial tile, exactly one tile, an
off-diagonal tile whose row window has one column, and three windows; c in
{1, 33, 1000} is less than one 32-row k-step, one step and a row, and 32
steps.  split_k = 3 leaves slices empty at c = 1 and 33 and uneven at 1000.

Measured on an MI355X (relative error: max|delta| / max|ref|, the worst of
KK and Ky over the whole grid): see profiles/PROFILES.md, round 18."""

import collections

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MS, CS = (1, 128, 129, 300), (1, 33, 1000)
SPLITS = (1, 3)
# (d + 2) fp32 roundings of q and the exponential's few ulp: about 1e-5 per
# K value, doubled for a product of two positive terms
GEN_TOL = 5e-5


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ext():
    from spark_gp_amd import _hip_ext
    return _hip_ext


def _acc(ext, dev, m, X, y, split_k, calls=1, **kw):
    KK = torch.zeros(m, m, dtype=torch.float64, device=dev)
    Ky = torch.zeros(m, dtype=torch.float64, device=dev)
    for _ in range(calls):
        ext.ppa_fp64_acc(X, y, Ky, KK, split_k, **kw)
    return KK.cpu(), Ky.cpu()


def _rel(a, ref):
    return float((a - ref).abs().max() / ref.abs().max())


_STAGED = {}


def _staged(c, m):
    """A positive fp32 chunk and y with their exact fp64 products."""
    if (c, m) not in _STAGED:
        g = torch.Generator().manual_seed(1000 * c + m)
        K = torch.rand(c, m, generator=g)
        y = torch.rand(c, generator=g) + 0.5
        _STAGED[(c, m)] = (K, y, K.double().T @ K.double(),
                           K.double().T @ y.double())
    return _STAGED[(c, m)]


@pytest.mark.parametrize("split_k", SPLITS)
@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("c", CS)
def test_staged_feeder_is_exact_fp64(dev, ext, c, m, split_k):
    """Products of widened floats are exact in fp64 and every term is
    positive, so only the order of at most 1000 additions separates the
    kernel from the CPU: c 2^-53 ~ 1.1e-13 relative."""
    K, y, KK_ref, Ky_ref = _staged(c, m)
    KK, Ky = _acc(ext, dev, m, K.to(dev), y.to(dev), split_k)
    np.testing.assert_allclose(KK.numpy(), KK_ref.numpy(), rtol=1e-12, atol=0)
    np.testing.assert_allclose(Ky.numpy(), Ky_ref.numpy(), rtol=1e-12, atol=0)


@pytest.mark.parametrize("split_k", SPLITS)
def test_two_calls_add(dev, ext, split_k):
    K, y, KK_ref, Ky_ref = _staged(33, 129)
    KK, Ky = _acc(ext, dev, 129, K.to(dev), y.to(dev), split_k, calls=2)
    np.testing.assert_allclose(KK.numpy(), 2 * KK_ref.numpy(), rtol=1e-12,
                               atol=0)
    np.testing.assert_allclose(Ky.numpy(), 2 * Ky_ref.numpy(), rtol=1e-12,
                               atol=0)


_PROBLEMS = {}


def _problem(base, n, m, d):
    """A kernel with scales u_j / sqrt(d), u in [0.5, 2], inputs in [0, 1]^d
    (so q <= 4), and the fp64 CPU oracle of KK and Ky."""
    key = (base, n, m, d)
    if key not in _PROBLEMS:
        from spark_gp_amd import kernels as ks
        cls, nup = {"rbf": (ks.ARDRBFKernel, 1.0),
                    "m32": (ks.ARDMatern32Kernel, 3.0),
                    "m52": (ks.ARDMatern52Kernel, 5.0)}[base]
        g = torch.Generator().manual_seed(100 * n + 10 * m + d)
        X = torch.rand(n, d, generator=g)
        A = torch.rand(m, d, generator=g)
        y = torch.sin(X.sum(-1)) + 1.5
        kernel = 1 * cls(d) + ks.Scalar(1e-3).const * ks.EyeKernel()
        u = np.random.default_rng(8).uniform(0.5, 2, d)
        kernel.set_hyperparameters(np.concatenate(
            [[1.2], u / np.sqrt(d * nup)]))
        K = kernel.cross_kernel(X.double(), A.double())
        _PROBLEMS[key] = (kernel, A, X, y, K.T @ K, K.T @ y.double())
    return _PROBLEMS[key]


@pytest.mark.parametrize("base", ["rbf", "m32", "m52"])
@pytest.mark.parametrize("d", [1, 32])
@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("c", CS)
def test_generating_feeder_vs_fp64_oracle(dev, ext, c, m, d, base):
    """K generated in the block, against ``kernel.cross_kernel`` in fp64 and
    against the error of the staged ``precision="fp64"`` branch, which a
    Gram-form generator would exceed many times over."""
    from spark_gp_amd.kernels import compile_kernel
    from spark_gp_amd.kernels.compiled import base_family
    from spark_gp_amd.ops import hip_backend
    kernel, A, X, y, KK_ref, Ky_ref = _problem(base, c, m, d)
    cs, theta = compile_kernel(kernel), kernel.get_hyperparameters()
    Xd, Ad, yd = X.to(dev), A.to(dev), y.to(dev)
    kw = dict(A=Ad, s2=hip_backend._s2_vector(cs, theta, d, dev),
              amp=float(cs.amp(theta)), family=base_family(cs.base))
    err = 0.0
    for split_k in SPLITS:
        KK, Ky = _acc(ext, dev, m, Xd, yd, split_k, **kw)
        err = max(err, _rel(KK, KK_ref), _rel(Ky, Ky_ref))
    KK0, Ky0 = hip_backend.kmn_knm_and_kmny(kernel, Ad, Xd, yd,
                                            precision="fp64")
    err0 = max(_rel(KK0.cpu(), KK_ref), _rel(Ky0.cpu(), Ky_ref))
    print(f"{base} (c, m, d)={(c, m, d)}: fused {err:.3e}  staged {err0:.3e}")
    assert err <= GEN_TOL
    assert err <= 4 * err0


@pytest.mark.parametrize("gen", [True, False], ids=["generate", "staged"])
def test_same_bits_on_every_run(dev, ext, gen):
    kernel, A, X, y, _, _ = _problem("rbf", 1000, 300, 8)
    if gen:
        kw = dict(A=A.to(dev), s2=torch.full((8,), 0.3, device=dev), amp=1.2)
        src = X.to(dev)
    else:
        kw, src = {}, _staged(1000, 300)[0].to(dev)
    runs = [_acc(ext, dev, 300, src, y.to(dev), 3, **kw) for _ in range(2)]
    assert torch.equal(runs[0][0], runs[1][0])
    assert torch.equal(runs[0][1], runs[1][1])


def _spied(monkeypatch, names):
    from spark_gp_amd import _hip_ext
    from spark_gp_amd.ops import hip_backend
    calls = collections.Counter()

    class _Spy:
        def __getattr__(self, name):
            attr = getattr(_hip_ext, name)
            if name not in names:
                return attr

            def counted(*a, **kw):
                calls[name] += 1
                return attr(*a, **kw)
            return counted

    monkeypatch.setattr(hip_backend, "ext", _Spy())
    return calls


@pytest.mark.parametrize("d,fused,expected", [
    (8, True, {"ppa_fp64_acc": 2}),
    (33, True, {"ppa_fp64_acc": 2, "cross_kernel_tile": 2}),
    (8, False, {"cross_kernel_tile": 2}),
], ids=["generate", "staged", "flag-unset"])
def test_routing(dev, monkeypatch, d, fused, expected):
    """1000 rows in chunks of 512 and 488; m = 300."""
    from spark_gp_amd.ops import hip_backend
    kernel, A, X, y, KK_ref, Ky_ref = _problem("rbf", 1000, 300, d)
    calls = _spied(monkeypatch, ("ppa_fp64_acc", "cross_kernel_tile"))
    KK, Ky = hip_backend.kmn_knm_and_kmny(
        kernel, A.to(dev), X.to(dev), y.to(dev), chunk_rows=512,
        precision="fp64", **({"fused_fp64": True} if fused else {}))
    assert dict(calls) == expected
    assert KK.shape == (300, 300) and KK.dtype == torch.float64
    assert _rel(KK.cpu(), KK_ref) <= GEN_TOL
    assert _rel(Ky.cpu(), Ky_ref) <= GEN_TOL


def test_fit_with_the_flag(dev, monkeypatch):
    """The configuration and quality gate of test_hip_kernels.py's
    test_gpu_fit_end_to_end, with the PPA stage on the fused kernel."""
    from spark_gp_amd import GaussianProcessRegression, rmse
    from spark_gp_amd.kernels import ARDRBFKernel
    rng = np.random.default_rng(0)
    X = rng.random((30000, 4)).astype(np.float32)
    y = (np.sin(5.0 * X[:, 0]) + X[:, 1]).astype(np.float32)
    calls = _spied(monkeypatch, ("ppa_fp64_acc",))
    gp = (GaussianProcessRegression()
          .setKernel(lambda: 1 * ARDRBFKernel(4))
          .setDatasetSizeForExpert(100)
          .setActiveSetSize(300)
          .setSigma2(1e-3)
          .setMaxIter(15)
          .setSeed(3)
          .setFusedPpaFp64(True)
          .setDevice("cuda:0"))
    model = gp.fit(X, y)
    assert calls["ppa_fp64_acc"] == 1
    err = rmse(y[:3000], model.predict(X[:3000]))
    assert err < 0.02, f"GPU fit rmse {err}"

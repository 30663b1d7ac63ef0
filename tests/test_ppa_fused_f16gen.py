"""GPU tests of the two K_nm generators of the fused PPA accumulation
(``ppa_fused_acc(..., gen=)``): the split-f16 generator against the fp32 one
and the two-kernel pair, each against the fp64 CPU oracle built the way
``test_ppa_fused.py::_setup`` builds it.

Acceptance, per case: the f16 generator's error is below 4 x the larger of
the fp32 generator's and the pair's (the factor test_ppa_fused.py grants
between the fused kernel and the pair), on KK and on Ky, next to that file's
absolute bounds."""

import pytest
import torch

pytestmark = pytest.mark.gpu

AMP = 1.3
NUP = {0: 1.0, 1: 3.0, 2: 5.0}            # family code -> nu' (RBF: none)

# (c, m, d, split_k): what each exercises in the generator
SHAPES = [
    (31, 257, 32, 4),       # c below one k-block; a window with one real column
    (513, 130, 5, 3),       # d not a multiple of 8: k-lane groups partly padded
    (96, 256, 1, 1),        # a single feature; one full window
    (70, 300, 17, 2),       # d odd and above 16: the last pair half padded
    (1000, 300, 8, 1),      # second window partly filled
    (8192, 1000, 32, 25),   # the headline tile set
]

# inputs that stress the split: name -> (X, A) in place
INPUTS = ("uniform", "coincident", "span", "zero_column")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ext():
    from spark_gp_amd import _hip_ext
    return _hip_ext


def _kernel_class(family):
    from spark_gp_amd.kernels import (ARDMatern32Kernel, ARDMatern52Kernel,
                                      ARDRBFKernel)
    return (ARDRBFKernel, ARDMatern32Kernel, ARDMatern52Kernel)[family]


_SETUPS = {}


def _setup(c, m, d, family, kind, dev):
    """Pre-scaled inputs and the fp64 CPU reference of one case, built once,
    shared by the tests that use it and never modified."""
    key = (c, m, d, family, kind)
    if key in _SETUPS:
        return _SETUPS[key]
    g = torch.Generator().manual_seed(1000 * c + 10 * m + d)
    X = torch.rand(c, d, generator=g)
    A = torch.rand(m, d, generator=g)
    y = torch.rand(c, generator=g)
    beta = torch.rand(d, generator=g) + 0.5
    if kind == "coincident":
        # 32 active rows copied from X: q = 0, where the cancellation in
        # n_x + n_a - 2 x'.a' sets the error of either generator
        A[:32] = X[:32]
    elif kind == "span":
        # coordinates from 1e-7 to 10, one decade range per feature: hi is
        # zeroed for the small ones and lo is subnormal for the smallest
        expo = torch.linspace(-7.0, 1.0, d) if d > 1 else torch.ones(1)
        X = X * 10.0 ** expo
        A = A * 10.0 ** expo
    elif kind == "zero_column":
        X[:, d // 2] = 0.0
        A[:, d // 2] = 0.0
    elif kind == "outlier":
        # one sample far outside the f16 range after scaling
        X[0, 0] = 7e4 / float(beta[0])
    kernel = AMP * _kernel_class(family)(beta.numpy())
    K = kernel.cross_kernel(X.double(), A.double())       # [c, m] fp64
    s = beta * NUP[family] ** 0.5
    Xs = (X * s).to(dev).contiguous()
    As = (A * s).to(dev).contiguous()
    _SETUPS[key] = dict(
        args=(Xs, As, (Xs * Xs).sum(-1).contiguous(),
              (As * As).sum(-1).contiguous(), AMP, y.to(dev)),
        KK_ref=K.T @ K, Ky_ref=K.T @ y.double())
    return _SETUPS[key]


def _fused(ext, s, m, split_k, family, dev, **kw):
    KK = torch.zeros(m, m, dtype=torch.float32, device=dev)
    Ky = torch.zeros(m, dtype=torch.float64, device=dev)
    ext.ppa_fused_acc(*s["args"], Ky, KK, split_k, family=family, **kw)
    return KK, Ky


def _pair(ext, s, m, split_k, family, dev):
    KK = torch.zeros(m, m, dtype=torch.float32, device=dev)
    Ky = torch.zeros(m, dtype=torch.float64, device=dev)
    KcT, KlT = ext.cross_mfma_ppa(*s["args"], Ky, family=family)
    ext.syrk_bf16_acc(KcT, KlT, KK, split_k)
    return KK, Ky


def _errors(s, KK, Ky):
    return (float((KK.cpu().double() - s["KK_ref"]).abs().max()),
            float((Ky.cpu() - s["Ky_ref"]).abs().max()))


def _check(ext, dev, c, m, d, split_k, family, kind):
    s = _setup(c, m, d, family, kind, dev)
    KK16, Ky16 = _fused(ext, s, m, split_k, family, dev, gen="f16")
    KK32, Ky32 = _fused(ext, s, m, split_k, family, dev, gen="f32")
    KKp, Kyp = _pair(ext, s, m, split_k, family, dev)
    torch.cuda.synchronize()
    scale = float(s["KK_ref"].abs().max())
    e16, y16 = _errors(s, KK16, Ky16)
    e32, y32 = _errors(s, KK32, Ky32)
    ep, yp = _errors(s, KKp, Kyp)
    print(f"family {family} {kind} (c,m,d,split_k)={(c, m, d, split_k)} "
          f"scale={scale:.4e}  KK err f16={e16:.4e} f32={e32:.4e} "
          f"pair={ep:.4e}  Ky err f16={y16:.4e} f32={y32:.4e} pair={yp:.4e}")
    assert scale > 0.0                     # the case is not vacuous
    assert e16 < 1e-4 * scale, (e16, scale)
    assert e16 < 4 * max(e32, ep, 1e-30), (e16, e32, ep)
    assert y16 < 4 * max(y32, yp, 1e-30), (y16, y32, yp)
    torch.testing.assert_close(Ky16.cpu(), s["Ky_ref"], rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("family", [0, 1, 2])
@pytest.mark.parametrize("c,m,d,split_k", SHAPES)
def test_f16_vs_f32_pair_and_oracle(dev, ext, c, m, d, split_k, family):
    _check(ext, dev, c, m, d, split_k, family, "uniform")


@pytest.mark.parametrize("kind", INPUTS[1:])
@pytest.mark.parametrize("c,m,d,split_k", [(513, 130, 5, 3),
                                           (513, 130, 32, 3)])
def test_f16_on_stress_inputs(dev, ext, c, m, d, split_k, kind):
    """The d = 5 shape of the list above and the same at d = 32, RBF (the
    generator does not depend on the family); "uniform" at (513, 130, 5, 3)
    is a case of the test above."""
    _check(ext, dev, c, m, d, split_k, 0, kind)


def test_uniform_d32_stress_shape(dev, ext):
    _check(ext, dev, 513, 130, 32, 3, 0, "uniform")


def test_auto_routes_out_of_range_features_to_f32(dev, ext):
    """One sample at 7e4 after scaling is beyond the f16 images' range:
    "auto" takes the maxima of Xs and As itself and runs the fp32 generator,
    bit for bit; the result matches the oracle (that sample's K row is 0)."""
    c, m, d, split_k = 513, 130, 5, 1
    s = _setup(c, m, d, 0, "outlier", dev)
    KKa, Kya = _fused(ext, s, m, split_k, 0, dev)             # gen="auto"
    KK32, Ky32 = _fused(ext, s, m, split_k, 0, dev, gen="f32")
    torch.cuda.synchronize()
    assert torch.equal(KKa, KK32)          # one k-slice: no atomic reorder
    scale = float(s["KK_ref"].abs().max())
    e, _ = _errors(s, KKa, Kya)
    assert e < 1e-4 * scale, (e, scale)
    torch.testing.assert_close(Kya.cpu(), s["Ky_ref"], rtol=1e-4, atol=1e-4)


def test_f16_refused_out_of_range(dev, ext):
    """An explicit gen="f16" is refused there, not silently replaced, by the
    binding's own reduction and by a caller's bound alike; KK stays as it
    was."""
    c, m, d = 513, 130, 5
    s = _setup(c, m, d, 0, "outlier", dev)
    KK = torch.zeros(m, m, dtype=torch.float32, device=dev)
    Ky = torch.zeros(m, dtype=torch.float64, device=dev)
    with pytest.raises(RuntimeError, match="f16"):
        ext.ppa_fused_acc(*s["args"], Ky, KK, 1, gen="f16")
    ok = _setup(c, m, d, 0, "uniform", dev)
    with pytest.raises(RuntimeError, match="f16"):
        ext.ppa_fused_acc(*ok["args"], Ky, KK, 1, gen="f16", absmax=7e4)
    with pytest.raises(RuntimeError, match="gen must be"):
        ext.ppa_fused_acc(*ok["args"], Ky, KK, 1, gen="bf16")
    torch.cuda.synchronize()
    assert not KK.any() and not Ky.any()


def test_auto_in_range_is_f16(dev, ext):
    c, m, d, split_k = 513, 130, 5, 1
    s = _setup(c, m, d, 0, "uniform", dev)
    KKa, _ = _fused(ext, s, m, split_k, 0, dev)
    KKb, _ = _fused(ext, s, m, split_k, 0, dev, absmax=2.0)
    KK16, _ = _fused(ext, s, m, split_k, 0, dev, gen="f16")
    torch.cuda.synchronize()
    assert torch.equal(KKa, KK16) and torch.equal(KKb, KK16)


@pytest.mark.parametrize("c,m,d,split_k", [(513, 130, 5, 3),
                                           (8192, 1000, 32, 25)])
def test_f16_is_deterministic(dev, ext, c, m, d, split_k):
    """Two calls on the same inputs give the same KK bits, for any number of
    k-slices: the slices are summed in a fixed order."""
    s = _setup(c, m, d, 0, "uniform", dev)
    KK1, Ky1 = _fused(ext, s, m, split_k, 0, dev, gen="f16")
    KK2, Ky2 = _fused(ext, s, m, split_k, 0, dev, gen="f16")
    torch.cuda.synchronize()
    assert torch.equal(KK1, KK2)

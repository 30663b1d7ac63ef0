"""GPU tests of the fused PPA accumulation (``ppa_fused_acc``): the SYRK
that generates its K_nm operand windows in the block, against the fp64
oracle and against the two-kernel pair (``cross_mfma_ppa`` +
``syrk_bf16_acc``) on the same inputs."""

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


# (c, m, d, split_k): what each exercises
CASES = [
    # second window partly filled; c not a multiple of 32
    (1000, 300, 8, 1),
    # d not a multiple of 4; odd c; a single diagonal tile
    (513, 130, 5, 3),
    # c smaller than one k-block (most slices empty); a window with one
    # real column
    (31, 257, 32, 4),
    # the headline tile set: 4 windows, 10 tiles
    (8192, 1000, 32, 1),
    (8192, 1000, 32, 25),
]

_SETUPS = {}


def _setup(c, m, d, dev):
    """Inputs and the fp64 CPU reference of one shape, built once and shared
    by every test and split_k that uses the shape (never modified)."""
    key = (c, m, d)
    if key not in _SETUPS:
        from spark_gp_amd.kernels import ARDRBFKernel
        g = torch.Generator().manual_seed(1000 * c + 10 * m + d)
        X = torch.rand(c, d, generator=g)
        A = torch.rand(m, d, generator=g)
        y = torch.rand(c, generator=g)
        beta = torch.rand(d, generator=g) + 0.5
        amp = 1.3
        kernel = amp * ARDRBFKernel(beta.numpy())
        K = kernel.cross_kernel(X.double(), A.double())       # [c, m] fp64
        KK_ref = K.T @ K
        Ky_ref = K.T @ y.double()
        Xs = (X * beta).to(dev).contiguous()
        As = (A * beta).to(dev).contiguous()
        nx = (Xs * Xs).sum(-1).contiguous()
        na = (As * As).sum(-1).contiguous()
        _SETUPS[key] = dict(Xs=Xs, As=As, nx=nx, na=na, y=y.to(dev), amp=amp,
                            KK_ref=KK_ref, Ky_ref=Ky_ref)
    return _SETUPS[key]


def _offdiag_tile_mask(m):
    t = torch.arange(m) // 256
    return t[:, None] != t[None, :]


@pytest.mark.parametrize("c,m,d,split_k", CASES)
def test_fused_vs_oracle_and_pair(dev, ext, c, m, d, split_k):
    """KK and Ky of the fused kernel against the fp64 reference and the
    two-kernel pair.

    Symmetry: both kernels write an off-diagonal tile and its mirror from
    the same register values, so with at most two addends per element
    (fp32 addition of two terms onto zero is order-independent) the
    off-diagonal tiles are symmetric to the last bit; with more k-slices the
    atomic order may differ between an element and its mirror, so there the
    fused result is required to be bit-symmetric whenever the pair's is."""
    s = _setup(c, m, d, dev)
    assert ext.ppa_fused_supported(m, d)
    Xs, As, nx, na, y, amp = (s[k] for k in ("Xs", "As", "nx", "na", "y",
                                             "amp"))
    KK_ref, Ky_ref = s["KK_ref"], s["Ky_ref"]

    KK_f = torch.zeros(m, m, dtype=torch.float32, device=dev)
    Ky_f = torch.zeros(m, dtype=torch.float64, device=dev)
    ext.ppa_fused_acc(Xs, As, nx, na, amp, y, Ky_f, KK_f, split_k)

    KK_p = torch.zeros(m, m, dtype=torch.float32, device=dev)
    Ky_p = torch.zeros(m, dtype=torch.float64, device=dev)
    KcT, KlT = ext.cross_mfma_ppa(Xs, As, nx, na, amp, y, Ky_p)
    ext.syrk_bf16_acc(KcT, KlT, KK_p, split_k)
    torch.cuda.synchronize()

    scale = float(KK_ref.abs().max())
    err_f = float((KK_f.cpu().double() - KK_ref).abs().max())
    err_p = float((KK_p.cpu().double() - KK_ref).abs().max())
    print(f"(c,m,d,split_k)={(c, m, d, split_k)} scale={scale:.4e} "
          f"err_fused={err_f:.4e} err_pair={err_p:.4e}")
    # K is bounded at 5e-5 elementwise (test_cross_mfma_ppa_vs_oracle); KK
    # is bilinear in K, so the bound doubles
    assert err_f < 1e-4 * scale, (err_f, scale)
    # same products, different summation order
    assert err_f < 4 * max(err_p, 1e-30), (err_f, err_p)

    # symmetry
    off = _offdiag_tile_mask(m)
    f_c, p_c = KK_f.cpu(), KK_p.cpu()
    f_sym = bool((f_c == f_c.T)[off].all())
    p_sym = bool((p_c == p_c.T)[off].all())
    kblocks = (c + 31) // 32
    per = -(-kblocks // split_k)
    addends = -(-kblocks // per)
    print(f"  k-slices with rows: {addends}  off-diagonal tiles bit-symmetric:"
          f" fused={f_sym} pair={p_sym}")
    if addends <= 2:
        assert p_sym and f_sym
    elif p_sym:
        assert f_sym

    ky_err = float((Ky_f.cpu() - Ky_ref).abs().max())
    print(f"  Ky max abs err fused={ky_err:.3e} "
          f"pair={float((Ky_p.cpu() - Ky_ref).abs().max()):.3e}")
    torch.testing.assert_close(Ky_f.cpu(), Ky_ref, rtol=1e-4, atol=1e-4)

    # accumulation: a second call doubles KK and Ky
    KK_1, Ky_1 = KK_f.clone(), Ky_f.clone()
    ext.ppa_fused_acc(Xs, As, nx, na, amp, y, Ky_f, KK_f, split_k)
    torch.cuda.synchronize()
    # 2x up to the rounding of the atomic adds onto a non-zero value
    torch.testing.assert_close(KK_f, 2 * KK_1, rtol=1e-5, atol=1e-5 * scale)
    torch.testing.assert_close(Ky_f, 2 * Ky_1, rtol=1e-12, atol=1e-12)


def test_fused_rejects_unsupported(dev, ext):
    assert not ext.ppa_fused_supported(1000, 33)
    assert not ext.ppa_fused_supported(6000, 32)      # 24 windows: 300 tiles
    Xs = torch.rand(64, 33, device=dev)
    As = torch.rand(10, 33, device=dev)
    with pytest.raises(RuntimeError):
        ext.ppa_fused_acc(Xs, As, torch.zeros(64, device=dev),
                          torch.zeros(10, device=dev), 1.0,
                          torch.zeros(64, device=dev),
                          torch.zeros(10, dtype=torch.float64, device=dev),
                          torch.zeros(10, 10, device=dev), 1)


def test_ppa_stats_fused_vs_two_kernel(dev, ext, monkeypatch):
    """End to end through hip_backend.kmn_knm_and_kmny (mixed precision):
    fused default against SPARK_GP_AMD_PPA_FUSED=0, inputs and tolerance of
    test_ppa_stats_hip_vs_torch."""
    from spark_gp_amd.kernels import ARDRBFKernel, EyeKernel, Scalar
    from spark_gp_amd.ops import hip_backend, torch_backend
    from spark_gp_amd.ops.ppa_gate import ppa_fused_chunk_rows
    g = torch.Generator().manual_seed(7)
    X = torch.rand(20000, 16, generator=g).to(dev)
    y = torch.sin(X.sum(-1)).to(dev)
    active = X[:200].clone()
    kernel = 1 * ARDRBFKernel(16) + Scalar(1e-3).const * EyeKernel()
    kernel.set_hyperparameters(
        np.concatenate([[1.2], np.random.default_rng(8).uniform(0.5, 2, 16)]))
    KK_t, Ky_t = torch_backend.kmn_knm_and_kmny(kernel, active.double().cpu(),
                                                X.double().cpu(),
                                                y.double().cpu())

    calls = []
    real = ext.ppa_fused_acc

    class _Spy:
        def __getattr__(self, name):
            if name == "ppa_fused_acc":
                def f(*a, **kw):
                    calls.append(1)
                    return real(*a, **kw)
                return f
            return getattr(ext, name)

    monkeypatch.setattr(hip_backend, "ext", _Spy())
    out = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("SPARK_GP_AMD_PPA_FUSED", flag)
        before = len(calls)
        KK_h, Ky_h = hip_backend.kmn_knm_and_kmny(
            kernel, active, X, y, chunk_rows=8192, precision="mixed")
        # the switch really selects the path (one fused launch per chunk)
        nchunk = -(-X.shape[0] // ppa_fused_chunk_rows(8192))
        assert len(calls) - before == (nchunk if flag == "1" else 0)
        np.testing.assert_allclose(KK_h.cpu().numpy(), KK_t.numpy(),
                                   rtol=2e-2,
                                   atol=2e-2 * float(KK_t.abs().max()))
        np.testing.assert_allclose(Ky_h.cpu().numpy(), Ky_t.numpy(),
                                   rtol=2e-2,
                                   atol=2e-2 * float(Ky_t.abs().max()))
        out[flag] = (KK_h.cpu(), Ky_h.cpu())
    dk = float((out["1"][0] - out["0"][0]).abs().max())
    print(f"fused vs two-kernel: max |dKK| = {dk:.3e} "
          f"(scale {float(KK_t.abs().max()):.3e})")

"""GPU tests of how ``ppa_fused_acc`` adds its k-slices into KK: every block
stores its tile of partial sums into a buffer of its own and one reduction
adds the slices to KK in ascending order, so KK is reproducible to the bit
and an off-diagonal tile equals its mirror for every split_k."""

import pytest
import torch

pytestmark = pytest.mark.gpu

D = 8
AMP = 1.3


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ext():
    from spark_gp_amd import _hip_ext
    return _hip_ext


_INPUTS = {}


def _inputs(c, m, dev):
    """(Xs, As, nx, na, amp, y) of one shape, built once and never modified."""
    if (c, m) not in _INPUTS:
        g = torch.Generator().manual_seed(100 * c + m)
        Xs = (torch.rand(c, D, generator=g) * 1.2).to(dev)
        As = (torch.rand(m, D, generator=g) * 1.2).to(dev)
        _INPUTS[(c, m)] = (Xs, As, (Xs * Xs).sum(-1), (As * As).sum(-1), AMP,
                           torch.rand(c, generator=g).to(dev))
    return _INPUTS[(c, m)]


def _acc(ext, args, m, split_k, dev, KK=None, **kw):
    if KK is None:
        KK = torch.zeros(m, m, dtype=torch.float32, device=dev)
    Ky = torch.zeros(m, dtype=torch.float64, device=dev)
    ext.ppa_fused_acc(*args, Ky, KK, split_k, **kw)
    return KK


# c = 31: one k-block, so all slices but the first are empty
@pytest.mark.parametrize("m", [130, 1000])
@pytest.mark.parametrize("c", [31, 8192])
@pytest.mark.parametrize("split_k", [1, 3, 25, 64])
def test_reproducible_symmetric_accumulating(dev, ext, split_k, c, m):
    args = _inputs(c, m, dev)
    KK1 = _acc(ext, args, m, split_k, dev)
    KK2 = _acc(ext, args, m, split_k, dev)
    assert torch.equal(KK1, KK2)

    # an off-diagonal tile and its mirror receive the same sums; inside a
    # diagonal tile (i, j) and (j, i) are separate dot products
    t = torch.arange(m, device=dev) // 256
    off = t[:, None] != t[None, :]
    assert bool((KK1 == KK1.T)[off].all())
    assert float(KK1.abs().max()) > 0.0

    # a second call onto the first result doubles it, up to the rounding of
    # the one add onto a non-zero value
    scale = float(KK1.abs().max())
    KK3 = _acc(ext, args, m, split_k, dev, KK=KK1.clone())
    torch.testing.assert_close(KK3, 2 * KK1, rtol=1e-5, atol=1e-5 * scale)

    # a caller's buffer, full of NaN where no block writes, changes nothing
    numel = ext.ppa_fused_partials_numel(c, m, split_k)
    part = torch.full((numel,), float("nan"), device=dev)
    KK4 = _acc(ext, args, m, split_k, dev, partials=part)
    assert torch.equal(KK4, KK1)
    # ... and may be larger than needed
    part = torch.full((numel + 1000,), float("nan"), device=dev)
    assert torch.equal(_acc(ext, args, m, split_k, dev, partials=part), KK1)


def test_partials_numel(ext):
    tile = 256 * 256
    # slices with rows x upper-triangle tiles x tile
    assert ext.ppa_fused_partials_numel(31, 130, 25) == 1 * 1 * tile
    assert ext.ppa_fused_partials_numel(8192, 1000, 25) == 24 * 10 * tile
    assert ext.ppa_fused_partials_numel(8192, 1000, 64) == 64 * 10 * tile
    assert ext.ppa_fused_partials_numel(8192, 130, 1) == 1 * 1 * tile


def test_partials_argument_checks(dev, ext):
    c, m, split_k = 8192, 130, 3
    args = _inputs(c, m, dev)
    numel = ext.ppa_fused_partials_numel(c, m, split_k)
    KK = torch.zeros(m, m, dtype=torch.float32, device=dev)
    Ky = torch.zeros(m, dtype=torch.float64, device=dev)
    with pytest.raises(RuntimeError, match="partials must have at least"):
        ext.ppa_fused_acc(*args, Ky, KK, split_k,
                          partials=torch.empty(numel - 1, device=dev))
    with pytest.raises(RuntimeError, match="partials must be"):
        ext.ppa_fused_acc(*args, Ky, KK, split_k,
                          partials=torch.empty(numel, dtype=torch.float64,
                                               device=dev))
    with pytest.raises(RuntimeError, match="partials must be on the GPU"):
        ext.ppa_fused_acc(*args, Ky, KK, split_k,
                          partials=torch.empty(numel))
    with pytest.raises(RuntimeError, match="partials must be contiguous"):
        ext.ppa_fused_acc(*args, Ky, KK, split_k,
                          partials=torch.empty(2 * numel, device=dev)[::2])
    torch.cuda.synchronize()
    assert not KK.any() and not Ky.any()

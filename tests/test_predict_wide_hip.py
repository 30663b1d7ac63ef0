"""The wide fused predict kernel (predict_wide.hip) and ``stream="wide"``.

Oracle and bound are those of test_predict_hip.py: the fp64 CPU cross kernel
c, ``c @ mv`` and ``kxx + ((c @ M) * c).sum(-1)``, with the cross-kernel
tolerance d_rj = 1e-4 |c_rj| + 1e-5 pushed exactly through both formulas.  A
wrong fragment map or a stale scratch slot is off by the value itself.
"""

import pytest
import torch

from tests.test_predict_hip import (_BASE, _bounds, _check, _kernel, _oracle,
                                    _random_predictor, dev, ext)  # noqa: F401
from tests.test_predict_stream import CHUNK, _FakeExt, _predictor

R, P = 128, 64        # PPW_R, PPW_P of kernel_geom.h

# (t, m, d, max_blocks).  t: one row, a tile less one, a tile, a tile plus one,
# and 3R+5 rows on one block (its slab reused by four tiles) and on two;
# m: below, at and above the 16-column MFMA tile and the P-deep panel of M, and
# 2P+3 (three column panels of up to three k panels); d: around the 32-wide
# d-pass.
SHAPES = [(1, 1, 1, 0), (R - 1, 15, 32, 0), (R, 16, 33, 0), (R + 1, 17, 1, 0),
          (R + 1, P, 32, 0), (R, P + 1, 33, 0), (R - 1, 2 * P + 3, 32, 0),
          (1, 2 * P + 3, 33, 0), (3 * R + 5, 2 * P + 3, 33, 1),
          (3 * R + 5, 2 * P + 3, 33, 2), (3 * R + 5, P + 1, 1, 1),
          (3 * R + 5, 17, 32, 2)]
CASES = ([("ard", s) for s in SHAPES]
         + [(b, (3 * R + 5, 2 * P + 3, 33, 1)) for b in _BASE if b != "ard"])


def _problem(t, m, d):
    g = torch.Generator().manual_seed(1000 * t + m + d)
    X, A = torch.rand(t, d, generator=g), torch.rand(m, d, generator=g)
    M = torch.randn(m, m, generator=g, dtype=torch.float64)
    return X, A, torch.randn(m, generator=g, dtype=torch.float64), 0.5 * (M + M.T)


@pytest.mark.gpu
@pytest.mark.parametrize(
    "base,shape", CASES, ids=[f"{b}-{'x'.join(map(str, s))}" for b, s in CASES])
def test_wide_kernel_vs_fp64_oracle(base, shape, dev, ext):
    from spark_gp_amd.ops import hip_backend
    t, m, d, max_blocks = shape
    assert ext.ppa_predict_wide_supported(m, d)
    X, A, mv, M = _problem(t, m, d)
    kernel = _kernel(base, d)
    c, mean_o, var_o = _oracle(kernel, X, A, mv, M)
    bm, bv = _bounds(c, mv, M)
    dv = [v.to(dev) for v in (X, A, mv, M)]
    assert hip_backend.supports_predict_wide(kernel, dv[0], m)
    mean, var = hip_backend.predict_wide(kernel, *dv, True, max_blocks)
    assert mean.dtype == var.dtype == torch.float64
    assert mean.shape == var.shape == (t,)
    _check("mean", mean, mean_o, bm)
    _check("var", var, var_o, bv)
    if shape == SHAPES[-4]:
        mean1, none = hip_backend.predict_wide(kernel, *dv, False, max_blocks)
        assert none is None
        _check("mean (mean-only)", mean1, mean_o, bm)


@pytest.mark.gpu
def test_stream_wide_past_the_narrow_gate(dev, ext, monkeypatch):
    from spark_gp_amd.ops import hip_backend
    t, m, d = 130, 2256, 3
    assert not ext.ppa_predict_supported(m, d)
    raw = _random_predictor(m, d, dev)
    X = torch.rand(t, d, generator=torch.Generator().manual_seed(5))
    c, mean_o, var_o = _oracle(raw.kernel, X, raw.active_set,
                               raw.magic_vector, raw.magic_matrix)
    bm, bv = _bounds(c, raw.magic_vector.cpu(), raw.magic_matrix.cpu())
    calls, real = [], hip_backend.predict_wide
    monkeypatch.setattr(hip_backend, "predict_wide",
                        lambda *a, **k: calls.append(1) or real(*a, **k))
    mean, var = raw.predict(X.to(dev), stream="wide")
    assert calls == [1]
    _check("mean", mean, mean_o, bm)
    _check("var", var, var_o, bv)


@pytest.mark.gpu
def test_scratch_is_bounded_by_the_grid(dev, ext):
    """test_no_t_by_m_buffer's assertion: the peak rises by less than the
    fp32 cross matrix; four blocks' slabs are an eighth of it here."""
    from spark_gp_amd.ops import hip_backend
    t, m, d = 4096, 2256, 4
    raw = _random_predictor(m, d, dev)
    X = torch.rand(t, d, generator=torch.Generator().manual_seed(2)).to(dev)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    mean, var = hip_backend.predict_wide(
        raw.kernel, X, raw.active_set, raw.magic_vector, raw.magic_matrix,
        True, max_blocks=4)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print(f"peak rise {rise} B against t*m*4 = {t * m * 4} B")
    assert rise < t * m * 4
    assert bool(torch.isfinite(mean).all()) and bool(torch.isfinite(var).all())


class _FakeWideExt(_FakeExt):
    """_FakeExt with the wide gate and binding; records the gate order."""

    def __init__(self, narrow, wide):
        super().__init__(narrow)
        self.wide, self.order = wide, []

    def ppa_predict_supported(self, m, d):
        self.order.append("narrow")
        return super().ppa_predict_supported(m, d)

    def ppa_predict_wide_supported(self, m, d):
        self.order.append("wide")
        return self.wide

    def ppa_predict_wide(self, *a, family=0, max_blocks=0):
        self.order.append("wide call")
        return super().ppa_predict(*a, family=family)


@pytest.mark.parametrize("narrow,wide,stream,order", [
    (True, True, "wide", ["narrow"]),
    (False, True, "wide", ["narrow", "wide", "wide call"]),
    (False, False, "wide", ["narrow", "wide"]),
    (False, True, True, ["narrow"]),
])
def test_gate_order(narrow, wide, stream, order, monkeypatch):
    from spark_gp_amd import ops
    from spark_gp_amd.ops import hip_backend
    raw, cs, theta, X = _predictor("ard_m52")
    fake = _FakeWideExt(narrow, wide)
    monkeypatch.setattr(hip_backend, "ext", fake)
    real = ops._backend_for
    monkeypatch.setattr(
        ops, "_backend_for", lambda what, t, required=True: hip_backend
        if what == "predict_stream" else real(what, t, required))
    mean, var = raw.predict(X, stream=stream, chunk_rows=CHUNK)
    assert fake.order == order
    assert len(fake.calls) == (1 if narrow or "wide call" in order else 0)
    want_mean, want_var = raw.predict(X)
    # fp32 X against the default path: test_gate_selects_fused_or_chunked
    torch.testing.assert_close(mean, want_mean, rtol=1e-5, atol=1e-4)
    torch.testing.assert_close(var, want_var, rtol=1e-5, atol=1e-4)
    with pytest.raises(ValueError, match="stream"):
        raw.predict(X, stream="narrow")

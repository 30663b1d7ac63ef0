"""Phase L of the expert kernel (lauum, K^-1 = V^T V on f32 MFMA): each
tile's sum starts at its own tile row, the masked LDS fragments are fetched
four steps at a time with no load under a lane condition, and two tiles of
a wave advance together.  Only phase L differs from the kernel before it;
the loops of the same shape around it (the panel solve C2 and the
off-diagonal inverse D in chol_invert_lower, phase H's W0 fragments) are
unchanged, and the shapes below also walk their tile edges.

Parity with the fp64 oracle at the sizes where a trimmed range or a batch
tail can go wrong, one Matern front (its upper-triangle cache holds t, not
Kb, so a fragment read that strays over the diagonal shows), the Laplace
kernels, which share chol_invert_lower, bitwise repeatability where a wave
owns two tiles, and the breakdown path behind a panel solve.  Every case
passes on the kernel before the change as well."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

AMP, NOISE = 1.1, 1e-2


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ext():
    from spark_gp_amd import _hip_ext
    return _hip_ext


def _coupled(E, k, d, seed, dev):
    """tests/test_diag_block_inverse.py's construction: inverse length
    scales small enough that every point sees every other.  In fp64 its
    condition number is at most 9.0e3 at every shape used here, and a
    float32 Cholesky succeeds on every expert."""
    g = torch.Generator().manual_seed(seed)
    X = torch.rand(E, k, d, generator=g).to(dev)
    y = torch.sin(3.0 * X.sum(-1)).to(dev)
    rng = np.random.default_rng(seed)
    beta = rng.uniform(0.1, 0.4, d) * (32.0 / d) ** 0.5
    return X, y, beta


# d = 8, k = 15, 16, 17: one tile, then two (L only).
# d = 32: 33, 36, 37: a second block of 1, 4, 5 rows, D's U loop of one
# step, a batch tail of 1; 48, 49, 52: a tile edge inside the second block;
# 64, 65, 68: two to three blocks, a wave with two D tiles; 80 .. 128: up to
# 36 L tiles (5 per wave), the largest C2 with two tiles per wave.
# (100, 128), (128, 128): H with eight column tiles; (40, 17): d % 4 != 0.
PARITY_SHAPES = (
    [(k, 8) for k in (15, 16, 17)]
    + [(k, 32) for k in (33, 36, 37, 48, 49, 52, 64, 65, 68, 80, 81, 84, 96,
                         97, 100, 112, 113, 128)]
    + [(100, 128), (128, 128), (40, 17)])


@pytest.mark.parametrize("k,d", PARITY_SHAPES)
def test_parity_with_fp64_oracle(dev, ext, k, d):
    from spark_gp_amd.kernels import (ARDRBFKernel, EyeKernel, Scalar,
                                      compile_kernel)
    from spark_gp_amd.ops import hip_backend, torch_backend
    E = 6
    X, y, beta = _coupled(E, k, d, seed=41, dev=dev)
    cs = compile_kernel(1 * ARDRBFKernel(d) + Scalar(NOISE).const * EyeKernel())
    theta = np.concatenate([[AMP], beta])
    scale = torch.as_tensor(beta, dtype=torch.float32, device=dev)
    *_, bad = ext.fused_expert_nll(X, y, scale, AMP, NOISE)
    assert int(bad.sum()) == 0, "experts fell back: kernel not exercised"
    nll_h, grad_h = hip_backend.nll_grad_compiled(cs, theta, X, y)
    nll_o, grad_o = torch_backend.nll_grad_compiled(
        cs, theta, X.double().cpu(), y.double().cpu())
    gmax = np.abs(grad_o).max()
    print(f"\n(k={k}, d={d}): nll rel err "
          f"{abs(nll_h - nll_o) / abs(nll_o):.3e}, grad max abs err / "
          f"max|grad| {np.abs(grad_h - grad_o).max() / gmax:.3e}")
    assert nll_h == pytest.approx(nll_o, rel=2e-4)
    np.testing.assert_allclose(grad_h, grad_o, rtol=3e-3, atol=2e-3 * gmax)


def test_matern52_front_across_two_blocks(dev, ext):
    """ard_m52 at (E, k, d) = (6, 65, 32), with the inputs, the oracle and
    the tolerances of tests/test_matern_hip.py."""
    from tests.test_matern_hip import test_fused_expert_nll_matern_vs_oracle
    test_fused_expert_nll_matern_vs_oracle(dev, ext, "ard_m52", 6, 65, 32)


@pytest.mark.parametrize("k", [36, 65, 100])
def test_laplace_kernels_share_the_loops(dev, ext, k):
    """fused_laplace_newton and fused_laplace_evidence from a cold start,
    E = 8, against tests/test_laplace_hip.py's oracles with its error
    measure and bounds: the latent against the fp64 mode, the evidence
    groups against the fp64 evidence at the mode, each bound scaled by what
    the generic path does in float32 on the same inputs."""
    from spark_gp_amd.ops import torch_backend as tb
    from tests import test_laplace_hip as tl
    E, d = 8, 8
    amp, noise = {36: (1.0, 1e-2), 65: (3.0, 1e-3), 100: (0.5, 0.1)}[k]
    c = tl.make_inputs(E, k, d, "ard", amp, noise, seed=4100 + k)
    fstar = tl.fp64_mode(c)
    ev64 = tl.evidence_groups(c, *tb.laplace_evidence_experts(
        c.cs, c.theta, c.X64, c.y64, fstar))
    f32 = torch.zeros(E, k)
    tb.laplace_nll_grad(c.kern, c.theta, c.X, c.y, f32, tl.TOL,
                        max_newton_iter=40)
    ev32 = tl.evidence_groups(c, *tb.laplace_evidence_experts(
        c.cs, c.theta, c.X, c.y, f32))
    f0 = torch.zeros(E, k)
    psi, sll, iters, bad, f_out = tl.run_kernel(
        ext.fused_laplace_newton, c, dev, f0, tl.TOL, 40)
    assert (bad == 0).all(), bad
    assert ((iters >= 1) & (iters <= 40)).all(), iters
    fails = []
    what = f"feed k={k} d={d}"
    tl.check_scaled(what, "f", tl.abs_err(f_out, fstar),
                    tl.abs_err(f32, fstar), tl.FLOOR_MODE, fails)
    logz, grad, iters_ev, bad_ev, f_ev = tl.run_kernel(
        ext.fused_laplace_evidence, c, dev, f0, tl.TOL, 40)
    assert (bad_ev == 0).all(), bad_ev
    assert torch.equal(iters_ev, iters)
    assert torch.equal(f_ev.view(torch.int32), f_out.view(torch.int32))
    tl.check_evidence(what, tl.evidence_groups(c, logz, grad), ev64, ev32,
                      fails)
    assert not fails, "\n".join(fails)


# three experts resident on each of the 256 CUs, one round; at k = 68 and
# k = 100 a wave owns up to four tiles in L (two pairs) and two in C2 and D
@pytest.mark.parametrize("k,d,E", [(68, 32, 768), (100, 32, 768)])
def test_batched_loops_are_race_free(dev, ext, k, d, E):
    """A missing barrier, or a tile written back before its last reader,
    shows as a bitwise difference between two launches, or between the
    batch and its first 8 experts launched alone."""
    X, y, beta = _coupled(E, k, d, seed=42, dev=dev)
    scale = torch.as_tensor(beta, dtype=torch.float32, device=dev)
    first = ext.fused_expert_nll(X, y, scale, AMP, NOISE)
    again = ext.fused_expert_nll(X, y, scale, AMP, NOISE)
    alone = ext.fused_expert_nll(X[:8], y[:8], scale, AMP, NOISE)
    assert len(first) == 5
    assert int(first[4].sum()) == 0
    for a, b, c in zip(first, again, alone):
        assert torch.equal(a, b)
        assert torch.equal(a[:8], c)


def test_breakdown_behind_a_panel_is_wave_uniform(dev, ext):
    """tests/test_diag_block_inverse.py's breakdown construction (K exactly
    I plus one 2x2 block of ones at rows (r, r+1)) at k = 68 with the
    repeated row at r = 40, inside the second block behind one C2 panel,
    and at r = 66, in the short third block behind two: flag 1, zero
    outputs, and the control expert bitwise what it is alone."""
    k, d, rs = 68, 4, [40, 66]
    E = len(rs) + 1
    X = torch.zeros(E, k, d)
    X[:, :, 0] = 20.0 * torch.arange(k, dtype=torch.float32)
    g = torch.Generator().manual_seed(43)
    y = torch.randn(E, k, generator=g)
    for e, r in enumerate(rs):
        X[e, r + 1] = X[e, r]
        y[e, r + 1] = y[e, r]
    X, y = X.to(dev), y.to(dev)
    scale = torch.ones(d, device=dev)
    nll, sw, trg, contr, bad = ext.fused_expert_nll(X, y, scale, 1.0, 0.0)
    ctl = E - 1
    assert bad.tolist() == [1] * len(rs) + [0]
    for e in range(len(rs)):
        assert float(nll[e]) == 0.0 and float(sw[e]) == 0.0
        assert float(trg[e]) == 0.0
        assert int(torch.count_nonzero(contr[e])) == 0
    alone = ext.fused_expert_nll(X[ctl:], y[ctl:], scale, 1.0, 0.0)
    assert int(alone[4][0]) == 0
    for a, b in zip((nll, sw, trg, contr), alone[:4]):
        assert torch.equal(a[ctl:], b)

"""The inverse of each 32x32 diagonal block in chol_invert_lower: every 8x8
sub-block factored and inverted by one 8-step elimination, and the block's
inverse assembled from the 8x8 inverses by recursive doubling (pairs of
sub-blocks, then the two 16-row halves) on the matrix pipe.

Parity with the fp64 oracle at the block sizes where the assembly changes
shape (one, two, three sub-blocks, short last sub-blocks, the same behind a
full block), breakdown classification at chosen pivots in exact arithmetic
and for non-finite inputs, bitwise repeatability at those sizes, and the
Laplace kernel, which calls the same function."""

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
    """Experts whose kernel matrix has a median off-diagonal of 0.74-0.85
    of the diagonal: the inverse length scales are small enough that every
    point sees every other (tests/test_chol_diag_wave.py's construction)."""
    g = torch.Generator().manual_seed(seed)
    X = torch.rand(E, k, d, generator=g).to(dev)
    y = torch.sin(3.0 * X.sum(-1)).to(dev)
    rng = np.random.default_rng(seed)
    beta = rng.uniform(0.1, 0.4, d) * (32.0 / d) ** 0.5
    return X, y, beta


# 4, 12: a partial sub-block alone and behind one full one (no assembly,
# level 1 with a short high block); 16: level 1 alone; 17, 23, 24: level 2
# with a 1-, 7- and 8-row high half; 25: four sub-blocks, the last of one
# row; 48, 56, 57: the same in the second block, behind a C2 panel
@pytest.mark.parametrize("k", [4, 12, 16, 17, 23, 24, 25, 48, 56, 57])
def test_parity_with_fp64_oracle_at_assembly_edges(dev, ext, k):
    from spark_gp_amd.kernels import (ARDRBFKernel, EyeKernel, Scalar,
                                      compile_kernel)
    from spark_gp_amd.ops import hip_backend, torch_backend
    E, d = 6, 8
    X, y, beta = _coupled(E, k, d, seed=31, dev=dev)
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


# k = 100: the first pivot pair, inside a sub-block, the first rows of the
# second sub-block (8: its first pivot pair; 14: inside it), the last row
# of block 3 with the first of the short block, inside the short block;
# k = 12: the partial sub-block
@pytest.mark.parametrize("k,rs", [(100, [0, 3, 8, 14, 95, 96]), (12, [9])])
def test_breakdown_at_chosen_pivot_fused_step(dev, ext, k, rs):
    """K is exactly I plus one 2x2 block of ones at rows (r, r+1): points at
    20*a on the first axis, expert e repeats row r as row r+1 (the
    construction of test_breakdown_at_chosen_pivot).  Every pivot before
    r+1 is exactly 1 and pivot r+1 exactly 0, whichever way the 8x8 step
    orders its arithmetic: the multiplier is 1 * (1 * 1)."""
    d = 4
    E = len(rs) + 1
    X = torch.zeros(E, k, d)
    X[:, :, 0] = 20.0 * torch.arange(k, dtype=torch.float32)
    g = torch.Generator().manual_seed(33)
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


def test_nonfinite_features_raise_the_flag(dev, ext):
    """A NaN and an Inf feature, each in one expert among good ones: the
    expert is flagged, its outputs are zero, and the other experts are
    bitwise what the clean batch gives.  The value of the flag is not
    asserted to be 2: the kernel build clamps the squared distance with
    `q > 0 ? q : 0`, which sends a NaN distance to 0 and the kernel value to
    1, so the factorization meets a vanished pivot (flag 1), never a
    non-finite one.  That is what the kernel did before the fused 8x8 step
    and the doubled assembly, and does with them: bad = [0, 1, 0, 0, 1, 0]
    in both.  No feature value reaches flag 2 through this entry point."""
    E, k, d = 6, 24, 8
    X, y, beta = _coupled(E, k, d, seed=34, dev=dev)
    scale = torch.as_tensor(beta, dtype=torch.float32, device=dev)
    clean = ext.fused_expert_nll(X, y, scale, AMP, NOISE)
    assert int(clean[4].sum()) == 0
    Xb = X.clone()
    Xb[1, 5, 2] = float("nan")
    Xb[4, 20, 0] = float("inf")
    nll, sw, trg, contr, bad = ext.fused_expert_nll(Xb, y, scale, AMP, NOISE)
    print(f"\nbad = {bad.tolist()}")
    assert [b != 0 for b in bad.tolist()] == [False, True, False, False,
                                              True, False]
    for e in (1, 4):
        assert float(nll[e]) == 0.0 and float(sw[e]) == 0.0
        assert float(trg[e]) == 0.0
        assert int(torch.count_nonzero(contr[e])) == 0
    good = [0, 2, 3, 5]
    for a, b in zip((nll, sw, trg, contr), clean[:4]):
        assert torch.equal(a[good], b[good])


# three sub-blocks with a full-height high half, and the same behind one
# full block; three experts resident on each of the 256 CUs, one round
@pytest.mark.parametrize("k,d,E", [(24, 8, 768), (56, 8, 768)])
def test_assembly_is_race_free(dev, ext, k, d, E):
    """A missing wave-scope wait between the level-1 stores and level 2's
    read of them, or a missing block barrier behind the assembly, shows as a
    bitwise difference between two launches, or between the batch and its
    first 64 experts launched alone."""
    X, y, beta = _coupled(E, k, d, seed=32, dev=dev)
    scale = torch.as_tensor(beta, dtype=torch.float32, device=dev)
    first = ext.fused_expert_nll(X, y, scale, AMP, NOISE)
    again = ext.fused_expert_nll(X, y, scale, AMP, NOISE)
    alone = ext.fused_expert_nll(X[:64], y[:64], scale, AMP, NOISE)
    assert len(first) == 5
    assert int(first[4].sum()) == 0
    for a, b, c in zip(first, again, alone):
        assert torch.equal(a, b)
        assert torch.equal(a[:64], c)


@pytest.mark.parametrize("k", [17, 24, 56])
def test_laplace_kernel_at_assembly_edges(dev, ext, k):
    """fused_laplace_kernel calls the same chol_invert_lower: the Newton
    loop and the evidence launch against the fp64 torch oracle, with the
    inputs and tolerances of test_fused_laplace_newton_vs_torch and
    test_fused_laplace_evidence_vs_torch."""
    from spark_gp_amd.kernels import (ARDRBFKernel, EyeKernel, Scalar,
                                      compile_kernel)
    from spark_gp_amd.ops import hip_backend, torch_backend
    E, d = 8, 8
    kernel = 1 * ARDRBFKernel(d) + Scalar(1e-2).const * EyeKernel()
    cs = compile_kernel(kernel)
    theta = np.concatenate([[1.0], np.full(d, 0.8)])

    g = torch.Generator().manual_seed(4)
    X = torch.rand(E, k, d, generator=g).to(dev)
    y = (X.sum(-1) > d / 2).to(torch.float32)
    tol = 1e-6
    f_hip = torch.zeros(E, k, device=dev)
    n_bad = hip_backend.laplace_newton(cs, theta, X, y, f_hip, tol, 200)
    assert n_bad == 0, "fused Newton fell back"
    f_ref = torch.zeros(E, k, dtype=torch.float64)
    torch_backend.laplace_nll_grad(kernel, theta, X.double().cpu(),
                                   y.double().cpu(), f_ref, tol)
    print(f"\nk={k}: newton max |f - f_ref| "
          f"{np.abs(f_hip.cpu().numpy() - f_ref.numpy()).max():.3e}")
    np.testing.assert_allclose(f_hip.cpu().numpy(), f_ref.numpy(),
                               rtol=2e-3, atol=2e-3)

    g = torch.Generator().manual_seed(11)
    X = torch.rand(E, k, d, generator=g).to(dev)
    y = (X.sum(-1) > d / 2).to(torch.float32)
    tol = 1e-5                        # >= LAPLACE_MIN_TOL: fused path ok
    assert hip_backend.supports_laplace_evidence(cs, X)
    f_hip = torch.zeros(E, k, device=dev)
    res = hip_backend.laplace_evidence(cs, theta, X, y, f_hip, tol, 200)
    assert res is not None, "fp32 breakdown on a benign batch"
    nll_hip, grad_hip = res
    f_ref = torch.zeros(E, k, dtype=torch.float64)
    nll_ref, grad_ref = torch_backend.laplace_nll_grad(
        kernel, theta, X.double().cpu(), y.double().cpu(), f_ref, tol)
    print(f"k={k}: evidence nll rel err "
          f"{abs(nll_hip - nll_ref) / abs(nll_ref):.3e}, grad max abs err / "
          f"max|grad| "
          f"{np.abs(grad_hip - grad_ref).max() / np.abs(grad_ref).max():.3e}")
    assert nll_hip == pytest.approx(nll_ref, rel=1e-3)
    np.testing.assert_allclose(grad_hip, grad_ref, rtol=2e-2,
                               atol=1e-3 * np.abs(grad_ref).max())
    np.testing.assert_allclose(f_hip.cpu().numpy(), f_ref.numpy(),
                               rtol=2e-3, atol=2e-3)

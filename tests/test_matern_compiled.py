"""The Matérn families on the compiled (fused-objective) path, on the CPU in
fp64: canonicalization of the four Matérn bases, the fp64 oracle
``torch_backend.nll_grad_compiled`` against the materialized-derivative
generic path, the ARD classes' derivatives and model IO, and
``hip_backend``'s host chain rule over a fake extension (in the manner of
``test_hip_backend_host_logic.py``)."""

import math

import numpy as np
import pytest
import torch

from spark_gp_amd import ARDMatern32Kernel as RootARDMatern32Kernel
from spark_gp_amd.kernels import (ARDMatern32Kernel, ARDMatern52Kernel,
                                  EyeKernel, Matern32Kernel, Matern52Kernel,
                                  RBFKernel, Scalar, WhiteNoiseKernel,
                                  compile_kernel, sqdist)
from spark_gp_amd.kernels.compiled import BASES as COMPILED_BASES
from spark_gp_amd.kernels.compiled import (FAM_M32, FAM_M52, base_family,
                                           base_is_ard, base_nup, base_scale,
                                           base_scale_grad)
from spark_gp_amd.ops import hip_backend, torch_backend
from tests.test_kernels import fd_gradient_check

# base -> (class, family code, nu', ARD)
BASES = {
    "m32": (Matern32Kernel, FAM_M32, 3.0, False),
    "m52": (Matern52Kernel, FAM_M52, 5.0, False),
    "ard_m32": (ARDMatern32Kernel, FAM_M32, 3.0, True),
    "ard_m52": (ARDMatern52Kernel, FAM_M52, 5.0, True),
}
SHAPES = [(4, 13, 5), (3, 33, 4)]


def _base_kernel(base, d, seed=5):
    cls, _, _, ard = BASES[base]
    if ard:
        return cls(np.random.default_rng(seed).uniform(0.5, 2.0, d))
    return cls(0.8)


def _tree(base, d):
    """C * Matern + trainable white noise + const * I, C = 0.9 trainable."""
    return (0.9 * _base_kernel(base, d) + WhiteNoiseKernel(0.05, 0, 1)
            + Scalar(1e-3).const * EyeKernel())


def _data(E, k, d):
    g = torch.Generator().manual_seed(100 * E + k + d)
    X = torch.rand(E, k, d, generator=g, dtype=torch.float64)
    return X, torch.sin(3 * X.sum(-1))


def test_exported_from_package_root():
    assert RootARDMatern32Kernel is ARDMatern32Kernel
    import spark_gp_amd
    assert spark_gp_amd.ARDMatern52Kernel is ARDMatern52Kernel


@pytest.mark.parametrize("base", list(BASES))
def test_compile_kernel_recognises_matern(base):
    cls, fam, nup, ard = BASES[base]
    d = 3
    p_base = d if ard else 1
    cs = compile_kernel(_tree(base, d))
    assert cs is not None
    assert cs.base == base
    # layout: [C, base hypers..., white noise]
    assert cs.amp_idx == 0
    assert cs.base_idx == slice(1, 1 + p_base)
    assert cs.noise_idx == [1 + p_base]
    assert cs.noise_const == pytest.approx(1e-3)
    assert cs.p == 2 + p_base
    assert (base_family(base), base_nup(base), base_is_ard(base)) == \
        (fam, nup, ard)
    # constant amplitude
    cs2 = compile_kernel(Scalar(2.5).const * _base_kernel(base, d)
                         + Scalar(1e-2).const * EyeKernel())
    assert cs2.base == base and cs2.amp_idx is None
    assert cs2.amp_const == 2.5 and cs2.noise_const == pytest.approx(1e-2)
    assert cs2.base_idx == slice(0, p_base) and cs2.noise_idx == []


def test_compile_kernel_two_bases_is_none():
    eye = Scalar(1e-3).const * EyeKernel()
    assert compile_kernel(2.0 * Matern32Kernel(1.0) + Matern52Kernel(2.0)
                          + eye) is None
    assert compile_kernel(Matern52Kernel(1.0) + RBFKernel(1.0)) is None
    assert compile_kernel(1 * ARDMatern52Kernel(2) + 1 * ARDMatern32Kernel(2)
                          + eye) is None


@pytest.mark.parametrize("base", list(BASES))
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_compiled_canonical_matches_tree(base, seed):
    """C*Kb + nu*I from the canonicalizer == direct DSL evaluation."""
    d, n = 3, 6
    k = _tree(base, d)
    cs = compile_kernel(k)
    assert cs is not None
    theta = k.get_hyperparameters()
    X = torch.as_tensor(np.random.default_rng(seed).normal(size=(n, d)))
    direct = k.training_kernel(X).numpy()
    s = torch.as_tensor(base_scale(base, theta[cs.base_idx], d))
    Xs = X * s
    Kb, _ = torch_backend.family_kb_kd(base_family(base), sqdist(Xs, Xs))
    canon = (cs.amp(theta) * Kb
             + cs.noise(theta) * torch.eye(n, dtype=X.dtype)).numpy()
    np.testing.assert_allclose(direct, canon, rtol=1e-12, atol=1e-14)


@pytest.mark.parametrize("base", COMPILED_BASES)
def test_base_scale_grad_is_the_transposed_jacobian(base):
    """base_scale_grad(g_s) against central differences of g_s . base_scale
    over the base hypers.  The map is linear or 1/length, so at a step of
    1e-6 theta the truncation error is ~1e-12 relative and the rounding
    error ~1e-10."""
    d = 3
    rng = np.random.default_rng(11)
    theta = rng.uniform(0.5, 2.0, d if base_is_ard(base) else 1)
    g_s = rng.standard_normal(d)
    got = base_scale_grad(base, theta, g_s)
    assert got.shape == theta.shape
    want = np.empty_like(theta)
    for i in range(theta.size):
        h = np.zeros_like(theta)
        h[i] = 1e-6 * theta[i]
        want[i] = (g_s @ base_scale(base, theta + h, d)
                   - g_s @ base_scale(base, theta - h, d)) / (2.0 * h[i])
    print(f"{base}: max rel {np.max(np.abs(got - want) / np.abs(want)):.2e}")
    np.testing.assert_allclose(got, want, rtol=1e-7)


@pytest.mark.parametrize("base", list(BASES))
@pytest.mark.parametrize("E,k,d", SHAPES)
def test_oracle_matches_generic(base, E, k, d):
    """The fused fp64 form == materialized derivatives + batched Cholesky."""
    X, y = _data(E, k, d)
    kernel = _tree(base, d)
    cs = compile_kernel(kernel)
    assert cs is not None and cs.base == base
    theta = kernel.get_hyperparameters()
    nll_c, grad_c = torch_backend.nll_grad_compiled(cs, theta, X, y)
    nll_g, grad_g = torch_backend.nll_grad_generic(kernel, theta, X, y)
    print(f"{base} {(E, k, d)}: nll rel "
          f"{abs(nll_c - nll_g) / abs(nll_g):.2e}, grad max rel "
          f"{np.max(np.abs(grad_c - grad_g) / np.abs(grad_g)):.2e}")
    assert nll_c == pytest.approx(nll_g, rel=1e-9)
    np.testing.assert_allclose(grad_c, grad_g, rtol=1e-9)


@pytest.mark.parametrize("cls", [ARDMatern32Kernel, ARDMatern52Kernel])
def test_ard_matern_derivative_fd(cls):
    X = torch.as_tensor(np.random.default_rng(3).normal(size=(5, 3)))
    fd_gradient_check(cls(np.array([0.5, 2.0, 1.1])), X)


@pytest.mark.parametrize("cls,nup", [(ARDMatern32Kernel, 3.0),
                                     (ARDMatern52Kernel, 5.0)])
def test_ard_matern_matches_isotropic(cls, nup):
    """Equal betas 1/l reproduce the isotropic class; layout and bounds are
    ARDRBFKernel's."""
    X = torch.as_tensor(np.random.default_rng(4).normal(size=(6, 3)))
    Z = X[:2] + 0.3
    iso = (Matern32Kernel if nup == 3.0 else Matern52Kernel)(0.8)
    ard = cls(3, beta=1.0 / 0.8)
    np.testing.assert_allclose(ard.training_kernel(X).numpy(),
                               iso.training_kernel(X).numpy(), atol=1e-12)
    np.testing.assert_allclose(ard.cross_kernel(Z, X).numpy(),
                               iso.cross_kernel(Z, X).numpy(), atol=1e-12)
    assert ard.num_hyperparameters == 3
    lo, hi = ard.hyperparameter_bounds()
    assert (lo == 0.0).all() and np.isinf(hi).all()
    assert torch.equal(ard.training_kernel_diag(X),
                       torch.ones(6, dtype=X.dtype))


@pytest.mark.parametrize("cls", [ARDMatern32Kernel, ARDMatern52Kernel])
def test_ard_matern_model_io_roundtrip(cls):
    from spark_gp_amd.models.model_io import kernel_from_spec, kernel_to_spec
    k = 1.5 * cls(np.array([0.5, 2.0]), lower=1e-3,
                  upper=np.array([10.0, math.inf])) \
        + Scalar(1e-3).const * EyeKernel()
    k2 = kernel_from_spec(kernel_to_spec(k))
    np.testing.assert_array_equal(k2.get_hyperparameters(),
                                  k.get_hyperparameters())
    for a, b in zip(k2.hyperparameter_bounds(), k.hyperparameter_bounds()):
        np.testing.assert_array_equal(a, b)
    X = torch.as_tensor(np.random.default_rng(0).normal(size=(4, 2)))
    assert torch.equal(k2.training_kernel(X), k.training_kernel(X))
    base = kernel_from_spec(kernel_to_spec(cls(np.array([0.5, 2.0]))))
    assert type(base) is cls


# ---- hip_backend's host chain rule over a fake extension -------------------

def _raw_stats(cs, theta, X, y):
    """The fused kernel's raw per-expert outputs (expert_nll.hip) in fp64
    torch: (nll, sum G o Kb, tr G, contr, bad) with
    contr_j = sum_ab (G o Kd)_ab (x_aj - x_bj)^2."""
    C, nu = cs.amp(theta), cs.noise(theta)
    d, k = X.shape[-1], X.shape[-2]
    Xs = X * torch.as_tensor(base_scale(cs.base, theta[cs.base_idx], d))
    Kb, Kd = torch_backend.family_kb_kd(base_family(cs.base), sqdist(Xs, Xs))
    K = C * Kb + nu * torch.eye(k, dtype=X.dtype)
    L = torch.linalg.cholesky(K)
    logdet = 2.0 * torch.log(L.diagonal(dim1=-2, dim2=-1)).sum(-1)
    Kinv = torch.cholesky_inverse(L)
    alpha = (Kinv @ y.unsqueeze(-1)).squeeze(-1)
    nll = 0.5 * (y * alpha).sum(-1) + 0.5 * logdet
    G = alpha.unsqueeze(-1) * alpha.unsqueeze(-2) - Kinv
    W = G * Kd
    diff2 = (X.unsqueeze(-2) - X.unsqueeze(-3)) ** 2           # [E, k, k, d]
    contr = (W.unsqueeze(-1) * diff2).sum((-2, -3))
    return (nll, (G * Kb).sum((-1, -2)),
            G.diagonal(dim1=-2, dim2=-1).sum(-1), contr,
            torch.zeros(X.shape[0], dtype=torch.int32))


class _FakeExt:
    """Stands in for the HIP extension; carries the exact fp64 theta and
    checks the family code and the scale vector it is called with."""

    def __init__(self, cs, theta):
        self.cs, self.theta, self.calls = cs, theta, 0

    def fused_expert_nll(self, X, y, scale, amp, noise, family=0):
        assert family == base_family(self.cs.base)
        want = base_scale(self.cs.base, self.theta[self.cs.base_idx],
                          X.shape[-1])
        np.testing.assert_allclose(scale.numpy(), want, rtol=1e-6)
        assert amp == self.cs.amp(self.theta)
        assert noise == self.cs.noise(self.theta)
        self.calls += 1
        return _raw_stats(self.cs, self.theta, X.double(), y.double())

    @staticmethod
    def fused_expert_nll_supported(k, d):
        return True

    fused_laplace_newton_supported = fused_expert_nll_supported
    fused_laplace_evidence_supported = fused_expert_nll_supported


@pytest.mark.parametrize("base", list(BASES))
def test_host_chain_rule_matches_oracle(base, monkeypatch):
    E, k, d = 4, 13, 5
    X, y = _data(E, k, d)
    kernel = _tree(base, d)
    cs = compile_kernel(kernel)
    assert cs is not None
    theta = kernel.get_hyperparameters()
    fake = _FakeExt(cs, theta)
    monkeypatch.setattr(hip_backend, "ext", fake)
    nll_h, grad_h = hip_backend.nll_grad_compiled(cs, theta, X, y)
    assert fake.calls == 1
    nll_t, grad_t = torch_backend.nll_grad_compiled(cs, theta, X, y)
    # y crosses the extension boundary in fp32, as in
    # test_hip_backend_host_logic.py
    assert nll_h == pytest.approx(nll_t, rel=1e-6)
    np.testing.assert_allclose(grad_h, grad_t, rtol=1e-4)


@pytest.mark.parametrize("base", list(BASES))
def test_laplace_gates_reject_matern(base, monkeypatch):
    d = 4
    cs = compile_kernel(_tree(base, d))
    monkeypatch.setattr(hip_backend, "ext", _FakeExt(cs, None))
    X = torch.rand(3, 16, d)
    assert hip_backend.supports_nll(cs, X)
    assert not hip_backend.supports_laplace(cs, X)
    assert not hip_backend.supports_laplace_evidence(cs, X)
    # ... and still take the RBF family
    cs_rbf = compile_kernel(1 * RBFKernel(1.0) + Scalar(1e-3).const
                            * EyeKernel())
    assert hip_backend.supports_laplace(cs_rbf, X)
    assert hip_backend.supports_laplace_evidence(cs_rbf, X)

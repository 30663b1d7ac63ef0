"""Batched PyTorch implementations of the GP compute kernels.

This backend serves two roles:

1. the *correctness oracle* — float64 on CPU, numerically equivalent to the
   reference's per-expert Breeze math (``regression/GaussianProcessRegression.scala:55-68``,
   ``classification/GaussianProcessClassifier.scala:74-129``);
2. the fallback path on GPU for kernel trees the fused HIP kernels do not
   cover.

Everything is *batched over experts*: an ``[E, k, k]`` problem batch executes
as a handful of tensor ops instead of E independent tasks (the reference runs
one Spark task per expert).  Scalar accumulations (nll, gradient) are always
done in float64 regardless of the compute dtype.
"""

from __future__ import annotations

import math
from typing import Tuple

import numpy as np
import torch

from ..kernels.base import Kernel, sqdist
from ..kernels.compiled import (CompiledKernel, FAM_M32, FAM_M52, FAM_RBF,
                                base_family, base_scale)


def logdet_and_inv(K: torch.Tensor, force_lu: bool = False
                   ) -> Tuple[torch.Tensor, torch.Tensor]:
    """(logdet [...,], Kinv [..., k, k]) from one factorization per matrix.

    Mirrors ``commons/util/logDetAndInv.scala`` (single LU there).  Here:
    Cholesky (cheaper, PD-correct); experts whose Cholesky fails fall back to
    LU-based slogdet+inv so non-PD iterates behave like the reference instead
    of aborting (the reference's LU never fails on merely-indefinite K).
    ``force_lu`` skips the Cholesky attempt (used when the caller already
    knows it breaks down, e.g. the HIP kernel's bad-expert fallback)."""
    if force_lu:
        # ONE LU factorization for both logdet and inverse, like the
        # reference's logDetAndInv (dgetrf once, then dgetri)
        LU, piv = torch.linalg.lu_factor(K)
        logdet = torch.log(LU.diagonal(dim1=-2, dim2=-1).abs()).sum(-1)
        eye = torch.eye(K.shape[-1], dtype=K.dtype,
                        device=K.device).expand_as(K)
        return logdet, torch.linalg.lu_solve(LU, piv, eye)
    L, info = torch.linalg.cholesky_ex(K)
    bad = info > 0
    if bad.any():
        logdet = torch.empty(K.shape[:-2], dtype=K.dtype, device=K.device)
        Kinv = torch.empty_like(K)
        good = ~bad
        if good.any():
            Lg = L[good]
            logdet[good] = 2.0 * torch.log(Lg.diagonal(dim1=-2, dim2=-1)).sum(-1)
            Kinv[good] = torch.cholesky_inverse(Lg)
        Kb = K[bad]
        _, logabsdet = torch.linalg.slogdet(Kb)
        logdet[bad] = logabsdet
        Kinv[bad] = torch.linalg.inv(Kb)
        return logdet, Kinv
    logdet = 2.0 * torch.log(L.diagonal(dim1=-2, dim2=-1)).sum(-1)
    return logdet, torch.cholesky_inverse(L)


# ---------------------------------------------------------------------------
# Fused regression objective (compiled kernel canonical form)
# ---------------------------------------------------------------------------

def family_kb_kd(family: int, q: torch.Tensor):
    """(Kb(q), Kd(q) = -dKb/dq) of a covariance family at the scaled squared
    distance q >= 0 (kernels/matern.py has the table)."""
    if family == FAM_RBF:
        Kb = torch.exp(-q)
        return Kb, Kb
    t = torch.sqrt(q.clamp_min(0.0))
    e = torch.exp(-t)
    if family == FAM_M32:
        return (1.0 + t) * e, 0.5 * e
    if family == FAM_M52:
        return (1.0 + t + t * t / 3.0) * e, (1.0 + t) * e / 6.0
    raise ValueError(f"unknown covariance family {family}")


def _base_matrices(cs: CompiledKernel, theta: np.ndarray, X: torch.Tensor):
    """Kb(q) and Kd(q) = -dKb/dq of the canonical base at
    q = ||(a - b) o s||^2; returns (Kb, Kd, s) with s the fp64 [d] scale."""
    s = base_scale(cs.base, theta[cs.base_idx], X.shape[-1])
    Xs = X * torch.as_tensor(s, dtype=X.dtype, device=X.device)
    Kb, Kd = family_kb_kd(base_family(cs.base), sqdist(Xs, Xs))
    return Kb, Kd, s


def _diff2_contraction(W: torch.Tensor, X: torch.Tensor) -> torch.Tensor:
    """contr_j = sum_ab W_ab (x_aj - x_bj)^2 for symmetric W [E, k, k], as
    two GEMMs instead of the [E, k, k, d] difference tensor; [E, d]."""
    t1 = (X * X * W.sum(-1).unsqueeze(-1)).sum(-2)
    t2 = (X * (W @ X)).sum(-2)
    return 2.0 * t1 - 2.0 * t2


def nll_grad_compiled(cs: CompiledKernel, theta: np.ndarray,
                      X: torch.Tensor, y: torch.Tensor,
                      force_lu: bool = False) -> Tuple[float, np.ndarray]:
    """Sum over the expert batch of the per-expert BCM negative log marginal
    likelihood and its gradient w.r.t. the full hyperparameter vector.

    nll_e = 1/2 y^T K^-1 y + 1/2 log|K|;  grad_i = -1/2 sum(dK_i * (aa^T - K^-1))
    (``regression/GaussianProcessRegression.scala:55-68``), computed WITHOUT
    materializing the [p, k, k] derivative tensor: the derivative
    contraction reduces to two GEMMs per batch (see K5 fusion plan,
    SURVEY.md §2.4).  With Kd = -dKb/dq and dq/ds_j = 2 s_j (x_aj - x_bj)^2
    the gradient over the scale is g_s = C s o contr, contr the contraction
    of G o Kd; ``cs.assemble_grad`` maps it onto theta."""
    C = cs.amp(theta)
    nu = cs.noise(theta)
    Kb, Kd, s = _base_matrices(cs, theta, X)
    k = X.shape[-2]
    K = C * Kb + nu * torch.eye(k, dtype=X.dtype, device=X.device)

    logdet, Kinv = logdet_and_inv(K, force_lu=force_lu)
    alpha = (Kinv @ y.unsqueeze(-1)).squeeze(-1)                 # [E, k]
    nll = (0.5 * (y * alpha).sum(-1).double() + 0.5 * logdet.double()).sum()

    G = alpha.unsqueeze(-1) * alpha.unsqueeze(-2) - Kinv         # [E, k, k]
    contr = _diff2_contraction(G * Kd, X).double().sum(0).cpu().numpy()  # [d]
    trG = float(G.diagonal(dim1=-2, dim2=-1).double().sum())
    grad = cs.assemble_grad(
        theta, g_scale=(C * s) * contr,
        g_amp=float(-0.5 * (G * Kb).double().sum()), g_noise=-0.5 * trG)
    return float(nll), grad


# ---------------------------------------------------------------------------
# Generic regression objective (any kernel tree; materialized derivatives)
# ---------------------------------------------------------------------------

def nll_grad_generic(kernel: Kernel, theta: np.ndarray,
                     X: torch.Tensor, y: torch.Tensor
                     ) -> Tuple[float, np.ndarray]:
    kernel.set_hyperparameters(theta)
    K, dK = kernel.training_kernel_and_derivative(X)   # [E,k,k], [E,p,k,k]
    logdet, Kinv = logdet_and_inv(K)
    alpha = (Kinv @ y.unsqueeze(-1)).squeeze(-1)
    nll = (0.5 * (y * alpha).sum(-1).double() + 0.5 * logdet.double()).sum()
    G = alpha.unsqueeze(-1) * alpha.unsqueeze(-2) - Kinv
    grad_e = -0.5 * (dK * G.unsqueeze(-3)).sum((-1, -2))          # [E, p]
    grad = grad_e.double().sum(0).cpu().numpy()
    return float(nll), grad


# ---------------------------------------------------------------------------
# Batched Laplace approximation for GP classification
# ---------------------------------------------------------------------------

def laplace_nll_grad(kernel: Kernel, theta: np.ndarray,
                     X: torch.Tensor, y: torch.Tensor, f: torch.Tensor,
                     tol: float, max_newton_iter: int = 200,
                     newton: bool = True,
                     likelihood=None) -> Tuple[float, np.ndarray]:
    """Batched Newton iteration (R&W Algorithm 3.1 with step halving) +
    Algorithm 5.1 evidence/gradient, mirroring
    ``classification/GaussianProcessClassifier.scala:74-129``.

    ``f`` ([E, k]) is the per-expert latent vector, updated IN PLACE so it
    warm-starts across L-BFGS evaluations (reference mutates cached RDD
    state, ``GaussianProcessClassifier.scala:52-60``).

    Experts converge at different Newton iteration counts: converged experts
    are masked out of subsequent iterations (per-expert convergence mask —
    SURVEY.md hard part #5).

    ``likelihood``: a ``spark_gp_amd.likelihoods.Likelihood`` — Algorithms
    3.1/5.1 only touch the likelihood through log p and its first three
    f-derivatives.  Default: the reference's logistic link."""
    from ..likelihoods import LogisticLikelihood
    lik = likelihood if likelihood is not None else LogisticLikelihood()
    kernel.set_hyperparameters(theta)
    K, dK = kernel.training_kernel_and_derivative(X)   # [E,k,k], [E,p,k,k]
    E, k = y.shape
    dev, dt = X.device, X.dtype
    eyek = torch.eye(k, dtype=dt, device=dev)

    old_obj = torch.full((E,), -math.inf, dtype=torch.float64, device=dev)
    new_obj = torch.full((E,), -torch.finfo(torch.float64).max,
                         dtype=torch.float64, device=dev)
    step = torch.ones(E, dtype=torch.float64, device=dev)
    # final per-expert state needed by the evidence computation
    L_out = torch.empty_like(K)
    a_out = torch.empty_like(f)
    sqw_out = torch.empty_like(f)
    f_eval_out = f.clone()         # latent at the last Newton EVALUATION

    active = torch.ones(E, dtype=torch.bool, device=dev)
    if not newton:
        # f already converged (fused HIP Newton pre-pass): evaluate the
        # exit-state quantities of Algorithm 3.1 once at the current f
        w = lik.w(f, y)
        sqw = torch.sqrt(w)
        B = eyek + sqw.unsqueeze(-1) * K * sqw.unsqueeze(-2)
        L_out = torch.linalg.cholesky(B)
        grad_logp = lik.d1(f, y)
        b = w * f + grad_logp
        Kb = (K @ b.unsqueeze(-1)).squeeze(-1)
        v = torch.cholesky_solve((sqw * Kb).unsqueeze(-1), L_out).squeeze(-1)
        a_out = b - sqw * v
        sqw_out = sqw
        fc = (K @ a_out.unsqueeze(-1)).squeeze(-1)
        new_obj = (-0.5 * (a_out * fc).sum(-1).double()
                   + lik.log_lik(fc, y).double().sum(-1))
        active = torch.zeros(E, dtype=torch.bool, device=dev)

    it = 0
    while bool(active.any()) and it < max_newton_iter:
        it += 1
        idx = active.nonzero(as_tuple=True)[0]
        Ki, fi, yi = K[idx], f[idx], y[idx]
        w = lik.w(fi, yi)
        sqw = torch.sqrt(w)
        B = eyek + sqw.unsqueeze(-1) * Ki * sqw.unsqueeze(-2)
        Li = torch.linalg.cholesky(B)
        grad_logp = lik.d1(fi, yi)
        b = w * fi + grad_logp
        Kb = (Ki @ b.unsqueeze(-1)).squeeze(-1)
        v = torch.cholesky_solve((sqw * Kb).unsqueeze(-1), Li).squeeze(-1)
        a = b - sqw * v
        si = step[idx].to(dt).unsqueeze(-1)
        f_cand = (1.0 - si) * fi + si * (Ki @ a.unsqueeze(-1)).squeeze(-1)
        obj_cand = (-0.5 * (a * f_cand).sum(-1).double()
                    + lik.log_lik(f_cand, yi).double().sum(-1))

        accept = obj_cand > old_obj[idx]
        # store the state computed at the current f for every active expert —
        # at loop exit it corresponds to the last iteration, as in the ref.
        L_out[idx], a_out[idx] = Li, a
        sqw_out[idx], f_eval_out[idx] = sqw, fi

        acc_idx = idx[accept]
        if acc_idx.numel():
            f[acc_idx] = f_cand[accept]
            old_obj[acc_idx] = new_obj[acc_idx]
            new_obj[acc_idx] = obj_cand[accept]
        rej_idx = idx[~accept]
        if rej_idx.numel():
            step[rej_idx] *= 0.5
        still = (torch.abs(old_obj[idx] - new_obj[idx]) > tol) & (step[idx] > tol)
        active[idx] = still

    # ---- Algorithm 5.1: evidence and gradient --------------------------
    L, a, sqw = L_out, a_out, sqw_out
    logZ = new_obj - torch.log(L.diagonal(dim1=-2, dim2=-1)).double().sum(-1)

    sqwD = torch.diag_embed(sqw)
    R = sqw.unsqueeze(-1) * torch.cholesky_solve(sqwD, L)         # [E,k,k]
    Cm = torch.linalg.solve_triangular(L, sqw.unsqueeze(-1) * K,
                                       upper=False)               # [E,k,k]
    d3 = lik.d3_evidence(f_eval_out, f, y)
    diagK = K.diagonal(dim1=-2, dim2=-1)
    diagCtC = (Cm * Cm).sum(-2)
    s2 = -0.5 * (diagK - diagCtC) * d3                            # [E,k]

    grad_logp = lik.d1(f_eval_out, y)
    p = dK.shape[-3]
    grad = torch.zeros(p, dtype=torch.float64)
    KR = K @ R                                                    # [E,k,k]
    for i in range(p):
        Di = dK[:, i]
        s1 = (0.5 * (a.unsqueeze(-2) @ Di @ a.unsqueeze(-1)).squeeze(-1).squeeze(-1)
              - 0.5 * (R * Di).sum((-1, -2)))
        b = (Di @ grad_logp.unsqueeze(-1)).squeeze(-1)
        s3 = b - (KR @ b.unsqueeze(-1)).squeeze(-1)
        grad[i] = (s1.double() + (s2 * s3).sum(-1).double()).sum()

    return float(-logZ.sum()), -grad.cpu().numpy()


# ---------------------------------------------------------------------------
# PPA accumulation (K12): K_mn K_nm and K_mn y over the local shard
# ---------------------------------------------------------------------------

def kmn_knm_and_kmny(kernel: Kernel, active: torch.Tensor,
                     X: torch.Tensor, y: torch.Tensor,
                     chunk_rows: int = 262144
                     ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Accumulate (K_mn K_nm [m,m], K_mn y [m]) over the local rows.

    Mirrors ``commons/ProjectedGaussianProcessHelper.scala:20-36`` but
    flattened: experts partition the rows, so the per-expert sum equals the
    full-shard product.  Chunked so the [c, m] cross-kernel block never
    exceeds a few hundred MB; cross-chunk accumulation is float64."""
    m = active.shape[0]
    n = X.shape[0]
    KK = torch.zeros(m, m, dtype=torch.float64, device=X.device)
    Ky = torch.zeros(m, dtype=torch.float64, device=X.device)
    for s in range(0, n, chunk_rows):
        e = min(n, s + chunk_rows)
        A = kernel.cross_kernel(X[s:e], active)      # [c, m]
        KK += (A.transpose(0, 1) @ A).double()
        Ky += (A.transpose(0, 1) @ y[s:e].unsqueeze(-1)).squeeze(-1).double()
    return KK, Ky


def laplace_evidence_experts(cs: CompiledKernel, theta: np.ndarray,
                             X: torch.Tensor, y: torch.Tensor,
                             f: torch.Tensor
                             ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Per-expert Algorithm 5.1 evidence and gradient at an already-converged
    latent f: (logZ [E], g [E, d + 2]) in fp64, g the gradient of logZ over
    the coordinate scale s, then the amplitude, then the noise — the contract
    of ``ext.fused_laplace_evidence``.

    Computed WITHOUT materializing the [E, p, k, k] derivative tensor (the
    K11 contraction fusion): for the canonical kernel
    C*Kb(q) + nu*I, dK/ds_j = -2 s_j C Kd o (x_j - x'_j)^2, so the dK_j
    contractions reduce to batched GEMMs via the regression path's identities
    with G := a a^T - R, and the dK_j matvecs (s3) via
    (dK_j v) = -2 s_j (C Kd) @ [v, X o v, X^2 o v] recombined."""
    C = cs.amp(theta)
    nu = cs.noise(theta)
    Kb, Kd, s = _base_matrices(cs, theta, X)
    E, k = y.shape
    d = X.shape[-1]
    dt, dev = X.dtype, X.device
    s = torch.as_tensor(s, dtype=dt, device=dev)
    eyek = torch.eye(k, dtype=dt, device=dev)
    K = C * Kb + nu * eyek

    # exit-state quantities of Algorithm 3.1 at f
    pi = torch.sigmoid(f)
    w = pi * (1.0 - pi)
    sqw = torch.sqrt(w)
    B = eyek + sqw.unsqueeze(-1) * K * sqw.unsqueeze(-2)
    L = torch.linalg.cholesky(B)
    v = y - pi                                   # grad log p
    b = w * f + v
    Kb_vec = (K @ b.unsqueeze(-1)).squeeze(-1)
    t = torch.cholesky_solve((sqw * Kb_vec).unsqueeze(-1), L).squeeze(-1)
    a = b - sqw * t
    fc = (K @ a.unsqueeze(-1)).squeeze(-1)
    psi = (-0.5 * (a * fc).sum(-1).double()
           + torch.nn.functional.logsigmoid((2.0 * y - 1.0) * fc)
           .double().sum(-1))
    logZ = psi - torch.log(L.diagonal(dim1=-2, dim2=-1)).double().sum(-1)

    R = sqw.unsqueeze(-1) * torch.cholesky_solve(torch.diag_embed(sqw), L)
    KR = K @ R
    d3 = -(2.0 * pi - 1.0) * pi * pi * torch.exp(-f)
    # (K R K)_ii = sum_j (KR)_ij K_ji = (KR o K).sum(-1) since K is
    # symmetric — avoids materializing the full [E, k, k] product
    diagKRK = (KR * K).sum(-1)
    s2 = -0.5 * (K.diagonal(dim1=-2, dim2=-1) - diagKRK) * d3

    # shared pieces: s1_i = 1/2 sum(G o dK_i) with G = a a^T - R;
    # s3_i = b_i - K R b_i with b_i = dK_i v
    G = a.unsqueeze(-1) * a.unsqueeze(-2) - R

    def s2_dot_s3(Bmat):
        """sum_a s2_a (Bmat - K R Bmat)_a per trailing column -> [E, cols]"""
        return (s2.unsqueeze(-1) * (Bmat - KR @ Bmat)).sum(-2)

    # scale: s1_j = 1/2 sum(G o dK_j) = -s_j C contr_j
    s1 = -s * C * _diff2_contraction(G * Kd, X)                  # [E, d]
    # one batched GEMM for all three dK_j-matvec ingredients
    U = (C * Kd) @ torch.cat([v.unsqueeze(-1), X * v.unsqueeze(-1),
                              X * X * v.unsqueeze(-1)], dim=-1)
    u0, U1, U2 = U[..., 0], U[..., 1:1 + d], U[..., 1 + d:]
    Bm = -2.0 * s * (X * X * u0.unsqueeze(-1) - 2.0 * X * U1 + U2)
    g_scale = s1.double() + s2_dot_s3(Bm).double()
    # amplitude: dK/dC = Kb
    s1a = (0.5 * (a.unsqueeze(-2) @ (Kb @ a.unsqueeze(-1))).reshape(E)
           - 0.5 * (R * Kb).sum((-1, -2)))
    g_amp = s1a.double() + s2_dot_s3(Kb @ v.unsqueeze(-1)).squeeze(-1).double()
    # noise: dK/dnu = I
    s1n = 0.5 * (a * a).sum(-1) - 0.5 * R.diagonal(dim1=-2, dim2=-1).sum(-1)
    g_noise = s1n.double() + s2_dot_s3(v.unsqueeze(-1)).squeeze(-1).double()
    return logZ, torch.cat([g_scale, g_amp.unsqueeze(-1),
                            g_noise.unsqueeze(-1)], dim=-1)


def laplace_evidence_compiled(cs: CompiledKernel, theta: np.ndarray,
                              X: torch.Tensor, y: torch.Tensor,
                              f: torch.Tensor) -> Tuple[float, np.ndarray]:
    """Negative Laplace evidence summed over the expert batch and its
    gradient over theta, at an already-converged latent f."""
    logZ, g = laplace_evidence_experts(cs, theta, X, y, f)
    d = X.shape[-1]
    g = g.sum(0).cpu().numpy()
    grad = cs.assemble_grad(theta, g[:d], float(g[d]), float(g[d + 1]))
    return float(-logZ.sum()), -grad



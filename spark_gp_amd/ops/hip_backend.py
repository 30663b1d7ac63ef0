"""Python wrapper over the hand-written CDNA4 HIP kernels (_hip_ext).

Every compiled base is Kb(q) with q = ||(a - b) o s||^2: the kernels take the
scale vector s and the family code, and return raw contractions.  This module
turns those into a gradient over (s, amplitude, noise) and hands it to
``CompiledKernel.assemble_grad`` (kernels/compiled.py), the one place that
knows how s depends on a base's hypers — as ``torch_backend`` does, so the
two backends are drop-in interchangeable and unit-diffable.
"""

from __future__ import annotations

import os
from typing import Tuple

import numpy as np
import torch

from ..kernels.base import Kernel
from ..kernels.compiled import (BASES, RBF_BASES, CompiledKernel,
                                base_family, base_scale, compile_kernel)
from .. import _hip_ext as ext
from . import torch_backend
from . import ppa_plan


def _scale_vector(cs: CompiledKernel, theta: np.ndarray, d: int,
                  device, dtype=torch.float32) -> torch.Tensor:
    """Coordinate scale s of the base: the kernels work on x' = x o s with
    q = ||x'_a - x'_b||^2 (kernels/compiled.py lists s per base)."""
    s = base_scale(cs.base, theta[cs.base_idx], d)
    return torch.as_tensor(s, dtype=dtype, device=device)


def _supports_expert(cs, X: torch.Tensor, kd_supported, bases) -> bool:
    """A kernel with one of ``bases`` on [E, k, d] fp32 experts whose (k, d)
    the fused kernel's LDS budget takes (``kd_supported``: an
    ``ext.*_supported``)."""
    if cs is None or cs.base not in bases:
        return False
    if X.dtype != torch.float32 or X.dim() != 3:
        return False
    E, k, d = X.shape
    return bool(kd_supported(k, d))


def supports_nll(cs: CompiledKernel, X: torch.Tensor) -> bool:
    return _supports_expert(cs, X, ext.fused_expert_nll_supported, BASES)


def nll_grad_compiled(cs: CompiledKernel, theta: np.ndarray,
                      X: torch.Tensor, y: torch.Tensor
                      ) -> Tuple[float, np.ndarray]:
    E, k, d = X.shape
    C = cs.amp(theta)
    nu = cs.noise(theta)
    s = base_scale(cs.base, theta[cs.base_idx], d)
    scale = torch.as_tensor(s, dtype=torch.float32, device=X.device)
    # sumW0 = sum(G o Kb), contr_j = sum_ab (G o Kd)_ab (x_aj - x_bj)^2
    nll, sumW0, trG, contr, bad = ext.fused_expert_nll(
        X, y.to(torch.float32), scale, float(C), float(nu),
        family=base_family(cs.base))

    # single device->host transfer for all reductions (one sync per eval)
    stats = torch.cat([nll.sum().reshape(1), sumW0.sum().reshape(1),
                       trG.sum().reshape(1), bad.sum().double().reshape(1),
                       bad.max().double().reshape(1),
                       contr.sum(0)]).cpu().numpy()
    nll_total, sumW0_t, trG_t = float(stats[0]), float(stats[1]), float(stats[2])
    n_bad = int(stats[3])
    if stats[4] >= 2.0:
        # a non-finite kernel matrix (overflowing line-search iterate): the
        # reference's LAPACK would propagate NaN and L-BFGS-B backtracks;
        # return +inf instead of recomputing every expert on the fallback
        return float("inf"), np.zeros(cs.p)
    contr_t = stats[5:]                               # [d]

    # dq/ds_j = 2 s_j (x_aj - x_bj)^2, so the gradient over s is C s o contr
    grad = cs.assemble_grad(theta, g_scale=(C * s) * contr_t,
                            g_amp=-0.5 * sumW0_t, g_noise=-0.5 * trG_t)

    if n_bad:
        # fp32 Cholesky broke down for these experts (huge-amplitude
        # iterates); recompute them on the torch path (LU fallback inside)
        idx = (bad != 0).nonzero(as_tuple=True)[0]
        nll_b, grad_b = torch_backend.nll_grad_compiled(
            cs, theta, X[idx], y[idx], force_lu=True)
        nll_total += nll_b
        grad += grad_b
    return nll_total, grad


# ---------------------------------------------------------------------------
# Laplace Newton pre-pass (GPC)
# ---------------------------------------------------------------------------

# Tolerance floor for the fused Newton/evidence kernels.  The kernel's
# psi accumulates in fp64 (block_sum doubles), so the fp32 matrix noise,
# not the summation, sets the floor: measured oracle parity IMPROVES with
# tighter tol (grad max-rel 2.6e-4 at 1e-5, 1.9e-6 at 1e-6, 9.8e-7 at
# 1e-7 — BASELINE.md round 2), so the default floor matches the
# reference's default tol.  Below it, a fp64 torch polish finishes from
# the warm latent (see ops.__init__.laplace_nll_grad).
LAPLACE_MIN_TOL = float(os.environ.get("SPARK_GP_AMD_LAPLACE_MIN_TOL",
                                       "1e-6"))


def supports_laplace(cs: CompiledKernel, X: torch.Tensor) -> bool:
    # laplace.hip is exp(-q) only
    return _supports_expert(cs, X, ext.fused_laplace_newton_supported,
                            RBF_BASES)


def _fused_laplace(entry, cs: CompiledKernel, theta: np.ndarray,
                   X: torch.Tensor, y: torch.Tensor, f: torch.Tensor,
                   tol: float, max_newton: int):
    """Call one of the two fused Laplace entry points; ``f`` is updated IN
    PLACE.  The fused loop is a warm-starter: a torch pass finishes
    convergence with reference semantics where needed, so the fp32
    iterations are capped (the fp32 objective noise floor can sit above a
    tight tol) and tol is loosened to the fp32-representable level."""
    if not f.is_contiguous():
        raise ValueError("latent f must be contiguous")
    scale = _scale_vector(cs, theta, X.shape[-1], X.device)
    return entry(X, y.to(torch.float32), f, scale, float(cs.amp(theta)),
                 float(cs.noise(theta)), max(float(tol), LAPLACE_MIN_TOL),
                 min(int(max_newton), 40))


def laplace_newton(cs: CompiledKernel, theta: np.ndarray, X: torch.Tensor,
                   y: torch.Tensor, f: torch.Tensor, tol: float,
                   max_newton: int) -> int:
    """Run the fused per-expert Newton loop to convergence, updating the
    latent ``f`` IN PLACE.  Returns the number of experts the fp32 kernel
    could not handle (their f is left unchanged; the torch evidence pass
    converges them from their warm state)."""
    psi, sll, iters, bad = _fused_laplace(ext.fused_laplace_newton, cs, theta,
                                          X, y, f, tol, max_newton)
    return int((bad != 0).sum())


def supports_laplace_evidence(cs: CompiledKernel, X: torch.Tensor) -> bool:
    return _supports_expert(cs, X, ext.fused_laplace_evidence_supported,
                            RBF_BASES)


def laplace_evidence(cs: CompiledKernel, theta: np.ndarray, X: torch.Tensor,
                     y: torch.Tensor, f: torch.Tensor, tol: float,
                     max_newton: int):
    """Fully fused K10+K11: Newton to convergence AND the Algorithm 5.1
    evidence/gradient in one launch (laplace.hip evidence tail).  Updates
    f in place.  Returns (nll, grad) with the torch-path sign convention,
    or None when any expert's fp32 factor broke down (caller falls back
    to the warm torch Newton)."""
    d = X.shape[-1]
    logz, grad, iters, bad = _fused_laplace(ext.fused_laplace_evidence, cs,
                                            theta, X, y, f, tol, max_newton)
    # one device->host transfer for everything
    stats = torch.cat([logz.sum().reshape(1), bad.sum().double().reshape(1),
                       grad.sum(0)]).cpu().numpy()
    if int(stats[1]):
        return None
    logZ = float(stats[0])
    g = stats[2:]
    # the kernel differentiates logZ w.r.t. the scale, amplitude and noise
    out = cs.assemble_grad(theta, g[:d], float(g[d]), float(g[d + 1]))
    return float(-logZ), -out


# ---------------------------------------------------------------------------
# PPA path
# ---------------------------------------------------------------------------

def supports_ppa(kernel: Kernel, X: torch.Tensor) -> bool:
    cs = compile_kernel(kernel)
    return (cs is not None and cs.base in BASES
            and X.dtype == torch.float32)


def _s2_vector(cs: CompiledKernel, theta: np.ndarray, d: int, device):
    s = _scale_vector(cs, theta, d, device, dtype=torch.float64)
    return (s * s).to(torch.float32)


_SYNC_TILE_CACHE: dict = {}


def _syrk_sync_tiles(m: int, device):
    """ppa_plan.syrk_sync_tile_lists uploaded once per (m, device, patch)."""
    patch = ppa_plan.syrk_sync_patch()
    key = (m, str(device), patch)
    if key not in _SYNC_TILE_CACHE:
        _SYNC_TILE_CACHE[key] = [
            (torch.tensor(tiles, dtype=torch.int32, device=device), nactive)
            for tiles, nactive in ppa_plan.syrk_sync_tile_lists(m, patch)]
    return _SYNC_TILE_CACHE[key]


def kmn_knm_and_kmny(kernel: Kernel, active: torch.Tensor,
                     X: torch.Tensor, y: torch.Tensor,
                     chunk_rows: int = 262144, precision: str = "fp64"
                     ) -> Tuple[torch.Tensor, torch.Tensor]:
    cs = compile_kernel(kernel)
    theta = kernel.get_hyperparameters()
    n, d = X.shape
    m = active.shape[0]
    C = float(cs.amp(theta))
    fam = base_family(cs.base)
    s2 = _s2_vector(cs, theta, d, X.device)
    act32 = active.to(torch.float32).contiguous()
    y32 = y.to(torch.float32)

    Ky = torch.zeros(m, dtype=torch.float64, device=X.device)
    if precision == "fp64":
        # reference-parity numerics: K_nm values from the HIP cross kernel
        # (fp32, ~6e-8 quantization), products and accumulation in fp64
        KK64 = torch.zeros(m, m, dtype=torch.float64, device=X.device)
        for s in range(0, n, chunk_rows):
            e = min(n, s + chunk_rows)
            Kc = ext.cross_kernel_tile(X[s:e].contiguous(), act32, s2, C,
                                       False, False, False, family=fam)[0]
            K64 = Kc.double()
            KK64 += K64.transpose(0, 1) @ K64
            Ky += K64.transpose(0, 1) @ y[s:e].double()
        return KK64, Ky

    # 'mixed': hi/lo bf16 split — KK += hi^T hi + hi^T lo + lo^T hi on the
    # MFMA SYRK keeps input-quantization error at fp32 class while running
    # at bf16 matrix-core rate.  ppa_plan picks the K_nm generator, the SYRK
    # kernel, split_k and the chunk length.
    plan = ppa_plan.ppa_plan(m, d, X.dtype, chunk_rows)
    KK = torch.zeros(m, m, dtype=torch.float32, device=X.device)
    if plan.generator != "elementwise":
        # pre-scaled coordinates and their squared norms: the generators
        # compute sqdist as ||x'||^2 + ||a'||^2 - 2 x'.a'
        svec = _scale_vector(cs, theta, d, X.device)
        As = (act32 * svec).contiguous()
        na = (As * As).sum(-1).contiguous()
    if plan.generator == "fused" and n > 0:
        # the f16 generator needs the scaled coordinates inside its range:
        # bound them once for all chunks (one pass over X, one host read)
        xlo, xhi = torch.aminmax(X)
        alo, ahi = torch.aminmax(As)
        absmax = float(torch.maximum(
            torch.maximum(-xlo, xhi) * svec.abs().max(),
            torch.maximum(-alo, ahi)))
        gen = ppa_plan.ppa_fused_gen(absmax)
        # scratch of the k-slices' partial tiles, shared by all chunks
        partials = torch.empty(
            ppa_plan.ppa_fused_partials_numel(m, plan.split_k),
            dtype=torch.float32, device=X.device)
    if plan.syrk == "sync":
        sync_tiles = _syrk_sync_tiles(m, X.device)
    for s in range(0, n, plan.chunk_rows):
        e = min(n, s + plan.chunk_rows)
        yc = y32[s:e].contiguous()
        if plan.generator != "elementwise":
            # assigned here, not in a helper: the previous chunk's Xs is
            # released before the Xs * Xs temporary is allocated
            Xs = (X[s:e] * svec).contiguous()
            nx = (Xs * Xs).sum(-1).contiguous()
        if plan.generator == "fused":
            ext.ppa_fused_acc(Xs, As, nx, na, C, yc, Ky, KK, plan.split_k,
                              family=fam, gen=gen, absmax=absmax,
                              partials=partials)
            continue
        if plan.generator == "mfma":
            KcT, KlT = ext.cross_mfma_ppa(Xs, As, nx, na, C, yc, Ky,
                                          family=fam)
        else:
            KcT, KlT = ext.cross_kernel_tile_ppa(X[s:e].contiguous(), act32,
                                                 s2, C, yc, Ky, family=fam)
        if plan.syrk == "sync":
            for tiles, nactive in sync_tiles:
                ext.syrk_bf16_sync_acc(KcT, KlT, KK, tiles,
                                       ppa_plan.SYNC_KPB, nactive)
        else:
            ext.syrk_bf16_acc(KcT, KlT, KK, plan.split_k)
    return KK.double(), Ky


# ---------------------------------------------------------------------------
# K13: hand-written blocked fp64 Cholesky path for the magic solves
# ---------------------------------------------------------------------------
# Replaces torch.linalg (rocSOLVER) in ppa.magic_vector_matrix on GPU:
# big_chol.hip's one-workgroup 64x64 diagonal factors + MFMA-f64 GEMM
# tiles for panel solve / trailing SYRK / blocked triangular solves.
# Matrices are padded to a multiple of 64 with an identity block (its
# factor and inverse are exact, so the un-padded region is unaffected).


def _pad64_spd(M: torch.Tensor) -> torch.Tensor:
    m = M.shape[0]
    mp = (m + 63) & ~63
    A = torch.zeros(mp, mp, dtype=torch.float64, device=M.device)
    A[:m, :m] = M
    if mp > m:
        A.diagonal()[m:] = 1.0
    return A


def _dpotrf(Apad: torch.Tensor):
    mp = Apad.shape[0]
    V = torch.empty(mp // 64, 64, 64, dtype=torch.float64,
                    device=Apad.device)
    bad = torch.zeros(1, dtype=torch.int32, device=Apad.device)
    ext.dpotrf64(Apad, V, bad)
    return V, bad


def chol_factor64(M: torch.Tensor, max_tries: int = 6):
    """Blocked fp64 Cholesky over the escalating-jitter ladder of
    ppa.jitter_ladder (PD check = the factor's breakdown flag, not an
    eigSym pass).  Returns (L_padded [mp,mp], diag-block inverses V)."""
    from ..ppa import NotPositiveDefiniteError, jitter_ladder
    for Mj in jitter_ladder(M, max_tries):
        Apad = _pad64_spd(Mj)
        V, bad = _dpotrf(Apad)
        if int(bad.item()) == 0:
            return Apad, V
    raise NotPositiveDefiniteError()


def chol_solve64(L: torch.Tensor, V: torch.Tensor, B: torch.Tensor,
                 m: int) -> torch.Tensor:
    """X = (L L^T)^{-1} B for B [m, r]; returns [m, r]."""
    mp = L.shape[0]
    Bp = torch.zeros(mp, B.shape[1], dtype=torch.float64, device=B.device)
    Bp[:m] = B
    ext.dchol_solve64(L, V, Bp)
    return Bp[:m]


def chol_inverse64(L: torch.Tensor, V: torch.Tensor, m: int) -> torch.Tensor:
    mp = L.shape[0]
    B = torch.eye(mp, dtype=torch.float64, device=L.device)
    ext.dchol_solve64(L, V, B, rhs_identity=True)
    return B[:m, :m]


def magic_vector_matrix(kernel: Kernel, KK: torch.Tensor, Ky: torch.Tensor,
                        active: torch.Tensor):
    """GPU magic quantities, entirely on the hand-written K13 kernels
    (ProjectedGaussianProcessHelper.scala:49-60 semantics; fp64)."""
    active64 = active.double()
    Kmm = kernel.training_kernel(active64)
    nu = kernel.white_noise_var()
    PD = nu * Kmm + KK

    Lp, Vp = chol_factor64(PD)
    m = KK.shape[0]
    mv = chol_solve64(Lp, Vp, Ky.unsqueeze(-1), m).squeeze(-1)
    PDinv = chol_inverse64(Lp, Vp, m)
    Lm, Vm = chol_factor64(Kmm)
    Kmminv = chol_inverse64(Lm, Vm, m)
    return mv, PDinv * nu - Kmminv


def supports_predict(kernel: Kernel, X: torch.Tensor, m: int) -> bool:
    """A canonical tree on [t, d] fp32 rows whose (m, d) the fused predict
    kernel's LDS plan takes (``ext.ppa_predict_supported``)."""
    cs = compile_kernel(kernel)
    if cs is None or cs.base not in BASES:
        return False
    if X.dtype != torch.float32 or X.dim() != 2:
        return False
    return bool(ext.ppa_predict_supported(int(m), int(X.shape[1])))


def predict(kernel: Kernel, X: torch.Tensor, active: torch.Tensor,
            mv: torch.Tensor, M: torch.Tensor, with_var: bool = True):
    """K14 in one launch (predict.hip): mean [t] and, with ``with_var``,
    var [t] in fp64, with no [t, m] array in memory."""
    cs = compile_kernel(kernel)
    theta = kernel.get_hyperparameters()
    d = X.shape[-1]
    s2 = _s2_vector(cs, theta, d, X.device)
    # k(x, x) of a canonical tree is the same for every row: amp + noise
    kxx = float(kernel.self_kernel(torch.zeros(1, d, dtype=torch.float64))[0])
    mean, var = ext.ppa_predict(
        X, active.to(X.device, torch.float32), s2, float(cs.amp(theta)),
        mv.to(X.device, torch.float64), M.to(X.device, torch.float64), kxx,
        bool(with_var),
        family=base_family(cs.base))
    return mean, var


def cross_kernel(kernel: Kernel, Xtest: torch.Tensor,
                 Xtrain: torch.Tensor) -> torch.Tensor:
    cs = compile_kernel(kernel)
    theta = kernel.get_hyperparameters()
    d = Xtest.shape[-1]
    C = cs.amp(theta)
    s2 = _s2_vector(cs, theta, d, Xtest.device)
    Kc = ext.cross_kernel_tile(Xtest.to(torch.float32).contiguous(),
                               Xtrain.to(torch.float32).contiguous(),
                               s2, float(C), False, False, False,
                               family=base_family(cs.base))[0]
    return Kc.to(Xtest.dtype)

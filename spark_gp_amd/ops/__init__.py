"""Compute-op dispatch: hand-written HIP/CDNA4 kernels on MI355X, batched
PyTorch everywhere else.

Policy (see repo README):
* On a CUDA/ROCm device, ops covered by the HIP extension MUST run through it;
  if the extension is missing on a GPU machine the op raises instead of
  silently falling back to eager PyTorch (set
  ``SPARK_GP_AMD_ALLOW_TORCH_FALLBACK=1`` to override, e.g. for A/B
  comparisons in tests).
* On CPU the torch backend is the float64 oracle.
"""

from __future__ import annotations

import os
from typing import Optional, Tuple

import numpy as np
import torch

from ..kernels.base import Kernel
from ..kernels.compiled import BASES, CompiledKernel, compile_kernel
from . import torch_backend

_hip = None
_hip_err: Optional[str] = None


def _load_hip():
    global _hip, _hip_err
    if _hip is not None or _hip_err is not None:
        return _hip
    try:
        from . import hip_backend
        _hip = hip_backend
    except Exception as e:  # extension not built / not importable
        _hip_err = f"{type(e).__name__}: {e}"
    return _hip


def _env_set(name: str) -> bool:
    return os.environ.get(name, "0") == "1"


def hip_available() -> bool:
    return _load_hip() is not None


def _backend_for(what: str, t: torch.Tensor, required: bool = True):
    """Which backend runs op ``what`` on tensor ``t``: the HIP backend
    module, or None for the torch path (CPU tensor, the debug/A-B switch
    SPARK_GP_AMD_FORCE_TORCH, or a missing extension where ``required`` or
    the fallback switch allow it; raises otherwise)."""
    if not t.is_cuda or _env_set("SPARK_GP_AMD_FORCE_TORCH"):
        return None
    hip = _load_hip()
    if hip is None and required and \
            not _env_set("SPARK_GP_AMD_ALLOW_TORCH_FALLBACK"):
        raise RuntimeError(
            f"{what}: running on a GPU but the spark_gp_amd HIP extension is "
            f"not loadable ({_hip_err}); build it with `python setup.py "
            f"build_ext --inplace` (PYTORCH_ROCM_ARCH=gfx950) or set "
            f"SPARK_GP_AMD_ALLOW_TORCH_FALLBACK=1 to explicitly allow the "
            f"eager PyTorch path")
    return hip


def nll_grad_compiled(cs: CompiledKernel, theta: np.ndarray,
                      X: torch.Tensor, y: torch.Tensor
                      ) -> Tuple[float, np.ndarray]:
    hip = (_backend_for("nll_grad_compiled", X)
           if cs.base in BASES else None)
    if hip is not None and hip.supports_nll(cs, X):
        return hip.nll_grad_compiled(cs, theta, X, y)
    return torch_backend.nll_grad_compiled(cs, theta, X, y)


def nll_grad_generic(kernel: Kernel, theta: np.ndarray,
                     X: torch.Tensor, y: torch.Tensor):
    return torch_backend.nll_grad_generic(kernel, theta, X, y)


def laplace_nll_grad(kernel: Kernel, theta: np.ndarray, X: torch.Tensor,
                     y: torch.Tensor, f: torch.Tensor, tol: float,
                     max_newton_iter: int = 200, likelihood=None):
    from ..kernels.compiled import compile_kernel
    from ..likelihoods import LogisticLikelihood
    logistic = likelihood is None or isinstance(likelihood,
                                                LogisticLikelihood)
    # the fused HIP Newton kernel implements the logistic link on compiled
    # kernels; everything else runs on the batched torch path
    cs = compile_kernel(kernel) if X.is_cuda and logistic else None
    hip = _backend_for("laplace_nll_grad", X) if cs is not None else None
    if hip is not None:
        if tol >= hip.LAPLACE_MIN_TOL and \
                hip.supports_laplace_evidence(cs, X):
            # fully fused K10+K11: Newton AND the Algorithm 5.1 evidence
            # in one launch; None -> fp32 breakdown, warm torch fallback
            res = hip.laplace_evidence(cs, theta, X, y, f, tol,
                                       max_newton_iter)
            if res is not None:
                return res
            return torch_backend.laplace_nll_grad(
                kernel, theta, X, y, f, tol, max_newton_iter)
        if hip.supports_laplace(cs, X):
            # fused Newton loop runs each expert to convergence on the GPU
            # (updates f in place); the torch pass below then converges in
            # 2-3 cheap iterations and computes the Algorithm 5.1 evidence
            # with the reference's exact semantics.
            n_bad = hip.laplace_newton(cs, theta, X, y, f, tol,
                                       max_newton_iter)
            if n_bad == 0 and tol >= hip.LAPLACE_MIN_TOL:
                # Algorithm 5.1 at the converged f via the contraction
                # form — no [E, p, k, k] derivative tensor
                return torch_backend.laplace_evidence_compiled(
                    cs, theta, X, y, f)
            # Some experts fell back, or the user asked for a tol tighter
            # than the fp32 kernel's clamp (LAPLACE_MIN_TOL): the torch
            # Newton polish continues from the warm f with the exact
            # requested tolerance (a few cheap iterations).
            return torch_backend.laplace_nll_grad(
                kernel, theta, X, y, f, tol, max_newton_iter)
    return torch_backend.laplace_nll_grad(kernel, theta, X, y, f, tol,
                                          max_newton_iter,
                                          likelihood=likelihood)


def kmn_knm_and_kmny(kernel: Kernel, active: torch.Tensor,
                     X: torch.Tensor, y: torch.Tensor,
                     chunk_rows: int = 262144, precision: str = "fp64"):
    hip = _backend_for("kmn_knm_and_kmny", X)
    if hip is not None and hip.supports_ppa(kernel, X):
        return hip.kmn_knm_and_kmny(kernel, active, X, y, chunk_rows,
                                    precision)
    return torch_backend.kmn_knm_and_kmny(kernel, active, X, y, chunk_rows)


def magic_vector_matrix(kernel: Kernel, KK: torch.Tensor, Ky: torch.Tensor,
                        active: torch.Tensor):
    """On the K13 kernels; None where ppa's CPU oracle should run."""
    hip = _backend_for("magic_vector_matrix", KK)
    return hip and hip.magic_vector_matrix(kernel, KK, Ky, active)


def cross_kernel(kernel: Kernel, Xtest: torch.Tensor, Xtrain: torch.Tensor):
    """Cross-kernel dispatch for prediction paths (the torch kernel serves
    where the extension is missing)."""
    hip = _backend_for("cross_kernel", Xtest, required=False)
    if hip is not None and hip.supports_ppa(kernel, Xtest):
        return hip.cross_kernel(kernel, Xtest, Xtrain)
    return kernel.cross_kernel(Xtest, Xtrain)


def predict_stream(kernel: Kernel, X: torch.Tensor, active: torch.Tensor,
                   mv: torch.Tensor, M: torch.Tensor, with_var: bool = True,
                   chunk_rows: int = 262144):
    """PPA mean [t] and (``with_var``) variance [t] in fp64 with peak memory
    bounded independently of t: the fused HIP kernel (no [t, m] array at
    all) where its gate takes the kernel tree and (m, d); otherwise the
    staged cross-kernel / GEMV / quadratic form over row chunks of
    ``chunk_rows`` — any tree, any m, and on CPU."""
    cs = compile_kernel(kernel)
    hip = (_backend_for("predict_stream", X)
           if cs is not None and cs.base in BASES else None)
    if hip is not None and hip.supports_predict(kernel, X, active.shape[0]):
        return hip.predict(kernel, X, active, mv, M, with_var)
    if chunk_rows < 1:
        raise ValueError(f"chunk_rows must be >= 1, got {chunk_rows}")
    t = X.shape[0]
    mv = mv.to(X.device)
    mean = torch.empty(t, dtype=torch.float64, device=X.device)
    var = torch.empty_like(mean) if with_var else None
    if with_var:
        M = M.to(X.device)
    for s in range(0, t, chunk_rows):
        e = min(t, s + chunk_rows)
        cross = cross_kernel(kernel, X[s:e], active).double()
        mean[s:e] = cross @ mv
        if with_var:
            var[s:e] = (kernel.self_kernel(X[s:e]).double()
                        + ((cross @ M) * cross).sum(-1))
    return mean, var

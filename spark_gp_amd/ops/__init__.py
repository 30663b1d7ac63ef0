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
                      X: torch.Tensor, y: torch.Tensor, panel: bool = False,
                      fused_fp64: bool = False) -> Tuple[float, np.ndarray]:
    """``panel``: let experts of 128 < k <= 1024 rows (d <= 128, fp32, on
    the GPU) take the fused HIP panel kernel.  Default False: those shapes
    take the batched torch path, as before; every other input takes the
    path it always took, whatever ``panel`` says.

    ``fused_fp64``: let experts of k <= 128 rows (d <= 128, fp32 or fp64,
    contiguous, on the GPU) take the full-fp64 fused HIP kernel: the fp64
    objective of the rows as given.  Ignored on the CPU and where that
    kernel's gate refuses; default False changes nothing."""
    hip = (_backend_for("nll_grad_compiled", X)
           if cs.base in BASES else None)
    if fused_fp64 and hip is not None and hip.supports_nll_f64(cs, X):
        return hip.nll_grad_compiled(cs, theta, X, y, f64=True)
    if hip is not None and hip.supports_nll(cs, X):
        return hip.nll_grad_compiled(cs, theta, X, y)
    if panel and hip is not None and hip.supports_nll_panel(cs, X):
        return hip.nll_grad_compiled(cs, theta, X, y, panel=True)
    return torch_backend.nll_grad_compiled(cs, theta, X, y)


def nll_grad_generic(kernel: Kernel, theta: np.ndarray,
                     X: torch.Tensor, y: torch.Tensor):
    return torch_backend.nll_grad_generic(kernel, theta, X, y)


def laplace_nll_grad(kernel: Kernel, theta: np.ndarray, X: torch.Tensor,
                     y: torch.Tensor, f: torch.Tensor, tol: float,
                     max_newton_iter: int = 200, likelihood=None,
                     fused_matern: bool = False, fused_wide: bool = False,
                     fused_probit: bool = False):
    """``fused_matern``: let the Matern 3/2 and 5/2 bases take the fused HIP
    Laplace kernels as well (opt-in; the RBF bases always do).
    ``fused_wide``: let RBF-base experts with more feature dimensions than
    rows (up to 1024) take the streamed-feature HIP kernels (opt-in; without
    it those shapes run the batched torch path).
    ``fused_probit``: let a ``ProbitLikelihood`` on an RBF base take the
    fused HIP kernels' probit instantiations, through the branches the
    logistic link takes (opt-in; without it, and for every other
    likelihood, a non-logistic call runs the batched torch path)."""
    from ..kernels.compiled import compile_kernel
    from ..likelihoods import LogisticLikelihood, ProbitLikelihood
    logistic = likelihood is None or isinstance(likelihood,
                                                LogisticLikelihood)
    probit = fused_probit and isinstance(likelihood, ProbitLikelihood)
    # the fused HIP Newton kernel implements the logistic link, and the
    # probit link on request, on compiled kernels; everything else runs on
    # the batched torch path
    cs = compile_kernel(kernel) if X.is_cuda and (logistic or probit) \
        else None
    hip = _backend_for("laplace_nll_grad", X) if cs is not None else None
    if probit and hip is not None and \
            not hip.supports_laplace_link(cs, "probit", fused_matern):
        hip = None
    # a probit call names its link to the kernels and its likelihood to every
    # torch pass behind them; a logistic call is the call it always was
    link = {"link": "probit"} if probit else {}
    lik = {"likelihood": likelihood} if probit else {}
    if hip is not None:
        if tol >= hip.LAPLACE_MIN_TOL and \
                hip.supports_laplace_evidence(cs, X, fused_matern):
            # fully fused K10+K11: Newton AND the Algorithm 5.1 evidence
            # in one launch; None -> fp32 breakdown, warm torch fallback
            res = hip.laplace_evidence(cs, theta, X, y, f, tol,
                                       max_newton_iter, **link)
            if res is not None:
                return res
            return torch_backend.laplace_nll_grad(
                kernel, theta, X, y, f, tol, max_newton_iter, **lik)
        if hip.supports_laplace(cs, X, fused_matern):
            # fused Newton loop runs each expert to convergence on the GPU
            # (updates f in place); the torch pass below then converges in
            # 2-3 cheap iterations and computes the Algorithm 5.1 evidence
            # with the reference's exact semantics.
            n_bad = hip.laplace_newton(cs, theta, X, y, f, tol,
                                       max_newton_iter, **link)
            if n_bad == 0 and tol >= hip.LAPLACE_MIN_TOL:
                # Algorithm 5.1 at the converged f via the contraction
                # form — no [E, p, k, k] derivative tensor
                return torch_backend.laplace_evidence_compiled(
                    cs, theta, X, y, f, **lik)
            # Some experts fell back, or the user asked for a tol tighter
            # than the fp32 kernel's clamp (LAPLACE_MIN_TOL): the torch
            # Newton polish continues from the warm f with the exact
            # requested tolerance (a few cheap iterations).
            return torch_backend.laplace_nll_grad(
                kernel, theta, X, y, f, tol, max_newton_iter, **lik)
        if fused_wide and hip.supports_laplace_wide(cs, X):
            # the two branches above on laplace_wide.hip, which streams X
            # (d > k, up to 1024 dimensions)
            if tol >= hip.LAPLACE_MIN_TOL:
                res = hip.laplace_evidence(cs, theta, X, y, f, tol,
                                           max_newton_iter, wide=True,
                                           **link)
                if res is not None:
                    return res
            else:
                hip.laplace_newton(cs, theta, X, y, f, tol, max_newton_iter,
                                   wide=True, **link)
            return torch_backend.laplace_nll_grad(
                kernel, theta, X, y, f, tol, max_newton_iter, **lik)
    return torch_backend.laplace_nll_grad(kernel, theta, X, y, f, tol,
                                          max_newton_iter,
                                          likelihood=likelihood)


def kmn_knm_and_kmny(kernel: Kernel, active: torch.Tensor,
                     X: torch.Tensor, y: torch.Tensor,
                     chunk_rows: int = 262144, precision: str = "fp64",
                     fused_fp64: bool = False):
    """``fused_fp64``: the HIP backend's fp64 branch on the f64 matrix cores
    (opt-in; the torch backend is fp64 throughout and ignores it)."""
    hip = _backend_for("kmn_knm_and_kmny", X)
    if hip is not None and hip.supports_ppa(kernel, X):
        if not fused_fp64:
            return hip.kmn_knm_and_kmny(kernel, active, X, y, chunk_rows,
                                        precision)
        return hip.kmn_knm_and_kmny(kernel, active, X, y, chunk_rows,
                                    precision, fused_fp64=True)
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


def greedy_state(kernel: Kernel, X: torch.Tensor, y: torch.Tensor, m: int):
    """State object of the incremental greedy forward selection of ``m``
    points among the local rows (``append`` / ``scores`` / ``best``): on the
    kernels of greedy.hip where the tree is canonical and the gate takes
    (n, m, d), in fp64 torch otherwise (any tree, and on CPU)."""
    hip = _backend_for("greedy_state", X)
    if hip is not None and hip.supports_greedy(kernel, X, m):
        return hip.GreedyState(kernel, X, y, m)
    return torch_backend.GreedyState(kernel, X, y, m)


def kmeans_step(X: torch.Tensor, centers: torch.Tensor,
                chunk_rows: int = 1 << 18, work=None):
    """One Lloyd step, ``(sums, counts, assign)`` with fp64 sums [m, d] and
    counts [m]: on the kernels of kmeans.hip where the gate takes X and the
    centres (contiguous fp32, m up to 8192), in torch over chunks of
    ``chunk_rows`` rows otherwise (any dtype, and on CPU).  ``work``: a dict
    the caller keeps across the steps of a loop, for the HIP buffers."""
    hip = _backend_for("kmeans_step", X)
    if hip is not None and hip.supports_kmeans(X, centers):
        return hip.kmeans_step(X, centers, work)
    return torch_backend.kmeans_step(X, centers, chunk_rows, work)


def predict_stream(kernel: Kernel, X: torch.Tensor, active: torch.Tensor,
                   mv: torch.Tensor, M: torch.Tensor, with_var: bool = True,
                   chunk_rows: int = 262144, stream=True):
    """PPA mean [t] and (``with_var``) variance [t] in fp64 with peak memory
    bounded independently of t: the fused HIP kernel (no [t, m] array at
    all) where its gate takes the kernel tree and (m, d); otherwise the
    staged cross-kernel / GEMV / quadratic form over row chunks of
    ``chunk_rows`` — any tree, any m, and on CPU.

    ``stream="wide"`` (as the predict methods take it) puts the wide fused
    kernel between the two: where the first gate refuses and its own takes
    the call (m up to 8192), one launch with a scratch of
    min(ceil(t / 128), compute units) x 128 x m floats."""
    if isinstance(stream, str) and stream != "wide":
        raise ValueError(f"stream must be a bool or 'wide', got {stream!r}")
    cs = compile_kernel(kernel)
    hip = (_backend_for("predict_stream", X)
           if cs is not None and cs.base in BASES else None)
    if hip is not None and hip.supports_predict(kernel, X, active.shape[0]):
        return hip.predict(kernel, X, active, mv, M, with_var)
    if (stream == "wide" and hip is not None
            and hip.supports_predict_wide(kernel, X, active.shape[0])):
        return hip.predict_wide(kernel, X, active, mv, M, with_var)
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

"""Binary Gaussian Process Classification (logistic link, Laplace
approximation).

Mirrors ``classification/GaussianProcessClassifier.scala``: per-expert Newton
optimization of the latent posterior (R&W Algorithm 3.1 with step halving),
Algorithm 5.1 approximate evidence + gradient, latent f warm-started across
L-BFGS evaluations, and the PPA fit on the latent f as regression target
(``GaussianProcessClassifier.scala:62-65``).
"""

from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from .. import ops
from ..parallel.dist import get_comm
from ..utils.instrumentation import Instrumentation
from .base import GaussianProcessCommons, group_experts
from .predictor import GaussianProjectedProcessRawPredictor


class GaussianProcessClassifier(GaussianProcessCommons):
    _PARAMS = dict(GaussianProcessCommons._PARAMS,
                   max_newton_iter="_max_newton_iter",
                   link="_link")

    def __init__(self, **params):
        self._max_newton_iter = 200
        self._link = "logistic"
        super().__init__(**params)

    def setMaxNewtonIter(self, v: int):
        self._max_newton_iter = int(v)
        return self

    def setLink(self, link: str):
        """Response link: 'logistic' (the reference's sigmoid link,
        default) or 'probit' (Phi link; BASELINE config 3).  Algorithms
        3.1/5.1 only touch the likelihood through log p and its first
        three f-derivatives (see ``likelihoods.py``)."""
        if link not in ("logistic", "probit"):
            raise ValueError("link must be 'logistic' or 'probit'")
        self._link = link
        return self

    def _resolve_likelihood(self):
        from ..likelihoods import LogisticLikelihood, ProbitLikelihood
        return (LogisticLikelihood() if self._link == "logistic"
                else ProbitLikelihood())

    def fit(self, X, y) -> "GaussianProcessClassificationModel":
        instr = Instrumentation("GaussianProcessClassifier")
        comm = get_comm()
        Xt, yt = self._prepare(X, y)

        # labels must be {0, 1} (``GaussianProcessClassifier.scala:68-72``);
        # C8: allreduce(MIN) of the local check
        ok = bool(torch.isin(yt, torch.tensor([0.0, 1.0], dtype=yt.dtype,
                                              device=yt.device)).all())
        ok = comm.allreduce_scalar(1.0 if ok else 0.0, op="min") > 0.5
        if not ok:
            raise ValueError("only 0 and 1 labels are supported")

        groups = group_experts(Xt, yt, self._dataset_size_for_expert)
        kernel = self._get_kernel()
        lik = self._resolve_likelihood()
        # latent f per expert, zero-initialized, warm-started across evals
        fs = [torch.zeros_like(yg) for _, _, yg in groups]

        def local_obj(theta: np.ndarray) -> Tuple[float, np.ndarray]:
            nll_total, grad_total = 0.0, np.zeros_like(theta)
            for (idx, Xg, yg), fg in zip(groups, fs):
                nll, grad = ops.laplace_nll_grad(
                    kernel, theta, Xg, yg, fg, self._tol,
                    self._max_newton_iter, likelihood=lik)
                nll_total += nll
                grad_total += grad
            return nll_total, grad_total

        theta = self._optimize_hypers(instr, comm, local_obj)
        # refresh f at theta* (one more Laplace pass, ref :60)
        local_obj(theta)

        # PPA over (f, kernel): latent targets replace the labels
        f_flat = torch.empty_like(yt)
        for (idx, _, _), fg in zip(groups, fs):
            f_flat[idx] = fg.reshape(-1)
        raw = self._produce_predictor(instr, comm, Xt, f_flat, theta)
        instr.log_success()
        model = GaussianProcessClassificationModel(raw, link=self._link)
        model._instr = instr
        self.model_ = model           # sklearn-interop handle
        return model


class GaussianProcessClassificationModel:
    num_classes = 2

    def __init__(self, raw: GaussianProjectedProcessRawPredictor,
                 link: str = "logistic"):
        self.raw = raw
        self.link = link
        self._instr: Optional[Instrumentation] = None

    def _squash(self, f: torch.Tensor) -> torch.Tensor:
        return (torch.sigmoid(f) if self.link == "logistic"
                else torch.special.ndtr(f))

    def _squash_np(self, z: np.ndarray) -> np.ndarray:
        if self.link == "logistic":
            return 1.0 / (1.0 + np.exp(-z))
        from scipy.special import ndtr
        return ndtr(z)

    def _latent(self, X, stream: bool = False, chunk_rows: int = 262144
                ) -> Tuple[torch.Tensor, torch.Tensor]:
        """Latent (mean, var); ``stream=True`` bounds peak memory for any
        number of rows (the raw predictor's ``predict``)."""
        Xt = torch.as_tensor(X, dtype=self.raw.active_set.dtype,
                             device=self.raw.active_set.device)
        if Xt.dim() == 1:
            Xt = Xt.unsqueeze(0)
        if stream:
            return self.raw.predict(Xt, with_var=True, stream=True,
                                    chunk_rows=chunk_rows)
        return self.raw.predict(Xt, with_var=True)

    def predict_raw(self, X, stream: bool = False,
                    chunk_rows: int = 262144) -> np.ndarray:
        """(-f, f) scores per row (``GaussianProcessClassifier.scala:153-156``)."""
        f, _ = self._latent(X, stream, chunk_rows)
        f = f.cpu().numpy()
        return np.stack([-f, f], axis=-1)

    def predict_proba(self, X, averaged: bool = False,
                      quadrature_points: int = 32, stream: bool = False,
                      chunk_rows: int = 262144) -> np.ndarray:
        """[p(y=0), p(y=1)] per row.

        Default: sigmoid of the latent mean, matching the reference's
        ``raw2probabilityInPlace`` (:141-149).  ``averaged=True`` additionally
        integrates the sigmoid over the latent posterior with Gauss-Hermite
        quadrature — the capability the reference's dead ``Integrator``
        (``commons/util/Integrator.scala``) was built for."""
        f, var = self._latent(X, stream, chunk_rows)
        if averaged:
            from ..utils.integrator import Integrator
            integ = Integrator(quadrature_points)
            p1 = integ.expected_of_function_of_normal_batch(
                f.cpu().numpy(), var.clamp_min(0.0).cpu().numpy(),
                self._squash_np)
        else:
            p1 = self._squash(f).cpu().numpy()
        return np.stack([1.0 - p1, p1], axis=-1)

    def predict(self, X, stream: bool = False,
                chunk_rows: int = 262144) -> np.ndarray:
        f, _ = self._latent(X, stream, chunk_rows)
        return (f.cpu().numpy() > 0).astype(np.float64)

    def transform(self, X):
        return self.predict(X)

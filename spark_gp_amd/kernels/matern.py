"""Matérn-family stationary kernels (additive capability — the reference
ships only the RBF family, ``kernel/RBFKernel.scala`` /
``kernel/ARDRBFKernel.scala``; Matérn 3/2 and 5/2 are the standard
rough-process complements, Rasmussen & Williams ch. 4.2).

Isotropic, one trainable lengthscale ``l``:

* ``Matern32Kernel`` — k(r) = (1 + s) exp(-s),            s = sqrt(3) r / l,
  dk/dl = s^2 exp(-s) / l.
* ``Matern52Kernel`` — k(r) = (1 + s + s^2/3) exp(-s),    s = sqrt(5) r / l,
  dk/dl = s^2 (1 + s) exp(-s) / (3 l).

ARD, one trainable inverse lengthscale ``beta_j`` per input dimension, with
``ARDRBFKernel``'s constructors, bounds and hyperparameter layout:

* ``ARDMatern32Kernel`` / ``ARDMatern52Kernel`` — the same k(s) at
  s = sqrt(nu' ||(a - b) o beta||^2), nu' = 3 resp. 5.

All four share one form in the scaled squared distance q = s^2 (t = sqrt q):

    Kb(q) = (1 + t) e^-t            Kd(q) := -dKb/dq = e^-t / 2          (3/2)
    Kb(q) = (1 + t + t^2/3) e^-t    Kd(q) = (1 + t) e^-t / 6             (5/2)

so dk/dbeta_j = -2 nu' Kd beta_j (a_j - b_j)^2, with no singularity at t = 0.

They plug into the same DSL (`+`, scalar `*`, ``TrainableScalar``).  A tree
``C * Matern + noise`` canonicalizes (``kernels/compiled.py``) and trains on
the fused objective — the hand-written HIP kernels on a GPU, instantiated per
family — and predicts through the HIP cross kernel and PPA accumulation.
Other trees (two stationary bases, say) run the generic path through the
materialized derivatives below.  The fused Laplace kernels stay RBF-only: a
Matérn classifier runs the torch Laplace path.
"""

from __future__ import annotations

import math
from typing import Tuple

import numpy as np
import torch

from .base import Kernel, sqdist, _as_f64
from .rbf import ARDRBFKernel

_EPS = 1e-30  # guards r=0 in d/dl (the derivative -> 0 there anyway)


class _MaternBase(Kernel):
    def __init__(self, l: float = 1.0, lower: float = 1e-6,
                 upper: float = math.inf):
        self.l = float(l)
        self.lower = float(lower)
        self.upper = float(upper)

    def get_hyperparameters(self):
        return np.array([self.l])

    def set_hyperparameters(self, value):
        self.l = float(_as_f64(value)[0])
        return self

    @property
    def num_hyperparameters(self):
        return 1

    def hyperparameter_bounds(self):
        return np.array([self.lower]), np.array([self.upper])

    def white_noise_var(self):
        return 0.0

    def training_kernel_diag(self, X):
        return torch.ones(X.shape[:-1], dtype=X.dtype, device=X.device)

    def self_kernel(self, Xtest):
        return torch.ones(Xtest.shape[:-1], dtype=Xtest.dtype,
                          device=Xtest.device)

    def _r(self, A, B):
        return torch.sqrt(sqdist(A, B).clamp_min(0.0) + _EPS)


class Matern32Kernel(_MaternBase):
    def _k_of_s(self, s):
        return (1.0 + s) * torch.exp(-s)

    def training_kernel(self, X):
        s = self._r(X, X) * (math.sqrt(3.0) / self.l)
        return self._k_of_s(s)

    def training_kernel_and_derivative(self, X) -> Tuple[torch.Tensor, torch.Tensor]:
        s = self._r(X, X) * (math.sqrt(3.0) / self.l)
        e = torch.exp(-s)
        K = (1.0 + s) * e
        dK = (s * s * e / self.l).unsqueeze(-3)          # [..., 1, n, n]
        return K, dK

    def cross_kernel(self, Xtest, Xtrain):
        s = self._r(Xtest, Xtrain) * (math.sqrt(3.0) / self.l)
        return self._k_of_s(s)

    def __repr__(self):
        return f"Matern32Kernel(l={self.l:.1e})"


class Matern52Kernel(_MaternBase):
    def _k_of_s(self, s):
        return (1.0 + s + s * s / 3.0) * torch.exp(-s)

    def training_kernel(self, X):
        s = self._r(X, X) * (math.sqrt(5.0) / self.l)
        return self._k_of_s(s)

    def training_kernel_and_derivative(self, X) -> Tuple[torch.Tensor, torch.Tensor]:
        s = self._r(X, X) * (math.sqrt(5.0) / self.l)
        e = torch.exp(-s)
        K = (1.0 + s + s * s / 3.0) * e
        dK = (s * s * (1.0 + s) * e / (3.0 * self.l)).unsqueeze(-3)
        return K, dK

    def cross_kernel(self, Xtest, Xtrain):
        s = self._r(Xtest, Xtrain) * (math.sqrt(5.0) / self.l)
        return self._k_of_s(s)

    def __repr__(self):
        return f"Matern52Kernel(l={self.l:.1e})"


class _ARDMaternBase(Kernel):
    """k = Kb(nu' ||(a - b) o beta||^2); constructors, bounds and layout are
    ``ARDRBFKernel``'s."""

    NUP = 0.0                     # nu': 3 (Matérn 3/2) or 5 (Matérn 5/2)

    __init__ = ARDRBFKernel.__init__
    get_hyperparameters = ARDRBFKernel.get_hyperparameters
    set_hyperparameters = ARDRBFKernel.set_hyperparameters
    num_hyperparameters = ARDRBFKernel.num_hyperparameters
    hyperparameter_bounds = ARDRBFKernel.hyperparameter_bounds
    white_noise_var = ARDRBFKernel.white_noise_var
    training_kernel_diag = ARDRBFKernel.training_kernel_diag
    self_kernel = ARDRBFKernel.self_kernel
    _beta_t = ARDRBFKernel._beta_t

    @staticmethod
    def _kb_kd(t):
        """(Kb, Kd) at t = sqrt(q)."""
        raise NotImplementedError

    def _t(self, A, B):
        s = self._beta_t(B) * math.sqrt(self.NUP)
        return torch.sqrt(sqdist(A * s, B * s).clamp_min(0.0))

    def training_kernel(self, X):
        return self._kb_kd(self._t(X, X))[0]

    def training_kernel_and_derivative(self, X):
        K, Kd = self._kb_kd(self._t(X, X))
        beta = self._beta_t(X)
        diff = X.unsqueeze(-2) - X.unsqueeze(-3)          # [..., n, n, d]
        dK = (-2.0 * self.NUP * beta) * (diff * diff)     # [..., n, n, d]
        dK = dK.permute(*range(dK.dim() - 3), -1, -3, -2) # [..., d, n, n]
        return K, dK * Kd.unsqueeze(-3)

    def cross_kernel(self, Xtest, Xtrain):
        return self._kb_kd(self._t(Xtest, Xtrain))[0]

    def __repr__(self):
        vals = ", ".join(f"{b:.1e}" for b in self.beta)
        return f"{type(self).__name__}(beta=[{vals}])"


class ARDMatern32Kernel(_ARDMaternBase):
    NUP = 3.0

    @staticmethod
    def _kb_kd(t):
        e = torch.exp(-t)
        return (1.0 + t) * e, 0.5 * e


class ARDMatern52Kernel(_ARDMaternBase):
    NUP = 5.0

    @staticmethod
    def _kb_kd(t):
        e = torch.exp(-t)
        return (1.0 + t + t * t / 3.0) * e, (1.0 + t) * e / 6.0

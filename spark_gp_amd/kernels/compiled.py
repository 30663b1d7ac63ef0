"""Kernel-tree canonicalization for the fused training fast path.

The effective training kernel is always
``user_kernel + sigma2.const * EyeKernel`` (see
``commons/GaussianProcessCommons.scala:18``).  The flagship shapes —
``1 * ARDRBFKernel(d) + noise`` and ``1 * RBFKernel(s) + noise`` — canonicalize
to

    K(theta) = C * Kb(theta_base)  +  nu(theta) * I

with Kb a single stationary base, C either a constant or one trainable hyper,
and nu = const + sum of trainable white-noise hypers.  Six bases are
recognised, each a function of q = ||(a - b) o s||^2 in coordinates scaled
per dimension by s:

    base       class               family       c         s_j
    'rbf'      RBFKernel           exp(-q)      1/sqrt(2) c / sigma
    'ard'      ARDRBFKernel        exp(-q)      1         c beta_j
    'm32'      Matern32Kernel      Matérn 3/2   sqrt(3)   c / l
    'ard_m32'  ARDMatern32Kernel   Matérn 3/2   sqrt(3)   c beta_j
    'm52'      Matern52Kernel      Matérn 5/2   sqrt(5)   c / l
    'ard_m52'  ARDMatern52Kernel   Matérn 5/2   sqrt(5)   c beta_j

(``base_family``, ``base_nup``, ``base_is_ard``, ``base_scale`` and its
transposed Jacobian ``base_scale_grad`` below; the family functions Kb(q) and
Kd(q) = -dKb/dq are in ``kernels/matern.py``.)  Every gradient over theta is
assembled here, by ``CompiledKernel.assemble_grad``, from a gradient with
respect to s, the amplitude and the noise.  The
fused objective (torch batched or the hand-written HIP kernel) consumes this
``CompiledKernel`` and computes the per-expert negative log marginal
likelihood *and its full gradient* without ever materializing the
``[p, k, k]`` derivative tensor the reference builds per expert
(``kernel/ARDRBFKernel.scala:61-79``).

Trees that do not match the pattern (two stationary bases in one tree, nested
trainable scalars, ...) fall back to the generic batched path
(materialized derivatives) — full API generality is preserved.
"""

from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

from .base import (ConstantTimesKernel, EyeKernel, Kernel, SumOfKernels,
                   TrainableScalarTimesKernel)
from .matern import (ARDMatern32Kernel, ARDMatern52Kernel, Matern32Kernel,
                     Matern52Kernel)
from .rbf import ARDRBFKernel, RBFKernel

# covariance family codes, as in ops/csrc/kernel_geom.h (GEOM_FAM_*)
FAM_RBF, FAM_M32, FAM_M52 = 0, 1, 2

# base string of each recognised class, and per base: (family code, nu', ARD)
_BASE_OF = {RBFKernel: 'rbf', ARDRBFKernel: 'ard',
            Matern32Kernel: 'm32', Matern52Kernel: 'm52',
            ARDMatern32Kernel: 'ard_m32', ARDMatern52Kernel: 'ard_m52'}
_BASE_INFO = {'rbf': (FAM_RBF, None, False), 'ard': (FAM_RBF, None, True),
              'm32': (FAM_M32, 3.0, False), 'ard_m32': (FAM_M32, 3.0, True),
              'm52': (FAM_M52, 5.0, False), 'ard_m52': (FAM_M52, 5.0, True)}
BASES = tuple(_BASE_INFO)
RBF_BASES = ('ard', 'rbf')


def base_family(base: str) -> int:
    """Family code the HIP kernels are instantiated for."""
    return _BASE_INFO[base][0]


def base_nup(base: str) -> Optional[float]:
    """nu' of a Matérn base (3 or 5: q = nu' r^2 / l^2); None for RBF."""
    return _BASE_INFO[base][1]


def base_is_ard(base: str) -> bool:
    """One scale hyper per input dimension (else a single length hyper)."""
    return _BASE_INFO[base][2]


def base_scale(base: str, theta_base, d: int) -> np.ndarray:
    """The [d] coordinate scale s of the table above, in fp64."""
    nup = base_nup(base)
    if base_is_ard(base):
        s = np.asarray(theta_base, dtype=np.float64)
        return s if nup is None else math.sqrt(nup) * s
    length = float(theta_base[0])
    return np.full(d, 1.0 / (math.sqrt(2.0) * length) if nup is None
                   else math.sqrt(nup) / length)


def base_scale_grad(base: str, theta_base, g_s) -> np.ndarray:
    """Gradient over the base hypers of a function whose gradient over
    s = base_scale(base, theta_base, d) is ``g_s`` [d]: the transpose of
    base_scale's Jacobian, one entry per base hyper.  With c of the table,
    s = c beta gives g_beta = c g_s and s_j = c / l gives
    g_l = -(c / l^2) sum(g_s)."""
    nup = base_nup(base)
    g_s = np.asarray(g_s, dtype=np.float64)
    if base_is_ard(base):
        c = 1.0 if nup is None else math.sqrt(nup)
        return c * g_s
    c = math.sqrt(0.5 if nup is None else nup)
    length = float(theta_base[0])
    return np.array([-(c / length ** 2) * g_s.sum()])


@dataclass
class CompiledKernel:
    """Canonical form  C * base(theta_base) + nu * I.

    Index fields refer to positions in the *global* hyperparameter vector of
    the kernel tree (reference layout: Sum concatenates, TrainableScalar
    prepends)."""

    p: int                               # total number of hyperparameters
    base: str                            # one of BASES
    base_idx: slice                      # slice of theta for the base kernel
    amp_idx: Optional[int]               # index of trainable amplitude C, or None
    amp_const: float                     # amplitude when amp_idx is None
    noise_const: float                   # constant white-noise variance
    noise_idx: List[int] = field(default_factory=list)  # trainable noise hypers

    def amp(self, theta) -> float:
        return float(theta[self.amp_idx]) if self.amp_idx is not None else self.amp_const

    def noise(self, theta) -> float:
        return self.noise_const + sum(float(theta[i]) for i in self.noise_idx)

    def assemble_grad(self, theta, g_scale, g_amp: float,
                      g_noise: float) -> np.ndarray:
        """The [p] gradient over theta from its gradient over the coordinate
        scale s ([d]), the amplitude C and the noise nu."""
        grad = np.zeros(self.p)
        if self.amp_idx is not None:
            grad[self.amp_idx] = g_amp
        grad[self.base_idx] = base_scale_grad(self.base, theta[self.base_idx],
                                              g_scale)
        for i in self.noise_idx:
            grad[i] += g_noise
        return grad


class _Acc:
    def __init__(self):
        self.base = None          # (base, base_idx_slice, amp_idx, amp_const)
        self.noise_const = 0.0
        self.noise_idx: List[int] = []
        self.ok = True


def _walk(k: Kernel, offset: int, scale_const: float,
          scale_idx: Optional[int], acc: _Acc) -> int:
    """Walk the tree accumulating canonical terms.  Returns hypers consumed.

    ``scale_const``/``scale_idx``: the product of enclosing scalar factors —
    at most one may be trainable for the pattern to hold."""
    if isinstance(k, SumOfKernels):
        n1 = _walk(k.k1, offset, scale_const, scale_idx, acc)
        n2 = _walk(k.k2, offset + n1, scale_const, scale_idx, acc)
        return n1 + n2
    if isinstance(k, TrainableScalarTimesKernel):
        if scale_idx is not None:
            acc.ok = False          # nested trainable scalars: not canonical
            return k.num_hyperparameters
        _walk(k.kernel, offset + 1, scale_const, offset, acc)
        return k.num_hyperparameters
    if isinstance(k, ConstantTimesKernel):
        _walk(k.kernel, offset, scale_const * k.C, scale_idx, acc)
        return k.num_hyperparameters
    if isinstance(k, EyeKernel):
        if scale_idx is not None:
            acc.noise_idx.append(scale_idx)
            if scale_const != 1.0:
                acc.ok = False      # const * trainable * I: not canonical
        else:
            acc.noise_const += scale_const
        return 0
    kind = next((b for cls, b in _BASE_OF.items() if isinstance(k, cls)),
                None)
    if kind is not None:
        if acc.base is not None:
            acc.ok = False          # two stationary bases: fall back
            return k.num_hyperparameters
        p = k.num_hyperparameters
        acc.base = (kind, slice(offset, offset + p), scale_idx,
                    scale_const if scale_idx is None else 1.0)
        if scale_idx is not None and scale_const != 1.0:
            acc.ok = False
        return p
    acc.ok = False                  # unknown kernel type
    return k.num_hyperparameters


def compile_kernel(kernel: Kernel) -> Optional[CompiledKernel]:
    """Return the canonical form, or None if the tree does not match."""
    acc = _Acc()
    p = _walk(kernel, 0, 1.0, None, acc)
    if not acc.ok or acc.base is None:
        return None
    kind, base_idx, amp_idx, amp_const = acc.base
    return CompiledKernel(p=p, base=kind, base_idx=base_idx, amp_idx=amp_idx,
                          amp_const=amp_const, noise_const=acc.noise_const,
                          noise_idx=acc.noise_idx)

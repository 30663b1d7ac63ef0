"""The size-m projected-process predictor shared by GPR and GPC.

Mirrors ``GaussianProjectedProcessRawPredictor``
(``commons/GaussianProcessCommons.scala:118-126``): the model is the magic
vector (m), magic matrix (m x m), the active set (m x d) and the kernel with
optimal hyperparameters; prediction cost is independent of the training set
size.  Prediction here is batched: an [t, m] cross-kernel GEMM + GEMV for the
mean and a rowwise quadratic form for the variance (K14 in SURVEY.md §2.4).
"""

from __future__ import annotations

from typing import Tuple

import torch

from ..kernels.base import Kernel
from .. import ops


class GaussianProjectedProcessRawPredictor:
    def __init__(self, magic_vector: torch.Tensor, magic_matrix: torch.Tensor,
                 kernel: Kernel, active_set: torch.Tensor):
        self.magic_vector = magic_vector.double()
        self.magic_matrix = magic_matrix.double()
        self.kernel = kernel
        self.active_set = active_set

    def predict(self, X: torch.Tensor, with_var: bool = True,
                stream: bool = False, chunk_rows: int = 262144
                ) -> Tuple[torch.Tensor, torch.Tensor]:
        """X: [t, d] -> (mean [t], var [t]).

        mean = cross . magicVector
        var  = k(x,x) + cross . magicMatrix . cross^T   (rowwise)

        ``stream=True`` bounds peak memory independently of t
        (``ops.predict_stream``): the fused HIP kernel where its gate allows,
        else this computation over row chunks of ``chunk_rows``.
        """
        act = self.active_set.to(X.dtype).to(X.device)
        if stream:
            return ops.predict_stream(
                self.kernel, X, act, self.magic_vector.to(X.device),
                self.magic_matrix.to(X.device), with_var, chunk_rows)
        cross = ops.cross_kernel(self.kernel, X, act).double()
        mv = self.magic_vector.to(cross.device)
        mean = cross @ mv
        if not with_var:
            return mean, None
        mm = self.magic_matrix.to(cross.device)
        var = (self.kernel.self_kernel(X).double()
               + ((cross @ mm) * cross).sum(-1))
        return mean, var

"""Active-set (inducing point) providers.

Mirrors ``commons/ActiveSetProvider.scala``:
* ``RandomActiveSetProvider``   — uniform global sample (:48-56)
* ``KMeansActiveSetProvider``   — k-means centroids as synthetic inducing
                                  points (:26-43; Spark MLlib KMeans there,
                                  GPU Lloyd iterations with allreduce here)
* ``GreedilyOptimizingActiveSetProvider`` — Seeger et al. 2003 fast forward
                                  selection (:63-136), batched over all
                                  candidate rows per round.
"""

from __future__ import annotations

import math
import numpy as np
import torch

from .kernels.base import Kernel
from .parallel.dist import Comm
from .ppa import NotPositiveDefiniteError


class ActiveSetProvider:
    def __call__(self, m: int, X: torch.Tensor, y: torch.Tensor,
                 kernel: Kernel, theta: np.ndarray, seed: int,
                 comm: Comm) -> torch.Tensor:
        raise NotImplementedError


class RandomActiveSetProvider(ActiveSetProvider):
    def __call__(self, m, X, y, kernel, theta, seed, comm):
        return comm.sample_rows(X, m, seed)


class KMeansActiveSetProvider(ActiveSetProvider):
    """Lloyd iterations over the sharded data; per-iteration allreduce of
    (centroid sums, counts) — C9 in SURVEY.md §2.5.  Centroids are synthetic
    points, matching the reference's use of MLlib cluster centers.

    ``fused=True`` runs each iteration's local work as one
    ``ops.kmeans_step``: on GPU the kernels of kmeans.hip (no [chunk, m]
    score matrix, no atomics, so the same centres to the bit on every run),
    on CPU the arithmetic below.  Near-ties may fall to another centre than
    with ``fused=False``, which is why it is not the default."""

    def __init__(self, max_iter: int = 20, chunk_rows: int = 1 << 18,
                 fused: bool = False):
        self.max_iter = max_iter
        self.chunk_rows = chunk_rows
        self.fused = bool(fused)

    def _fused(self, m, X, seed, comm):
        from . import ops
        centers = comm.sample_rows(X, m, seed)          # seeded init
        work = {}                                       # the step's buffers
        for _ in range(self.max_iter):
            sums, counts, _ = ops.kmeans_step(X, centers, self.chunk_rows,
                                              work)
            comm.allreduce_(sums)
            comm.allreduce_(counts)
            nonempty = counts > 0
            centers = centers.clone()
            centers[nonempty] = (sums[nonempty]
                                 / counts[nonempty].unsqueeze(-1)).to(X.dtype)
        return centers

    def __call__(self, m, X, y, kernel, theta, seed, comm):
        if self.fused:
            return self._fused(m, X, seed, comm)
        centers = comm.sample_rows(X, m, seed)          # seeded init
        n, d = X.shape
        for _ in range(self.max_iter):
            sums = torch.zeros(m, d, dtype=torch.float64, device=X.device)
            counts = torch.zeros(m, dtype=torch.float64, device=X.device)
            c2 = (centers * centers).sum(-1)
            for s in range(0, n, self.chunk_rows):
                xb = X[s:min(n, s + self.chunk_rows)]
                # argmin_j ||x - c_j||^2 = argmin_j (||c_j||^2 - 2 x.c_j)
                assign = (c2 - 2.0 * (xb @ centers.T)).argmin(-1)
                sums.index_add_(0, assign, xb.double())
                counts.index_add_(0, assign,
                                  torch.ones(len(xb), dtype=torch.float64,
                                             device=X.device))
            comm.allreduce_(sums)
            comm.allreduce_(counts)
            nonempty = counts > 0
            centers = centers.clone()
            centers[nonempty] = (sums[nonempty]
                                 / counts[nonempty].unsqueeze(-1)).to(X.dtype)
        return centers


class GreedilyOptimizingActiveSetProvider(ActiveSetProvider):
    """Fast forward selection (Seeger et al. 2003).

    Per round (``ActiveSetProvider.scala:84-136``): with the current active
    set of size mc, compute K_mm^-1 and (sigma2 K_mm + Kmn Knm)^-1, then score
    every candidate row i:

        l_i = sqrt(K_ii - p_i);  xi_i = 1/((s/l_i)^2 + 1 - q_i)
        kappa_i = xi_i (1 + 2 (s/l_i)^2)
        delta_i = -log(s/l_i) - (log xi_i
                   + xi_i (1-kappa_i)/sigma2 (y_i-mu_i)^2 - kappa_i + 2)/2

    with p_i = c^T K_mm^-1 c, q_i = c^T PD^-1 c, mu_i = c^T magicVector and
    c the candidate's cross-kernel column; NaN-filtered distributed argmax
    (C6/C7 collectives) picks the next inducing point.

    ``incremental=True`` keeps p, q and mu up to date instead of recomputing
    them: two Cholesky factors grow by one row per round and every candidate
    is updated from one new cross-kernel column (``ops.greedy_state``; the
    fused HIP kernels on GPU).  O(n mc) work and an allreduce of mc + 2
    doubles per round instead of O(n mc^2) and mc (mc + 1), for the same
    selection; the state takes 12 n m bytes on GPU, 16 n m on CPU."""

    def __init__(self, incremental: bool = False):
        self.incremental = bool(incremental)

    def _select_incremental(self, m, X, y, kernel, seed, comm):
        from . import ops
        active = comm.sample_rows(X, 1, seed)           # 1 random start
        if m <= 1:
            return active
        state = ops.greedy_state(kernel, X, y, m - 1)
        state.append(active[0], comm)
        while True:
            best_local, best_val = state.best()
            # distributed argmax: max value, then lowest owning rank wins
            gmax = comm.allreduce_scalar(best_val, op="max")
            my = comm.rank if (best_val == gmax) else 1 << 30
            winner = int(comm.allreduce_scalar(float(my), op="min"))
            row = torch.zeros(1, X.shape[1], dtype=X.dtype, device=X.device)
            if comm.rank == winner:
                row[0] = X[best_local]
            comm.allreduce_(row)
            active = torch.cat([active, row], dim=0)
            if active.shape[0] >= m:
                return active
            state.append(row[0], comm)

    def __call__(self, m, X, y, kernel, theta, seed, comm):
        if self.incremental:
            return self._select_incremental(m, X, y, kernel, seed, comm)
        active = comm.sample_rows(X, 1, seed)           # 1 random start
        sigma2 = kernel.white_noise_var()
        s = math.sqrt(sigma2)
        diagK = kernel.training_kernel_diag(X)          # [n], includes noise
        # On GPU the [n, mc] cross kernel comes from the HIP tile kernel
        # (fp32) and the O(n mc^2) scoring GEMMs run in fp32; the small
        # mc x mc factorizations and the KK/Ky statistics stay fp64.  On
        # CPU everything is fp64 (the oracle the distributed-exact tests
        # pin).  (Round-1 weakness: the all-fp64 torch path made greedy
        # unusable beyond small m on GPU.)
        from . import ops
        gpu = X.is_cuda
        while active.shape[0] < m:
            Kmm = kernel.training_kernel(active.double())
            Lmm, info = torch.linalg.cholesky_ex(Kmm)
            if int(info) > 0:
                raise NotPositiveDefiniteError()
            Kinv = torch.cholesky_inverse(Lmm)

            if gpu:
                cross = ops.cross_kernel(kernel, X, active)      # fp32 HIP
            else:
                cross = kernel.cross_kernel(X, active).double()  # [n, mc]
            cd = cross.double() if gpu else cross
            KK = cd.T @ cd
            Ky = cd.T @ y.double()
            comm.allreduce_(KK)
            comm.allreduce_(Ky)
            PD = sigma2 * Kmm + KK
            Lpd, info = torch.linalg.cholesky_ex(PD)
            if int(info) > 0:
                raise NotPositiveDefiniteError()
            PDinv = torch.cholesky_inverse(Lpd)
            magic = torch.cholesky_solve(Ky.unsqueeze(-1), Lpd).squeeze(-1)

            p = ((cross @ Kinv.to(cross.dtype)) * cross).sum(-1).double()
            q = ((cross @ PDinv.to(cross.dtype)) * cross).sum(-1).double()
            mu = (cross @ magic.to(cross.dtype)).double()
            li = torch.sqrt(diagK.double() - p)
            sl2 = (s / li) ** 2
            xi = 1.0 / (sl2 + 1.0 - q)
            kappa = xi * (1.0 + 2.0 * sl2)
            delta = (-torch.log(s / li)
                     - (torch.log(xi)
                        + xi * (1.0 - kappa) / sigma2 * (y.double() - mu) ** 2
                        - kappa + 2.0) / 2.0)
            delta = torch.nan_to_num(delta, nan=-math.inf)
            best_local = int(delta.argmax())
            best_val = float(delta[best_local])

            # distributed argmax: max value, then lowest owning rank wins
            gmax = comm.allreduce_scalar(best_val, op="max")
            my = comm.rank if (best_val == gmax) else 1 << 30
            winner = int(comm.allreduce_scalar(float(my), op="min"))
            row = torch.zeros(1, X.shape[1], dtype=X.dtype, device=X.device)
            if comm.rank == winner:
                row[0] = X[best_local]
            comm.allreduce_(row)
            active = torch.cat([active, row], dim=0)
        return active

"""``KMeansActiveSetProvider(fused=True)`` on CPU runs ``torch_backend.
kmeans_step``, the arithmetic of the unfused loop body: the same centres to
the bit.  And the shape gate of the HIP step, where the extension imports."""

import numpy as np
import pytest
import torch

from spark_gp_amd import KMeansActiveSetProvider
from spark_gp_amd.parallel.dist import Comm


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("n,d,m,chunk", [(500, 3, 12, 1 << 18),
                                         (500, 3, 12, 128), (40, 2, 30, 16)])
def test_fused_equals_unfused_on_cpu(dtype, n, d, m, chunk):
    X = torch.tensor(np.random.default_rng(11).random((n, d)), dtype=dtype)
    if m == 30:
        X[:30] = X[0]       # 29 equal centres among the 30 sampled: empties
    runs = [KMeansActiveSetProvider(max_iter=4, chunk_rows=chunk, fused=f)(
        m, X, None, None, None, 3, Comm()) for f in (False, True)]
    assert runs[0].dtype == dtype and torch.equal(runs[0], runs[1])


def test_an_empty_cluster_keeps_its_centre():
    from spark_gp_amd.ops import torch_backend
    X = torch.tensor([[0.0], [0.1], [1.0]], dtype=torch.float64)
    centers = torch.tensor([[0.0], [0.0], [1.0]], dtype=torch.float64)
    sums, counts, assign = torch_backend.kmeans_step(X, centers)
    assert assign.tolist() == [0, 0, 2] and counts.tolist() == [2.0, 0.0, 1.0]
    assert sums.dtype == torch.float64 and sums[:, 0].tolist() == [0.1, 0., 1.]


def test_gate_refuses_what_the_kernels_do_not_take():
    from spark_gp_amd.ops import hip_backend
    X = torch.zeros(10, 3)

    def ok(X, m, d):
        return hip_backend.supports_kmeans(X, torch.zeros(m, d, dtype=X.dtype))

    assert ok(X, 1, 3) and ok(X, 8192, 3)
    assert not ok(X, 0, 3) and not ok(X, 8193, 3)
    assert not ok(torch.zeros(10, 0), 4, 0)
    assert not ok(X.double(), 4, 3) and not ok(X.T, 4, 10)

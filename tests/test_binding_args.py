"""Argument validation of the extension's bindings.

Shape, dtype and range rules run before the device checks, so they are
tested with CPU tensors: a violated rule must raise a RuntimeError that
names the argument, and correctly shaped CPU tensors must be turned away by
the device check — nothing may reach a launcher.  The mixed-device cases
need a GPU."""

import pytest
import torch

from spark_gp_amd import _hip_ext as ext

E, K, D = 3, 8, 4           # experts
C, M = 64, 10               # PPA chunk rows, active points

f32 = torch.float32
f64 = torch.float64
bf16 = torch.bfloat16


def _expert(**over):
    a = dict(X=torch.zeros(E, K, D), y=torch.zeros(E, K),
             scale=torch.ones(D))
    a.update(over)
    return a["X"], a["y"], a["scale"], 1.0, 1e-3


def _laplace(**over):
    a = dict(X=torch.zeros(E, K, D), y=torch.zeros(E, K),
             f=torch.zeros(E, K), scale=torch.ones(D))
    a.update(over)
    return a["X"], a["y"], a["f"], a["scale"], 1.0, 1e-3, 1e-6, 10


def _ppa(dev="cpu", **over):
    """(Xs, As, nx, na, amp, y, Ky) of cross_mfma_ppa; ppa_fused_acc appends
    (KK, split_k)."""
    a = dict(Xs=torch.rand(C, D, device=dev), As=torch.rand(M, D, device=dev),
             nx=torch.rand(C, device=dev), na=torch.rand(M, device=dev),
             y=torch.rand(C, device=dev),
             Ky=torch.zeros(M, dtype=f64, device=dev))
    a.update(over)
    return a["Xs"], a["As"], a["nx"], a["na"], 1.0, a["y"], a["Ky"]


def _syrk(**over):
    a = dict(KcT=torch.zeros(M, C, dtype=bf16), KlT=None,
             KK=torch.zeros(M, M))
    a.update(over)
    return a["KcT"], a["KlT"], a["KK"]


_TILES = torch.tensor([[0, 0]] + [[-1, -1]] * 7, dtype=torch.int32)
_CHOL = dict(A=torch.eye(64, dtype=f64), V=torch.zeros(1, 64, 64, dtype=f64),
             B=torch.zeros(64, 2, dtype=f64))

# (id, call, argument named in the message)
RULES = [
    ("nll short scale",
     lambda: ext.fused_expert_nll(*_expert(scale=torch.ones(D - 1))), "scale"),
    ("nll y not [E, k]",
     lambda: ext.fused_expert_nll(*_expert(y=torch.zeros(E, K + 1))), "y"),
    ("newton y not [E, k]",
     lambda: ext.fused_laplace_newton(*_laplace(y=torch.zeros(E + 1, K))),
     "y"),
    ("newton f not [E, k]",
     lambda: ext.fused_laplace_newton(*_laplace(f=torch.zeros(E, K - 1))),
     "f"),
    ("evidence f not [E, k]",
     lambda: ext.fused_laplace_evidence(*_laplace(f=torch.zeros(K, E))), "f"),
    ("newton short scale",
     lambda: ext.fused_laplace_newton(*_laplace(scale=torch.ones(D - 1))),
     "scale"),
    ("evidence short scale",
     lambda: ext.fused_laplace_evidence(*_laplace(scale=torch.ones(1))),
     "scale"),
    ("evidence d > k",
     lambda: ext.fused_laplace_evidence(*_laplace(
         X=torch.zeros(E, K, K + 1), scale=torch.ones(K + 1))), "X"),
    ("tile short s2v",
     lambda: ext.cross_kernel_tile(torch.zeros(C, D), torch.zeros(M, D),
                                   torch.ones(D - 1), 1.0, False, False),
     "s2v"),
    ("tile_ppa short s2v",
     lambda: ext.cross_kernel_tile_ppa(
         torch.zeros(C, D), torch.zeros(M, D), torch.ones(D - 1), 1.0,
         torch.zeros(C), torch.zeros(M, dtype=f64)), "s2v"),
    ("mfma short nx",
     lambda: ext.cross_mfma_ppa(*_ppa(nx=torch.zeros(C - 1))), "nx"),
    ("mfma short y",
     lambda: ext.cross_mfma_ppa(*_ppa(y=torch.zeros(C - 1))), "y"),
    ("colsum wrong Ky length",
     lambda: ext.colsum_gemv_acc(torch.zeros(C, M, dtype=bf16),
                                 torch.zeros(C),
                                 torch.zeros(M + 1, dtype=f64)), "Ky"),
    ("colsum wrong y length",
     lambda: ext.colsum_gemv_acc(torch.zeros(C, M, dtype=bf16),
                                 torch.zeros(C + 1),
                                 torch.zeros(M, dtype=f64)), "y"),
    ("colsum strided Ky",
     lambda: ext.colsum_gemv_acc(torch.zeros(C, M, dtype=bf16),
                                 torch.zeros(C),
                                 torch.zeros(2 * M, dtype=f64)[::2]), "Ky"),
    ("syrk non-contiguous KK",
     lambda: ext.syrk_bf16_acc(*_syrk(KK=torch.zeros(M, 2 * M)[:, ::2]), 1),
     "KK"),
    ("syrk split_k = 0",
     lambda: ext.syrk_bf16_acc(*_syrk(), 0), "split_k"),
    ("syrk split_k = 65536",
     lambda: ext.syrk_bf16_acc(*_syrk(), 65536), "split_k"),
    ("sync kpb = 0",
     lambda: ext.syrk_bf16_sync_acc(*_syrk(), _TILES, 0, 1), "kpb"),
    ("sync nactive too large",
     lambda: ext.syrk_bf16_sync_acc(*_syrk(), _TILES, 128, 9), "nactive"),
    ("sync nactive negative",
     lambda: ext.syrk_bf16_sync_acc(*_syrk(), _TILES, 128, -1), "nactive"),
    ("sync non-contiguous KK",
     lambda: ext.syrk_bf16_sync_acc(
         *_syrk(KK=torch.zeros(M, 2 * M)[:, ::2]), _TILES, 128, 1), "KK"),
    ("solve float32 V",
     lambda: ext.dchol_solve64(_CHOL["A"], _CHOL["V"].float(), _CHOL["B"]),
     "V"),
]


@pytest.mark.parametrize("call,name", [r[1:] for r in RULES],
                         ids=[r[0] for r in RULES])
def test_rule_names_its_argument(call, name):
    with pytest.raises(RuntimeError, match=rf"^{name}\b"):
        call()


# correctly shaped CPU tensors: every binding's device check turns them away
ON_CPU = [
    ("fused_expert_nll", lambda: ext.fused_expert_nll(*_expert())),
    ("fused_expert_nll_profile",
     lambda: ext.fused_expert_nll_profile(*_expert(), True)),
    ("fused_laplace_newton", lambda: ext.fused_laplace_newton(*_laplace())),
    ("fused_laplace_evidence",
     lambda: ext.fused_laplace_evidence(*_laplace())),
    ("cross_kernel_tile",
     lambda: ext.cross_kernel_tile(torch.zeros(C, D), torch.zeros(M, D),
                                   torch.ones(D), 1.0, False, False)),
    ("cross_kernel_tile_ppa",
     lambda: ext.cross_kernel_tile_ppa(
         torch.zeros(C, D), torch.zeros(M, D), torch.ones(D), 1.0,
         torch.zeros(C), torch.zeros(M, dtype=f64))),
    ("cross_mfma_ppa", lambda: ext.cross_mfma_ppa(*_ppa())),
    ("ppa_fused_acc",
     lambda: ext.ppa_fused_acc(*_ppa(), torch.zeros(M, M), 1)),
    ("syrk_bf16_acc", lambda: ext.syrk_bf16_acc(*_syrk(), 1)),
    ("syrk_bf16_acc hi/lo",
     lambda: ext.syrk_bf16_acc(
         *_syrk(KlT=torch.zeros(M, C, dtype=bf16)), 1)),
    ("syrk_bf16_sync_acc",
     lambda: ext.syrk_bf16_sync_acc(*_syrk(), _TILES, 128, 1)),
    ("colsum_gemv_acc",
     lambda: ext.colsum_gemv_acc(torch.zeros(C, M, dtype=bf16),
                                 torch.zeros(C), torch.zeros(M, dtype=f64))),
    ("dpotrf64",
     lambda: ext.dpotrf64(_CHOL["A"].clone(), _CHOL["V"].clone(),
                          torch.zeros(1, dtype=torch.int32))),
    ("dchol_solve64",
     lambda: ext.dchol_solve64(_CHOL["A"], _CHOL["V"], _CHOL["B"].clone())),
    ("dgemm64",
     lambda: ext.dgemm64(torch.zeros(4, 5, dtype=f64),
                         torch.zeros(5, 6, dtype=f64), False, False)),
]


@pytest.mark.parametrize("call", [c[1] for c in ON_CPU],
                         ids=[c[0] for c in ON_CPU])
def test_cpu_tensors_stop_at_the_device_check(call):
    with pytest.raises(RuntimeError, match="must be on the GPU"):
        call()


def _mixed_device_cases(dev):
    """(call, tensor the kernel would have written).  One argument stays on
    the CPU; before the device checks its host pointer reached the kernel."""
    KK = torch.full((M, M), 7.0, device=dev)
    Ky = torch.full((M,), 7.0, dtype=f64, device=dev)
    yield "nx", (lambda: ext.cross_mfma_ppa(
        *_ppa(dev, nx=torch.rand(C), Ky=Ky))), (Ky,)
    yield "y", (lambda: ext.ppa_fused_acc(
        *_ppa(dev, y=torch.rand(C), Ky=Ky), KK, 1)), (Ky, KK)
    yield "scale", (lambda: ext.fused_expert_nll(
        torch.rand(E, K, D, device=dev), torch.rand(E, K, device=dev),
        torch.ones(D), 1.0, 1e-3)), ()


@pytest.mark.gpu
def test_mixed_devices_are_rejected_before_launch():
    dev = torch.device("cuda:0")
    for name, call, outputs in _mixed_device_cases(dev):
        with pytest.raises(RuntimeError, match=rf"^{name} must be on the GPU"):
            call()
        torch.cuda.synchronize()
        for out in outputs:
            assert bool((out == 7.0).all()), name

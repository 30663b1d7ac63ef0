"""Argument validation of the ``family`` argument of the extension's
bindings, in the manner of ``test_binding_args.py``: the rule runs before the
device checks, so it is tested with CPU tensors.  An unknown code must raise a
RuntimeError that names the argument; a known one must get as far as the
device check, with and without the keyword."""

import pytest
import torch

from spark_gp_amd import _hip_ext as ext

E, K, D = 3, 8, 4           # experts
C, M = 64, 10               # PPA chunk rows, active points


def _expert():
    return torch.zeros(E, K, D), torch.zeros(E, K), torch.ones(D), 1.0, 1e-3


def _tile():
    return torch.rand(C, D), torch.rand(M, D), torch.ones(D), 1.0


def _ppa():
    return (torch.rand(C, D), torch.rand(M, D), torch.rand(C), torch.rand(M),
            1.0, torch.rand(C), torch.zeros(M, dtype=torch.float64))


# (id, call taking the family code)
CALLS = [
    ("fused_expert_nll",
     lambda f: ext.fused_expert_nll(*_expert(), family=f)),
    ("fused_expert_nll positional",
     lambda f: ext.fused_expert_nll(*_expert(), f)),
    ("fused_expert_nll_profile",
     lambda f: ext.fused_expert_nll_profile(*_expert(), True, family=f)),
    ("cross_kernel_tile",
     lambda f: ext.cross_kernel_tile(*_tile(), False, False, family=f)),
    ("cross_kernel_tile positional",
     lambda f: ext.cross_kernel_tile(*_tile(), False, False, False, f)),
    ("cross_kernel_tile_ppa",
     lambda f: ext.cross_kernel_tile_ppa(
         *_tile(), torch.rand(C), torch.zeros(M, dtype=torch.float64),
         family=f)),
    ("cross_mfma_ppa", lambda f: ext.cross_mfma_ppa(*_ppa(), family=f)),
    ("ppa_fused_acc",
     lambda f: ext.ppa_fused_acc(*_ppa(), torch.zeros(M, M), 1, family=f)),
]


def test_family_codes_exported():
    from spark_gp_amd.kernels.compiled import FAM_M32, FAM_M52, FAM_RBF
    assert (ext.FAM_RBF, ext.FAM_M32, ext.FAM_M52) == (0, 1, 2)
    assert (FAM_RBF, FAM_M32, FAM_M52) == (0, 1, 2)


@pytest.mark.parametrize("name,call", CALLS, ids=[c[0] for c in CALLS])
@pytest.mark.parametrize("family", [-1, 3])
def test_unknown_family_names_the_argument(name, call, family):
    with pytest.raises(RuntimeError, match="family must be"):
        call(family)


@pytest.mark.parametrize("name,call", CALLS, ids=[c[0] for c in CALLS])
@pytest.mark.parametrize("family", [0, 1, 2])
def test_known_family_reaches_the_device_check(name, call, family):
    with pytest.raises(RuntimeError, match="must be on the GPU"):
        call(family)


@pytest.mark.parametrize("family", [-1, 3])
def test_occupancy_unknown_family(family):
    with pytest.raises(RuntimeError, match="family must be"):
        ext.fused_expert_nll_occupancy(100, 32, family)
    with pytest.raises(RuntimeError, match="family must be"):
        ext.fused_expert_nll_occupancy(100, 32, family=family)

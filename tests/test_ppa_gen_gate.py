"""CPU tests of the fused kernel's generator choice (ops/ppa_plan.py): the
range gate of the f16 generator, the ``SPARK_GP_AMD_PPA_GEN`` switch, and the
plan of the staged paths, which neither touches."""

import math

import pytest
import torch

from spark_gp_amd.ops import ppa_plan

_SWITCHES = ("SPARK_GP_AMD_PPA_GEN", "SPARK_GP_AMD_PPA_FUSED",
             "SPARK_GP_AMD_CROSS_MFMA", "SPARK_GP_AMD_SYRK_SYNC")
CHUNK = 4096


@pytest.fixture
def default_env(monkeypatch):
    for name in _SWITCHES:
        monkeypatch.delenv(name, raising=False)
    return monkeypatch


@pytest.mark.parametrize("absmax,gen", [
    (0.0, "f16"), (1.5, "f16"), (32767.9, "f16"),
    (32768.0, "f32"),                      # the bound itself is outside
    (7e4, "f32"), (math.inf, "f32"), (math.nan, "f32"),
])
def test_range_gate(default_env, absmax, gen):
    assert ppa_plan.ppa_fused_gen(absmax) == gen


def test_limit_is_inside_the_f16_range():
    """Both terms of the split stay finite: |hi| <= |v| rounded, |lo| <= |v|
    (the residual is at most 2^-11 |v|, scaled by 2^11)."""
    assert ppa_plan.FUSED_F16_ABS_LIMIT == 2.0 ** 15
    assert ppa_plan.FUSED_F16_ABS_LIMIT < float(torch.finfo(torch.float16).max)


@pytest.mark.parametrize("absmax", [0.0, 1.5, 7e4])
def test_switch_forces_f32(default_env, absmax):
    default_env.setenv("SPARK_GP_AMD_PPA_GEN", "f32")
    assert ppa_plan.ppa_fused_gen(absmax) == "f32"
    default_env.setenv("SPARK_GP_AMD_PPA_GEN", "auto")
    assert ppa_plan.ppa_fused_gen(1.5) == "f16"


def test_switch_rejects_other_values(default_env):
    default_env.setenv("SPARK_GP_AMD_PPA_GEN", "f16")    # cannot be forced
    with pytest.raises(ValueError, match="SPARK_GP_AMD_PPA_GEN"):
        ppa_plan.ppa_fused_gen(1.5)


@pytest.mark.parametrize("switch", [None, "f32"])
def test_plan_does_not_depend_on_the_switch(default_env, switch):
    """The generator is chosen per accumulation from the data; path, split-k
    and chunk length are as they were, for the fused and the staged paths."""
    if switch:
        default_env.setenv("SPARK_GP_AMD_PPA_GEN", switch)
    plan = ppa_plan.ppa_plan
    p = plan(1000, 32, torch.float32, CHUNK)
    assert (p.generator, p.syrk, p.split_k, p.chunk_rows) == \
        ("fused", None, 25, 2 * CHUNK)
    p = plan(1000, 33, torch.float32, CHUNK)
    assert (p.generator, p.syrk, p.split_k, p.chunk_rows) == \
        ("mfma", "splitk", 16, CHUNK)
    p = plan(5633, 32, torch.float32, CHUNK)
    assert (p.generator, p.syrk, p.split_k, p.chunk_rows) == \
        ("mfma", "sync", None, CHUNK)
    default_env.setenv("SPARK_GP_AMD_PPA_FUSED", "0")
    p = plan(1000, 32, torch.float32, CHUNK)
    assert (p.generator, p.syrk, p.split_k, p.chunk_rows) == \
        ("mfma", "splitk", 16, CHUNK)


def test_limit_mirrors_the_kernel_header():
    from spark_gp_amd import _hip_ext as ext
    assert ppa_plan.FUSED_F16_ABS_LIMIT == ext.SF_F16_ABS_LIMIT

"""CPU-only tests of the fused-PPA dispatch gate (no device, no extension)."""

import torch

from spark_gp_amd.ops import ppa_gate
from spark_gp_amd.ops.ppa_gate import (FUSED_MAX_D, ppa_fused_gate,
                                       ppa_fused_split_k)


def test_gate_on_for_headline(monkeypatch):
    monkeypatch.delenv("SPARK_GP_AMD_PPA_FUSED", raising=False)
    assert ppa_fused_gate(1000, 32, torch.float32)
    assert ppa_fused_gate(200, 4, torch.float32)


def test_gate_off_for_float64(monkeypatch):
    monkeypatch.delenv("SPARK_GP_AMD_PPA_FUSED", raising=False)
    assert not ppa_fused_gate(1000, 32, torch.float64)


def test_gate_off_above_d_limit(monkeypatch):
    monkeypatch.delenv("SPARK_GP_AMD_PPA_FUSED", raising=False)
    assert ppa_fused_gate(1000, FUSED_MAX_D, torch.float32)
    assert not ppa_fused_gate(1000, FUSED_MAX_D + 1, torch.float32)
    assert not ppa_fused_gate(1000, 128, torch.float32)
    assert not ppa_fused_gate(1000, 0, torch.float32)


def test_gate_off_when_tiles_exceed_256(monkeypatch):
    monkeypatch.delenv("SPARK_GP_AMD_PPA_FUSED", raising=False)
    # 22 windows -> 253 tiles (on); 23 windows -> 276 tiles (off)
    assert ppa_fused_gate(22 * 256, 32, torch.float32)
    assert not ppa_fused_gate(22 * 256 + 1, 32, torch.float32)
    assert not ppa_fused_gate(8192, 32, torch.float32)


def test_gate_off_by_environment_switch(monkeypatch):
    monkeypatch.setenv("SPARK_GP_AMD_PPA_FUSED", "0")
    assert not ppa_gate.ppa_fused_enabled()
    assert not ppa_fused_gate(1000, 32, torch.float32)
    monkeypatch.setenv("SPARK_GP_AMD_PPA_FUSED", "1")
    assert ppa_fused_gate(1000, 32, torch.float32)


def test_fused_chunk_is_a_multiple_of_the_callers():
    assert ppa_gate.ppa_fused_chunk_rows(262144) == \
        262144 * ppa_gate.FUSED_CHUNK_FACTOR
    assert 1 <= ppa_gate.FUSED_CHUNK_FACTOR <= 8


def test_split_k_fills_the_device_once():
    assert ppa_fused_split_k(1000) == 25          # 10 tiles x 25 = 250 blocks
    assert ppa_fused_split_k(200) == 64           # capped
    assert ppa_fused_split_k(22 * 256) == 1

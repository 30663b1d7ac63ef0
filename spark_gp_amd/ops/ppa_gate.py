"""Dispatch gate of the fused PPA accumulation (``ppa_fused_acc``).

A pure function of ``(m, d, dtype)`` and one environment switch, kept free
of the extension import so it can be tested without a device.
"""

from __future__ import annotations

import os

import torch

# Largest feature dimension the fused kernel takes: the fp32 A' windows of
# one tile (2 x 256 x 36 floats) share the 160 KB LDS with the four bf16
# operand tiles, which leaves room for 32 d-slots per row.  Generation cost
# also grows as 512*d/32 f32 MFMAs per k-step, paid by every tile that uses
# a window, so larger d stays on the staged two-kernel path.
FUSED_MAX_D = 32

# The split-k SYRK family owns tile sets up to 256 (m <= 5632); larger ones
# go to the k-synchronized kernel, which needs K_nm in memory.
FUSED_MAX_TILES = 256


# The caller's chunk_rows bounds the staged path's two [m, chunk] bf16
# buffers (4*m bytes per row).  The fused path's only temporary is the
# scaled X chunk (4*d bytes per row), and every k-slice ends in a full tile
# of fp32 atomics, so longer chunks are cheaper — but they lengthen the fp32
# register accumulation.  Measured (PROFILES.md, round 3): 1x/2x/4x give
# 83.6/77.4/74.7 ms for the 10M-row stage; KK error against the fp64
# branch at 2M rows is 1.00/1.11/1.31 x the two-kernel path's, and the
# fitted magic_vector's distance to the fp64 fit at 10M rows
# 0.95/1.15/1.84 x.  2x keeps the results in the two-kernel path's error
# class; 4x buys 3 ms more and sits too close to the 2x acceptance bound.
FUSED_CHUNK_FACTOR = 2


def ppa_fused_chunk_rows(chunk_rows: int) -> int:
    return chunk_rows * FUSED_CHUNK_FACTOR


def ppa_fused_enabled() -> bool:
    """``SPARK_GP_AMD_PPA_FUSED=0`` selects the two-kernel path (A/B)."""
    return os.environ.get("SPARK_GP_AMD_PPA_FUSED", "1") == "1"


def ppa_fused_gate(m: int, d: int, dtype) -> bool:
    if not ppa_fused_enabled():
        return False
    if dtype != torch.float32:
        return False
    if m < 1 or d < 1 or d > FUSED_MAX_D:
        return False
    ntile = (m + 255) // 256
    return ntile * (ntile + 1) // 2 <= FUSED_MAX_TILES


def ppa_fused_split_k(m: int) -> int:
    """k-slices per chunk: with no operand windows to keep cache-resident,
    the only concern is filling the 256 CUs once with whole blocks."""
    ntile = (m + 255) // 256
    tiles = ntile * (ntile + 1) // 2
    # capped: every slice ends in a full tile of fp32 atomics
    return max(1, min(64, 256 // tiles))

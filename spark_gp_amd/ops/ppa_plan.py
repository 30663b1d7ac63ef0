"""Host-side plan of the mixed-precision PPA accumulation (KK += K^T K,
Ky += K^T y): which K_nm generator and SYRK kernel run, with what split-k,
chunk length and tile lists.

Pure functions of ``(m, d, dtype)`` and the environment switches, free of
the extension import so they can be tested without a device.  The constants
mirror ``csrc/kernel_geom.h``; tests/test_ppa_plan.py checks them.
"""

from __future__ import annotations

import os
from dataclasses import dataclass
from typing import List, Optional, Tuple

import torch

# Output tile edge of the SYRK kernels (SY_CT).
SYRK_TILE = 256

# Largest feature dimension the fused kernel takes (SF_DMAX): the fp32 A'
# windows of one tile (2 x 256 x 36 floats) share the 160 KB LDS with the
# four bf16 operand tiles, which leaves room for 32 d-slots per row.
# Generation costs 192 f16 MFMAs (16x16x32: its K extent is the 32 d-slots) per
# k-step of an off-diagonal tile, next to the 768 bf16 MFMAs of the products;
# the fp32 generator it replaces by default costs 512*d/32 f32 MFMAs at twice
# the cycles each.  Either is paid by every tile that uses a window, and a
# larger d needs a second K pass and more LDS, so it stays on the staged
# two-kernel path.
FUSED_MAX_D = 32

# The fused kernel's f16 generator splits every scaled coordinate into two
# f16 terms, which overflow at 65504: it takes coordinates below this bound
# (SF_F16_ABS_LIMIT) and the fp32 generator takes the rest.
FUSED_F16_ABS_LIMIT = 32768.0

# The split-k SYRK family owns tile sets up to 256 (m <= 5632,
# SY_SPLITK_MAX_TILES); larger ones go to the k-synchronized kernel, which
# needs K_nm in memory.
FUSED_MAX_TILES = 256

# The caller's chunk_rows bounds the staged path's two [m, chunk] bf16
# buffers (4*m bytes per row).  The fused path's only temporary is the
# scaled X chunk (4*d bytes per row), and every k-slice ends in a full tile
# stored and reduced (fp32 atomics when this was measured), so longer chunks
# are cheaper — but they lengthen the fp32
# register accumulation.  Measured (PROFILES.md, round 3): 1x/2x/4x give
# 83.6/77.4/74.7 ms for the 10M-row stage; KK error against the fp64
# branch at 2M rows is 1.00/1.11/1.31 x the two-kernel path's, and the
# fitted magic_vector's distance to the fp64 fit at 10M rows
# 0.95/1.15/1.84 x.  2x keeps the results in the two-kernel path's error
# class; 4x buys 3 ms more and sits too close to the 2x acceptance bound.
FUSED_CHUNK_FACTOR = 2

# k-synchronized SYRK: one block owns one output tile for a whole launch, so
# a launch carries at most 224 tiles (blocks beyond the resident set would
# break the k-cohort).
SYNC_MAX_TILES = 224
N_XCD = 8         # the dispatcher places block b on XCD b % 8 (observed)
SYNC_KPB = 128    # k-blocks per pacing phase (measured, PROFILES.md round 2)


def _tile_windows(m: int) -> int:
    return (m + SYRK_TILE - 1) // SYRK_TILE


def syrk_tile_count(m: int) -> int:
    """Lower-triangle output tiles of an [m, m] SYRK."""
    ntile = _tile_windows(m)
    return ntile * (ntile + 1) // 2


def _env_on(name: str) -> bool:
    return os.environ.get(name, "1") == "1"


def ppa_fused_chunk_rows(chunk_rows: int) -> int:
    return chunk_rows * FUSED_CHUNK_FACTOR


def ppa_fused_enabled() -> bool:
    """``SPARK_GP_AMD_PPA_FUSED=0`` selects the two-kernel path (A/B)."""
    return _env_on("SPARK_GP_AMD_PPA_FUSED")


def ppa_fused_gate(m: int, d: int, dtype) -> bool:
    if not ppa_fused_enabled():
        return False
    if dtype != torch.float32:
        return False
    if m < 1 or d < 1 or d > FUSED_MAX_D:
        return False
    return syrk_tile_count(m) <= FUSED_MAX_TILES


def ppa_fused_gen(absmax: float) -> str:
    """Generator of the fused kernel, ``"f16"`` or ``"f32"``, for scaled
    coordinates bounded by ``absmax`` (of X' and A' together).  The f16
    generator runs inside its range; a NaN bound is outside it.
    ``SPARK_GP_AMD_PPA_GEN=f32`` selects the fp32 generator (A/B)."""
    switch = os.environ.get("SPARK_GP_AMD_PPA_GEN", "auto")
    if switch not in ("auto", "f32"):
        raise ValueError("SPARK_GP_AMD_PPA_GEN must be 'auto' or 'f32', got "
                         f"{switch!r}")
    if switch == "f32":
        return "f32"
    return "f16" if absmax < FUSED_F16_ABS_LIMIT else "f32"


def ppa_fused_split_k(m: int) -> int:
    """k-slices per chunk: with no operand windows to keep cache-resident,
    the only concern is filling the 256 CUs once with whole blocks (capped:
    every slice ends in a full partial tile, stored and reduced)."""
    return max(1, min(64, 256 // syrk_tile_count(m)))


def ppa_fused_partials_numel(m: int, split_k: int) -> int:
    """fp32 elements of the fused kernel's partial-tile buffer for any chunk
    length: one tile per (k-slice, output tile).  With the plan's split_k =
    256 // tiles that is at most 256 tiles of 256 KB, 64 MB."""
    return split_k * syrk_tile_count(m) * SYRK_TILE * SYRK_TILE


def syrk_staged_split_k(m: int) -> int:
    """k-slices of the staged split-k SYRK (measured sweep, PROFILES.md:
    shorter per-block k-ranges keep the drifting column windows closer to L3
    residency); 16 for every tile set the default dispatch sends here."""
    return max(1, min(16, round(4096 / syrk_tile_count(m))))


@dataclass(frozen=True)
class PpaPlan:
    generator: str              # "fused" | "mfma" | "elementwise"
    syrk: Optional[str]         # None (fused) | "splitk" | "sync"
    split_k: Optional[int]      # None for the sync SYRK
    chunk_rows: int


def ppa_plan(m: int, d: int, dtype, chunk_rows: int) -> PpaPlan:
    """Resolve the path of one accumulation; reads the switches
    ``SPARK_GP_AMD_PPA_FUSED``, ``SPARK_GP_AMD_CROSS_MFMA`` and
    ``SPARK_GP_AMD_SYRK_SYNC`` at call time.

    * ``fused``: the SYRK blocks generate their K_nm operand windows from
      the pre-scaled inputs; no [m, chunk] hi/lo buffers (the default).
    * ``mfma``: the MFMA cross tile (K1 plan: sqdist via ||x'||^2 + ||a'||^2
      - 2 x'.a' on f32 matrix cores) stages transposed hi/lo copies.
    * ``elementwise``: the ~3-VALU-issues-per-(element, dim) generator
      (``SPARK_GP_AMD_CROSS_MFMA=0``), the fallback/AB path.
    """
    mfma = _env_on("SPARK_GP_AMD_CROSS_MFMA")
    if mfma and ppa_fused_gate(m, d, dtype):
        return PpaPlan("fused", None, ppa_fused_split_k(m),
                       ppa_fused_chunk_rows(chunk_rows))
    generator = "mfma" if mfma else "elementwise"
    # the k-synchronized persistent SYRK wins once the tile set exceeds the
    # resident-block set (m=4096: the split-k kernel is still ahead, 526 vs
    # ~494 TF — PROFILES.md round-2 SYRK section)
    if (syrk_tile_count(m) > FUSED_MAX_TILES
            and _env_on("SPARK_GP_AMD_SYRK_SYNC")):
        return PpaPlan(generator, "sync", None, chunk_rows)
    return PpaPlan(generator, "splitk", syrk_staged_split_k(m), chunk_rows)


def syrk_sync_patch() -> Tuple[int, int]:
    """``SPARK_GP_AMD_SYRK_PATCH=RxC``: tile-patch shape of the sync lists."""
    pr, pc = os.environ.get("SPARK_GP_AMD_SYRK_PATCH", "2x4").split("x")
    return int(pr), int(pc)


def syrk_sync_tile_lists(m: int, patch: Tuple[int, int] = (2, 4)
                         ) -> List[Tuple[List[Tuple[int, int]], int]]:
    """XCD-clustered tile lists for the k-synchronized SYRK: per launch, the
    padded list of ``(ti, tj)`` pairs (``(-1, -1)`` pads) and the number of
    real tiles in it.  Every lower-triangle tile occurs exactly once — the
    kernel accumulates without atomics because each element has one owner.

    Each launch list interleaves N_XCD per-XCD sequences whose tiles are
    sorted by ``patch``-tile patches — an XCD's resident tiles then share a
    handful of 256-row/column operand windows that fit its 4 MB L2 at the
    256-k phase width."""
    pr, pc = patch
    tiles = [(ti, tj) for ti in range(_tile_windows(m))
             for tj in range(ti + 1)]
    tiles.sort(key=lambda t: (t[0] // pr, t[1] // pc))
    launches = []
    for s in range(0, len(tiles), SYNC_MAX_TILES):
        grp = tiles[s:s + SYNC_MAX_TILES]
        per = (len(grp) + N_XCD - 1) // N_XCD
        padded = [(-1, -1)] * (per * N_XCD)
        for x in range(N_XCD):
            for j, t in enumerate(grp[x * per:(x + 1) * per]):
                padded[j * N_XCD + x] = t
        launches.append((padded, len(grp)))
    return launches

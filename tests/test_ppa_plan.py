"""CPU tests of the PPA plan (ops/ppa_plan.py): the path, split-k and chunk
length per (m, d, dtype, environment), the tile lists of the k-synchronized
SYRK, and the module's constants against the ones the extension exports.

The expected values are worked out from the dispatch formulas as they stood
before the plan module existed (tiles = T(T+1)/2 with T = ceil(m / 256);
fused split_k = max(1, min(64, 256 // tiles)); staged split_k =
max(1, min(16, round(4096 / tiles))); sync above 256 tiles; at most 224
tiles per sync launch, padded to a multiple of 8)."""

import pytest
import torch

from spark_gp_amd.ops import ppa_plan
from spark_gp_amd.ops.ppa_plan import ppa_plan as plan_for

_SWITCHES = ("SPARK_GP_AMD_PPA_FUSED", "SPARK_GP_AMD_CROSS_MFMA",
             "SPARK_GP_AMD_SYRK_SYNC")
CHUNK = 4096


@pytest.fixture
def default_env(monkeypatch):
    for name in _SWITCHES:
        monkeypatch.delenv(name, raising=False)
    return monkeypatch


@pytest.mark.parametrize("m,d,generator,syrk,split_k,chunk", [
    (1000, 32, "fused", None, 25, 2 * CHUNK),
    (1000, 33, "mfma", "splitk", 16, CHUNK),
    (300, 32, "fused", None, 64, 2 * CHUNK),
    (5632, 32, "fused", None, 1, 2 * CHUNK),
    (5633, 32, "mfma", "sync", None, CHUNK),
])
def test_plan_default_environment(default_env, m, d, generator, syrk,
                                  split_k, chunk):
    p = plan_for(m, d, torch.float32, CHUNK)
    assert (p.generator, p.syrk, p.split_k, p.chunk_rows) == \
        (generator, syrk, split_k, chunk)


def test_plan_is_frozen(default_env):
    p = plan_for(1000, 32, torch.float32, CHUNK)
    with pytest.raises(Exception):
        p.split_k = 3


def test_plan_fused_switch_off(default_env):
    default_env.setenv("SPARK_GP_AMD_PPA_FUSED", "0")
    p = plan_for(1000, 32, torch.float32, CHUNK)
    assert (p.generator, p.syrk, p.split_k, p.chunk_rows) == \
        ("mfma", "splitk", 16, CHUNK)


@pytest.mark.parametrize("fused", [None, "1"])
def test_plan_elementwise_generator(default_env, fused):
    """CROSS_MFMA=0 selects the elementwise generator whatever PPA_FUSED
    says: the fused kernel shares the MFMA generator's inputs."""
    default_env.setenv("SPARK_GP_AMD_CROSS_MFMA", "0")
    if fused is not None:
        default_env.setenv("SPARK_GP_AMD_PPA_FUSED", fused)
    p = plan_for(1000, 32, torch.float32, CHUNK)
    assert (p.generator, p.syrk, p.split_k, p.chunk_rows) == \
        ("elementwise", "splitk", 16, CHUNK)


@pytest.mark.parametrize("m,split_k", [(5888, 15), (8192, 8)])
def test_plan_sync_switch_off(default_env, m, split_k):
    assert plan_for(m, 32, torch.float32, CHUNK).syrk == "sync"
    default_env.setenv("SPARK_GP_AMD_SYRK_SYNC", "0")
    p = plan_for(m, 32, torch.float32, CHUNK)
    assert (p.generator, p.syrk, p.split_k, p.chunk_rows) == \
        ("mfma", "splitk", split_k, CHUNK)


def test_plan_float64_takes_the_staged_path(default_env):
    assert plan_for(1000, 32, torch.float64, CHUNK).generator == "mfma"


def test_tile_count():
    assert [ppa_plan.syrk_tile_count(m) for m in (1, 256, 257, 1000, 5632,
                                                  5633, 8192)] == \
        [1, 1, 3, 10, 253, 276, 528]


@pytest.mark.parametrize("m,shape", [
    (300, [(8, 3)]),
    (5888, [(224, 224), (56, 52)]),
    (8192, [(224, 224), (224, 224), (80, 80)]),
])
def test_sync_tile_list_shapes(m, shape):
    launches = ppa_plan.syrk_sync_tile_lists(m, (2, 4))
    assert [(len(tiles), nactive) for tiles, nactive in launches] == shape
    assert ppa_plan.syrk_sync_tile_lists(m) == launches     # default patch


@pytest.mark.parametrize("patch", [(2, 4), (1, 1)])
@pytest.mark.parametrize("m", [300, 5888, 8192])
def test_sync_tile_lists_own_every_tile_once(m, patch):
    """One owner per output element is what lets syrk_bf16_sync_kernel
    accumulate without atomics."""
    ntile = -(-m // 256)
    seen = []
    for tiles, nactive in ppa_plan.syrk_sync_tile_lists(m, patch):
        real = [t for t in tiles if t != (-1, -1)]
        assert len(real) == nactive <= 224
        assert len(tiles) % 8 == 0 and len(tiles) - nactive < 8
        assert all(0 <= tj <= ti < ntile for ti, tj in real)
        seen += real
    assert sorted(seen) == [(ti, tj) for ti in range(ntile)
                            for tj in range(ti + 1)]


def test_sync_patch_switch(monkeypatch):
    monkeypatch.delenv("SPARK_GP_AMD_SYRK_PATCH", raising=False)
    assert ppa_plan.syrk_sync_patch() == (2, 4)
    monkeypatch.setenv("SPARK_GP_AMD_SYRK_PATCH", "1x3")
    assert ppa_plan.syrk_sync_patch() == (1, 3)


def test_constants_mirror_the_kernel_header(default_env):
    """ppa_plan is kept free of the extension import; its copies of the
    kernel geometry must equal what kernel_geom.h compiled into it."""
    from spark_gp_amd import _hip_ext as ext
    assert ppa_plan.SYRK_TILE == ext.SY_CT
    assert ppa_plan.FUSED_MAX_D == ext.SF_DMAX
    assert ppa_plan.FUSED_MAX_TILES == ext.SY_SPLITK_MAX_TILES
    assert ext.SY_BK == 32
    for m in (1, 255, 256, 257, 5632, 5633, 8192):
        for d in (0, 1, 32, 33):
            assert ppa_plan.ppa_fused_gate(m, d, torch.float32) == \
                ext.ppa_fused_supported(m, d), (m, d)

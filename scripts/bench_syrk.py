"""SYRK microbenchmark: numerics vs fp64 and sustained throughput.

Usage (GPU box):  python scripts/bench_syrk.py [rows] [m]
Prints achieved bf16 TFLOP/s (counting all 3 hi/lo MFMA products) and the
max relative error of KK against a torch fp64 reference.

    python scripts/bench_syrk.py ROWS M --fused [D] [--gen f16|f32]
times one whole PPA chunk both ways on the same inputs, alternating: the
staged pair (cross_mfma_ppa + syrk_bf16_acc) against ppa_fused_acc (with the
f16 generator, or the fp32 one) over a split_k sweep (the tables in
profiles/PROFILES.md, rounds 3 and 12).
"""
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

import torch

from spark_gp_amd import _hip_ext as ext  # fail loudly if missing

rows = int(sys.argv[1]) if len(sys.argv) > 1 else 131072
m = int(sys.argv[2]) if len(sys.argv) > 2 else 1000

torch.manual_seed(0)
dev = "cuda"


def _fused_ab(rows, m, d):
    """--fused [d]: the whole PPA chunk both ways on the same inputs,
    alternating — cross_mfma_ppa + syrk_bf16_acc (the dispatch's split_k)
    against ppa_fused_acc over a split_k sweep.  Times are per chunk."""
    from spark_gp_amd.ops.ppa_plan import (ppa_fused_split_k,
                                           syrk_staged_split_k,
                                           syrk_tile_count)
    X = torch.rand(rows, d, device=dev)
    A = torch.rand(m, d, device=dev)
    y = torch.rand(rows, device=dev)
    beta = torch.rand(d, device=dev) + 0.5
    Xs, As = (X * beta).contiguous(), (A * beta).contiguous()
    nx, na = (Xs * Xs).sum(-1).contiguous(), (As * As).sum(-1).contiguous()
    KK = torch.zeros(m, m, device=dev)
    Ky = torch.zeros(m, dtype=torch.float64, device=dev)
    tiles = syrk_tile_count(m)
    sk_pair = syrk_staged_split_k(m)
    # --gen f16|f32: the fused kernel's generator; the bound is taken once
    # here so the timed calls do not reduce the inputs again
    gen = sys.argv[sys.argv.index("--gen") + 1] if "--gen" in sys.argv \
        else "f16"
    absmax = float(torch.maximum(Xs.abs().max(), As.abs().max()))

    def pair():
        KcT, KlT = ext.cross_mfma_ppa(Xs, As, nx, na, 1.3, y, Ky)
        ext.syrk_bf16_acc(KcT, KlT, KK, sk_pair)

    def timed(fn, reps=5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps * 1e3

    print(f"fused A/B rows={rows} m={m} d={d} tiles={tiles} gen={gen} "
          f"pair split_k={sk_pair} fused default split_k="
          f"{ppa_fused_split_k(m)}")
    if not ext.ppa_fused_supported(m, d):
        pair()
        print(f"  pair {min(timed(pair) for _ in range(3)):8.3f} ms   "
              f"fused: unsupported (m, d)")
        return
    # every slice ends in a full tile of atomics: keep blocks <= 1024
    sks = sorted(sk for sk in {1, 2, 4, 8, 16, 25, 32, 64,
                               ppa_fused_split_k(m), max(1, 512 // tiles)}
                 if sk == 1 or tiles * sk <= 1024)
    pair()
    for sk in sks:
        def fused():
            ext.ppa_fused_acc(Xs, As, nx, na, 1.3, y, Ky, KK, sk, gen=gen,
                              absmax=absmax)
        fused()
        tp, tf = [], []
        for _ in range(3):                # alternate
            tp.append(timed(pair))
            tf.append(timed(fused))
        print(f"  split_k={sk:3d}: pair {min(tp):8.3f} ms (max "
              f"{max(tp):8.3f})   fused {min(tf):8.3f} ms (max "
              f"{max(tf):8.3f})   x{min(tp) / min(tf):.2f}")


if "--fused" in sys.argv:
    i = sys.argv.index("--fused")
    _fused_ab(rows, m, int(sys.argv[i + 1]) if len(sys.argv) > i + 1 else 32)
    sys.exit(0)

# hi/lo split of a synthetic fp32 kernel block in (0, 1]
V = torch.rand(rows, m, device=dev, dtype=torch.float32)
Kc = V.to(torch.bfloat16)
Kl = (V - Kc.float()).to(torch.bfloat16)
KcT = Kc.T.contiguous()              # SYRK takes transposed operands [m, c]
KlT = Kl.T.contiguous()

from spark_gp_amd.ops.ppa_plan import ppa_fused_split_k  # noqa: E402

split_k = ppa_fused_split_k(m)      # fills the 256 CUs once
print(f"rows={rows} m={m} split_k={split_k}")

# numerics: KK vs fp64 of the REPRESENTED value (hi+lo), which is what the
# 3-product SYRK computes (lo x lo term ~2^-32, below fp32 resolution)
KK = torch.zeros(m, m, device=dev, dtype=torch.float32)
ext.syrk_bf16_acc(KcT, KlT, KK, split_k)
torch.cuda.synchronize()
Vr = Kc.double() + Kl.double()
ref = Vr.T @ Vr
err = (KK.double() - ref).abs().max().item()
rel = err / ref.abs().max().item()
print(f"max abs err {err:.3e}  rel {rel:.3e}")
assert rel < 3e-5, "SYRK numerics out of tolerance"

# throughput (sustained; caller should pin clocks)
flops = 3 * 2.0 * rows * m * m          # 3 MFMA products
for _ in range(3):
    ext.syrk_bf16_acc(KcT, KlT, KK, split_k)
torch.cuda.synchronize()
reps = 20
t0 = time.perf_counter()
for _ in range(reps):
    ext.syrk_bf16_acc(KcT, KlT, KK, split_k)
torch.cuda.synchronize()
dt = (time.perf_counter() - t0) / reps
print(f"{dt * 1e3:.3f} ms/call  ->  {flops / dt / 1e12:.1f} TF bf16 "
      f"({flops / 3 / dt / 1e12:.1f} TF fp32-equivalent)")

# optional split_k sweep: shorter per-block k-ranges shrink the live
# column-window working set toward L3/L2 residency (the round-1 TCC
# analysis: 38% hit, ~6x compulsory traffic from drifting tiles) at the
# price of split_k-fold output atomic traffic — measure the trade.
if "--sweep" in sys.argv:
    for sk in (split_k, 8, 16, 32, 64, 128, 256):
        for _ in range(2):
            ext.syrk_bf16_acc(KcT, KlT, KK, sk)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(10):
            ext.syrk_bf16_acc(KcT, KlT, KK, sk)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / 10
        print(f"  split_k={sk:4d}: {dt * 1e3:8.3f} ms  "
              f"{flops / dt / 1e12:6.1f} TF bf16")

# A/B the k-synchronized persistent path (m >= 4096)
if "--sync" in sys.argv and m >= 4096:
    from spark_gp_amd.ops import hip_backend as hb
    from spark_gp_amd.ops.ppa_plan import syrk_sync_patch
    launches = hb._syrk_sync_tiles(m, "cuda")
    print(f"sync patch={'x'.join(map(str, syrk_sync_patch()))}: "
          f"{len(launches)} launches, tiles {[n for _, n in launches]}")

    for kpb in (128,):
        def run_sync():
            for tt, nact in launches:
                ext.syrk_bf16_sync_acc(KcT, KlT, KK, tt, kpb, nact)
        for _ in range(2):
            run_sync()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(8):
            run_sync()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / 8
        print(f"sync kpb={kpb:3d}: {dt * 1e3:8.3f} ms/call  ->  "
              f"{flops / dt / 1e12:6.1f} TF bf16")

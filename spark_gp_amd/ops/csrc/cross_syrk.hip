// PPA accumulation kernels for MI355X (gfx950, CDNA4):
//
//  * cross_kernel_tile  — K_nm[c, m] = amp * Kb(q), q = sum_d s2_d (x - a)^2,
//    the rectangular kernel block (K6 in SURVEY.md §2.4), bf16 or fp32 out.
//  * syrk_bf16          — KK[m, m] += K_nm^T K_nm over a chunk (K12, the
//    rows/sec-dominating GEMM): MFMA bf16 16x16x32 tiles, LDS-staged with
//    both operand tiles stored k-major so every fragment load is one
//    ds_read_b128; split-K over the chunk for occupancy; fp32 atomic
//    accumulation into the output.
//  * cross_mfma         — the round-2 PPA fast path: sqdist via
//    ||x'||^2 + ||a'||^2 - 2 x'.a' on f32 matrix cores, transposed hi/lo
//    outputs only, Ky += K^T y fused into the epilogue.
//  * syrk_fused_gen     — the round-3 PPA default (d <= 32, <= 256 tiles):
//    syrk_bf16's tiles and products with the K_nm operand windows
//    GENERATED in the block by cross_mfma's formula instead of staged
//    through HBM (x'.a' from split-f16 operands on the 16-bit matrix pipe by
//    default); Ky += K^T y fused into the diagonal tiles; the k-slices'
//    tiles are summed by syrk_fused_reduce in a fixed order, not by atomics.
//  * syrk_bf16_sync     — k-synchronized persistent SYRK for large m
//    (one block owns one tile; bounded best-effort pacing).
//  * colsum_gemv        — Ky[m] += K_nm^T y (fp64 accumulation;
//    superseded on the PPA path by the fused epilogues, kept as the
//    standalone op).
//
// The three SYRK kernels are one tile body with three fronts.  Defined once
// and shared: the bf16 product pass (syrk_mfma_pass), the tile epilogue of the
// staged kernels (syrk_epilogue, atomic or plain; syrk_fused_gen stores
// partial tiles instead), the k-slice range (syrk_kslice), and for
// the two kernels that stage operands from HBM the lane decomposition,
// the load / LDS-write / prefetch pipeline and its k-loop
// (syrk_staged_steps).  The K_nm value formula (knm_value) and the hi/lo
// split (split_hilo) are shared by the kernel that stores K_nm and the one
// that generates it.  Tile constants shared with the host: kernel_geom.h.
//
// The three kernels that evaluate the covariance function (cross_kernel_tile,
// cross_mfma, syrk_fused_gen) are templates over the family code of
// kernel_geom.h (RBF: Kb = exp(-q); Matern 3/2 and 5/2 over t = sqrt(q)) and
// are instantiated for each; nothing else here depends on the family.  The
// RBF instances are instruction for instruction the kernels they were before
// the template parameter.
//
// Replaces ProjectedGaussianProcessHelper.scala:20-36's per-expert
// crossKernel + breeze gemm accumulation.

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <math.h>

#include "kernel_geom.h"    // SY_CT, SY_BK, SF_DMAX (shared with the host)
#include "launchers.h"

typedef __bf16 bf16;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;

// K_nm from pre-scaled inputs: q = ||x'||^2 + ||a'||^2 - 2 x'.a' clamped at
// 0, v = amp Kb(q) of the family (kernel_geom.h; RBF: amp exp(-q)).
// cross_mfma_kernel stores these values and syrk_fused_gen_kernel generates
// them; both call this one definition.
template <int FAM>
__device__ __forceinline__ float knm_value(const float nx, const float na,
                                           const float dot, const float amp) {
  const float q = nx + na - 2.0f * dot;
  return amp * family_kb<FAM>(q);
}

// hi/lo split: hi + lo carries ~16 mantissa bits, so the SYRK's
// input-quantization error drops to fp32 class
__device__ __forceinline__ void split_hilo(const float v, bf16& hi, bf16& lo) {
  hi = (bf16)v;
  lo = (bf16)(v - (float)hi);
}

// Two-term f16 image of a scaled coordinate for syrk_fused_gen's f16
// generator: v ~ hi + lo * 2^-11 carries 22 significand bits.  hi is zeroed
// below the f16 normal range, so no result depends on how the matrix core
// treats f16 subnormal inputs: such a v goes entirely into lo (absolute error
// below 2e-8).  |v| must be below the f16 range (65504): the host gates on
// 2^15.
typedef _Float16 f16;
typedef __attribute__((ext_vector_type(2))) _Float16 f16x2;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
#define SF_LO_SCALE 2048.0f               // 2^11
#define SF_LO_INV (1.0f / 2048.0f)

__device__ __forceinline__ void split_f16(const float v, f16& hi, f16& lo) {
  hi = (fabsf(v) < 0x1p-14f) ? (f16)0.f : (f16)v;
  lo = (f16)((v - (float)hi) * SF_LO_SCALE);
}

// ---------------------------------------------------------------------------
// cross_kernel_tile: 128x128 output tile per 256-thread block, d-chunked LDS
// ---------------------------------------------------------------------------
// out is written bf16 when out_bf16 != 0, else fp32.

#define CK_TILE 128
#define CK_DBLK 32

template <int FAM>
__global__ void __launch_bounds__(256)
cross_kernel_tile_kernel(const float* __restrict__ X,    // [c, d]
                         const float* __restrict__ A,    // [m, d]
                         const float* __restrict__ s2v,  // [d] scale^2
                         const float amp,
                         const int c, const int m, const int d,
                         bf16* __restrict__ out_bf,      // [c, m] or null
                         bf16* __restrict__ out_lo,      // [c, m] or null:
                                                         // residual v - hi
                         bf16* __restrict__ out_bfT,     // [m, c] or null
                         bf16* __restrict__ out_loT,     // [m, c] or null
                         float* __restrict__ out_f32,    // [c, m] or null
                         const float* __restrict__ yv,   // [c] or null
                         double* __restrict__ Ky) {      // [m] (with yv)
  __shared__ float xs[CK_TILE][CK_DBLK + 1];
  __shared__ float as[CK_TILE][CK_DBLK + 1];
  __shared__ float s2s[CK_DBLK];
  __shared__ double kyred[16][16 + 1];    // fused colsum partials

  const int row0 = blockIdx.x * CK_TILE;
  const int col0 = blockIdx.y * CK_TILE;
  const int tid = threadIdx.x;
  // 16 x 16 thread grid, each thread owns an 8x8 micro-tile
  const int tr = (tid >> 4) * 8;      // row offset within tile
  const int tc = (tid & 15) * 8;      // col offset within tile

  float acc[8][8];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[i][j] = 0.f;

  for (int d0 = 0; d0 < d; d0 += CK_DBLK) {
    const int dl = min(CK_DBLK, d - d0);
    // stage: 256 threads load 128 rows x dl cols of X and A
    for (int f = tid; f < CK_TILE * dl; f += 256) {
      int r = f / dl, q = f - r * dl;
      int gr = row0 + r;
      xs[r][q] = (gr < c) ? X[(size_t)gr * d + d0 + q] : 0.f;
      int gc = col0 + r;
      as[r][q] = (gc < m) ? A[(size_t)gc * d + d0 + q] : 0.f;
    }
    for (int q = tid; q < dl; q += 256) s2s[q] = s2v[d0 + q];
    __syncthreads();

    for (int q = 0; q < dl; ++q) {
      const float w = s2s[q];
      float xf[8], af[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) xf[i] = xs[tr + i][q];
#pragma unroll
      for (int j = 0; j < 8; ++j) af[j] = as[tc + j][q];
#pragma unroll
      for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float t = xf[i] - af[j];
          acc[i][j] += w * t * t;
        }
    }
    __syncthreads();
  }

  // finalize the 8x8 micro-tile once
  bf16 hv[8][8], lv[8][8];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      // acc is a sum of squares: no clamp
      const float v = amp * (FAM == GEOM_FAM_RBF ? __expf(-acc[i][j])
                                                 : family_kb<FAM>(acc[i][j]));
      acc[i][j] = v;
      split_hilo(v, hv[i][j], lv[i][j]);
    }

#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int gr = row0 + tr + i;
    if (gr >= c) continue;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int gc = col0 + tc + j;
      if (gc >= m) continue;
      if (out_bf) {
        out_bf[(size_t)gr * m + gc] = hv[i][j];
        if (out_lo) out_lo[(size_t)gr * m + gc] = lv[i][j];
      } else if (out_f32) {
        out_f32[(size_t)gr * m + gc] = acc[i][j];
      }
    }
  }

  if (out_bfT) {
    // transposed copies [m, c] so the SYRK can stage k-contiguous: per
    // output column j, the 8 row values are contiguous -> one b128 store
    const int gr0 = row0 + tr;
    const bool vec = (c % 8 == 0) && (gr0 + 8 <= c);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int gc = col0 + tc + j;
      if (gc >= m) continue;
      bf16 th[8], tl[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) { th[i] = hv[i][j]; tl[i] = lv[i][j]; }
      if (vec) {
        *(uint4*)&out_bfT[(size_t)gc * c + gr0] = *(uint4*)th;
        if (out_loT) *(uint4*)&out_loT[(size_t)gc * c + gr0] = *(uint4*)tl;
      } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          if (gr0 + i >= c) break;
          out_bfT[(size_t)gc * c + gr0 + i] = th[i];
          if (out_loT) out_loT[(size_t)gc * c + gr0 + i] = tl[i];
        }
      }
    }
  }

  if (yv) {
    // fused colsum (K12's K_mn^T y): accumulate this tile's column sums
    // of K * y straight from the fp32 register values — the separate
    // colsum pass used to RE-READ the whole [c, m] block from HBM (and
    // was the only consumer of the non-transposed copies)
    float s[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float sj = 0.f;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int gr = row0 + tr + i;
        const float yw = (gr < c) ? yv[gr] : 0.f;
        sj += acc[i][j] * yw;
      }
      s[j] = sj;
    }
    const int thr = threadIdx.x >> 4;       // tr / 8 in thread units
    const int thc = threadIdx.x & 15;       // tc / 8 in thread units
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      __syncthreads();
      kyred[thr][thc] = (double)s[j];
      __syncthreads();
      if (thr == 0) {
        double t = 0.0;
#pragma unroll
        for (int r = 0; r < 16; ++r) t += kyred[r][thc];
        const int gc = col0 + thc * 8 + j;
        if (gc < m) atomicAdd(&Ky[gc], t);
      }
    }
  }
}

// ---------------------------------------------------------------------------
// cross_mfma: the K1 MFMA plan — sqdist via ||x||^2 + ||a||^2 - 2 x.a on
// f32 matrix cores (v_mfma_f32_16x16x4_f32: exact fp32 at 157 TF, vs the
// elementwise kernel's ~3 VALU issues per (element, dim)).  PPA mode only:
// inputs arrive PRE-SCALED (x' = x * s per dim) with per-row squared norms;
// outputs are the transposed hi/lo bf16 tiles + the fused Ky += K^T y.
// ---------------------------------------------------------------------------

#define CM_TILE 128
#define CM_DBLK 32
#define CM_STR 36           // f32 LDS row stride ([i][k] layout)

typedef __attribute__((ext_vector_type(4))) float f32x4_;

template <int FAM>
__global__ void __launch_bounds__(256)
cross_mfma_kernel(const float* __restrict__ Xs,   // [c, d] pre-scaled
                  const float* __restrict__ As,   // [m, d] pre-scaled
                  const float* __restrict__ nx,   // [c] ||x'||^2
                  const float* __restrict__ na,   // [m] ||a'||^2
                  const float amp,
                  const int c, const int m, const int d,
                  bf16* __restrict__ out_bfT,     // [m, c]
                  bf16* __restrict__ out_loT,     // [m, c]
                  const float* __restrict__ yv,   // [c]
                  double* __restrict__ Ky) {      // [m]
  __shared__ float xt[CM_TILE * CM_STR];
  __shared__ float at[CM_TILE * CM_STR];
  __shared__ float kyd[CM_TILE];

  const int row0 = blockIdx.x * CM_TILE;          // x rows
  const int col0 = blockIdx.y * CM_TILE;          // a rows (K columns)
  const int tid = threadIdx.x;
  const int wave = tid >> 6;                      // 4 waves, 2x2 grid
  const int lane = tid & 63;
  const int wr = (wave >> 1) * 64;
  const int wc = (wave & 1) * 64;
  const int l16 = lane & 15, kg = lane >> 4;

  for (int f = tid; f < CM_TILE; f += 256) kyd[f] = 0.f;

  // 4x4 tiles of 16x16 per wave = a 64x64 sub-tile
  f32x4_ acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = {0.f, 0.f, 0.f, 0.f};

  for (int d0 = 0; d0 < d; d0 += CM_DBLK) {
    const int dl = min(CM_DBLK, d - d0);
    for (int f = tid; f < CM_TILE * CM_DBLK; f += 256) {
      const int r = f >> 5, q = f & 31;           // [i][k], coalesced on k
      const int gr = row0 + r, gc = col0 + r;
      xt[r * CM_STR + q] = (gr < c && q < dl)
                               ? Xs[(size_t)gr * d + d0 + q] : 0.f;
      at[r * CM_STR + q] = (gc < m && q < dl)
                               ? As[(size_t)gc * d + d0 + q] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int kc = 0; kc < CM_DBLK / 4; ++kc) {
      const int fk = kg + kc * 4;
      float xa[4], ab[4];
#pragma unroll
      for (int a = 0; a < 4; ++a)
        xa[a] = xt[(wr + a * 16 + l16) * CM_STR + fk];
#pragma unroll
      for (int b = 0; b < 4; ++b)
        ab[b] = at[(wc + b * 16 + l16) * CM_STR + fk];
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b)
          acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(
              xa[a], ab[b], acc[a][b], 0, 0, 0);
    }
    __syncthreads();
  }

  // epilogue: q = nx + na - 2 dot; v = amp exp(-q); hi/lo bf16; stores
  // transposed (4 consecutive x-rows per fragment reg -> one 8-B store);
  // fused Ky partials through LDS.
  // f32 16x16x4 D map: col = lane&15, row = (lane>>4)*4 + reg (the
  // dtype-independent standard map — unlike the f64 form, which was
  // measured transposed in reg; verified by the parity unit test).
  const int crow = (lane >> 4) * 4;
  const int ccol = l16;
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const int gr0 = row0 + wr + a * 16 + crow;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int gc = col0 + wc + b * 16 + ccol;
      if (gc >= m) continue;
      const float nav = na[gc];
      bf16 th[4], tl[4];
      float kysum = 0.f;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int gr = gr0 + r;
        float v = 0.f;
        if (gr < c) {
          v = knm_value<FAM>(nx[gr], nav, acc[a][b][r], amp);
          kysum += v * yv[gr];
        }
        split_hilo(v, th[r], tl[r]);
      }
      if ((c % 4 == 0) && gr0 + 4 <= c) {   // 8-B alignment needs 4 | c
        *(uint2*)&out_bfT[(size_t)gc * c + gr0] = *(uint2*)th;
        *(uint2*)&out_loT[(size_t)gc * c + gr0] = *(uint2*)tl;
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if (gr0 + r < c) {
            out_bfT[(size_t)gc * c + gr0 + r] = th[r];
            out_loT[(size_t)gc * c + gr0 + r] = tl[r];
          }
        }
      }
      atomicAdd(&kyd[wc + b * 16 + ccol], kysum);
    }
  }
  __syncthreads();
  for (int f = tid; f < CM_TILE; f += 256) {
    const int gc = col0 + f;
    if (gc < m && kyd[f] != 0.f) atomicAdd(&Ky[gc], (double)kyd[f]);
  }
}

// ---------------------------------------------------------------------------
// The SYRK tile body shared by syrk_bf16, syrk_fused_gen and syrk_bf16_sync
// ---------------------------------------------------------------------------
// 512-thread block = 8 waves in a 4x2 grid; 256x256 output tile per block
// (the largest tile the LDS+register budget allows: per-CU VMEM return
// throughput (~10 B/cyc/CU HBM-bound) is the wall, and bytes/flop scales
// as (M+N)/(M*N), so 256^2 halves traffic vs 128^2); each wave computes a
// 64x128 sub-tile as 4x8 mfma_f32_16x16x32_bf16 tiles.  K-loop: SY_BK=32
// rows held k-major in LDS.  The three kernels differ in where the operand
// tiles come from (staged from HBM or generated), in how blocks are paced,
// and in atomic vs plain accumulation; everything below is common.

#define SY_WG 512
#define SY_STR 40     // k-major [SY_CT][SY_STR] bf16: 32 k + 8 pad = 80-B
                      // rows.  80 B x 16 consecutive lanes covers all 64
                      // LDS banks exactly (20c mod 64 is a permutation of
                      // 4-bank blocks), so staging b128 writes AND fragment
                      // b128 reads are both conflict-free.  4 operands x
                      // 20 KB = 80 KB -> one 8-wave block/CU (2 waves/SIMD).

typedef f32x4 SyAcc[4][8];                // a wave's 64x128 fp32 sub-tile

struct SyLane {
  int tid, wave, lane;
  int wr, wc;                             // wave row / col offset in tile
  int l16;                                // fragment row/col
  int kgrp;                               // 0..3 -> k-subblock of 8
};

__device__ __forceinline__ SyLane sy_lane() {
  SyLane L;
  L.tid = threadIdx.x;
  L.wave = L.tid >> 6;                    // 0..7
  L.lane = L.tid & 63;
  L.wr = (L.wave >> 1) * 64;
  L.wc = (L.wave & 1) * 128;
  L.l16 = L.lane & 15;
  L.kgrp = L.lane >> 4;
  return L;
}

__device__ __forceinline__ void sy_zero(SyAcc& acc) {
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 8; ++b) acc[a][b] = {0.f, 0.f, 0.f, 0.f};
}

// the four k-major bf16 operand tiles of one k-block: rows i0.. (lt) and
// j0.. (rt) of hi^T, and the same of lo^T (ltl, rtl; unused without HILO)
struct SyTiles {
  bf16 *lt, *rt, *ltl, *rtl;
};

__device__ __forceinline__ int syrk_kblocks(const int c) {
  return (c + SY_BK - 1) / SY_BK;
}

// k-blocks [kb0, kb1) of slice `slice` out of split_k; false when empty
__device__ __forceinline__ bool syrk_kslice(const int c, const int split_k,
                                            const int slice, int& kb0,
                                            int& kb1) {
  const int kblocks = syrk_kblocks(c);
  const int per = (kblocks + split_k - 1) / split_k;
  kb0 = slice * per;
  kb1 = min(kblocks, kb0 + per);
  return kb0 < kb1;
}

// one bf16 product pass acc += at^T bt over a k-block, in two b-halves of
// 16 INDEPENDENT MFMAs (no accumulator chaining between consecutive
// issues); fb covers 4 of the 8 column tiles at a time to stay inside the
// register budget.  (This takes the lane's offsets as four ints, not as a
// SyLane: syrk_fused_gen calls it too, see its note.)
__device__ __forceinline__ void syrk_mfma_pass(SyAcc& acc, const bf16* at,
                                               const bf16* bt, const int wr,
                                               const int wc, const int l16,
                                               const int kgrp) {
  bf16x8 fa[4], fb[4];
  const int ko = kgrp * 8;
#pragma unroll
  for (int a = 0; a < 4; ++a)
    fa[a] = *(const bf16x8*)&at[(wr + a * 16 + l16) * SY_STR + ko];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
#pragma unroll
    for (int b = 0; b < 4; ++b)
      fb[b] = *(const bf16x8*)&bt[(wc + (h * 4 + b) * 16 + l16) * SY_STR
                                  + ko];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b)
        acc[a][h * 4 + b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            fa[a], fb[b], acc[a][h * 4 + b], 0, 0, 0);
  }
}

// the products of one k-block: hi^T hi, and with HILO + hi^T lo + lo^T hi
// (lo^T lo ~ 2^-32, dropped), for the staged kernels.  syrk_fused_gen
// issues the same three passes itself, with scheduling barriers between
// them and the operands aliased on diagonal tiles.
template <bool HILO>
__device__ __forceinline__ void syrk_products(SyAcc& acc, const SyTiles& T,
                                              const SyLane& L) {
  syrk_mfma_pass(acc, T.lt, T.rt, L.wr, L.wc, L.l16, L.kgrp);     // hi * hi
  if (HILO) {
    syrk_mfma_pass(acc, T.lt, T.rtl, L.wr, L.wc, L.l16, L.kgrp);  // hi * lo
    syrk_mfma_pass(acc, T.ltl, T.rt, L.wr, L.wc, L.l16, L.kgrp);  // lo * hi
  }
}

// KK tile (i0, j0) += acc, plus its transpose when `mirror`.  C/D layout of
// 16x16x32: col = lane&15, row = (lane>>4)*4 + r.  ATOMIC: several blocks
// (k-slices) add into one element; otherwise the block is the element's
// only owner in this launch and accumulates plainly.
template <bool ATOMIC>
__device__ __forceinline__ void syrk_epilogue(const SyAcc& acc,
                                              float* __restrict__ KK,
                                              const int m, const int i0,
                                              const int j0, const bool mirror,
                                              const int wr, const int wc,
                                              const int l16, const int kgrp) {
  const int crow = kgrp * 4;
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 8; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int gi = i0 + wr + a * 16 + crow + r;
        const int gj = j0 + wc + b * 16 + l16;
        if (gi < m && gj < m) {
          if (ATOMIC) {
            atomicAdd(&KK[(size_t)gi * m + gj], acc[a][b][r]);
            if (mirror) atomicAdd(&KK[(size_t)gj * m + gi], acc[a][b][r]);
          } else {
            KK[(size_t)gi * m + gj] += acc[a][b][r];
            if (mirror) KK[(size_t)gj * m + gi] += acc[a][b][r];
          }
        }
      }
}

// ---------------------------------------------------------------------------
// Staged operands: the TRANSPOSED chunk KcT [m, c] (and KlT) read from HBM
// ---------------------------------------------------------------------------
// Operands arrive TRANSPOSED ([m, c], written for free by the cross
// kernel's register tile), so k runs along the contiguous axis: staging
// is one uint4 global load (8 lanes = one full 128-B line) + one
// conflict-free b128 LDS write per thread, and every MFMA fragment is
// one b128 LDS read.  The old [c, m]-operand versions were LDS- or
// VMEM-instruction bound (8 scalar ops per fragment either way).
//
// thread -> (column, 8-deep k segment); 256 cols x 4 segs = 1024 slots per
// operand = 2 iterations of 512 threads.  Adjacent 4 lanes take the 4
// k-segments of one column (64-B half-lines; the other half of each 128-B
// line is the next k-block's data and hits L2).

struct SyOperands {
  const bf16* KcT;                        // [m, cpitch] hi^T
  const bf16* KlT;                        // [m, cpitch] lo^T (HILO)
  int c, m, cpitch;
};

typedef uint4 SyPrefetch[2][4];           // [iteration][operand]

// 8 consecutive k of column gc; zeros for gc >= m and k >= c
__device__ __forceinline__ uint4 syrk_load8(const bf16* mat,
                                            const SyOperands& P,
                                            const int gc, const int gk0) {
  uint4 v;
  bf16* vals = (bf16*)&v;
  const bool vec_ok = (P.cpitch % 8 == 0);   // 16-B aligned row starts
  if (gc < P.m && vec_ok && gk0 + 8 <= P.c) {
    v = *(const uint4*)(mat + (size_t)gc * P.cpitch + gk0);
  } else if (gc < P.m) {
#pragma unroll
    for (int u = 0; u < 8; ++u)
      vals[u] = (gk0 + u < P.c) ? mat[(size_t)gc * P.cpitch + gk0 + u]
                                : (bf16)0.f;
  } else {
#pragma unroll
    for (int u = 0; u < 8; ++u) vals[u] = (bf16)0.f;
  }
  return v;
}

template <bool HILO>
__device__ __forceinline__ void syrk_stage_load(SyPrefetch& sv,
                                                const SyOperands& P,
                                                const int i0, const int j0,
                                                const int kb, const int tid) {
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int f = tid + it * SY_WG;       // 0..1023
    const int col = f >> 2;
    const int gk0 = kb * SY_BK + (f & 3) * 8;
    sv[it][0] = syrk_load8(P.KcT, P, i0 + col, gk0);
    sv[it][1] = syrk_load8(P.KcT, P, j0 + col, gk0);
    if (HILO) {
      sv[it][2] = syrk_load8(P.KlT, P, i0 + col, gk0);
      sv[it][3] = syrk_load8(P.KlT, P, j0 + col, gk0);
    }
  }
}

template <bool HILO>
__device__ __forceinline__ void syrk_stage_write(const SyPrefetch& sv,
                                                 const SyTiles& T,
                                                 const int tid) {
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int f = tid + it * SY_WG;
    const int o = (f >> 2) * SY_STR + (f & 3) * 8;
    *(uint4*)&T.lt[o] = sv[it][0];
    *(uint4*)&T.rt[o] = sv[it][1];
    if (HILO) {
      *(uint4*)&T.ltl[o] = sv[it][2];
      *(uint4*)&T.rtl[o] = sv[it][3];
    }
  }
}

// k-blocks [kb0, kb1) of tile (i0, j0), with block kb0 already in sv.
// Single-buffer T14 register pipeline: the loads for block kb+1 (while
// kb + 1 < kb_end) are issued before the MFMA phase of block kb, which
// covers their latency; the per-CU VMEM return rate (~10 B/cyc HBM-bound)
// is the wall, which is why the tile is as large as LDS allows.
template <bool HILO>
__device__ __forceinline__ void syrk_staged_steps(
    SyAcc& acc, SyPrefetch& sv, const SyOperands& P, const int i0,
    const int j0, const int kb0, const int kb1, const int kb_end,
    const SyTiles& T, const SyLane& L) {
  for (int kb = kb0; kb < kb1; ++kb) {
    syrk_stage_write<HILO>(sv, T, L.tid);   // LDS free: readers passed barrier
    __syncthreads();
    if (kb + 1 < kb_end) syrk_stage_load<HILO>(sv, P, i0, j0, kb + 1, L.tid);
    syrk_products<HILO>(acc, T, L);
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------
// syrk_bf16: KK[m, m] += K^T K, split-K over the chunk rows for occupancy
// ---------------------------------------------------------------------------
// Grid: (ntile^2, split_k); lower-triangle tile indices exit at once.
// Diagonal tiles (ti == tj) compute the full SY_CT x SY_CT tile and write it
// (the a/b loops cover both halves), so no mirror is needed there; the
// mirror fills the strict lower triangle from the strict upper tiles,
// leaving KK fully populated.
// Resources on gfx950 (hipcc -O3, -Rpass-analysis=kernel-resource-usage):
// <false>: 198 VGPRs, 0 AGPRs, 0 B scratch, 40,960 B LDS; <true>: 256 VGPRs,
// 0 AGPRs, 0 B scratch, 81,920 B LDS; both 2 waves/SIMD.

template <bool HILO>
__global__ void __launch_bounds__(SY_WG, 2)  // force 2 waves/SIMD occupancy
syrk_bf16_kernel(const bf16* __restrict__ KcT,  // [m, cpitch] hi^T
                 const bf16* __restrict__ KlT,  // [m, cpitch] lo^T (HILO)
                 const int c, const int m, const int cpitch, const int ntile,
                 const int split_k,
                 float* __restrict__ KK) {      // [m, m] accumulated
  __shared__ __align__(16) bf16 lt[SY_CT * SY_STR];
  __shared__ __align__(16) bf16 rt[SY_CT * SY_STR];
  __shared__ __align__(16) bf16 ltl[HILO ? SY_CT * SY_STR : 1];
  __shared__ __align__(16) bf16 rtl[HILO ? SY_CT * SY_STR : 1];
  const SyTiles T = {lt, rt, ltl, rtl};

  const int tile = blockIdx.x;
  const int ti = tile / ntile, tj = tile % ntile;
  if (tj < ti) return;                     // upper-triangle tiles only
  const int i0 = ti * SY_CT, j0 = tj * SY_CT;
  int kb0, kb1;
  if (!syrk_kslice(c, split_k, blockIdx.y, kb0, kb1)) return;

  const SyLane L = sy_lane();
  const SyOperands P = {KcT, KlT, c, m, cpitch};
  SyAcc acc;
  sy_zero(acc);
  SyPrefetch sv;
  syrk_stage_load<HILO>(sv, P, i0, j0, kb0, L.tid);
  syrk_staged_steps<HILO>(acc, sv, P, i0, j0, kb0, kb1, kb1, T, L);
  syrk_epilogue<true>(acc, KK, m, i0, j0, ti != tj, L.wr, L.wc, L.l16, L.kgrp);
}

// ---------------------------------------------------------------------------
// syrk_fused_gen: the SYRK above with its operands GENERATED in the block
// ---------------------------------------------------------------------------
// K_nm is a pure function of a d-float row of X' and a d-float row of A',
// so instead of staging hi/lo windows that cross_mfma_kernel wrote to HBM
// (2 x 2 B x c x m per chunk, re-read once per tile that uses a window),
// every block recomputes the two 32 x 256 operand windows of its k-step:
//
//  * tile geometry, wave layout, accumulators and the three bf16 MFMA passes
//    are the shared tile body above, as in syrk_bf16_kernel<true>;
//  * where that kernel prefetches k-block kb+1 into registers around the
//    MFMA phase of kb, this one generates it: wave w owns the 16-column
//    groups 2w and 2w+1 of each window and both 16-row halves of the
//    k-block, i.e. 8 fragments (4 on a diagonal tile) of x'.a', then
//    cross_mfma_kernel's knm_value() and split_hilo();
//  * x'.a' comes from one of two generators, a compile-time switch (G16) on
//    the same tile function.  f32: mfma_f32_16x16x4_f32 over d in
//    cross_mfma_kernel's d order, so the values are the numbers that kernel
//    would store.  f16 (the default inside its range): x' and a' are each
//    split into two f16 terms (split_f16: 22 bits) and x'.a' = xh.ah +
//    2^-11 (xh.al + xl.ah) is three mfma_f32_16x16x32_f16 chained on one fp32
//    accumulator, smallest products first: 3 x 16 cycles per fragment for 8 x
//    32.  The dropped xl.al term is 2^-22 relative, the size of an fp32
//    rounding of the sum; the values are fp32-class but not bit-equal to
//    cross_mfma_kernel's (measured against fp64: PROFILES.md round 12).  d <=
//    32 is exactly the K extent of that MFMA; d-slots >= d hold zeros;
//  * the f32 D layout (col = lane&15, row = (lane>>4)*4 + r) hands each
//    lane 4 consecutive k of one column: one 8-B store per operand into the
//    k-major LDS tiles (80-B column pitch: conflict-free per half-wave),
//    held in registers across the barrier like the old prefetch;
//  * the two fp32 A' windows of the tile (2 x 256 x 36 floats = 72 KB) sit
//    in LDS for the block's lifetime next to the four bf16 operand tiles
//    (80 KB) and the X' stage (4.5 KB): 160,256 B of the 160 KB.  Holding
//    the A' fragments in registers instead was tried first and spilled
//    (143 VGPRs of scratch next to the 128 accumulators).  Both fp32 images
//    are stored fragment-major (slot kgrp*8 + kc holds d-index kgrp + 4*kc),
//    so a lane fetches 4 consecutive kc with one conflict-free b128 read
//    while the MFMAs still run over d in cross_mfma_kernel's order.  The f16
//    generator keeps the same rows and pitch (144 B) and stores hi (64 B)
//    and lo (64 B) of a row side by side in d order, split once per block
//    for A' and at the staging write for X': a lane's 8 consecutive d of one
//    image are one b128 read, the 16x16x32 operand layout, at the bank
//    offsets of the fp32 reads (36 dwords x l16), so equally conflict-free;
//  * X', nx and y of one k-step (32 x 34 floats) are staged through LDS,
//    prefetched one step ahead in registers — the only global reads in
//    the loop;
//  * rows >= c and columns >= m generate exact zeros in hi and lo;
//  * diagonal tiles generate one window, multiply it against itself, and
//    are the only blocks that accumulate Ky += K^T y for their window: from
//    the fp32 values before the split, folded into fp64 registers every
//    k-step, one fp64 atomic per column per block;
//  * the grid holds the upper-triangle tiles only; blocks are independent;
//  * a block ends by storing its 256 x 256 accumulator with plain 16-B stores
//    into its own slot of `partials` ([k-slice][tile], fragment-major, 1 KB
//    per wave store); syrk_fused_reduce_kernel, next in the stream, adds the
//    slices of each element to KK in ascending slice order and gives an
//    off-diagonal element and its mirror the same sum.  No fp32 atomics: KK
//    does not vary from run to run, and off-diagonal tiles are bit-symmetric
//    for every split_k.  Only Ky keeps atomics.
//
// d <= SF_DMAX: the LDS budget above has room for 32 d-slots per row.
// Resources on gfx950 (hipcc -O3, -Rpass-analysis=kernel-resource-usage),
// all six instances (3 families x 2 generators): 232 VGPRs, 0 AGPRs, 0 B
// scratch, no spills, 160,256 B LDS, 2 waves/SIMD (one 8-wave block per CU).
//
// This kernel sits 24 VGPRs under the limit and its register allocation
// follows small changes of form.  It shares syrk_mfma_pass,
// syrk_kslice, knm_value and split_hilo with the other kernels; the
// compiler emits the same instructions for it with or without that sharing.
// Three small pieces stay written out in sf_tile because every shared form
// tried moved the allocation (up to 242 VGPRs, or 36 B of scratch): the
// lane decomposition and accumulator zeroing (sy_lane / sy_zero), the
// fenced three-pass product sequence (syrk_products has no barriers and no
// diagonal aliasing), and the mfma_pass lambda around syrk_mfma_pass.

#define SF_XSTR 36   // X' staging pitch in floats: 32 d-slots, nx, y, pad;
                      // 36*l16 mod 64 is a permutation of 4-bank blocks, so
                      // the A-fragment reads (l16 rows x 4 k) are conflict-free

#define SF_HSTR (2 * SF_XSTR)   // the same pitch in f16 units (144 B)

template <bool DIAG, int FAM, bool G16>
__device__ __forceinline__ void
sf_tile(const float* __restrict__ Xs, const float* __restrict__ As,
        const float* __restrict__ nx, const float* __restrict__ na,
        const float amp, const float* __restrict__ yv,
        const int c, const int m, const int d, const int i0, const int j0,
        const int kb0, const int kb1,
        bf16* __restrict__ lt, bf16* __restrict__ rt,
        bf16* __restrict__ ltl, bf16* __restrict__ rtl,
        float* __restrict__ xs, float* __restrict__ aw,
        double* __restrict__ Ky, float* __restrict__ part) {
  constexpr int NG = DIAG ? 2 : 4;        // generated column groups per wave
  // sy_lane() and sy_zero(), written out (see the note above)
  const int tid = threadIdx.x;
  const int wave = tid >> 6;              // 0..7
  const int lane = tid & 63;
  const int wr = (wave >> 1) * 64;        // wave row offset in tile
  const int wc = (wave & 1) * 128;        // wave col offset in tile
  const int l16 = lane & 15;
  const int kgrp = lane >> 4;
  const int crow = kgrp * 4;              // f32 D fragment: first row of 4

  SyAcc acc;
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 8; ++b) acc[a][b] = {0.f, 0.f, 0.f, 0.f};

  // generation role: group g -> window g>>1 (0 = rows i0.., 1 = cols j0..),
  // 16-column group 2*wave + (g&1) of that window; lane's column = l16
  float nav[NG];
  bool cok[NG];
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    const int gc = ((g >> 1) ? j0 : i0) + (wave * 2 + (g & 1)) * 16 + l16;
    cok[g] = gc < m;
    nav[g] = cok[g] ? na[gc] : 0.f;
  }

  // A' windows -> LDS once per block, fragment-major: slot kgrp*8 + kc holds
  // d-index kgrp + 4*kc, so a lane's 4 consecutive kc are one b128 read.
  // Columns >= m and d-slots >= d are zeros.
  // G16: the same rows hold the two f16 images instead, in d order: hi at
  // f16 slots 0..31 and lo at 32..63 (128 B of the 144-B pitch), so a lane's
  // 8 consecutive d of either image are one b128 read at the same bank
  // offsets (36 dwords x l16) as the fp32 reads.
  f16* const awh = (f16*)aw;
  f16* const xsh = (f16*)xs;
  for (int f = tid; f < (DIAG ? 1 : 2) * SY_CT * SF_DMAX; f += SY_WG) {
    const int w = f / (SY_CT * SF_DMAX);
    const int col = (f / SF_DMAX) % SY_CT, q = f % SF_DMAX;
    const int gc = (w ? j0 : i0) + col;
    const float v = (gc < m && q < d) ? As[(size_t)gc * d + q] : 0.f;
    if constexpr (G16) {
      f16 vh, vl;
      split_f16(v, vh, vl);
      awh[(w * SY_CT + col) * SF_HSTR + q] = vh;
      awh[(w * SY_CT + col) * SF_HSTR + SF_DMAX + q] = vl;
    } else {
      aw[(w * SY_CT + col) * SF_XSTR + (q & 3) * 8 + (q >> 2)] = v;
    }
  }

  // X' staging (same fragment-major slots, + nx at 32, y at 33): thread ->
  // (row, d-slots xsl and xsl+16); lanes 0/1 of each 16 also carry the
  // row's nx / y.  Rows >= c stage zeros.  G16: d-slots 2 xsl and 2 xsl + 1,
  // split here, so each image takes one packed 4-B store; nx and y stay fp32
  // in the same two slots.
  const int xrow = tid >> 4, xsl = tid & 15;
  const int xq0 = G16 ? 2 * xsl : xsl, xq1 = G16 ? 2 * xsl + 1 : xsl + 16;
  float px0, px1, pe;
  auto gload = [&](int kb) {
    const int gr = kb * SY_BK + xrow;
    const bool ok = gr < c;
    px0 = (ok && xq0 < d) ? Xs[(size_t)gr * d + xq0] : 0.f;
    px1 = (ok && xq1 < d) ? Xs[(size_t)gr * d + xq1] : 0.f;
    pe = 0.f;
    if (ok && xsl == 0) pe = nx[gr];
    if (ok && xsl == 1) pe = yv[gr];
  };
  auto xwrite = [&]() {
    if constexpr (G16) {
      f16x2 vh, vl;
      f16 h, l;
      split_f16(px0, h, l);
      vh[0] = h; vl[0] = l;
      split_f16(px1, h, l);
      vh[1] = h; vl[1] = l;
      *(f16x2*)&xsh[xrow * SF_HSTR + xq0] = vh;
      *(f16x2*)&xsh[xrow * SF_HSTR + SF_DMAX + xq0] = vl;
    } else {
      const int o = xrow * SF_XSTR + (xsl & 3) * 8 + (xsl >> 2);
      xs[o] = px0;
      xs[o + 4] = px1;                    // d-slot xsl + 16 -> kc + 4
    }
    if (xsl < 2) xs[xrow * SF_XSTR + 32 + xsl] = pe;
  };

  uint2 gh[2][NG], gl[2][NG];             // generated hi/lo, 4 k per lane
  double kyacc[NG] = {0.0};               // DIAG only: Ky partial per group
  auto generate = [&](int kb) {
    f32x4 dacc[2][NG];
    if constexpr (G16) {
      // x'.a' = xh.ah + 2^-11 (xh.al + xl.ah) [+ 2^-22 xl.al, dropped]: three
      // 16x16x32 f16 MFMAs chained on one accumulator, the smaller products
      // first, one rescale between.  One window (two column groups, four
      // fragments) at a time: the A' images of a window are 16 registers and
      // the four chains cover each other's latency.
      f16x8 xh[2], xl[2];
#pragma unroll
      for (int rg = 0; rg < 2; ++rg) {
        const f16* xr = &xsh[(rg * 16 + l16) * SF_HSTR + kgrp * 8];
        xh[rg] = *(const f16x8*)xr;
        xl[rg] = *(const f16x8*)(xr + SF_DMAX);
      }
#pragma unroll
      for (int w = 0; w < NG / 2; ++w) {
        f16x8 ah[2], al[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const f16* ar = &awh[(w * SY_CT + (wave * 2 + j) * 16 + l16) *
                                   SF_HSTR + kgrp * 8];
          ah[j] = *(const f16x8*)ar;
          al[j] = *(const f16x8*)(ar + SF_DMAX);
        }
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int rg = 0; rg < 2; ++rg)
#pragma unroll
          for (int j = 0; j < 2; ++j)
            dacc[rg][w * 2 + j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(
                xh[rg], al[j], zero, 0, 0, 0);
#pragma unroll
        for (int rg = 0; rg < 2; ++rg)
#pragma unroll
          for (int j = 0; j < 2; ++j)
            dacc[rg][w * 2 + j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(
                xl[rg], ah[j], dacc[rg][w * 2 + j], 0, 0, 0);
#pragma unroll
        for (int rg = 0; rg < 2; ++rg)
#pragma unroll
          for (int j = 0; j < 2; ++j) {
#pragma unroll
            for (int r = 0; r < 4; ++r) dacc[rg][w * 2 + j][r] *= SF_LO_INV;
            dacc[rg][w * 2 + j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(
                xh[rg], ah[j], dacc[rg][w * 2 + j], 0, 0, 0);
          }
        // one window's A' images live at a time (register budget)
        __builtin_amdgcn_sched_barrier(0);
      }
    } else {
#pragma unroll
      for (int rg = 0; rg < 2; ++rg)
#pragma unroll
        for (int g = 0; g < NG; ++g) dacc[rg][g] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int h = 0; h < 2; ++h) {       // kc = 4h .. 4h+3, in d order
        if (h * 16 < d) {                 // uniform; skipped slots are 0*0
          f32x4 xa[2], ab[NG];
#pragma unroll
          for (int rg = 0; rg < 2; ++rg)
            xa[rg] = *(const f32x4*)&xs[(rg * 16 + l16) * SF_XSTR +
                                        kgrp * 8 + h * 4];
#pragma unroll
          for (int g = 0; g < NG; ++g)
            ab[g] = *(const f32x4*)&aw[((g >> 1) * SY_CT +
                                        (wave * 2 + (g & 1)) * 16 + l16) *
                                           SF_XSTR + kgrp * 8 + h * 4];
#pragma unroll
          for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int rg = 0; rg < 2; ++rg)
#pragma unroll
              for (int g = 0; g < NG; ++g)
                dacc[rg][g] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                    xa[rg][u], ab[g][u], dacc[rg][g], 0, 0, 0);
        }
        // keep the second half's fragment loads out of the first half's
        // live range (register budget)
        __builtin_amdgcn_sched_barrier(0);
      }
    }
#pragma unroll
    for (int rg = 0; rg < 2; ++rg) {
      const int lr0 = rg * 16 + crow;
      const int gr0 = kb * SY_BK + lr0;
      float nxr[4], yr[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        nxr[r] = xs[(lr0 + r) * SF_XSTR + 32];
        if (DIAG) yr[r] = xs[(lr0 + r) * SF_XSTR + 33];
      }
#pragma unroll
      for (int g = 0; g < NG; ++g) {
        bf16 th[4], tl[4];
        float kysum = 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float v = knm_value<FAM>(nxr[r], nav[g], dacc[rg][g][r], amp);
          v = (cok[g] && gr0 + r < c) ? v : 0.f;   // exact zeros outside
          if (DIAG) kysum += v * yr[r];            // y stages 0 for rows >= c
          split_hilo(v, th[r], tl[r]);
        }
        gh[rg][g] = *(uint2*)th;
        gl[rg][g] = *(uint2*)tl;
        if (DIAG) kyacc[g] += (double)kysum;
      }
    }
  };
  auto write_gen = [&]() {
#pragma unroll
    for (int rg = 0; rg < 2; ++rg)
#pragma unroll
      for (int g = 0; g < NG; ++g) {
        const int lc = (wave * 2 + (g & 1)) * 16 + l16;
        const int o = lc * SY_STR + rg * 16 + crow;
        *(uint2*)&((g >> 1) ? rt : lt)[o] = gh[rg][g];
        *(uint2*)&((g >> 1) ? rtl : ltl)[o] = gl[rg][g];
      }
  };
  auto mfma_pass = [&](const bf16* at, const bf16* bt) {
    syrk_mfma_pass(acc, at, bt, wr, wc, l16, kgrp);
  };

  gload(kb0);
  xwrite();
  __syncthreads();
  if (kb0 + 1 < kb1) gload(kb0 + 1);
  generate(kb0);
  for (int kb = kb0; kb < kb1; ++kb) {
    const bool more = kb + 1 < kb1;       // block-uniform
    __syncthreads();                      // xs and the tiles are free
    write_gen();                          // operands of block kb
    if (more) xwrite();                   // X' of block kb+1
    __syncthreads();
    if (more && kb + 2 < kb1) gload(kb + 2);   // covered by a whole step
    // Generation of kb+1 and the products of kb are independent, but they
    // share the matrix pipe, and their transient registers (X'/A'
    // fragments + f32 tiles vs. bf16 fragments) must not be live together:
    // the sched barriers keep the phases apart (234 VGPRs, no scratch;
    // without them the allocator spills).  Running the two phases in
    // opposite order on the two waves of a SIMD was measured: no gain.
    if (more) generate(kb + 1);
    __builtin_amdgcn_sched_barrier(0);
    mfma_pass(lt, DIAG ? lt : rt);        // hi * hi
    __builtin_amdgcn_sched_barrier(0);
    mfma_pass(lt, DIAG ? ltl : rtl);      // hi * lo
    __builtin_amdgcn_sched_barrier(0);
    mfma_pass(ltl, DIAG ? lt : rt);       // lo * hi
  }

  // the block's tile of partial sums -> its own slot, fragment-major
  // ([a*8 + b][thread] f32x4): every wave store is 1 KB contiguous
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 8; ++b)
      *(f32x4*)&part[((a * 8 + b) * SY_WG + tid) * 4] = acc[a][b];

  if (DIAG) {
    // the 4 k-groups of a wave hold partials of the same 16 columns
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      double t = kyacc[g];
      t += __shfl_xor(t, 16);
      t += __shfl_xor(t, 32);
      const int gc = i0 + (wave * 2 + g) * 16 + l16;
      if (kgrp == 0 && gc < m) atomicAdd(&Ky[gc], t);
    }
  }
}

template <int FAM, bool G16>
__global__ void __launch_bounds__(SY_WG, 2)
syrk_fused_gen_kernel(const float* __restrict__ Xs,   // [c, d] pre-scaled
                      const float* __restrict__ As,   // [m, d] pre-scaled
                      const float* __restrict__ nx,   // [c] ||x'||^2
                      const float* __restrict__ na,   // [m] ||a'||^2
                      const float amp,
                      const float* __restrict__ yv,   // [c]
                      const int c, const int m, const int d, const int ntile,
                      const int split_k,
                      double* __restrict__ Ky,        // [m] accumulated
                      float* __restrict__ partials) { // [slice][tile] tiles
  __shared__ __align__(16) bf16 lt[SY_CT * SY_STR];
  __shared__ __align__(16) bf16 rt[SY_CT * SY_STR];
  __shared__ __align__(16) bf16 ltl[SY_CT * SY_STR];
  __shared__ __align__(16) bf16 rtl[SY_CT * SY_STR];
  __shared__ __align__(16) float xs[SY_BK * SF_XSTR];
  __shared__ __align__(16) float aw[2 * SY_CT * SF_XSTR];

  // blockIdx.x enumerates the upper triangle row by row
  int ti = 0, rem = blockIdx.x;
  while (rem >= ntile - ti) { rem -= ntile - ti; ++ti; }
  const int tj = ti + rem;
  int kb0, kb1;                           // empty slice: block-uniform exit
  if (!syrk_kslice(c, split_k, blockIdx.y, kb0, kb1)) return;
  float* part = partials + sf_partial_offset(blockIdx.y, blockIdx.x,
                                             gridDim.x);

  if (ti == tj)
    sf_tile<true, FAM, G16>(Xs, As, nx, na, amp, yv, c, m, d, ti * SY_CT,
                            tj * SY_CT, kb0, kb1, lt, rt, ltl, rtl, xs, aw,
                            Ky, part);
  else
    sf_tile<false, FAM, G16>(Xs, As, nx, na, amp, yv, c, m, d, ti * SY_CT,
                             tj * SY_CT, kb0, kb1, lt, rt, ltl, rtl, xs, aw,
                             Ky, part);
}

// KK += the k-slices' partial tiles of syrk_fused_gen_kernel, summed per
// element in ascending slice order; an off-diagonal tile's element and its
// mirror receive the same sum.  Grid (tiles, 32 fragments), SY_WG threads:
// thread t of block (tile, f) owns the f32x4 that thread t of the tile's
// blocks stored for fragment f, i.e. 4 consecutive rows of one column, so
// each KK element has one owner and is accumulated plainly.  Slices without
// rows wrote nothing and are not read: they are the trailing ones of
// syrk_kslice.
__global__ void __launch_bounds__(SY_WG)
syrk_fused_reduce_kernel(const float* __restrict__ partials,
                         const int c, const int m, const int ntile,
                         const int split_k,
                         float* __restrict__ KK) {      // [m, m] accumulated
  int ti = 0, rem = blockIdx.x;
  while (rem >= ntile - ti) { rem -= ntile - ti; ++ti; }
  const int tj = ti + rem;
  const int frag = blockIdx.y, a = frag >> 3, b = frag & 7;
  const SyLane L = sy_lane();

  f32x4 sum = {0.f, 0.f, 0.f, 0.f};
  for (int s = 0; s < split_k; ++s) {
    int kb0, kb1;
    if (!syrk_kslice(c, split_k, s, kb0, kb1)) break;
    sum += *(const f32x4*)&partials[sf_partial_offset(s, blockIdx.x,
                                                      gridDim.x) +
                                    (frag * SY_WG + L.tid) * 4];
  }
  const int gj = tj * SY_CT + L.wc + b * 16 + L.l16;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int gi = ti * SY_CT + L.wr + a * 16 + L.kgrp * 4 + r;
    if (gi < m && gj < m) {
      KK[(size_t)gi * m + gj] += sum[r];
      if (ti != tj) KK[(size_t)gj * m + gi] += sum[r];
    }
  }
}

// ---------------------------------------------------------------------------
// syrk_bf16_sync:k-SYNCHRONIZED variant for large m (round-2, TODO item 1)
// ---------------------------------------------------------------------------
// At m >= 4096 the plain kernel's co-scheduled tiles drift apart in k, so
// no XCD's L2 ever holds the column windows its tiles are reading (round-1
// TCC analysis: 38% hit, ~6x compulsory HBM traffic).  This variant keeps
// every live tile on the SAME k-phase: one block owns ONE output tile for
// the whole launch (accumulators never leave AGPRs), the host passes a
// tile list clustered so each XCD's blocks share row/column windows, and
// blocks pace each other between k-phases through a per-phase arrival
// counter.  The pacing spin is BOUNDED and best-effort: there is no data
// dependency between blocks, so a timeout only loses locality, never
// correctness — no grid-residency assumption, no deadlock risk.

// Resources on gfx950 (same flags as above):
// <false>: 198 VGPRs, 0 AGPRs, 0 B scratch, 40,960 B LDS; <true>: 254 VGPRs,
// 0 AGPRs, 0 B scratch, 81,920 B LDS; both 2 waves/SIMD.

template <bool HILO>
__global__ void __launch_bounds__(SY_WG, 2)
syrk_bf16_sync_kernel(const bf16* __restrict__ KcT,   // [m, cpitch] hi^T
                      const bf16* __restrict__ KlT,   // [m, cpitch] lo^T
                      const int c, const int m, const int cpitch,
                      const int* __restrict__ tiles,  // [nb, 2]; -1 = idle
                      const int kpb,                  // k-blocks per phase
                      int* __restrict__ phase_ctr,    // [nphases], zeroed
                      const int nactive,
                      float* __restrict__ KK) {
  const int ti = tiles[2 * blockIdx.x];
  const int tj = tiles[2 * blockIdx.x + 1];
  if (ti < 0) return;
  const int i0 = ti * SY_CT, j0 = tj * SY_CT;
  const int kblocks = syrk_kblocks(c);

  __shared__ __align__(16) bf16 lt[SY_CT * SY_STR];
  __shared__ __align__(16) bf16 rt[SY_CT * SY_STR];
  __shared__ __align__(16) bf16 ltl[HILO ? SY_CT * SY_STR : 1];
  __shared__ __align__(16) bf16 rtl[HILO ? SY_CT * SY_STR : 1];
  const SyTiles T = {lt, rt, ltl, rtl};

  const SyLane L = sy_lane();
  const SyOperands P = {KcT, KlT, c, m, cpitch};
  SyAcc acc;
  sy_zero(acc);
  SyPrefetch sv;
  syrk_stage_load<HILO>(sv, P, i0, j0, 0, L.tid);
  const int nphases = (kblocks + kpb - 1) / kpb;
  for (int p = 0; p < nphases; ++p) {
    syrk_staged_steps<HILO>(acc, sv, P, i0, j0, p * kpb,
                            min(kblocks, (p + 1) * kpb), kblocks, T, L);
    // best-effort pacing: arrive, then wait (bounded) for the cohort.
    // Relaxed atomics only — nothing is communicated, so no fences.
    if (p + 1 < nphases) {
      if (L.tid == 0) {
        __hip_atomic_fetch_add(&phase_ctr[p], 1, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
        int spins = 0;
        while (__hip_atomic_load(&phase_ctr[p], __ATOMIC_RELAXED,
                                 __HIP_MEMORY_SCOPE_AGENT) < nactive &&
               ++spins < 1500)
          __builtin_amdgcn_s_sleep(8);
      }
      __syncthreads();
    }
  }

  // single owner per element per launch -> plain accumulate
  syrk_epilogue<false>(acc, KK, m, i0, j0, ti != tj, L.wr, L.wc, L.l16, L.kgrp);
}

// ---------------------------------------------------------------------------
// colsum_gemv: Ky[m] += Kc^T y (fp64 accumulate per block, one atomic per
// column)
// ---------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(256)
colsum_gemv_kernel(const bf16* __restrict__ Kc,   // [c, m]
                   const float* __restrict__ y,   // [c]
                   const int c, const int m,
                   const int rows_per_block,
                   double* __restrict__ Ky) {     // [m] fp64
  const int col = blockIdx.x * 64 + (threadIdx.x & 63);
  const int rseg = blockIdx.y;
  const int warp = threadIdx.x >> 6;        // 4 waves split the row range
  if (col >= m) return;
  const int r0 = rseg * rows_per_block + warp;
  const int r1 = min(c, rseg * rows_per_block + rows_per_block);
  double acc = 0.0;
  for (int r = r0; r < r1; r += 4) {
    acc += (double)(float)Kc[(size_t)r * m + col] * (double)y[r];
  }
  // one fp64 atomic per (column, wave, rseg)
  atomicAdd(&Ky[col], acc);
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------
// KERNEL<family[, further template arguments]>, or null for an unknown
// family code
#define FAMILY_KERNEL(KERNEL, family, ...)                            \
  ((family) == GEOM_FAM_RBF   ? KERNEL<GEOM_FAM_RBF, ##__VA_ARGS__>   \
   : (family) == GEOM_FAM_M32 ? KERNEL<GEOM_FAM_M32, ##__VA_ARGS__>   \
   : (family) == GEOM_FAM_M52 ? KERNEL<GEOM_FAM_M52, ##__VA_ARGS__>   \
                              : nullptr)

extern "C" hipError_t launch_cross_kernel_tile(
    const float* X, const float* A, const float* s2v, float amp,
    int c, int m, int d, void* out, void* out_lo, void* out_t,
    void* out_lo_t, int out_is_bf16, const float* yv, double* Ky,
    int family, hipStream_t stream) {
  const auto kern = FAMILY_KERNEL(cross_kernel_tile_kernel, family);
  if (!kern) return hipErrorInvalidValue;
  dim3 grid((c + CK_TILE - 1) / CK_TILE, (m + CK_TILE - 1) / CK_TILE);
  hipLaunchKernelGGL(kern, grid, dim3(256), 0, stream,
                     X, A, s2v, amp, c, m, d,
                     out_is_bf16 ? (bf16*)out : nullptr,
                     out_is_bf16 ? (bf16*)out_lo : nullptr,
                     (bf16*)out_t, (bf16*)out_lo_t,
                     out_is_bf16 ? nullptr : (float*)out, yv, Ky);
  return hipGetLastError();
}

extern "C" hipError_t launch_cross_mfma(const float* Xs, const float* As,
                                         const float* nx, const float* na,
                                         float amp, int c, int m, int d,
                                         void* out_bfT, void* out_loT,
                                         const float* yv, double* Ky,
                                         int family, hipStream_t stream) {
  const auto kern = FAMILY_KERNEL(cross_mfma_kernel, family);
  if (!kern) return hipErrorInvalidValue;
  dim3 grid((c + CM_TILE - 1) / CM_TILE, (m + CM_TILE - 1) / CM_TILE);
  hipLaunchKernelGGL(kern, grid, dim3(256), 0, stream,
                     Xs, As, nx, na, amp, c, m, d,
                     (bf16*)out_bfT, (bf16*)out_loT, yv, Ky);
  return hipGetLastError();
}

extern "C" hipError_t launch_syrk_bf16_sync(const void* KcT, const void* KlT,
                                            int c, int m, int cpitch,
                                            const int* tiles, int nb,
                                            int kpb, int* phase_ctr,
                                            int nactive, float* KK,
                                            hipStream_t stream) {
  if (KlT) {
    hipLaunchKernelGGL((syrk_bf16_sync_kernel<true>), dim3(nb), dim3(SY_WG),
                       0, stream, (const bf16*)KcT, (const bf16*)KlT, c, m,
                       cpitch, tiles, kpb, phase_ctr, nactive, KK);
  } else {
    hipLaunchKernelGGL((syrk_bf16_sync_kernel<false>), dim3(nb), dim3(SY_WG),
                       0, stream, (const bf16*)KcT, nullptr, c, m,
                       cpitch, tiles, kpb, phase_ctr, nactive, KK);
  }
  return hipGetLastError();
}

extern "C" hipError_t launch_syrk_bf16(const void* KcT, const void* KlT,
                                       int c, int m, int cpitch, int split_k,
                                       float* KK, hipStream_t stream) {
  const int ntile = (m + SY_CT - 1) / SY_CT;
  dim3 grid(ntile * ntile, split_k);
  if (KlT) {
    hipLaunchKernelGGL((syrk_bf16_kernel<true>), grid, dim3(SY_WG), 0,
                       stream, (const bf16*)KcT, (const bf16*)KlT, c, m,
                       cpitch, ntile, split_k, KK);
  } else {
    hipLaunchKernelGGL((syrk_bf16_kernel<false>), grid, dim3(SY_WG), 0,
                       stream, (const bf16*)KcT, nullptr, c, m, cpitch,
                       ntile, split_k, KK);
  }
  return hipGetLastError();
}

extern "C" hipError_t launch_syrk_fused_gen(
    const float* Xs, const float* As, const float* nx, const float* na,
    float amp, const float* yv, int c, int m, int d, int split_k,
    double* Ky, float* KK, float* partials, int family, int gen_f16,
    hipStream_t stream) {
  const auto kern =
      gen_f16 ? FAMILY_KERNEL(syrk_fused_gen_kernel, family, true)
              : FAMILY_KERNEL(syrk_fused_gen_kernel, family, false);
  if (!kern) return hipErrorInvalidValue;
  const int ntile = (m + SY_CT - 1) / SY_CT;
  dim3 grid(ntile * (ntile + 1) / 2, split_k);   // upper-triangle tiles
  hipLaunchKernelGGL(kern, grid, dim3(SY_WG), 0, stream,
                     Xs, As, nx, na, amp, yv, c, m, d, ntile, split_k, Ky,
                     partials);
  // same stream: runs after every block's partial tile is written
  hipLaunchKernelGGL(syrk_fused_reduce_kernel, dim3(grid.x, 32), dim3(SY_WG),
                     0, stream, partials, c, m, ntile, split_k, KK);
  return hipGetLastError();
}

extern "C" hipError_t launch_colsum_gemv(const void* Kc, const float* y,
                                         int c, int m, double* Ky,
                                         hipStream_t stream) {
  const int rows_per_block = 4096;
  dim3 grid((m + 63) / 64, (c + rows_per_block - 1) / rows_per_block);
  hipLaunchKernelGGL(colsum_gemv_kernel, grid, dim3(256), 0, stream,
                     (const bf16*)Kc, y, c, m, rows_per_block, Ky);
  return hipGetLastError();
}

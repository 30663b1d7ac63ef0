// Fused per-expert BCM negative-log-marginal-likelihood + gradient kernel for
// experts of 128 < k <= 1024 rows on MI355X (gfx950, CDNA4): what
// expert_nll.hip computes, for matrices that do not fit LDS.
//
// Persistent workgroups (512 threads = 8 waves), grid = min(E, resident
// workgroups, scratch bound, caller's cap); workgroup b walks the experts b,
// b + grid, ... and keeps the kp x kp fp32 matrix of the one it is on in ITS
// slab of a global scratch [grid, kp, kp] (kp: k up to whole super-blocks of
// SB rows).  The padding rows and columns carry an identity, so that every
// block of every phase is a full SB x SB block: no ragged tile anywhere, and
// the padding adds log 1 to the determinant and nothing to any product that
// is read.  The slab is rewritten from phase B on for every expert; nothing
// is carried from one expert to the next.
//
// Every O(k^3) phase is a sequence of SB x SB block products
//   acc[i][j] += sum_c Aop[i][c] Bop[c][j]
// on v_mfma_f32_16x16x4_f32: the two operands are staged from the slab into
// LDS NLP_KC contraction indices at a time (As[i][c], Bs[j][c], row stride
// NLP_KS), transposed and masked to a lower triangle on the way where the
// phase asks for it, so that the MFMA loop itself carries no condition; a
// wave holds its 16x16 output tiles (8 at SB = 128, 2 at SB = 64) in
// registers over the whole contraction and writes them once, after the
// barrier behind the last fragment read (the register-tiles-across-a-barrier
// idiom of expert_nll.hip), which is what makes the in-place updates safe.
//
//   B  lower = amp Kb + noise I, strict upper = the cache phase W reads (Kb
//      for RBF, t = sqrt(q) for the Matern families), block by block:
//      q = n_a + n_b - 2 x'_a . x'_b over scaled-X slabs staged in LDS
//   C  left-looking blocked Cholesky: block (I, J) less sum_{K<J} L_IK L_JK^T;
//      the diagonal block goes to LDS and through chol_invert_lower
//      (linalg_lds.h, unchanged: L, then V_JJ = L_JJ^-1, fp64 log-det, bad
//      flag), V_JJ replaces it in the slab (L_JJ has no reader left), and the
//      panel is L_IJ = A_IJ V_JJ^T, a plain block product
//   D  V_IJ = -V_II sum_{J<=K<I} L_IK V_KJ, rows top to bottom, columns left
//      to right, in place (the sum is parked in block (I, J) in between)
//   E  alpha = V^T (V y), fp64 sums; nll = 1/2 y.alpha + 1/2 logdet
//   L  K^-1 = V^T V, lower triangle, rows top to bottom, the diagonal block
//      of a row last
//   W  W0 = (alpha alpha^T - K^-1) o Kd in 64 x 64 tiles, the mirrored tile
//      transposed through LDS so that both triangles move in whole lines;
//      trG and sumW0 = sum G o Kb in fp64; W0 = 0 on the padding
//   H  contr'_j = 2 sum_a x'_aj (x'_aj r_a - (W0 X')_aj): row sums r, then
//      W0 X' as block products against scaled-X slabs, folded per fragment
//      into per-(row tile, column) partials and summed in fp64 by the one
//      thread that owns the column; de-scaled by s^2 at output
//
// All reductions run in a fixed order, without atomics: the outputs of an
// expert do not depend on the grid or on which workgroup took it.  A failed
// leaf ends the expert there with out_bad set (the host recomputes it) and
// the workgroup goes on to its next one.
//
// Numerics: fp32 storage and factorization, fp64 scalar accumulation.
// Constraints: 128 < k <= 1024, d <= 128 (nlp_supported_kd).

#include <hip/hip_runtime.h>
#include <math.h>

#define WG 512
#include "linalg_lds.h"
#include "kernel_geom.h"
#include "launchers.h"

typedef __attribute__((ext_vector_type(4))) float mfma_f32x4;

template <int SB>
struct PanelGeom {
  static constexpr int NT = SB / 16;                 // tiles per block edge
  static constexpr int NTW = NT * NT / (WG / 64);    // tiles per wave
  static constexpr int SAB = SB + 4;                 // = geom_sa(SB)
  static_assert(SB == 64 || SB == 128, "super-block of 64 or 128 rows");
  static_assert(WG % SB == 0 && SB % NLP_WT == 0, "whole staging passes");
};

struct PanelLds {
  double* red;   // 8 (per-wave partials)
  double* misc;  // 2: logdet, scratch
  double* hs;    // NLP_D_MAX: the gradient contraction per column
  float* P;      // nlp_pbuf_floats: the leaf's block; phase W's tile
  float* T;      // nlp_tsz: the leaf's temp
  float* As;     // SB x NLP_KS
  float* Bs;     // SB x NLP_KS
  float* Hp;     // (SB / 16) x SB: phase H's per-row-tile partials
  float* yb;     // kp each: y (0 on the padding)
  float* alpha;
  float* tvec;
  float* rrow;
  float* nrm;
  float* sc;     // d: scale
  float* s2;     // d: scale^2
  int* bad;
};

// Region sizes: nlp_lds_bytes (kernel_geom.h) lists them in this order.
__device__ inline PanelLds panel_carve(char* base, int sb, int kp, int d) {
  PanelLds L;
  char* p = base;
  L.red = (double*)p;  L.misc = L.red + 8;
  p += a16(sizeof(double) * 10);
  L.hs = (double*)p;   p += a16(sizeof(double) * NLP_D_MAX);
  L.P = (float*)p;     p += a16(sizeof(float) * nlp_pbuf_floats(sb));
  L.T = (float*)p;     p += a16(sizeof(float) * nlp_tsz(sb));
  L.As = (float*)p;    p += a16(sizeof(float) * (size_t)sb * NLP_KS);
  L.Bs = (float*)p;    p += a16(sizeof(float) * (size_t)sb * NLP_KS);
  L.Hp = (float*)p;    p += a16(sizeof(float) * (size_t)(sb / 16) * sb);
  L.yb = (float*)p;    p += a16(sizeof(float) * kp);
  L.alpha = (float*)p; p += a16(sizeof(float) * kp);
  L.tvec = (float*)p;  p += a16(sizeof(float) * kp);
  L.rrow = (float*)p;  p += a16(sizeof(float) * kp);
  L.nrm = (float*)p;   p += a16(sizeof(float) * kp);
  L.sc = (float*)p;    p += a16(sizeof(float) * d);
  L.s2 = (float*)p;    p += a16(sizeof(float) * d);
  L.bad = (int*)p;
  return L;
}

// ---- operand staging --------------------------------------------------
// A chunk dst[SB][NLP_KS] holds the contraction indices c0 .. c0 + NLP_KC of
// an operand.  `src` is the origin of an SB x SB block of the slab (row
// stride ld); `lower` keeps the elements of the block with row >= column and
// zeroes the rest (a triangular factor whose other half holds the cache).
// The load is unconditional (the whole block is inside the slab) and the
// mask a select behind it.

// dst[i][c] = src[i][c0 + c]: 128-B lines along c
template <int SB>
__device__ __forceinline__ void stage_n(float* dst, const float* src,
                                        const int ld, const int c0,
                                        const bool lower, const int tid) {
  const int c = tid & (NLP_KC - 1);
#pragma unroll
  for (int i = tid / NLP_KC; i < SB; i += WG / NLP_KC) {
    const float v = src[(size_t)i * ld + c0 + c];
    dst[i * NLP_KS + c] = (lower && c0 + c > i) ? 0.f : v;
  }
}

// dst[i][c] = src[c0 + c][i]: lines along i
template <int SB>
__device__ __forceinline__ void stage_t(float* dst, const float* src,
                                        const int ld, const int c0,
                                        const bool lower, const int tid) {
  const int i = tid & (SB - 1);
#pragma unroll
  for (int c = tid / SB; c < NLP_KC; c += WG / SB) {
    const float v = src[(size_t)(c0 + c) * ld + i];
    dst[i * NLP_KS + c] = (lower && c0 + c < i) ? 0.f : v;
  }
}

// dst[i][c] = x'[r0 + i][c0 + c], zero past k rows or d columns
template <int SB>
__device__ __forceinline__ void stage_x_rows(float* dst,
                                             const float* __restrict__ Xe,
                                             const float* sc, const int r0,
                                             const int k, const int d,
                                             const int c0, const int tid) {
  const int c = tid & (NLP_KC - 1), col = c0 + c;
  const float s = col < d ? sc[col] : 0.f;
#pragma unroll
  for (int i = tid / NLP_KC; i < SB; i += WG / NLP_KC) {
    const int row = r0 + i;
    dst[i * NLP_KS + c] =
        (row < k && col < d) ? Xe[(size_t)row * d + col] * s : 0.f;
  }
}

// dst[j][c] = x'[r0 + c0 + c][j0 + j], zero past k rows or d columns
template <int SB>
__device__ __forceinline__ void stage_x_cols(float* dst,
                                             const float* __restrict__ Xe,
                                             const float* sc, const int r0,
                                             const int j0, const int k,
                                             const int d, const int c0,
                                             const int tid) {
  const int j = tid & (SB - 1), col = j0 + j;
  const float s = col < d ? sc[col] : 0.f;
#pragma unroll
  for (int c = tid / SB; c < NLP_KC; c += WG / SB) {
    const int row = r0 + c0 + c;
    dst[j * NLP_KS + c] =
        (row < k && col < d) ? Xe[(size_t)row * d + col] * s : 0.f;
  }
}

// ---- the block product ------------------------------------------------
// Tile u of wave w is tile w NTW + u of the block in row-major order: at
// SB = 128 a wave owns one tile row (one A fragment feeds its 8 MFMAs of a
// step), at SB = 64 half of one.
template <int SB>
__device__ __forceinline__ void tile_of(const int wave, const int u, int& ti,
                                        int& tj) {
  const int t = wave * PanelGeom<SB>::NTW + u;
  ti = t / PanelGeom<SB>::NT;
  tj = t % PanelGeom<SB>::NT;
}

// one staged chunk: NLP_KC / 4 MFMA steps of every tile of the wave.
// Fragment element (row l16, k index kg) of step c: As[16 ti + l16][c + kg].
template <int SB>
__device__ __forceinline__ void mma_chunk(
    mfma_f32x4 (&acc)[PanelGeom<SB>::NTW], const float* As, const float* Bs,
    const int wave, const int l16, const int kg) {
  constexpr int NTW = PanelGeom<SB>::NTW;
#pragma unroll
  for (int c = 0; c < NLP_KC; c += 4) {
    float av[NTW], bv[NTW];
#pragma unroll
    for (int u = 0; u < NTW; ++u) {
      int ti, tj;
      tile_of<SB>(wave, u, ti, tj);
      av[u] = As[(ti * 16 + l16) * NLP_KS + c + kg];
      bv[u] = Bs[(tj * 16 + l16) * NLP_KS + c + kg];
    }
#pragma unroll
    for (int u = 0; u < NTW; ++u)
      acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u], bv[u], acc[u],
                                                    0, 0, 0);
  }
}

// acc += over `depth` contraction indices (a multiple of NLP_KC), the
// chunk at c0 staged by sa(c0) into As and sb(c0) into Bs.  Ends behind a
// barrier: every operand read of the product is complete on return, so the
// caller may overwrite an operand block with the result.
template <int SB, class FA, class FB>
__device__ __forceinline__ void gemm_loop(
    mfma_f32x4 (&acc)[PanelGeom<SB>::NTW], const int depth, const float* As,
    const float* Bs, const int wave, const int l16, const int kg, FA&& sa,
    FB&& sb) {
  for (int c0 = 0; c0 < depth; c0 += NLP_KC) {
    sa(c0);
    sb(c0);
    __syncthreads();
    mma_chunk<SB>(acc, As, Bs, wave, l16, kg);
    __syncthreads();
  }
}

template <int SB>
__device__ __forceinline__ void zero_acc(
    mfma_f32x4 (&acc)[PanelGeom<SB>::NTW]) {
#pragma unroll
  for (int u = 0; u < PanelGeom<SB>::NTW; ++u) acc[u] = {0.f, 0.f, 0.f, 0.f};
}

// f(row, column, value) for every element this lane holds, block-local
// (D map of the MFMA: row = 4 (lane >> 4) + r, column = lane & 15)
template <int SB, class F>
__device__ __forceinline__ void each_elem(
    const mfma_f32x4 (&acc)[PanelGeom<SB>::NTW], const int wave,
    const int l16, const int kg, F&& f) {
#pragma unroll
  for (int u = 0; u < PanelGeom<SB>::NTW; ++u) {
    int ti, tj;
    tile_of<SB>(wave, u, ti, tj);
#pragma unroll
    for (int r = 0; r < 4; ++r)
      f(ti * 16 + kg * 4 + r, tj * 16 + l16, acc[u][r]);
  }
}

template <int FAM, int SB>
__global__ void __launch_bounds__(WG)
fused_expert_nll_panel_kernel(const float* __restrict__ Xg,
                              const float* __restrict__ yg,
                              const float* __restrict__ scale,   // [d]
                              const float amp, const float noise,
                              const int E, const int k, const int d,
                              float* scratch,          // [grid, kp, kp]
                              double* __restrict__ out_nll,      // [E]
                              double* __restrict__ out_sumW0,    // [E]
                              double* __restrict__ out_trG,      // [E]
                              double* __restrict__ out_contr,    // [E, d]
                              int* __restrict__ out_bad) {       // [E]
  using G = PanelGeom<SB>;
  constexpr int SAB = G::SAB;
  extern __shared__ char lds_raw[];
  const int kp = nlp_kp(k, SB), nb = kp / SB;
  const PanelLds S = panel_carve(lds_raw, SB, kp, d);
  float* const A = scratch + (size_t)blockIdx.x * kp * kp;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l16 = lane & 15, kg = lane >> 4;
  // block (I, J) of the slab
  const auto blk = [&](const int I, const int J) {
    return A + (size_t)I * SB * kp + (size_t)J * SB;
  };

  for (int j = tid; j < d; j += WG) {
    const float s = scale[j];
    S.sc[j] = s;
    S.s2[j] = s * s;
  }

  for (int e = blockIdx.x; e < E; e += gridDim.x) {
    // the expert before is done with every LDS region (and sc is visible)
    __syncthreads();
    const float* Xe = Xg + (size_t)e * k * d;
    const float* ye = yg + (size_t)e * k;

    // ---- A: y and the row norms ||x'_a||^2, zero on the padding ------
    for (int i = tid; i < kp; i += WG) {
      float n = 0.f;
      if (i < k)
        for (int c = 0; c < d; ++c) {
          const float v = Xe[(size_t)i * d + c] * S.sc[c];
          n = __builtin_fmaf(v, v, n);
        }
      S.nrm[i] = n;
      S.yb[i] = i < k ? ye[i] : 0.f;
    }
    if (tid < NLP_D_MAX) S.hs[tid] = 0.0;
    if (tid == 0) { *S.bad = 0; S.misc[0] = 0.0; }
    __syncthreads();

    mfma_f32x4 acc[G::NTW];

    // ---- B: lower = amp Kb + noise I (identity on the padding); strict
    // upper = the cache of phase W ------------------------------------
    {
      const int dd = (d + NLP_KC - 1) / NLP_KC * NLP_KC;
      for (int I = 0; I < nb; ++I)
        for (int J = 0; J <= I; ++J) {
          zero_acc<SB>(acc);
          gemm_loop<SB>(
              acc, dd, S.As, S.Bs, wave, l16, kg,
              [&](int c0) {
                stage_x_rows<SB>(S.As, Xe, S.sc, I * SB, k, d, c0, tid);
              },
              [&](int c0) {
                stage_x_rows<SB>(S.Bs, Xe, S.sc, J * SB, k, d, c0, tid);
              });
          each_elem<SB>(acc, wave, l16, kg, [&](int li, int lj, float v) {
            const int gi = I * SB + li, gj = J * SB + lj;
            if (gj > gi) return;
            float* lo = A + (size_t)gi * kp + gj;
            if (gi >= k) {                  // padding: identity
              *lo = gi == gj ? 1.f : 0.f;
              return;
            }
            const float q = S.nrm[gi] + S.nrm[gj] - 2.0f * v;
            const float qc = q > 0.f ? q : 0.f;
            *lo = amp * family_kb<FAM>(q) + (gi == gj ? noise : 0.f);
            if (gi != gj)
              A[(size_t)gj * kp + gi] =
                  FAM == GEOM_FAM_RBF ? __expf(-qc) : sqrtf(qc);
          });
        }
      __syncthreads();                      // the slab is complete
    }

    // ---- C: left-looking blocked Cholesky; V_JJ on the diagonal ------
    for (int J = 0; J < nb; ++J) {
      zero_acc<SB>(acc);
      for (int K = 0; K < J; ++K)
        gemm_loop<SB>(
            acc, SB, S.As, S.Bs, wave, l16, kg,
            [&](int c0) { stage_n<SB>(S.As, blk(J, K), kp, c0, false, tid); },
            [&](int c0) { stage_n<SB>(S.Bs, blk(J, K), kp, c0, false, tid); });
      {
        const float* D = blk(J, J);
        each_elem<SB>(acc, wave, l16, kg, [&](int li, int lj, float v) {
          if (lj <= li) S.P[li * SAB + lj] = D[(size_t)li * kp + lj] - v;
        });
      }
      __syncthreads();
      chol_invert_lower(S.P, S.T, SB, SAB, tid, S.bad, S.misc);
      __syncthreads();
      if (*S.bad) break;
      {
        float* D = blk(J, J);
        for (int f = tid; f < SB * SB; f += WG) {
          const int li = f / SB, lj = f % SB;
          if (lj <= li) D[(size_t)li * kp + lj] = S.P[li * SAB + lj];
        }
      }
      __syncthreads();
      for (int I = J + 1; I < nb; ++I) {
        float* B = blk(I, J);
        if (J > 0) {
          zero_acc<SB>(acc);
          for (int K = 0; K < J; ++K)
            gemm_loop<SB>(
                acc, SB, S.As, S.Bs, wave, l16, kg,
                [&](int c0) {
                  stage_n<SB>(S.As, blk(I, K), kp, c0, false, tid);
                },
                [&](int c0) {
                  stage_n<SB>(S.Bs, blk(J, K), kp, c0, false, tid);
                });
          each_elem<SB>(acc, wave, l16, kg, [&](int li, int lj, float v) {
            B[(size_t)li * kp + lj] -= v;
          });
          __syncthreads();
        }
        // L_IJ = A_IJ V_JJ^T
        zero_acc<SB>(acc);
        gemm_loop<SB>(
            acc, SB, S.As, S.Bs, wave, l16, kg,
            [&](int c0) { stage_n<SB>(S.As, B, kp, c0, false, tid); },
            [&](int c0) { stage_n<SB>(S.Bs, blk(J, J), kp, c0, true, tid); });
        each_elem<SB>(acc, wave, l16, kg, [&](int li, int lj, float v) {
          B[(size_t)li * kp + lj] = v;
        });
        __syncthreads();
      }
    }
    if (*S.bad) {
      if (tid == 0) {
        out_bad[e] = *S.bad;     // 1: indefinite, 2: non-finite iterate
        out_nll[e] = 0.0; out_sumW0[e] = 0.0; out_trG[e] = 0.0;
      }
      for (int j = tid; j < d; j += WG) out_contr[(size_t)e * d + j] = 0.0;
      continue;
    }
    const double logdet = S.misc[0];

    // ---- D: V_IJ = -V_II sum_{J<=K<I} L_IK V_KJ, in place ------------
    for (int I = 1; I < nb; ++I)
      for (int J = 0; J < I; ++J) {
        float* B = blk(I, J);
        zero_acc<SB>(acc);
        for (int K = J; K < I; ++K)
          gemm_loop<SB>(
              acc, SB, S.As, S.Bs, wave, l16, kg,
              [&](int c0) {
                stage_n<SB>(S.As, blk(I, K), kp, c0, false, tid);
              },
              [&](int c0) {
                stage_t<SB>(S.Bs, blk(K, J), kp, c0, K == J, tid);
              });
        each_elem<SB>(acc, wave, l16, kg, [&](int li, int lj, float v) {
          B[(size_t)li * kp + lj] = v;
        });
        __syncthreads();
        zero_acc<SB>(acc);
        gemm_loop<SB>(
            acc, SB, S.As, S.Bs, wave, l16, kg,
            [&](int c0) { stage_n<SB>(S.As, blk(I, I), kp, c0, true, tid); },
            [&](int c0) { stage_t<SB>(S.Bs, B, kp, c0, false, tid); });
        each_elem<SB>(acc, wave, l16, kg, [&](int li, int lj, float v) {
          B[(size_t)li * kp + lj] = -v;
        });
        __syncthreads();
      }

    // ---- E: alpha = V^T (V y), y.alpha -------------------------------
    // t_i = sum_{c<=i} V_ic y_c: a wave per row, lanes along the row
    for (int i = wave; i < kp; i += WG / 64) {
      double s = 0.0;
      for (int c = lane; c <= i; c += 64)
        s += (double)A[(size_t)i * kp + c] * (double)S.yb[c];
      s = wave_sum(s);
      if (lane == 0) S.tvec[i] = (float)s;
    }
    __syncthreads();
    // alpha_a = sum_{c>=a} V_ca t_c: a thread per column, lines along a
    for (int a = tid; a < kp; a += WG) {
      double s0 = 0.0, s1 = 0.0;
      int c = a;
      for (; c + 1 < k; c += 2) {
        s0 += (double)A[(size_t)c * kp + a] * (double)S.tvec[c];
        s1 += (double)A[(size_t)(c + 1) * kp + a] * (double)S.tvec[c + 1];
      }
      if (c < k) s0 += (double)A[(size_t)c * kp + a] * (double)S.tvec[c];
      S.alpha[a] = a < k ? (float)(s0 + s1) : 0.f;
    }
    __syncthreads();
    double part = 0.0;
    for (int i = tid; i < k; i += WG)
      part += (double)S.yb[i] * (double)S.alpha[i];
    const double yta = block_sum(part, S.red, tid);

    // ---- L: K^-1 = V^T V, lower triangle -----------------------------
    // Block (I, J) = sum_{K>=I} V_KI^T V_KJ.  Rows top to bottom and the
    // diagonal block of a row last: V_IJ is read by the blocks above it in
    // its column and by row J, all done by then, and V_II by all of row I.
    for (int I = 0; I < nb; ++I)
      for (int J = 0; J <= I; ++J) {
        zero_acc<SB>(acc);
        for (int K = I; K < nb; ++K)
          gemm_loop<SB>(
              acc, SB, S.As, S.Bs, wave, l16, kg,
              [&](int c0) {
                stage_t<SB>(S.As, blk(K, I), kp, c0, K == I, tid);
              },
              [&](int c0) {
                stage_t<SB>(S.Bs, blk(K, J), kp, c0, K == J, tid);
              });
        float* B = blk(I, J);
        each_elem<SB>(acc, wave, l16, kg, [&](int li, int lj, float v) {
          if (I != J || lj <= li) B[(size_t)li * kp + lj] = v;
        });
        __syncthreads();
      }

    // ---- W: W0 = (aa^T - K^-1) o Kd, both triangles; trG, and sumW0 =
    // sum (aa^T - K^-1) o Kb.  Tile (bi, bj), bi >= bj, of the lower
    // triangle and its mirror U[c][r] = A[bj NLP_WT + c][bi NLP_WT + r],
    // which arrives holding the cache and leaves holding W0. -----------
    double trg_part = 0.0, sw_part = 0.0;
    {
      constexpr int WT = NLP_WT, US = NLP_WT + 1;
      float* U = S.P;
      const int ntw = kp / WT;
      for (int bi = 0; bi < ntw; ++bi)
        for (int bj = 0; bj <= bi; ++bj) {
          float* up = A + (size_t)bj * WT * kp + (size_t)bi * WT;
          for (int f = tid; f < WT * WT; f += WG) {
            const int c = f / WT, r = f % WT;
            U[c * US + r] = up[(size_t)c * kp + r];
          }
          __syncthreads();
          for (int f = tid; f < WT * WT; f += WG) {
            const int r = f / WT, c = f % WT;
            if (bi == bj && c > r) continue;
            const int a = bi * WT + r, b = bj * WT + c;
            float* lo = A + (size_t)a * kp + b;
            float w = 0.f;
            if (a < k) {                    // b <= a: off the padding
              const float g = S.alpha[a] * S.alpha[b] - *lo;
              float gkb;                    // g * Kb; w = g * Kd
              if (FAM == GEOM_FAM_RBF) {
                const float kb = (a == b) ? 1.0f : U[c * US + r];
                w = g * kb;
                gkb = w;
              } else {
                float kb, kd;
                family_kb_kd<FAM>((a == b) ? 0.0f : U[c * US + r], kb, kd);
                w = g * kd;
                gkb = g * kb;
              }
              if (a == b) {
                trg_part += (double)g;
                sw_part += (double)gkb;
              } else {
                sw_part += 2.0 * (double)gkb;
              }
            }
            *lo = w;
            if (a != b) U[c * US + r] = w;
          }
          __syncthreads();
          for (int f = tid; f < WT * WT; f += WG) {
            const int c = f / WT, r = f % WT;
            if (bi != bj || c < r) up[(size_t)c * kp + r] = U[c * US + r];
          }
          __syncthreads();
        }
    }
    const double trG = block_sum(trg_part, S.red, tid);
    const double sumW0 = block_sum(sw_part, S.red, tid);

    // ---- G: row sums of W0 -------------------------------------------
    for (int a = wave; a < kp; a += WG / 64) {
      double s = 0.0;
      for (int b = lane; b < kp; b += 64) s += (double)A[(size_t)a * kp + b];
      s = wave_sum(s);
      if (lane == 0) S.rrow[a] = (float)s;
    }
    __syncthreads();

    // ---- H: contr'_j = 2 sum_a x'_aj (x'_aj r_a - (W0 X')_aj) ---------
    // Row block I against the SB columns from j0 on: W0 X' as block
    // products over K, folded per fragment, one fp32 partial per (row tile,
    // column) into Hp, and those summed in fp64 into hs[column] by the
    // thread of that column.
    for (int I = 0; I < nb; ++I)
      for (int j0 = 0; j0 < d; j0 += SB) {
        zero_acc<SB>(acc);
        for (int K = 0; K < nb; ++K)
          gemm_loop<SB>(
              acc, SB, S.As, S.Bs, wave, l16, kg,
              [&](int c0) {
                stage_n<SB>(S.As, blk(I, K), kp, c0, false, tid);
              },
              [&](int c0) {
                stage_x_cols<SB>(S.Bs, Xe, S.sc, K * SB, j0, k, d, c0, tid);
              });
#pragma unroll
        for (int u = 0; u < G::NTW; ++u) {
          int ti, tj;
          tile_of<SB>(wave, u, ti, tj);
          const int gj = j0 + tj * 16 + l16;
          const float sj = gj < d ? S.sc[gj] : 0.f;
          float p = 0.f;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int gi = I * SB + ti * 16 + kg * 4 + r;
            if (gi < k && gj < d) {
              const float x = Xe[(size_t)gi * d + gj] * sj;
              p = __builtin_fmaf(2.0f * x, x * S.rrow[gi] - acc[u][r], p);
            }
          }
          // the 4 row groups sharing a column: lanes l, l+16, l+32, l+48
          p += __shfl_down(p, 32, 64);
          p += __shfl_down(p, 16, 64);
          if (kg == 0) S.Hp[ti * SB + tj * 16 + l16] = p;
        }
        __syncthreads();
        if (tid < SB && j0 + tid < d) {
          double s = 0.0;
#pragma unroll
          for (int ti = 0; ti < G::NT; ++ti) s += (double)S.Hp[ti * SB + tid];
          S.hs[j0 + tid] += s;
        }
        __syncthreads();
      }

    // the contraction ran in scaled coordinates: contr' = s2_j * contr;
    // s2_j == 0 => dK/dbeta_j == 0: emit 0 (the exact limit)
    for (int j = tid; j < d; j += WG) {
      const double s2j = (double)S.s2[j];
      out_contr[(size_t)e * d + j] = s2j > 0.0 ? S.hs[j] / s2j : 0.0;
    }
    if (tid == 0) {
      out_bad[e] = 0;
      out_nll[e] = 0.5 * yta + 0.5 * logdet;
      out_sumW0[e] = sumW0;
      out_trG[e] = trG;
    }
  }
}

typedef void (*nlp_kernel_t)(const float*, const float*, const float*, float,
                             float, int, int, int, float*, double*, double*,
                             double*, double*, int*);

template <int SB>
static nlp_kernel_t nlp_kernel_fam(int family) {
  switch (family) {
    case GEOM_FAM_RBF: return fused_expert_nll_panel_kernel<GEOM_FAM_RBF, SB>;
    case GEOM_FAM_M32: return fused_expert_nll_panel_kernel<GEOM_FAM_M32, SB>;
    case GEOM_FAM_M52: return fused_expert_nll_panel_kernel<GEOM_FAM_M52, SB>;
  }
  return nullptr;
}

// the front of a family code and super-block; null for an unknown one
static nlp_kernel_t nlp_kernel_of(int family, int sb) {
  if (sb == 64) return nlp_kernel_fam<64>(family);
  if (sb == 128) return nlp_kernel_fam<128>(family);
  return nullptr;
}

// dynamic LDS of a launch; 0 when the shape is not supported
static size_t nlp_launch_lds(int k, int d, int sb) {
  if (!nlp_supported_kd(k, d) || !nlp_sb_ok(sb)) return 0;
  const size_t lds = nlp_lds_bytes(sb, k, d);
  return lds <= GEOM_LDS_MAX ? lds : 0;
}

extern "C" hipError_t launch_fused_expert_nll_panel(
    const float* X, const float* y, const float* scale, float amp,
    float noise, int E, int k, int d, float* scratch, int grid, int sb,
    double* out_nll, double* out_sumW0, double* out_trG, double* out_contr,
    int* out_bad, int family, hipStream_t stream) {
  const nlp_kernel_t kern = nlp_kernel_of(family, sb);
  if (!kern) return hipErrorInvalidValue;
  const size_t lds = nlp_launch_lds(k, d, sb);
  if (!lds) return hipErrorInvalidConfiguration;
  if (grid < 1 || grid > E || !scratch ||
      nlp_scratch_floats(grid, k, sb) * sizeof(float) >
          NLP_SCRATCH_MAX_BYTES)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(WG), lds, stream, X, y, scale,
                     amp, noise, E, k, d, scratch, out_nll, out_sumW0,
                     out_trG, out_contr, out_bad);
  return hipGetLastError();
}

// workgroups of the kernel the runtime keeps resident per CU at the block
// size and dynamic LDS launch_fused_expert_nll_panel uses for (k, d, sb)
extern "C" hipError_t fused_expert_nll_panel_resident_wgs(int k, int d,
                                                          int family, int sb,
                                                          int* out) {
  const nlp_kernel_t kern = nlp_kernel_of(family, sb);
  if (!kern) return hipErrorInvalidValue;
  const size_t lds = nlp_launch_lds(k, d, sb);
  if (!lds) return hipErrorInvalidConfiguration;
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(out, kern, WG, lds);
}

// K14 — fused projected-process prediction for MI355X (gfx950, CDNA4):
//
//   mean_r = sum_j c_rj mv_j
//   var_r  = kxx + sum_ij c_ri M_ij c_rj        c_rj = amp Kb(q(x_r, a_j))
//
// for test rows X [t, d] against the active set A [m, d], with the magic
// vector mv [m] and the symmetric magic matrix M [m, m] in fp64.  One block
// owns a tile of TR rows and keeps their whole cross row c [TR, m] in LDS as
// fp32, so no [t, m] array exists in global memory in any precision:
//
//  1. cross values — q = sum_d s2_d (x_rd - a_jd)^2 by differences, the form
//     of cross_kernel_tile_kernel, staged PP_DBLK dims x PP_CB active points
//     at a time; the running q of a (row, column) lives in its c slot between
//     d-passes and the last pass replaces it by amp Kb(q) (family_kb).
//  2. mean — a wave per row, products and sum in fp64.
//  3. variance — U = C M on v_mfma_f64_16x16x4_f64: A fragments converted
//     from the fp32 c tile (exact), B fragments read straight from M (each
//     fragment row is 128 contiguous bytes) one 16-deep k block ahead of the
//     MFMAs that use them.  M is symmetric, so only its lower 16 x 16 blocks
//     are read and multiplied, the off-diagonal ones doubled: U is the lower
//     block triangle's share, and sum_j U_rj c_rj is still the whole form.
//     U never leaves the accumulators: the epilogue multiplies it by c and
//     reduces per row, in fp64.  Fragment and D maps:
//     big_chol.hip (A lane l -> [i = l&15][k = l>>4], B lane l ->
//     [k = l>>4][j = l&15], D lane l reg r -> [(l>>4) + 4r][l&15]).
//
// Tails are safe by construction: rows past t, active points past m and dims
// past d are staged as zeros, columns [m, mp) of c are written as zeros, the
// M loads are predicated on (k < m, j < m), and only rows < t are stored.
// Only M's lower triangle and its diagonal blocks' upper halves are read.
//
// Geometry (tile height, LDS carve, the gate): kernel_geom.h.

#include <hip/hip_runtime.h>
#include <math.h>

#include "kernel_geom.h"
#include "launchers.h"

typedef __attribute__((ext_vector_type(4))) double f64x4;

#define PP_WAVES (PP_THREADS / 64)
#define PP_KU 4   // k-steps (of 4) per prefetched B block: 16 k, the width of
                  // a column tile, so M's diagonal blocks are whole k blocks
static_assert(4 * PP_KU == 16, "a k block must span one 16-column tile");

__device__ __forceinline__ double pp_load_m(const double* __restrict__ M,
                                            const int m, const int k,
                                            const int j) {
  return (k < m && j < m) ? M[(size_t)k * m + j] : 0.0;
}

// The B fragments of the 16-deep k block at k0 for NB column tiles whose
// first starts at k = kb: tile b's diagonal block is the one at
// k0 = kb + 16 b; the blocks below it carry the factor 2 of the symmetric
// sum, the blocks above it are not read.
template <int NB>
__device__ __forceinline__ void pp_load_b(double (&bf)[PP_KU][NB],
                                          const double* __restrict__ M,
                                          const int m, const int k0,
                                          const int kb, const int kg,
                                          const int (&jc)[NB]) {
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    const int kd = kb + b * 16;
    const double w = k0 > kd ? 2.0 : 1.0;
#pragma unroll
    for (int s = 0; s < PP_KU; ++s)
      bf[s][b] = k0 >= kd ? w * pp_load_m(M, m, k0 + 4 * s + kg, jc[b]) : 0.0;
  }
}

template <int FAM, bool VAR, int TR>
__global__ void __launch_bounds__(PP_THREADS)
ppa_predict_kernel(const float* __restrict__ X,     // [t, d]
                   const float* __restrict__ A,     // [m, d]
                   const float* __restrict__ s2v,   // [d] scale^2
                   const float amp,
                   const double* __restrict__ mv,   // [m]
                   const double* __restrict__ M,    // [m, m] symmetric (VAR)
                   const double kxx,
                   const long t, const int m, const int d,
                   double* __restrict__ mean,       // [t]
                   double* __restrict__ var) {      // [t] (VAR)
  extern __shared__ char lds_raw[];
  const int mp = pp_mp(m);
  const int CSTR = pp_cstr(m);
  // carve: the order of pp_lds_bytes
  char* p = lds_raw;
  double* red = (double*)p;
  p += a16(sizeof(double) * PP_WAVES * (size_t)TR);
  float* cs = (float*)p;
  p += a16(sizeof(float) * (size_t)TR * CSTR);
  float (*as)[PP_DBLK + 1] = (float (*)[PP_DBLK + 1])p;
  p += a16(sizeof(float) * PP_CB * (PP_DBLK + 1));
  float (*xs)[PP_DBLK + 1] = (float (*)[PP_DBLK + 1])p;
  p += a16(sizeof(float) * (size_t)TR * (PP_DBLK + 1));
  float* s2s = (float*)p;

  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const long row0 = (long)blockIdx.x * TR;

  // ---- 1. cross values ---------------------------------------------------
  // 16 x 32 thread grid; a thread owns rows rg + 16 i and, per column pass,
  // columns cg + 32 j: the as reads of a wave fall on 32 distinct banks and
  // its xs reads are two broadcasts.
  constexpr int NR = TR / 16;
  const int rg = tid >> 5, cg = tid & 31;
  for (int d0 = 0; d0 < d; d0 += PP_DBLK) {
    const int dl = min(PP_DBLK, d - d0);
    const bool first = d0 == 0, last = d0 + PP_DBLK >= d;
    for (int f = tid; f < TR * dl; f += PP_THREADS) {
      const int r = f / dl, q = f - r * dl;
      const long gr = row0 + r;
      xs[r][q] = (gr < t) ? X[(size_t)gr * d + d0 + q] : 0.f;
    }
    for (int q = tid; q < dl; q += PP_THREADS) s2s[q] = s2v[d0 + q];
    for (int cb = 0; cb < mp; cb += PP_CB) {
      for (int f = tid; f < PP_CB * dl; f += PP_THREADS) {
        const int r = f / dl, q = f - r * dl;
        const int gc = cb + r;
        as[r][q] = (gc < m) ? A[(size_t)gc * d + d0 + q] : 0.f;
      }
      __syncthreads();
      float acc[NR][4];
#pragma unroll
      for (int i = 0; i < NR; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int col = cb + cg + 32 * j;
          acc[i][j] = (!first && col < mp)
                          ? cs[(size_t)(rg + 16 * i) * CSTR + col] : 0.f;
        }
      for (int q = 0; q < dl; ++q) {
        const float w = s2s[q];
        float xf[NR], af[4];
#pragma unroll
        for (int i = 0; i < NR; ++i) xf[i] = xs[rg + 16 * i][q];
#pragma unroll
        for (int j = 0; j < 4; ++j) af[j] = as[cg + 32 * j][q];
#pragma unroll
        for (int i = 0; i < NR; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float df = xf[i] - af[j];
            acc[i][j] += w * df * df;
          }
      }
#pragma unroll
      for (int i = 0; i < NR; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int col = cb + cg + 32 * j;
          if (col >= mp) continue;
          float v = acc[i][j];
          if (last) v = (col < m) ? amp * family_kb<FAM>(v) : 0.f;
          cs[(size_t)(rg + 16 * i) * CSTR + col] = v;
        }
      __syncthreads();
    }
  }

  // ---- 2. mean: a wave per row ------------------------------------------
  for (int r = wave; r < TR; r += PP_WAVES) {
    double s = 0.0;
    for (int j = lane; j < m; j += 64)
      s += (double)cs[(size_t)r * CSTR + j] * mv[j];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0 && row0 + r < t) mean[row0 + r] = s;
  }
  if (!VAR) return;

  // ---- 3. variance: U = C M on the f64 MFMA, var = kxx + rowsum(U o C) ---
  // A wave takes groups of NB 16-column tiles of U over all TR rows: NA x NB
  // independent accumulators (4, 4, 2 for TR = 64, 32, 16) cover the MFMA's
  // dependent latency, and each B fragment feeds NA MFMAs.
  constexpr int NA = TR / 16;
  constexpr int NB = NA >= 4 ? 1 : 2;
  const int l16 = lane & 15, kg = lane >> 4;
  const int ngrp = (mp / 16 + NB - 1) / NB;
  double vsum[NA][4];
#pragma unroll
  for (int a = 0; a < NA; ++a)
#pragma unroll
    for (int r = 0; r < 4; ++r) vsum[a][r] = 0.0;

  // M is symmetric: a column tile reads its 16 x 16 diagonal block once and
  // the blocks below it doubled (the factor 2 goes onto the B fragment, which
  // is exact), and never the blocks above.  A group's work shrinks with g, so
  // the waves take the groups of successive rounds in serpentine order.
  for (int gb = 0, it = 0; gb < ngrp; gb += PP_WAVES, ++it) {
    const int g = gb + ((it & 1) ? PP_WAVES - 1 - wave : wave);
    if (g >= ngrp) continue;                 // wave-uniform
    const int kb = g * NB * 16;              // first k of the first tile
    int jc[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) jc[b] = kb + b * 16 + l16;
    f64x4 acc[NA][NB];
#pragma unroll
    for (int a = 0; a < NA; ++a)
#pragma unroll
      for (int b = 0; b < NB; ++b) acc[a][b] = {0.0, 0.0, 0.0, 0.0};
    double bq[PP_KU][NB];
    pp_load_b<NB>(bq, M, m, kb, kb, kg, jc);
    for (int k0 = kb; k0 < mp; k0 += 4 * PP_KU) {
      // next block's B fragments (zeros past m, without a read)
      double bn[PP_KU][NB];
      pp_load_b<NB>(bn, M, m, k0 + 4 * PP_KU, kb, kg, jc);
#pragma unroll
      for (int s = 0; s < PP_KU; ++s) {
        double af[NA];
#pragma unroll
        for (int a = 0; a < NA; ++a)
          af[a] = (double)cs[(size_t)(a * 16 + l16) * CSTR + k0 + 4 * s + kg];
#pragma unroll
        for (int b = 0; b < NB; ++b) {
          if (k0 < kb + b * 16) continue;    // above tile b's diagonal
#pragma unroll
          for (int a = 0; a < NA; ++a)
            acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(
                af[a], bq[s][b], acc[a][b], 0, 0, 0);
        }
      }
#pragma unroll
      for (int s = 0; s < PP_KU; ++s)
#pragma unroll
        for (int b = 0; b < NB; ++b) bq[s][b] = bn[s][b];
    }
    // U[row][col] at lane l reg r: row = (l>>4) + 4r, col = l&15
#pragma unroll
    for (int a = 0; a < NA; ++a)
#pragma unroll
      for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = a * 16 + kg + 4 * r;
          const float cv = (jc[b] < mp) ? cs[(size_t)row * CSTR + jc[b]] : 0.f;
          vsum[a][r] += acc[a][b][r] * (double)cv;
        }
  }

  // sum over the 16 columns a lane group holds, then over the waves
#pragma unroll
  for (int a = 0; a < NA; ++a)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      double s = vsum[a][r];
#pragma unroll
      for (int o = 8; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
      if (l16 == 0) red[wave * TR + a * 16 + kg + 4 * r] = s;
    }
  __syncthreads();
  if (tid < TR && row0 + tid < t) {
    double s = kxx;
#pragma unroll
    for (int w = 0; w < PP_WAVES; ++w) s += red[w * TR + tid];
    var[row0 + tid] = s;
  }
}

// ---------------------------------------------------------------------------
// launcher
// ---------------------------------------------------------------------------

template <int FAM, bool VAR>
static hipError_t pp_launch(int tr, const float* X, const float* A,
                            const float* s2v, float amp, const double* mv,
                            const double* M, double kxx, long t, int m, int d,
                            double* mean, double* var, hipStream_t stream) {
  const size_t lds = pp_lds_bytes(tr, m);
  const dim3 grid((unsigned)((t + tr - 1) / tr)), blk(PP_THREADS);
#define PP_CASE(TR_)                                                        \
  hipLaunchKernelGGL((ppa_predict_kernel<FAM, VAR, TR_>), grid, blk, lds,   \
                     stream, X, A, s2v, amp, mv, M, kxx, t, m, d, mean, var)
  switch (tr) {
    case 64: PP_CASE(64); break;
    case 32: PP_CASE(32); break;
    case 16: PP_CASE(16); break;
    default: return hipErrorInvalidConfiguration;
  }
#undef PP_CASE
  return hipGetLastError();
}

extern "C" hipError_t launch_ppa_predict(
    const float* X, const float* A, const float* s2v, float amp,
    const double* mv, const double* M, double kxx, long t, int m, int d,
    double* mean, double* var, int family, hipStream_t stream) {
  if (!geom_family_ok(family)) return hipErrorInvalidValue;
  if (!ppa_predict_supported_md(m, d) || t < 0 ||
      (t + 15) / 16 > 0x7fffffffL)
    return hipErrorInvalidConfiguration;
  if (t == 0) return hipSuccess;
  const int tr = pp_tile_rows(m);
#define PP_FAM(FAM_)                                                        \
  (var ? pp_launch<FAM_, true>(tr, X, A, s2v, amp, mv, M, kxx, t, m, d,     \
                               mean, var, stream)                           \
       : pp_launch<FAM_, false>(tr, X, A, s2v, amp, mv, M, kxx, t, m, d,    \
                                mean, var, stream))
  switch (family) {
    case GEOM_FAM_RBF: return PP_FAM(GEOM_FAM_RBF);
    case GEOM_FAM_M32: return PP_FAM(GEOM_FAM_M32);
    default:           return PP_FAM(GEOM_FAM_M52);
  }
#undef PP_FAM
}

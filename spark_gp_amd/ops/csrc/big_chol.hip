// K13 — hand-written blocked fp64 Cholesky path for the m x m "magic"
// solves of the PPA (ProjectedGaussianProcessHelper
// .scala:49-65), m up to 8192, MI355X (gfx950, CDNA4):
//
//  * dpotrf_diag_kernel — one-workgroup 64x64 diagonal-block factor
//    (8x8 fp64 __shfl sub-factors, row-per-lane) that also emits the
//    block's explicit lower-triangular inverse V = L_JJ^{-1}, so the
//    panel solve and the later triangular solves become plain GEMMs;
//  * dgemm64_kernel — 64x64-tile fp64 GEMM on v_mfma_f64_16x16x4_f64
//    (2048 flop/instr; fp64 matrix peak ~78 TF), templated over
//    {A^T, B^T, store/subtract, SYRK-lower-only}; drives the panel
//    trsm (L21 = A21 V^T), the trailing update (A22 -= L21 L21^T) and
//    both blocked triangular solves (forward L Y = B, backward
//    L^T X = Y) with any number of right-hand sides (1 for the magic
//    vector, m for the explicit inverse).
//
// Host orchestration (the J loop) lives in bindings.cpp; matrices are
// padded to a multiple of 64 on the Python side (pad block = identity,
// factor/inverse of the pad is exact) so every kernel sees full blocks.
//
// The PD check is the factor's breakdown flag (replaces the reference's
// O(m^3) eigSym assert, ProjectedGaussianProcessHelper.scala:62-65); the
// escalating-jitter retry ladder stays on the host (ppa.py).

#include <hip/hip_runtime.h>
#include <math.h>

#include "launchers.h"

typedef __attribute__((ext_vector_type(4))) double f64x4;

#define DB 64          // diagonal / tile block edge
#define DSTR 66        // LDS row stride (doubles) for the factor kernel
#define GBK 32         // GEMM K-tile
#define GSTR 34        // LDS row stride (doubles) for GEMM tiles:
                       // fragment reads hit banks 4*i + 2*k (mod 64) --
                       // all distinct within each 32-lane read group

__device__ inline void tri_decode64(int f, int& a, int& b) {
  a = (int)((sqrtf(8.f * (float)f + 1.f) - 1.f) * 0.5f);
  while ((a + 1) * (a + 2) / 2 <= f) ++a;
  while (a * (a + 1) / 2 > f) --a;
  b = f - a * (a + 1) / 2;
}

// ---------------------------------------------------------------------------
// Diagonal block: factor L_JJ (in place in A) + emit V = L_JJ^{-1}
// ---------------------------------------------------------------------------
// One 256-thread workgroup.  The 64x64 block factors as 8 sequential 8x8
// sub-panels: wave 0 runs the 8x8 factor + forward-substitution inverse
// entirely in registers with __shfl row-per-lane (the round-1 fp32 pattern
// from linalg_lds.h, here in fp64); all 256 threads then apply the
// intra-block panel solve and trailing update.  The 64x64 inverse is
// assembled from the 8x8 inverses right-to-left.

extern "C" __global__ void __launch_bounds__(256)
dpotrf_diag_kernel(double* __restrict__ A, const long m, const int jb,
                   double* __restrict__ Vout,   // [64, 64] this block
                   int* __restrict__ bad) {
  __shared__ double Ab[DB * DSTR];      // the block: L in the lower triangle
  __shared__ double Vb[DB * DSTR];      // assembled inverse
  __shared__ double Vq[8 * 64];         // 8x8 sub-block inverses
  __shared__ double TS[448];            // assembly scratch
  __shared__ int sbad;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  if (tid == 0) sbad = 0;

  for (int f = tid; f < DB * DB; f += 256) {
    const int i = f >> 6, c = f & 63;
    Ab[i * DSTR + c] = (c <= i) ? A[(size_t)(jb + i) * m + jb + c] : 0.0;
  }
  __syncthreads();

  for (int q = 0; q < 8; ++q) {
    const int qb = q * 8;
    if (tid < 64) {
      // 8x8 factor, row j per lane; lanes 8..63 compute duplicates and
      // are masked off every store (uniform __shfl traffic).
      const int j = lane & 7;
      double row[8];
#pragma unroll
      for (int c = 0; c < 8; ++c)
        row[c] = (c <= j) ? Ab[(size_t)(qb + j) * DSTR + qb + c]
                          : (c == j ? 1.0 : 0.0);
      bool ok = true;
      double myrs = 1.0;
#pragma unroll
      for (int ss = 0; ss < 8; ++ss) {
        double l[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) l[c] = __shfl(row[ss], c, 64);
        const double piv = l[ss];
        ok = ok && isfinite(piv) && (piv > 0.0);
        const double rs = ok ? 1.0 / sqrt(piv) : 1.0;
        if (j == ss) myrs = rs;
        const double w = (j > ss) ? rs * row[ss] : 0.0;
#pragma unroll
        for (int c = ss + 1; c < 8; ++c) row[c] -= (rs * l[c]) * w;
      }
      // deferred column scaling: L[j][c] = row[c] * rs_c
#pragma unroll
      for (int c = 0; c < 8; ++c) row[c] *= __shfl(myrs, c, 64);
      if (lane < 8) {
#pragma unroll
        for (int c = 0; c < 8; ++c)
          if (c <= j) Ab[(size_t)(qb + j) * DSTR + qb + c] = row[c];
      }
      // trtri8: column j of the 8x8 inverse by forward substitution
      double v[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] = (i == j) ? myrs : 0.0;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        double rowi[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) rowi[c] = __shfl(row[c], i, 64);
        if (j < i) {
          double sacc = 0.0;
#pragma unroll
          for (int c = 0; c < 8; ++c)
            if (c >= j && c < i) sacc += rowi[c] * v[c];
          v[i] = -sacc / rowi[i];
        }
      }
      if (lane < 8) {
#pragma unroll
        for (int i = 0; i < 8; ++i) Vq[q * 64 + i * 8 + j] = v[i];
      }
      if (lane == 0 && !ok && sbad == 0) sbad = 1;
    }
    __syncthreads();
    if (sbad) break;

    const int p0 = qb + 8;
    const int pr = DB - p0;
    if (pr > 0) {
      // intra-block panel: P = A[p0.., qb..qb+8] * vq^T
      for (int f = tid; f < pr * 8; f += 256) {
        const int r = f >> 3, c = f & 7;
        double sacc = 0.0;
        const double* ar = Ab + (size_t)(p0 + r) * DSTR + qb;
        const double* vr = Vq + q * 64 + c * 8;
#pragma unroll
        for (int t = 0; t < 8; ++t)
          if (t <= c) sacc += ar[t] * vr[t];
        Vb[(size_t)r * 8 + c] = sacc;   // staging (Vb unused until assembly)
      }
      __syncthreads();
      for (int f = tid; f < pr * 8; f += 256) {
        const int r = f >> 3, c = f & 7;
        Ab[(size_t)(p0 + r) * DSTR + qb + c] = Vb[(size_t)r * 8 + c];
      }
      __syncthreads();
      // trailing: lower incl. diag of the remaining rows
      const int ntri = pr * (pr + 1) / 2;
      for (int f = tid; f < ntri; f += 256) {
        int a, b;
        tri_decode64(f, a, b);
        const double* pa = Ab + (size_t)(p0 + a) * DSTR + qb;
        const double* pb = Ab + (size_t)(p0 + b) * DSTR + qb;
        double sacc = 0.0;
#pragma unroll
        for (int t = 0; t < 8; ++t) sacc += pa[t] * pb[t];
        Ab[(size_t)(p0 + a) * DSTR + p0 + b] -= sacc;
      }
      __syncthreads();
    }
  }

  if (sbad) {
    if (tid == 0 && *bad == 0) *bad = 1;
    return;
  }

  // ---- assemble V = L^{-1} (64x64 lower) into Vb ------------------------
  for (int f = tid; f < DB * DB; f += 256) {
    const int i = f >> 6, c = f & 63;
    Vb[(size_t)i * DSTR + c] = (c <= i) ? Ab[(size_t)i * DSTR + c] : 0.0;
  }
  __syncthreads();
  for (int Jq = 7; Jq >= 0; --Jq) {
    const int jb8 = Jq * 8;
    const int nblks = 7 - Jq;
    for (int f = tid; f < nblks * 64; f += 256) {
      const int blk = f >> 6;
      const int ib = (Jq + 1 + blk) * 8;
      const int i = (f >> 3) & 7, j = f & 7;
      const int gi = ib + i;
      // U = sum_{c=jb8+8}^{gi} V[gi][c] * L[c][jb8+j]
      double u = 0.0;
      for (int c = jb8 + 8; c <= gi; ++c)
        u += Vb[(size_t)gi * DSTR + c] * Vb[(size_t)c * DSTR + jb8 + j];
      TS[f] = u;
    }
    __syncthreads();
    for (int f = tid; f < nblks * 64; f += 256) {
      const int blk = f >> 6;
      const int ib = (Jq + 1 + blk) * 8;
      const int i = (f >> 3) & 7, j = f & 7;
      const int gi = ib + i;
      double sacc = 0.0;
      const double* ts = TS + blk * 64 + i * 8;
      const double* vv = Vq + Jq * 64;
#pragma unroll
      for (int t = 0; t < 8; ++t) sacc += ts[t] * vv[t * 8 + j];
      Vb[(size_t)gi * DSTR + jb8 + j] = -sacc;
    }
    for (int f = tid; f < 64; f += 256) {
      const int i = (f >> 3) & 7, j = f & 7;
      if (j <= i)
        Vb[(size_t)(jb8 + i) * DSTR + jb8 + j] = Vq[Jq * 64 + f];
    }
    __syncthreads();
  }

  // write back: L into A (lower; strict upper left untouched), V to Vout
  for (int f = tid; f < DB * DB; f += 256) {
    const int i = f >> 6, c = f & 63;
    if (c <= i) A[(size_t)(jb + i) * m + jb + c] = Ab[(size_t)i * DSTR + c];
    Vout[(size_t)i * DB + c] = (c <= i) ? Vb[(size_t)i * DSTR + c] : 0.0;
  }
}

// ---------------------------------------------------------------------------
// fp64 MFMA GEMM: C (M x N) {=, -=} op(A) (M x K) @ op(B) (K x N)
// ---------------------------------------------------------------------------
// 256 threads = 4 waves in a 2x2 grid; 64x64 output tile per block; each
// wave computes a 32x32 sub-tile as 2x2 v_mfma_f64_16x16x4_f64 tiles (4
// independent accumulators cover the 64-cycle dependent latency).  A
// staged [i][k], B staged [j][k] in LDS (stride GSTR keeps the fragment
// read banks distinct); fragment map: A lane l -> A[i=l&15][k=l>>4],
// B lane l -> B[k=l>>4][j=l&15], D lane l reg r -> D[(l>>4)*4+r][l&15].
// SYRK mode: A==B, only lower-triangle tiles scheduled (1D grid +
// tri_decode), epilogue masked to gi >= gj.

template <bool TA, bool TB, bool SUB, bool SYRK>
__global__ void __launch_bounds__(256)
dgemm64_kernel(const double* __restrict__ A, const double* __restrict__ B,
               double* __restrict__ C, const int M, const int N, const int K,
               const long lda, const long ldb, const long ldc) {
  int ti, tj;
  if (SYRK) {
    tri_decode64(blockIdx.x, ti, tj);          // ti >= tj
  } else {
    ti = blockIdx.x;
    tj = blockIdx.y;
  }
  const int i0 = ti * DB, j0 = tj * DB;

  __shared__ double As[DB * GSTR];
  __shared__ double Bs[DB * GSTR];
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int wr = (wave >> 1) * 32, wc = (wave & 1) * 32;
  const int l16 = lane & 15, kg = lane >> 4;

  f64x4 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = {0.0, 0.0, 0.0, 0.0};

  for (int k0 = 0; k0 < K; k0 += GBK) {
    const int kl = min(GBK, K - k0);
    if (!TA) {
      // A[i][k] row-major: coalesce along k
      for (int f = tid; f < DB * GBK; f += 256) {
        const int i = f >> 5, k = f & 31;
        const int gi = i0 + i;
        As[i * GSTR + k] = (gi < M && k < kl)
                               ? A[(size_t)gi * lda + k0 + k] : 0.0;
      }
    } else {
      // op(A)[i][k] = A[k][i]: coalesce along i
      for (int f = tid; f < DB * GBK; f += 256) {
        const int i = f & 63, k = f >> 6;
        const int gi = i0 + i;
        As[i * GSTR + k] = (gi < M && k < kl)
                               ? A[(size_t)(k0 + k) * lda + gi] : 0.0;
      }
    }
    if (!TB) {
      // op(B)[k][j] = B[k][j]: coalesce along j
      for (int f = tid; f < DB * GBK; f += 256) {
        const int j = f & 63, k = f >> 6;
        const int gj = j0 + j;
        Bs[j * GSTR + k] = (gj < N && k < kl)
                               ? B[(size_t)(k0 + k) * ldb + gj] : 0.0;
      }
    } else {
      // op(B)[k][j] = B[j][k]: coalesce along k
      for (int f = tid; f < DB * GBK; f += 256) {
        const int j = f >> 5, k = f & 31;
        const int gj = j0 + j;
        Bs[j * GSTR + k] = (gj < N && k < kl)
                               ? B[(size_t)gj * ldb + k0 + k] : 0.0;
      }
    }
    __syncthreads();
#pragma unroll
    for (int kc = 0; kc < GBK / 4; ++kc) {
      const int fk = kg + kc * 4;
      const double a0 = As[(wr + l16) * GSTR + fk];
      const double a1 = As[(wr + 16 + l16) * GSTR + fk];
      const double b0 = Bs[(wc + l16) * GSTR + fk];
      const double b1 = Bs[(wc + 16 + l16) * GSTR + fk];
      acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0],
                                                       0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1],
                                                       0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0],
                                                       0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1],
                                                       0, 0, 0);
    }
    __syncthreads();
  }

#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        // D map measured on gfx950 (scripts/mfma_f64_probe.hip +
        // gpurun_out/mfma_probe.txt): D[row][col] at lane l reg r has
        // col = l&15, row = (l>>4) + 4*r  (r strides by 4 — NOT the
        // (l>>4)*4 + r grouping of the f32 16x16 shapes).
        const int gi = i0 + wr + a * 16 + kg + 4 * r;
        const int gj = j0 + wc + b * 16 + l16;
        if (gi < M && gj < N && (!SYRK || gi >= gj)) {
          double* p = &C[(size_t)gi * ldc + gj];
          if (SUB) *p -= acc[a][b][r];
          else *p = acc[a][b][r];
        }
      }
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------

extern "C" hipError_t launch_dpotrf_diag(double* A, long m, int jb,
                                         double* Vout, int* bad,
                                         hipStream_t stream) {
  hipLaunchKernelGGL(dpotrf_diag_kernel, dim3(1), dim3(256), 0, stream,
                     A, m, jb, Vout, bad);
  return hipGetLastError();
}

extern "C" hipError_t launch_dgemm64(int ta, int tb, int sub, int syrk,
                                     const double* A, const double* B,
                                     double* C, int M, int N, int K,
                                     long lda, long ldb, long ldc,
                                     hipStream_t stream) {
  const int nti = (M + DB - 1) / DB, ntj = (N + DB - 1) / DB;
  dim3 grid, blk(256);
  if (syrk) {
    grid = dim3(nti * (nti + 1) / 2);
  } else {
    grid = dim3(nti, ntj);
  }
#define DG_CASE(TA_, TB_, SUB_, SYRK_)                                     \
  hipLaunchKernelGGL((dgemm64_kernel<TA_, TB_, SUB_, SYRK_>), grid, blk,   \
                     0, stream, A, B, C, M, N, K, lda, ldb, ldc)
  const int code = (ta ? 8 : 0) | (tb ? 4 : 0) | (sub ? 2 : 0) | (syrk ? 1 : 0);
  switch (code) {
    case 0:  DG_CASE(false, false, false, false); break;   // NN store
    case 2:  DG_CASE(false, false, true, false); break;    // NN sub
    case 4:  DG_CASE(false, true, false, false); break;    // NT store (trsm)
    case 6:  DG_CASE(false, true, true, false); break;     // NT sub
    case 7:  DG_CASE(false, true, true, true); break;      // NT sub syrk
    case 8:  DG_CASE(true, false, false, false); break;    // TN store
    case 10: DG_CASE(true, false, true, false); break;     // TN sub
    case 12: DG_CASE(true, true, false, false); break;     // TT store (tests)
    default: return hipErrorInvalidValue;
  }
#undef DG_CASE
  return hipGetLastError();
}

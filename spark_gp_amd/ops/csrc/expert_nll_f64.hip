// Fused per-expert BCM negative-log-marginal-likelihood + gradient kernel in
// full fp64 for MI355X (gfx950, CDNA4): the five outputs of expert_nll.hip
// (nll, sumW0, trG, contr, bad) with every stored value and every product in
// double, the O(k^3) and O(k^2 d) products on v_mfma_f64_16x16x4_f64.
//
// One workgroup (512 threads = 8 waves) per expert, k <= 128, d <= 128.  The
// matrix is padded to kp = k up to whole 16-row tiles; the padding carries an
// identity (log 1 in the determinant, zeros in every product that is read),
// so no phase has a ragged tile and no fragment load sits under a bound.
//
// The resource picture is the reverse of the fp32 kernel's.  The kp x kp
// fp64 matrix takes most of the 160 KiB of LDS (102 KB at k = 100, 133 KB at
// k = 128): one workgroup per CU above k = 80, so a wave may use 256
// registers and LDS has no room for a second copy of anything.  What the fp32
// kernel round-trips through LDS therefore lives in registers (207 VGPRs, no
// scratch; that also keeps it at one workgroup per CU below k = 80, where
// LDS would hold two: bounded to 128 registers the chain spills 252 B):
//
//   B  Gram tiles x'.a' of the lower triangle, tile t = wave + 8 u of the
//      row-major triangle in accumulator u of its wave (at most 5: 40
//      registers).  x' = x o s is staged 16 feature columns at a time in T
//      ([kp][NLF_XS], zero past d, so d = 3 needs no tail code).  The epilogue
//      turns a tile IN ITS REGISTERS into K = amp Kb(q) + noise I with
//      q = n_a + n_b - 2 g clamped at 0 (0 exactly on the diagonal), and
//      writes only the cache into the strict upper triangle of A: Kb for
//      RBF, t = sqrt(q) for the Matern families.
//   C  right-looking Cholesky by 16-column blocks with the trailing matrix in
//      those registers: per block J the owners store column J's tiles; wave
//      0 factors the 16 x 16 diagonal block and inverts it (below); the panel
//      is the product L_IJ = A_IJ V_JJ^T, a tile per wave, in place; and every
//      owner of a tile (I, K), K > J, subtracts L_IJ L_KJ^T from its
//      accumulator.  A tile is written to LDS once, when its column is due.
//      V_JJ = L_JJ^-1 replaces the diagonal block (L_JJ has no reader left).
//   D  V_IJ = -V_II sum_{J<=K<I} L_IK V_KJ, rows top to bottom, all columns of
//      a row at once (a tile per wave, the sum parked in the tile in between)
//   E  alpha = V^T (V y); nll = 1/2 y.alpha + 1/2 logdet
//   L  K^-1 = V^T V, lower triangle: tile (ti, tj) summed from row 16 ti on,
//      all tiles of a wave in registers across the barrier that ends the
//      reads of V, then stored
//   W  W0 = (alpha alpha^T - K^-1) o Kd, both triangles, 0 on the padding;
//      trG and sumW0 = sum (alpha alpha^T - K^-1) o Kb
//   H  contr'_j = 2 sum_a x'_aj (x'_aj r_a - (W0 X')_aj), r the row sums of
//      W0: x' staged 16 columns at a time in T again, wave w owns row tile w
//      of W0 X', folds it against x' and r and leaves one partial per (row
//      tile, column); thread j sums them in row-tile order.  De-scaled by
//      s_j^2 at output.
//
// The serial chain: wave 0 holds the diagonal block a row per lane (16
// doubles), forms L left-looking with v_readlane broadcasts from static
// lanes (120 per block), takes ONE reciprocal square root per pivot
// (v_rsq_f64 refined by three Newton steps; L_jj = p rs, no divide and no
// square root), then V = L^-1 a column per lane by forward substitution with
// the same broadcasts.  A pivot that is <= 0 or not finite sets bad (1:
// indefinite, 2: not finite); the chain goes on with a pivot of 1 to the
// barrier every path ends in, and the workgroup leaves there with zeroed
// outputs.  log|K| = sum log p, in pivot order, in wave 0's registers.
//
// LDS: A has row stride SA = kp + 2 doubles.  Stride rule: SA = 2 (mod 4).
// The fragment read A[16 t + (l & 15)][c + (l >> 4)] of a 32-lane group is 16
// consecutive rows by 2 columns of 8 bytes: row i starts at dword 2 i SA =
// 4 i u (u odd) modulo 64 and takes 2 dwords per column, so the group covers
// the 64 banks once.  T has stride NLF_XS = 18 for the same reason.  The
// transposed read A[c + (l >> 4)][16 t + (l & 15)] is 16 contiguous doubles
// per row and 2-way conflicted at worst.
//
// Every reduction runs in a fixed order and there are no atomics: the outputs
// are the same bits on every run.  X arrives as float or double (TX) and is
// widened at the load; y, the scale vector, amp and noise are doubles.
// The plan is nllf64_lds_bytes (kernel_geom.h), which the gate shares.

#include <hip/hip_runtime.h>
#include <math.h>

#define WG 512
#include "linalg_lds.h"
#include "kernel_geom.h"
#include "launchers.h"

typedef __attribute__((ext_vector_type(4))) double f64x4;

#define NLF_MAXT 5   // ceil(36 lower tiles / 8 waves)
static_assert(NLF_K_MAX == 128 && NLF_TB == 16 && WG == 512,
              "8 x 8 tiles over 8 waves");

struct F64Lds {
  double* red;    // 8 (per-wave partials) + 2 spare
  double* A;      // kp x SA: upper cache; lower K columns -> L/V -> K^-1 -> W0
  double* T;      // kp x NLF_XS: a 16-column slab of x'
  double* Hp;     // 8 x 16: phase H's per-(row tile, column) partials
  double* hs;     // d: the gradient contraction per column
  double* yb;     // kp each
  double* alpha;
  double* tvec;
  double* rrow;
  double* nrm;
  double* sc;     // d: scale
  int* bad;
};

// Region sizes: nllf64_lds_bytes (kernel_geom.h) lists them in this order.
__device__ inline F64Lds f64_carve(char* base, int k, int d) {
  const size_t kp = nllf64_kp(k);
  F64Lds L;
  char* p = base;
  L.red = (double*)p;   p += a16(sizeof(double) * 10);
  L.A = (double*)p;     p += a16(sizeof(double) * kp * nllf64_sa(k));
  L.T = (double*)p;     p += a16(sizeof(double) * kp * NLF_XS);
  L.Hp = (double*)p;    p += a16(sizeof(double) * (NLF_K_MAX / NLF_TB) * NLF_XC);
  L.hs = (double*)p;    p += a16(sizeof(double) * d);
  L.yb = (double*)p;    p += a16(sizeof(double) * kp);
  L.alpha = (double*)p; p += a16(sizeof(double) * kp);
  L.tvec = (double*)p;  p += a16(sizeof(double) * kp);
  L.rrow = (double*)p;  p += a16(sizeof(double) * kp);
  L.nrm = (double*)p;   p += a16(sizeof(double) * kp);
  L.sc = (double*)p;    p += a16(sizeof(double) * d);
  L.bad = (int*)p;
  return L;
}

__device__ __forceinline__ f64x4 mma64(const double a, const double b,
                                       const f64x4 c) {
  return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}

// lane `src`'s x in every lane; the wave must be converged
__device__ __forceinline__ double bcast_d(const double x, const int src) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(x), src);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(x), src);
  return __hiloint2double(hi, lo);
}

// 1 / sqrt(p), p > 0 finite: the hardware estimate and three Newton steps
// y += y/2 (1 - p y^2), the residual by fma.  Exact where the result is
// representable (p = 1 gives 1).
__device__ __forceinline__ double rsqrt_newton(const double p) {
  double y = __builtin_amdgcn_rsq(p);
#pragma unroll
  for (int it = 0; it < 3; ++it) {
    const double e = __builtin_fma(-(p * y), y, 1.0);
    y = __builtin_fma(0.5 * y, e, y);
  }
  return y;
}

// Kb and Kd = -dKb/dq from the cache value c: Kb itself (RBF) or t = sqrt(q)
template <int FAM>
__device__ __forceinline__ void kb_kd_of_cache(const double c, double& kb,
                                               double& kd) {
  if (FAM == GEOM_FAM_RBF) {
    kb = c;
    kd = c;
  } else {
    const double e = exp(-c);
    if (FAM == GEOM_FAM_M32) {
      kb = (1.0 + c) * e;
      kd = 0.5 * e;
    } else {
      kb = (1.0 + c + c * c * (1.0 / 3.0)) * e;
      kd = (1.0 + c) * e * (1.0 / 6.0);
    }
  }
}

// T[i][c] = x'[i][c0 + c] for i < kp, c < 16; 0 past k rows or d columns.
// 16 lanes per row: whole 64-B (float) or 128-B (double) segments.
template <typename TX>
__device__ __forceinline__ void stage_x(double* T, const TX* __restrict__ Xe,
                                        const double* sc, const int k,
                                        const int d, const int kp,
                                        const int c0, const int tid) {
  const int c = tid & (NLF_XC - 1), col = c0 + c;
  const double s = col < d ? sc[col] : 0.0;
  for (int i = tid / NLF_XC; i < kp; i += WG / NLF_XC)
    T[i * NLF_XS + c] =
        (i < k && col < d) ? (double)Xe[(size_t)i * d + col] * s : 0.0;
}

// The serial chain of one 16 x 16 diagonal block at D (row stride SA), run by
// ONE converged wave: the lower triangle L L^T = D is replaced by V = L^-1.
// Lanes l and l + 16 k do the same work; the first 16 store.  logdet gains
// sum log(pivot); *flag gets 1 or 2 at the first failed pivot.
__device__ __forceinline__ void chol_invert_16(double* D, const int SA,
                                               const int lane, double& logdet,
                                               int& flag) {
  const int row = lane & 15;
  double a[16];
#pragma unroll
  for (int c = 0; c < 16; ++c) {
    const double v = D[row * SA + c];        // c > row: the cache, dropped
    a[c] = c <= row ? v : 0.0;
  }
  double myrs = 0.0;                         // lane j: 1 / L_jj
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    double s = a[j];
#pragma unroll
    for (int c = 0; c < j; ++c)
      s = __builtin_fma(-a[c], bcast_d(a[c], j), s);   // L_ic L_jc
    double p = bcast_d(s, j);
    if (!(p > 0.0 && p < INFINITY)) {        // uniform: p is
      if (flag == 0) flag = (p != p || p == INFINITY || p == -INFINITY) ? 2 : 1;
      p = 1.0;
    }
    const double rs = rsqrt_newton(p);
    logdet += log(p);
    if (row == j) myrs = rs;
    a[j] = row >= j ? s * rs : 0.0;          // lane j: p rs = sqrt(p)
  }
  double v[16];                              // column `row` of V
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    double s = i == row ? 1.0 : 0.0;
#pragma unroll
    for (int c = 0; c < i; ++c)
      s = __builtin_fma(-bcast_d(a[c], i), v[c], s);   // L_ic V_c,row
    v[i] = s * bcast_d(myrs, i);
  }
  if (lane < 16) {
#pragma unroll
    for (int i = 0; i < 16; ++i)
      if (i >= row) D[i * SA + row] = v[i];
  }
}

template <int FAM, typename TX>
__global__ void __launch_bounds__(WG)
fused_expert_nll_f64_kernel(const TX* __restrict__ Xg,
                            const double* __restrict__ yg,
                            const double* __restrict__ scale,   // [d]
                            const double amp, const double noise,
                            const int k, const int d,
                            double* __restrict__ out_nll,       // [E]
                            double* __restrict__ out_sumW0,     // [E]
                            double* __restrict__ out_trG,       // [E]
                            double* __restrict__ out_contr,     // [E, d]
                            int* __restrict__ out_bad) {        // [E]
  extern __shared__ char lds_raw[];
  const int kp = nllf64_kp(k), SA = nllf64_sa(k), nb = kp / NLF_TB;
  const F64Lds S = f64_carve(lds_raw, k, d);
  double* const A = S.A;
  const int e = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l16 = lane & 15, kg = lane >> 4;
  const TX* Xe = Xg + (size_t)e * k * d;
  const double* ye = yg + (size_t)e * k;

  // tile u of this wave: tile wave + 8 u of the row-major lower triangle
  const int ntri = nb * (nb + 1) / 2;
  int ti[NLF_MAXT], tj[NLF_MAXT];
  bool own[NLF_MAXT];
#pragma unroll
  for (int u = 0; u < NLF_MAXT; ++u) {
    const int t = wave + u * (WG / 64);
    own[u] = t < ntri;
    tri_decode(own[u] ? t : 0, ti[u], tj[u]);
  }

  // ---- A: y, scale ----------------------------------------------------
  for (int j = tid; j < d; j += WG) {
    S.sc[j] = scale[j];
    S.hs[j] = 0.0;
  }
  for (int i = tid; i < kp; i += WG) S.yb[i] = i < k ? ye[i] : 0.0;
  if (tid == 0) *S.bad = 0;
  __syncthreads();

  // ---- B: K tiles in registers, the cache in the strict upper triangle --
  f64x4 kt[NLF_MAXT];
#pragma unroll
  for (int u = 0; u < NLF_MAXT; ++u) kt[u] = {0.0, 0.0, 0.0, 0.0};
  {
    double nrm = 0.0;                        // row tid's ||x'||^2
    for (int c0 = 0; c0 < d; c0 += NLF_XC) {
      if (c0) __syncthreads();               // reads of the last slab done
      stage_x(S.T, Xe, S.sc, k, d, kp, c0, tid);
      __syncthreads();
      if (tid < kp) {
#pragma unroll
        for (int c = 0; c < NLF_XC; ++c) {
          const double v = S.T[tid * NLF_XS + c];
          nrm = __builtin_fma(v, v, nrm);
        }
      }
#pragma unroll
      for (int u = 0; u < NLF_MAXT; ++u) {
        if (!own[u]) continue;
        const double* xa = S.T + (ti[u] * 16 + l16) * NLF_XS + kg;
        const double* xb = S.T + (tj[u] * 16 + l16) * NLF_XS + kg;
#pragma unroll
        for (int s = 0; s < 4; ++s)
          kt[u] = mma64(xa[4 * s], xb[4 * s], kt[u]);
      }
    }
    if (tid < kp) S.nrm[tid] = nrm;
    __syncthreads();
    // D map of the f64 MFMA: row = (lane >> 4) + 4 r, column = lane & 15
#pragma unroll
    for (int u = 0; u < NLF_MAXT; ++u) {
      if (!own[u]) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int gi = ti[u] * 16 + kg + 4 * r, gj = tj[u] * 16 + l16;
        double kv;
        if (gi >= k || gj >= k) {
          kv = gi == gj ? 1.0 : 0.0;         // padding: identity
        } else {
          const double q =
              gi == gj ? 0.0 : S.nrm[gi] + S.nrm[gj] - 2.0 * kt[u][r];
          const double qc = q < 0.0 ? 0.0 : q;   // a NaN stays one
          double c, kb, kd;
          if (FAM == GEOM_FAM_RBF) c = exp(-qc); else c = sqrt(qc);
          kb_kd_of_cache<FAM>(c, kb, kd);
          kv = amp * kb + (gi == gj ? noise : 0.0);
          if (gi > gj) A[gj * SA + gi] = c;
        }
        kt[u][r] = kv;
      }
    }
  }

  // ---- C: right-looking Cholesky, trailing tiles in registers ----------
  double logdet = 0.0;                       // wave 0's
  for (int J = 0; J < nb; ++J) {
    // column J leaves the registers (the diagonal tile: lower half only)
#pragma unroll
    for (int u = 0; u < NLF_MAXT; ++u) {
      if (!own[u] || tj[u] != J) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int gi = ti[u] * 16 + kg + 4 * r, gj = J * 16 + l16;
        if (gj <= gi) A[gi * SA + gj] = kt[u][r];
      }
    }
    __syncthreads();
    if (wave == 0) {
      int flag = 0;
      chol_invert_16(A + (J * 16) * SA + J * 16, SA, lane, logdet, flag);
      if (flag && lane == 0) *S.bad = flag;
    }
    __syncthreads();
    if (*S.bad) break;
    // panel: L_IJ = A_IJ V_JJ^T, row tile J + 1 + wave
    {
      const int I = J + 1 + wave;
      if (I < nb) {
        const double* pa = A + (I * 16 + l16) * SA + J * 16 + kg;
        const double* pb = A + (J * 16 + l16) * SA + J * 16 + kg;
        f64x4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const double b = pb[4 * s];        // V_JJ[j][c], c <= j
          acc = mma64(pa[4 * s], 4 * s + kg <= l16 ? b : 0.0, acc);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r)
          A[(I * 16 + kg + 4 * r) * SA + J * 16 + l16] = acc[r];
      }
    }
    __syncthreads();
    // trailing update of the tiles still in registers
#pragma unroll
    for (int u = 0; u < NLF_MAXT; ++u) {
      if (!own[u] || tj[u] <= J) continue;
      const double* pa = A + (ti[u] * 16 + l16) * SA + J * 16 + kg;
      const double* pb = A + (tj[u] * 16 + l16) * SA + J * 16 + kg;
#pragma unroll
      for (int s = 0; s < 4; ++s) kt[u] = mma64(-pa[4 * s], pb[4 * s], kt[u]);
    }
    // column J + 1 is stored next: nobody reads those tiles in this step
  }
  if (*S.bad) {
    if (tid == 0) {
      out_bad[e] = *S.bad;
      out_nll[e] = 0.0; out_sumW0[e] = 0.0; out_trG[e] = 0.0;
    }
    for (int j = tid; j < d; j += WG) out_contr[(size_t)e * d + j] = 0.0;
    return;
  }

  // ---- D: V_IJ = -V_II sum_{J<=K<I} L_IK V_KJ, wave J of row I ---------
  for (int I = 1; I < nb; ++I) {
    const int J = wave;
    const bool on = J < I;
    f64x4 acc = {0.0, 0.0, 0.0, 0.0};
    if (on) {
      for (int K = J; K < I; ++K) {
        const double* pa = A + (I * 16 + l16) * SA + K * 16 + kg;
        const double* pb = A + (K * 16 + kg) * SA + J * 16 + l16;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const double b = pb[4 * s * SA];   // V_KJ[c][j]; K == J: c >= j
          acc = mma64(pa[4 * s], (K == J && 4 * s + kg < l16) ? 0.0 : b, acc);
        }
      }
    }
    __syncthreads();                         // row I's L blocks are read
    if (on) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        A[(I * 16 + kg + 4 * r) * SA + J * 16 + l16] = acc[r];
    }
    __syncthreads();
    if (on) {
      const double* pa = A + (I * 16 + l16) * SA + I * 16 + kg;
      const double* pb = A + (I * 16 + kg) * SA + J * 16 + l16;
      acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const double a = pa[4 * s];          // V_II[i][c], c <= i
        acc = mma64(4 * s + kg <= l16 ? a : 0.0, pb[4 * s * SA], acc);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r)
        A[(I * 16 + kg + 4 * r) * SA + J * 16 + l16] = -acc[r];
    }
    __syncthreads();
  }

  // ---- E: alpha = V^T (V y), y.alpha -----------------------------------
  if (tid < kp) {
    double s = 0.0;
    for (int c = 0; c <= tid; ++c)
      s = __builtin_fma(A[tid * SA + c], S.yb[c], s);
    S.tvec[tid] = s;
  }
  __syncthreads();
  if (tid < kp) {
    double s = 0.0;
    for (int c = tid; c < kp; ++c)
      s = __builtin_fma(A[c * SA + tid], S.tvec[c], s);
    S.alpha[tid] = s;
  }
  __syncthreads();
  const double yta =
      block_sum(tid < kp ? S.yb[tid] * S.alpha[tid] : 0.0, S.red, tid);

  // ---- L: K^-1 = V^T V, lower triangle ---------------------------------
  {
    f64x4 acc[NLF_MAXT];
#pragma unroll
    for (int u = 0; u < NLF_MAXT; ++u) {
      acc[u] = {0.0, 0.0, 0.0, 0.0};
      if (!own[u]) continue;
      const int ga = ti[u] * 16 + l16, gb = tj[u] * 16 + l16;
      // V[c][g] is inside the factor where c >= g; rows before 16 ti add 0
      for (int c0 = ti[u] * 16; c0 < kp; c0 += 4) {
        const int c = c0 + kg;
        const double a = A[c * SA + ga], b = A[c * SA + gb];
        acc[u] = mma64(c >= ga ? a : 0.0, c >= gb ? b : 0.0, acc[u]);
      }
    }
    __syncthreads();                         // all V reads complete
#pragma unroll
    for (int u = 0; u < NLF_MAXT; ++u) {
      if (!own[u]) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int gi = ti[u] * 16 + kg + 4 * r, gj = tj[u] * 16 + l16;
        if (gj <= gi) A[gi * SA + gj] = acc[u][r];
      }
    }
    __syncthreads();
  }

  // ---- W: W0 = (aa^T - K^-1) o Kd, both triangles, 0 on the padding ----
  double trg_part = 0.0, sw_part = 0.0;
  for (int f = tid; f < kp * kp; f += WG) {
    const int a = f / kp, b = f - a * kp;
    if (b > a) continue;
    double w = 0.0;
    if (a < k) {                             // b <= a: off the padding
      const double g = S.alpha[a] * S.alpha[b] - A[a * SA + b];
      const double c =
          a == b ? (FAM == GEOM_FAM_RBF ? 1.0 : 0.0) : A[b * SA + a];
      double kb, kd;
      kb_kd_of_cache<FAM>(c, kb, kd);
      w = g * kd;
      if (a == b) {
        trg_part += g;
        sw_part += g * kb;
      } else {
        sw_part += 2.0 * (g * kb);
      }
    }
    A[a * SA + b] = w;
    if (a != b) A[b * SA + a] = w;
  }
  const double trG = block_sum(trg_part, S.red, tid);     // ends in a barrier
  const double sumW0 = block_sum(sw_part, S.red, tid);

  // ---- G: row sums of W0 (column sums of a symmetric matrix) -----------
  if (tid < kp) {
    double s = 0.0;
    for (int b = 0; b < kp; ++b) s += A[b * SA + tid];
    S.rrow[tid] = s;
  }
  // (the barrier behind the first staging below orders this)

  // ---- H: contr'_j = 2 sum_a x'_aj (x'_aj r_a - (W0 X')_aj) ------------
  for (int j0 = 0; j0 < d; j0 += NLF_XC) {
    stage_x(S.T, Xe, S.sc, k, d, kp, j0, tid);
    __syncthreads();
    if (wave < nb) {
      const double* pa = A + (wave * 16 + l16) * SA + kg;   // W0[i][c]
      const double* pb = S.T + kg * NLF_XS + l16;           // x'[c][j]
      f64x4 acc = {0.0, 0.0, 0.0, 0.0};
      for (int c0 = 0; c0 < kp; c0 += 4)
        acc = mma64(pa[c0], pb[c0 * NLF_XS], acc);
      double p = 0.0;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int gi = wave * 16 + kg + 4 * r;
        const double x = S.T[gi * NLF_XS + l16];   // 0 on the padding
        p = __builtin_fma(2.0 * x, x * S.rrow[gi] - acc[r], p);
      }
      // the 4 row groups sharing a column: lanes l, l+16, l+32, l+48
      p += __shfl_down(p, 32, 64);
      p += __shfl_down(p, 16, 64);
      if (kg == 0) S.Hp[wave * NLF_XC + l16] = p;
    }
    __syncthreads();
    if (tid < NLF_XC && j0 + tid < d) {
      double s = 0.0;
      for (int t = 0; t < nb; ++t) s += S.Hp[t * NLF_XC + tid];
      S.hs[j0 + tid] = s;
    }
    __syncthreads();                         // T and Hp are free again
  }

  // the contraction ran in scaled coordinates: contr' = s_j^2 contr;
  // s_j == 0 => dK/ds_j == 0: emit 0 (the exact limit)
  for (int j = tid; j < d; j += WG) {
    const double s2j = S.sc[j] * S.sc[j];
    out_contr[(size_t)e * d + j] = s2j > 0.0 ? S.hs[j] / s2j : 0.0;
  }
  if (tid == 0) {
    out_bad[e] = 0;
    out_nll[e] = 0.5 * yta + 0.5 * logdet;
    out_sumW0[e] = sumW0;
    out_trG[e] = trG;
  }
}

template <typename TX>
using nlf_kernel_t = void (*)(const TX*, const double*, const double*, double,
                              double, int, int, double*, double*, double*,
                              double*, int*);

template <typename TX>
static nlf_kernel_t<TX> nlf_kernel_of(int family) {
  switch (family) {
    case GEOM_FAM_RBF: return fused_expert_nll_f64_kernel<GEOM_FAM_RBF, TX>;
    case GEOM_FAM_M32: return fused_expert_nll_f64_kernel<GEOM_FAM_M32, TX>;
    case GEOM_FAM_M52: return fused_expert_nll_f64_kernel<GEOM_FAM_M52, TX>;
  }
  return nullptr;
}

template <typename TX>
static hipError_t nlf_launch(const void* X, const double* y,
                             const double* scale, double amp, double noise,
                             int E, int k, int d, double* out_nll,
                             double* out_sumW0, double* out_trG,
                             double* out_contr, int* out_bad, int family,
                             hipStream_t stream) {
  const nlf_kernel_t<TX> kern = nlf_kernel_of<TX>(family);
  if (!kern) return hipErrorInvalidValue;
  if (!nllf64_supported(k, d) || E < 1) return hipErrorInvalidConfiguration;
  hipLaunchKernelGGL(kern, dim3(E), dim3(WG), nllf64_lds_bytes(k, d), stream,
                     (const TX*)X, y, scale, amp, noise, k, d, out_nll,
                     out_sumW0, out_trG, out_contr, out_bad);
  return hipGetLastError();
}

extern "C" hipError_t launch_fused_expert_nll_f64(
    const void* X, int x_is_f64, const double* y, const double* scale,
    double amp, double noise, int E, int k, int d, double* out_nll,
    double* out_sumW0, double* out_trG, double* out_contr, int* out_bad,
    int family, hipStream_t stream) {
  return x_is_f64
             ? nlf_launch<double>(X, y, scale, amp, noise, E, k, d, out_nll,
                                  out_sumW0, out_trG, out_contr, out_bad,
                                  family, stream)
             : nlf_launch<float>(X, y, scale, amp, noise, E, k, d, out_nll,
                                 out_sumW0, out_trG, out_contr, out_bad,
                                 family, stream);
}

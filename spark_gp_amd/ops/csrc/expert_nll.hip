// Fused per-expert BCM negative-log-marginal-likelihood + gradient kernel
// for MI355X (gfx950, CDNA4) — v2: blocked, in-place, single-LDS-buffer.
//
// One workgroup (512 threads = 8 waves) per expert; the whole per-expert
// pipeline that the reference runs as a chain of Breeze/LAPACK calls per
// Spark task (regression/GaussianProcessRegression.scala:55-68, kernel
// build + LU + inverse + alpha + trace products; kernel/ARDRBFKernel.scala:
// 48-79 — K and d derivative matrices) executes in LDS without touching HBM
// between stages, and WITHOUT materializing the [d, k, k] derivative tensor:
//
//   B  lower(A) = amp*Kb + noise*I,  strict upper(A) = Kb (cached base
//      kernel — read back in phase W, never recomputed; the Matern families
//      cache t = sqrt(q) there instead, see below); round 2: the
//      sqdist is q = n_a + n_b - 2 x'.a' over pre-SCALED coordinates on
//      f32 MFMA tiles (the gradient contraction runs in scaled space and
//      is de-scaled by s2 at output)
//   C  blocked right-looking Cholesky, IN PLACE, with look-ahead: the
//      q-loop over the 8-column sub-blocks of each 32-column diagonal
//      block belongs to wave 0 alone, with no workgroup barrier inside:
//      per q it factors AND inverts the 8x8 sub-diagonal in one 8-step
//      elimination (row-per-lane on 8 lanes, cross-lane traffic via
//      v_readlane broadcasts from STATIC lanes; branchless
//      frexp-accumulated log-det), forms the intra-block panel one row per
//      lane and applies the intra-block trailing update, ordered at wave
//      scope (wave_lds_sync); behind the loop it assembles the 32x32
//      inverse from the 8x8 inverses by recursive doubling on f32 MFMA —
//      WHILE waves 1-7 apply the previous panel's rank-32 trailing update
//      in one pass.  One barrier ends this on every path, a failed pivot
//      included.  The panel solve is a dense GEMM against the inverted
//      diagonal.  fp32; fp64 logdet.  (Design history and negative
//      results: profiles/PROFILES.md and TODO.md item 1.)
//   D  blocked in-place triangular inverse of the off-diagonal blocks
//      (right-to-left column blocks, rows fully parallel:
//       V_IJ = -(sum_{K>J} V_IK L_KJ) L_JJ^-1).
//   E  alpha = V^T (V y);  nll = 1/2 y.alpha + 1/2 logdet
//   L  lauum K^-1 = V^T V on f32 MFMA (masked fragments, fetched four
//      steps at a time with no load under a lane condition; tile (ti, tj)
//      summed from row 16 ti on, two tiles of a wave advanced alternately;
//      register tiles across a barrier; strictly lower+diagonal so the Kb
//      cache survives)
//   W  W0 = (alpha alpha^T - K^-1) o Kd, Kd = -dKb/dq (RBF: Kd = Kb, from
//      the upper-triangle cache); trG and sumW0 = sum (alpha alpha^T -
//      K^-1) o Kb accumulated on the fly
//   H  gradient contraction per input dim (the K5 fusion)
//      on f32 MFMA: W0 @ X' as 16x16x4 tiles, folded per fragment into
//      per-column partials; contr de-scaled by s2 at output
//
// Inner products with a contiguous operand are float4 (ds_read_b128)
// vectorized over 16-B-aligned LDS rows (strides padded to multiples of 4
// floats); the rest are multi-accumulator-unrolled scalars.  Single
// k x SA working buffer + one (k-32) x 36 temp; the scaled features have
// no LDS region of their own (B stages them inside the working buffer
// before anything else is written there and holds its tiles in registers
// across the barrier in front of its epilogue; H takes its fragments from
// global X) => 52 KB LDS at k=100, and at most 80 VGPRs at 6 waves/SIMD:
// three experts resident per CU (profiles/PROFILES.md rounds 4 and 5;
// fused_expert_nll_resident_wgs asks the runtime).
//
// Covariance families (kernel_geom.h): the kernel is compiled for exp(-q)
// (RBF / ARD-RBF) and for Matern 3/2 and 5/2 over the same scaled q; only
// the two epilogues of B and the products of W know the family.  With
// G = alpha alpha^T - K^-1 the gradient needs sum(G o Kb) (amplitude) and
// W = G o Kd (everything G and H contract); for RBF the two coincide.  The
// Matern kernels cache t = sqrt(q) in the strict upper triangle, which is
// exact and needs no LDS beyond the RBF plan's, and phase W forms Kb and Kd
// from one exp(-t) per lower-triangle element (the diagonal takes t = 0:
// Kb = 1, Kd = Kd(0), no 1/t anywhere).  Known edge: near-duplicate rows
// make the GEMM-form q noisy at the 1e-6 ||x'||^2 level, and after the square
// root Kd carries about 1e-3 relative error on those pairs only; Kb is
// unaffected to first order.
//
// Numerics: fp32 storage/factorization, fp64 scalar accumulation.  Experts
// whose fp32 Cholesky breaks down are flagged in out_bad and recomputed on
// the torch fallback path by the host.
//
// Constraints: k <= 128, d <= 128, LDS budget checked host-side.

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdlib.h>
#include <type_traits>

#define WG 512
#include "linalg_lds.h"
#include "kernel_geom.h"
#include "launchers.h"

typedef __attribute__((ext_vector_type(4))) float mfma_f32x4;

struct NllLds {
  float* A;     // k * SA (SA = k+1 up-aligned to 4): lower K -> L/V ->
                // K^-1 -> W0; upper: Kb cache
  float* T;     // temp: nll_tsz(k, d)
  float* yb;    // k
  float* alpha; // k
  float* tvec;  // k
  float* rrow;  // k
  float* s2;    // d: scale^2
  float* sc;    // d: scale (x' = x o scale is formed on the fly)
  double* red;  // 8 (per-wave partials)
  double* misc; // 2: logdet, scratch
  int* bad;     // 1
};

// Region sizes: kernel_geom.h (nll_lds_bytes lists them in this order).
__device__ inline NllLds carve(char* base, int k, int d) {
  NllLds L;
  char* p = base;
  L.red = (double*)p;   L.misc = L.red + 8;
  p += a16(sizeof(double) * 10);
  L.A = (float*)p;      p += a16(sizeof(float) * (size_t)k * geom_sa(k));
  L.T = (float*)p;      p += a16(sizeof(float) * nll_tsz(k, d));
  L.yb = (float*)p;     p += a16(sizeof(float) * k);
  L.alpha = (float*)p;  p += a16(sizeof(float) * k);
  L.tvec = (float*)p;   p += a16(sizeof(float) * k);
  L.rrow = (float*)p;   p += a16(sizeof(float) * k);
  L.s2 = (float*)p;     p += a16(sizeof(float) * d);
  L.sc = (float*)p;     p += a16(sizeof(float) * d);
  L.bad = (int*)p;
  return L;
}

// ||x o s||^2 of one global row, in the order dotv(x', x', 0, d) sums it
// (four strided partials, pairwise fold, scalar tail).
__device__ inline float scaled_sqnorm(const float* __restrict__ x,
                                      const float* sc, int d) {
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  int c = 0;
  // spelled out as the compiler has always built it (and as phase B's
  // staged form repeats it): rounded squares added to the partials, a
  // fused accumulate in the tail
  for (; c + 3 < d; c += 4) {
#pragma clang fp contract(off)
    const float v0 = x[c] * sc[c], v1 = x[c + 1] * sc[c + 1];
    const float v2 = x[c + 2] * sc[c + 2], v3 = x[c + 3] * sc[c + 3];
    const float q0 = v0 * v0, q1 = v1 * v1, q2 = v2 * v2, q3 = v3 * v3;
    a0 = a0 + q0; a1 = a1 + q1; a2 = a2 + q2; a3 = a3 + q3;
  }
  float s = (a0 + a1) + (a2 + a3);
  for (; c < d; ++c) {
    const float v = x[c] * sc[c];
    s = __builtin_fmaf(v, v, s);
  }
  return s;
}

// Phase B's epilogue for one element gi >= gj of the lower triangle at the
// scaled squared distance q: K = amp Kb(q) + noise I into the lower half of
// A, and in the mirrored upper element what phase H rebuilds Kb and Kd
// from: Kb itself for the RBF family, t = sqrt(q) for the Matern ones.
template <int FAM>
__device__ __forceinline__ void nll_b_store(float* A, const int SA,
                                            const int gi, const int gj,
                                            const float q, const float amp,
                                            const float noise) {
  if (FAM == GEOM_FAM_RBF) {
    const float kb = __expf(-(q > 0.f ? q : 0.f));
    A[(size_t)gi * SA + gj] = amp * kb + (gi == gj ? noise : 0.f);
    if (gi != gj) A[(size_t)gj * SA + gi] = kb;           // Kb cache upper
  } else {
    A[(size_t)gi * SA + gj] =
        amp * family_kb<FAM>(q) + (gi == gj ? noise : 0.f);
    if (gi != gj)                                         // t cache upper
      A[(size_t)gj * SA + gi] = sqrtf(q > 0.f ? q : 0.f);
  }
}

// MFMA k-steps whose global X fragments are fetched together, so that a
// tile pays one memory latency per XCH*4 contraction indices
#define XCH 4

// NS k-steps of NT (one or two) 16x16 output tiles of phase L on
// v_mfma_f32_16x16x4_f32, the fragments masked LDS reads of V (row stride
// SA).  Step s of tile t contracts the rows c[t] + 4 s + kg (kg = lane >> 4,
// c[t] the same in every lane) of the columns ga[t] (A fragment) and gb[t]
// (B fragment); an element V[cc][g] is inside the mask where cc < k, g < k
// and cc >= g.  All 2 NS NT fragments are fetched before the first MFMA: a
// masked element reads index 0 (always inside the buffer) and is zeroed by
// a select afterwards, so that no load sits under a lane condition (the
// form assemble_diag_inverse uses: a conditional load is issued, and waited
// for, in its own branch right before its MFMA).  The fragment index is a
// scalar that moves with the step plus a vector that does not.  The MFMAs
// run in ascending s; with two tiles they alternate, so that a tile's
// accumulator chain never waits on its own previous MFMA.
template <int NS, int NT>
__device__ __forceinline__ void lauum_feed(mfma_f32x4* acc, const float* V,
                                           const int SA, const int k,
                                           const int kg, const int (&c)[NT],
                                           const int (&ga)[NT],
                                           const int (&gb)[NT]) {
  float av[NT][NS], bv[NT][NS];
  bool oa[NT][NS], ob[NT][NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) {
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int cs = c[t] + 4 * s, cc = cs + kg;
      oa[t][s] = cc < k && ga[t] < k && cc >= ga[t];
      ob[t][s] = cc < k && gb[t] < k && cc >= gb[t];
      av[t][s] = V[oa[t][s] ? cs * SA + (kg * SA + ga[t]) : 0];
      bv[t][s] = V[ob[t][s] ? cs * SA + (kg * SA + gb[t]) : 0];
    }
  }
  // every load is issued before the first select waits for one
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int s = 0; s < NS; ++s) {
#pragma unroll
    for (int t = 0; t < NT; ++t)
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(
          oa[t][s] ? av[t][s] : 0.f, ob[t][s] ? bv[t][s] : 0.f, acc[t],
          0, 0, 0);
  }
}

// The kernel is compiled once per covariance family (kernel_geom.h), one
// front per translation unit: this file by itself gives the RBF front,
// fused_expert_nll_kernel, and the launchers; expert_nll_m32.hip and
// expert_nll_m52.hip define NLL_FAMILY, NLL_KERNEL and NLL_KERNEL_GETTER and
// include this file for the Matern fronts.  (Three instantiations of a
// template body in one file were tried first: the compiler then allocates
// every one of them differently, the RBF front at 80 VGPRs and 240 B of
// scratch where it has 72 and none alone.)
#ifndef NLL_FAMILY
#define NLL_FAMILY GEOM_FAM_RBF
#define NLL_KERNEL fused_expert_nll_kernel
#define NLL_LAUNCHERS
#endif

extern "C" __global__ void __launch_bounds__(WG, 6)
NLL_KERNEL(const float* __restrict__ Xg,
           const float* __restrict__ yg,
           const float* __restrict__ scale,   // [d]
           const float amp, const float noise,
           const int k, const int d,
           double* __restrict__ out_nll,      // [E]
           double* __restrict__ out_sumW0,    // [E]: sum(G o Kb)
           double* __restrict__ out_trG,      // [E]
           double* __restrict__ out_contr,    // [E, d]
           int* __restrict__ out_bad,
           unsigned long long* __restrict__ out_clk) { // [E,20]
           // optional phase profiling (wall_clock64 boundaries)
  constexpr int FAM = NLL_FAMILY;
  extern __shared__ char lds_raw[];
#define PH(n) do { if (out_clk && threadIdx.x == 0) \
    out_clk[(size_t)blockIdx.x * 20 + (n)] = wall_clock64(); } while (0)
  PH(0);
  NllLds S = carve(lds_raw, k, d);
  const int SA = (int)geom_sa(k);
  const int e = blockIdx.x;
  int tid = threadIdx.x;
  int lane = tid & 63;
  const int nblk = (k + NB - 1) / NB;
  const float* Xe = Xg + (size_t)e * k * d;
  const float* ye = yg + (size_t)e * k;

  // ---- A: stage y, scale, s2 ---------------------------------------
  // Scaled coordinates x' = x o s make the kernel build a plain GEMM
  // (q = ||x'||^2 + ||a'||^2 - 2 x'.a') and the gradient contraction
  // runs in scaled space, de-scaled by s2 at output (H phase).  x' is
  // not staged here: phase B stages it inside S.A for its own use, phase
  // H forms its fragments from global X (12.8 KB per expert at k=100,
  // d=32, cache-resident) times S.sc.
  for (int j = tid; j < d; j += WG) {
    float s = scale[j];
    S.sc[j] = s;
    S.s2[j] = s * s;
  }
  for (int i = tid; i < k; i += WG) S.yb[i] = ye[i];
  if (tid == 0) { *S.bad = 0; S.misc[0] = 0.0; }
  __syncthreads();

PH(1);
  // ---- B: lower = amp Kb + noise I; strict upper = Kb cache ---------
  // MFMA form (round 2): q_ab = n_a + n_b - 2 x'_a . x'_b with the dot
  // tiles on v_mfma_f32_16x16x4_f32 (exact fp32) — the elementwise
  // version cost ~3 VALU issues per (pair, dim).  Row norms stage
  // through S.alpha (free until phase E).
  const int bsw = nll_bslab(k, d);
  if (bsw) {
    // Staged form: nothing lives in S.A yet, so its front holds x' in
    // column slabs of bsw (a multiple of 16) columns, row stride bsw + 4,
    // zero-filled past d.  Each wave keeps ALL of its tiles in registers
    // over the slabs (ascending columns: the MFMA order per tile is that
    // of the global form) and across the barrier that ends the last
    // fragment read; only then does the epilogue overwrite the staging
    // area (the register-tiles-across-a-barrier idiom of phase L).
    const int ss = bsw + 4;
    const int nt = (k + 15) / 16;
    const int ntri = nt * (nt + 1) / 2;
    const int wave = tid >> 6;
    const int l16 = lane & 15, kg = lane >> 4;
    constexpr int MAXT = 5;                 // as in phase L
    mfma_f32x4 acc[MAXT];                   // compile-time indexed only
#pragma unroll
    for (int u = 0; u < MAXT; ++u) acc[u] = {0.f, 0.f, 0.f, 0.f};
    // row norm of row tid, in scaled_sqnorm's order; the four partials
    // are carried over the slabs (slab widths are multiples of 4)
    float n0 = 0.f, n1 = 0.f, n2 = 0.f, n3 = 0.f, nrm = 0.f;
    for (int s0 = 0; s0 < d; s0 += bsw) {
      const int sw = d - s0 < bsw ? (d - s0 + 15) & ~15 : bsw;
      if (s0) __syncthreads();              // reads of the last slab done
      // 16 lanes per (row, 16-column group): 64-B global segments
      for (int g = 0; g < sw; g += 16) {
        const int j = g + (tid & 15), c = s0 + j;
        for (int a = tid >> 4; a < k; a += WG / 16)
          S.A[(size_t)a * ss + j] =
              c < d ? Xe[(size_t)a * d + c] * S.sc[c] : 0.f;
      }
      __syncthreads();
      if (s0 == 0) PH(10);
      if (tid < k) {
        const float* xr = S.A + (size_t)tid * ss;
        int c = 0;
        // pinned to what the compiler makes of scaled_sqnorm: rounded
        // squares added to the partials, a fused accumulate in the tail
        for (; c < sw && s0 + c + 3 < d; c += 4) {
#pragma clang fp contract(off)
          const float4 v = *(const float4*)(xr + c);
          const float q0 = v.x * v.x, q1 = v.y * v.y;
          const float q2 = v.z * v.z, q3 = v.w * v.w;
          n0 = n0 + q0; n1 = n1 + q1; n2 = n2 + q2; n3 = n3 + q3;
        }
        if (s0 + sw >= d) {                 // last slab: fold, scalar tail
          nrm = (n0 + n1) + (n2 + n3);
          for (; s0 + c < d; ++c) nrm = __builtin_fmaf(xr[c], xr[c], nrm);
        }
      }
#pragma unroll
      for (int u = 0; u < MAXT; ++u) {
        const int t = wave + u * (WG / 64);
        if (t >= ntri) continue;
        int ti, tj;
        tri_decode(t, ti, tj);
        const int ia = ti * 16 + l16;       // A-fragment row
        const int jb = tj * 16 + l16;       // B-fragment column
        const float* xa = S.A + (size_t)ia * ss + kg;
        const float* xb = S.A + (size_t)jb * ss + kg;
        for (int k0 = 0; k0 < sw; k0 += 4 * XCH) {
          float av[XCH], bv[XCH];
#pragma unroll
          for (int v = 0; v < XCH; ++v) {
            av[v] = ia < k ? xa[k0 + 4 * v] : 0.f;
            bv[v] = jb < k ? xb[k0 + 4 * v] : 0.f;
          }
#pragma unroll
          for (int v = 0; v < XCH; ++v)
            if (s0 + k0 + 4 * v < d)
              acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[v], bv[v],
                                                            acc[u], 0, 0, 0);
        }
      }
    }
    if (tid < k) S.alpha[tid] = nrm;
    __syncthreads();          // fragment reads complete, norms visible
#pragma unroll
    for (int u = 0; u < MAXT; ++u) {
      const int t = wave + u * (WG / 64);
      if (t >= ntri) continue;
      int ti, tj;
      tri_decode(t, ti, tj);
      // D map: row = (lane>>4)*4 + r, col = lane&15
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int gi = ti * 16 + kg * 4 + r;
        const int gj = tj * 16 + l16;
        if (gi >= k || gj >= k || gj > gi) continue;
        const float q = S.alpha[gi] + S.alpha[gj] - 2.0f * acc[u][r];
        nll_b_store<FAM>(S.A, SA, gi, gj, q, amp, noise);
      }
    }
  } else {
    // no slab fits in S.A, or a single load latency is all there is to
    // save (nll_bslab): fragments from global X
    for (int a = tid; a < k; a += WG)
      S.alpha[a] = scaled_sqnorm(Xe + (size_t)a * d, S.sc, d);
    __syncthreads();
    const int nt = (k + 15) / 16;
    const int ntri = nt * (nt + 1) / 2;
    const int wave = tid >> 6;
    const int l16 = lane & 15, kg = lane >> 4;
    for (int t = wave; t < ntri; t += WG / 64) {
      int ti, tj;
      tri_decode(t, ti, tj);
      mfma_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      const int ia = ti * 16 + l16;        // A-fragment row
      const int jb = tj * 16 + l16;        // B-fragment column
      for (int k0 = 0; k0 < d; k0 += 4 * XCH) {
        float av[XCH], bv[XCH];
#pragma unroll
        for (int u = 0; u < XCH; ++u) {
          const int fk = k0 + 4 * u + kg;
          const float s = fk < d ? S.sc[fk] : 0.f;
          av[u] = (ia < k && fk < d) ? Xe[(size_t)ia * d + fk] * s : 0.f;
          bv[u] = (jb < k && fk < d) ? Xe[(size_t)jb * d + fk] * s : 0.f;
        }
#pragma unroll
        for (int u = 0; u < XCH; ++u)
          if (k0 + 4 * u < d)
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u], bv[u], acc,
                                                       0, 0, 0);
      }
      // D map: row = (lane>>4)*4 + r, col = lane&15
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int gi = ti * 16 + kg * 4 + r;
        const int gj = tj * 16 + l16;
        if (gi >= k || gj >= k || gj > gi) continue;
        const float q = S.alpha[gi] + S.alpha[gj] - 2.0f * acc[r];
        nll_b_store<FAM>(S.A, SA, gi, gj, q, amp, noise);
      }
    }
  }
  __syncthreads();

PH(2);
  // ---- C/D: in-place blocked Cholesky + triangular inverse ---------
  // (shared machinery: linalg_lds.h)  A: lower K -> V = L^-1; upper Kb
  // cache untouched; log|K| into misc[0]; bad flag on fp32 breakdown.
  chol_invert_lower(S.A, S.T, k, SA, tid, S.bad, S.misc,
                    out_clk ? out_clk + (size_t)e * 20 + 12 : nullptr);
  if (*S.bad) {
    if (tid == 0) {
      out_bad[e] = *S.bad;     // 1: indefinite, 2: non-finite iterate
      out_nll[e] = 0.0; out_sumW0[e] = 0.0; out_trG[e] = 0.0;
    }
    for (int j = tid; j < d; j += WG) out_contr[(size_t)e * d + j] = 0.0;
    return;
  }
  // log|K| = 2 sum log L_ii = sum log(ajj before sqrt), accumulated in C1
  const double logdet = S.misc[0];
  // as in chol_invert_lower: phases E..H recompute their thread indices
  // instead of keeping phase B's alive across the factorization
  asm volatile("" : "+v"(tid));
  lane = tid & 63;

PH(3);
  PH(4);
    // ---- E: alpha = V^T (V y), y.alpha ------------------------------
  for (int i = tid; i < k; i += WG)
    S.tvec[i] = dotv(S.A + (size_t)i * SA, S.yb, 0, i + 1);
  __syncthreads();
  for (int a = tid; a < k; a += WG)
    S.alpha[a] = dotm(S.tvec, S.A + a, SA, a, k);
  __syncthreads();
  double part = 0.0;
  for (int i = tid; i < k; i += WG)
    part += (double)S.yb[i] * (double)S.alpha[i];
  const double yta = block_sum(part, S.red, tid);

PH(5);
  // ---- L: K^-1 = V^T V (lauum) on f32 MFMA -------------------------
  // SYRK-shaped: Kinv_ij = sum_c V[c][i] V[c][j] (V = S.A lower; the
  // strict upper holds the Kb cache, so fragment reads are masked to
  // c >= i).  Each wave holds its output tiles in registers across a
  // barrier, then writes back — no staging buffer, no read/write race,
  // Kb cache untouched.  (Round-2 history: a strided-dot4 version ran
  // 18.3 us/expert at k=100; a register-accumulated chunk variant was
  // SLOWER, 21.3 us; this MFMA form replaces both.)
  {
    const int nt = (k + 15) / 16;
    const int ntri = nt * (nt + 1) / 2;
    // the wave index in an SGPR: tile indices and loop bounds are then
    // scalar, and the tile loops branch on SCC, not on exec
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l16 = lane & 15, kg = lane >> 4;
    constexpr int MAXT = 5;                 // ceil(36 tiles / 8 waves)
    // Tile (ti, tj), ti >= tj, has no unmasked A fragment before c = 16 ti,
    // so its sum starts there (the steps left out add +0).  Fragments come
    // in batches of XCH steps (lauum_feed above), and a wave's tiles go in
    // pairs: the second of a pair lies in a later tile row, starts later
    // and is the shorter one, so the pair runs together until the second
    // ends.
    mfma_f32x4 acc[MAXT];                   // compile-time indexed only
#pragma unroll
    for (int u = 0; u < MAXT; ++u) acc[u] = {0.f, 0.f, 0.f, 0.f};
    // tiles u and u + 1 of this wave, u a compile-time constant
    const auto pair = [&](auto uc) {
      constexpr int u = decltype(uc)::value;
      const int t = wave + u * (WG / 64), t2 = t + WG / 64;
      if (t >= ntri) return;
      int ti, tj;
      tri_decode(t, ti, tj);
      int c0 = 16 * ti;
      const int gi = ti * 16 + l16, gj = tj * 16 + l16;
      if constexpr (u + 1 < MAXT) {
        if (t2 < ntri) {
          int ti2, tj2;
          tri_decode(t2, ti2, tj2);
          const int ga[2] = {gi, ti2 * 16 + l16};
          const int gb[2] = {gj, tj2 * 16 + l16};
          for (int c2 = 16 * ti2; c2 < k; c0 += 4 * XCH, c2 += 4 * XCH)
            lauum_feed<XCH, 2>(&acc[u], S.A, SA, k, kg, {c0, c2}, ga, gb);
        }
      }
      for (; c0 < k; c0 += 4 * XCH)
        lauum_feed<XCH, 1>(&acc[u], S.A, SA, k, kg, {c0}, {gi}, {gj});
    };
    pair(std::integral_constant<int, 0>{});
    pair(std::integral_constant<int, 2>{});
    pair(std::integral_constant<int, 4>{});
    static_assert(MAXT <= 6, "phase L pairs its tiles by hand");
    __syncthreads();                        // all V reads complete
#pragma unroll
    for (int u = 0; u < MAXT; ++u) {
      const int t = wave + u * (WG / 64);
      if (t >= ntri) continue;
      int ti, tj;
      tri_decode(t, ti, tj);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int gi = ti * 16 + kg * 4 + r;
        const int gj = tj * 16 + l16;
        if (gi < k && gj < k && gj <= gi)
          S.A[(size_t)gi * SA + gj] = acc[u][r];
      }
    }
    __syncthreads();
  }

PH(6);
    // ---- W: W = (aa^T - K^-1) o Kd, in place + mirror; trG, and
    // sumW0 = sum (aa^T - K^-1) o Kb.  RBF: Kd = Kb, read from the cache.
    // Matern: t from the cache, one exp for Kb and Kd (diagonal: t = 0).
  double trg_part = 0.0, sw_part = 0.0;
  {
    const int nlow = k * (k + 1) / 2;
    for (int f = tid; f < nlow; f += WG) {
      int a, b;
      tri_decode(f, a, b);
      const float g = S.alpha[a] * S.alpha[b] - S.A[(size_t)a * SA + b];
      float w, gkb;                         // g * Kd, g * Kb
      if (FAM == GEOM_FAM_RBF) {
        const float kb = (a == b) ? 1.0f : S.A[(size_t)b * SA + a];
        w = g * kb;
        gkb = w;
      } else {
        float kb, kd;
        family_kb_kd<FAM>((a == b) ? 0.0f : S.A[(size_t)b * SA + a], kb, kd);
        w = g * kd;
        gkb = g * kb;
      }
      if (a == b) {
        trg_part += (double)g;
        sw_part += (double)gkb;
      } else {
        sw_part += 2.0 * (double)gkb;
      }
      S.A[(size_t)a * SA + b] = w;
      if (a != b) S.A[(size_t)b * SA + a] = w;
    }
  }
  const double trG = block_sum(trg_part, S.red, tid);
  const double sumW0 = block_sum(sw_part, S.red, tid);

PH(7);
    // ---- G: row sums of W0 ------------------------------------------
  for (int a = tid; a < k; a += WG) {
    const float* wr = S.A + (size_t)a * SA;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int b = 0;
    for (; b + 3 < k; b += 4) {
      s0 += wr[b]; s1 += wr[b + 1]; s2 += wr[b + 2]; s3 += wr[b + 3];
    }
    for (; b < k; ++b) s0 += wr[b];
    S.rrow[a] = (s0 + s1) + (s2 + s3);
  }
  __syncthreads();

PH(8);
  // ---- H: contraction on f32 MFMA ----------------------------------
  // contr'_j = 2 sum_a x'_aj (x'_aj r_a - (W0 X')_aj) with W0 = S.A
  // (full symmetric after phase W) and X' the scaled coordinates: the
  // W0 @ X' product is a [k, d] GEMM on 16x16x4 f32 tiles; each wave
  // owns whole output tiles, folds its fragment against x' and r, and
  // drops one fp32 partial per (row-tile, column) into T; a final pass
  // sums the row-tile partials in fp64 and de-scales by s2_j.
  {
    const int nti = (k + 15) / 16;
    const int ntj = (d + 15) / 16;
    const int wave = tid >> 6;
    const int l16 = lane & 63 & 15, kg = (lane & 63) >> 4;
    for (int f = tid; f < nti * d; f += WG) S.T[f] = 0.f;
    __syncthreads();
    for (int t = wave; t < nti * ntj; t += WG / 64) {
      const int ti = t / ntj, tj = t - ti * ntj;
      mfma_f32x4 a = {0.f, 0.f, 0.f, 0.f};
      const int fi = ti * 16 + l16;         // W0 row (A fragment)
      const int fj = tj * 16 + l16;         // X' column (B fragment)
      const float sj = fj < d ? S.sc[fj] : 0.f;
      for (int c0 = 0; c0 < k; c0 += 4 * XCH) {
        float bv[XCH];
#pragma unroll
        for (int u = 0; u < XCH; ++u) {
          const int cc = c0 + 4 * u + kg;
          bv[u] = (cc < k && fj < d) ? Xe[(size_t)cc * d + fj] * sj : 0.f;
        }
#pragma unroll
        for (int u = 0; u < XCH; ++u) {
          const int cc = c0 + 4 * u + kg;
          if (c0 + 4 * u >= k) break;
          const float av = (fi < k && cc < k)
                               ? S.A[(size_t)fi * SA + cc] : 0.f;
          a = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv[u], a, 0, 0, 0);
        }
      }
      // fold: per fragment element (row gi, col gj):
      //   part += 2 x'(gi,gj) * (x'(gi,gj) * r_gi - wx)
      float part = 0.f;
      const int gj = tj * 16 + l16;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int gi = ti * 16 + kg * 4 + r;
        if (gi < k && gj < d) {
          // spelled out so that it does not depend on what the compiler
          // chooses to contract: rounded product, rounded difference,
          // fused accumulate
#pragma clang fp contract(off)
          const float x = Xe[(size_t)gi * d + gj] * sj;
          const float xr = x * S.rrow[gi];
          part = __builtin_fmaf(2.0f * x, xr - a[r], part);
        }
      }
      // reduce the 4 row-groups sharing this column: lanes l, l+16,
      // l+32, l+48
      part += __shfl_down(part, 32, 64);
      part += __shfl_down(part, 16, 64);
      if ((lane >> 4) == 0 && gj < d) S.T[ti * d + gj] = part;
    }
    __syncthreads();
    for (int j = tid; j < d; j += WG) {
      double acc = 0.0;
      for (int ti = 0; ti < nti; ++ti) acc += (double)S.T[ti * d + j];
      // contraction ran in scaled coordinates: contr' = s2_j * contr.
      // s2_j == 0 (beta at its zero bound) => dK/dbeta_j == 0 and the
      // host multiplies by beta_j anyway: emit 0 (the exact limit).
      const double s2j = (double)S.s2[j];
      out_contr[(size_t)e * d + j] = s2j > 0.0 ? acc / s2j : 0.0;
    }
    __syncthreads();
  }

  PH(9);
  if (tid == 0) {
    out_bad[e] = 0;
    out_nll[e] = 0.5 * yta + 0.5 * logdet;
    out_sumW0[e] = sumW0;
    out_trG[e] = trG;
  }
#undef PH
}

typedef void (*nll_kernel_t)(
    const float*, const float*, const float*, float, float, int, int,
    double*, double*, double*, double*, int*, unsigned long long*);

#ifndef NLL_LAUNCHERS

// a Matern translation unit: hand its front to the launchers
extern "C" const void* NLL_KERNEL_GETTER() { return (const void*)NLL_KERNEL; }

#else   // the RBF translation unit: the launchers of every family

extern "C" const void* nll_kernel_m32();   // expert_nll_m32.hip
extern "C" const void* nll_kernel_m52();   // expert_nll_m52.hip

// the front of a family code; null for an unknown one
static nll_kernel_t nll_kernel_of(int family) {
  switch (family) {
    case GEOM_FAM_RBF: return fused_expert_nll_kernel;
    case GEOM_FAM_M32: return (nll_kernel_t)nll_kernel_m32();
    case GEOM_FAM_M52: return (nll_kernel_t)nll_kernel_m52();
  }
  return nullptr;
}

// dynamic LDS of a launch; 0 when the shape is not supported
static size_t nll_launch_lds(int k, int d) {
  if (k < 1 || k > 128 || d > 128) return 0;
  size_t lds = nll_lds_bytes(k, d);
  // occupancy experiment knob: lower the resident WGs per CU by padding
  // the LDS ask (measures how much co-resident expert WGs overlap)
  if (const char* pad = getenv("SPARK_GP_AMD_NLL_LDS_PAD"))
    lds += (size_t)atol(pad);
  return lds <= GEOM_LDS_MAX ? lds : 0;
}

// host-callable launcher (used by bindings.cpp)
extern "C" hipError_t launch_fused_expert_nll(
    const float* X, const float* y, const float* scale,
    float amp, float noise, int E, int k, int d,
    double* out_nll, double* out_sumW0, double* out_trG, double* out_contr,
    int* out_bad, unsigned long long* out_clk, int family,
    hipStream_t stream) {
  const nll_kernel_t kern = nll_kernel_of(family);
  if (!kern) return hipErrorInvalidValue;
  const size_t lds = nll_launch_lds(k, d);
  if (!lds) return hipErrorInvalidConfiguration;
  hipLaunchKernelGGL(kern, dim3(E), dim3(WG), lds, stream,
                     X, y, scale, amp, noise, k, d,
                     out_nll, out_sumW0, out_trG, out_contr, out_bad,
                     out_clk);
  return hipGetLastError();
}

// workgroups of the kernel the runtime keeps resident per CU at the block
// size and dynamic LDS launch_fused_expert_nll uses for (k, d)
extern "C" hipError_t fused_expert_nll_resident_wgs(int k, int d, int family,
                                                    int* out) {
  const nll_kernel_t kern = nll_kernel_of(family);
  if (!kern) return hipErrorInvalidValue;
  const size_t lds = nll_launch_lds(k, d);
  if (!lds) return hipErrorInvalidConfiguration;
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(out, kern, WG, lds);
}

#endif  // NLL_LAUNCHERS

// Streamed-feature forms of the fused Laplace kernel (the WIDE instantiations
// of laplace.hip, compiled in laplace_wide.hip): X is never resident in LDS.
// It is read from global memory in slabs of LAPW_SW columns into one of two
// k-row slab buffers (kernel_geom.h: lapw_lds_bytes), which is all the two
// consumers of X need:
//   - the Kb cache, built once on the fp32 matrix cores from the Gram tiles of
//     the scaled rows (lapw_kb_cache), and
//   - the evidence tail's two loops over feature columns, which take 8 columns
//     at a time, two chunks to a slab.
// A slab moves in two halves so that its global latency hides behind the work
// on the slab before it: lapw_load issues the loads into four registers per
// thread, and lapw_store puts them into the other buffer once that work is
// done, in front of the barrier that ends it.
// Included by laplace.hip (needs WG, kernel_geom.h and linalg_lds.h).
#pragma once
#include <hip/hip_runtime.h>

// thread tid moves the elements f = tid + u WG of a slab, f = 16 row + column:
// 16 lanes per row read one 64-B global segment
#define LAPW_PER (128 * LAPW_SW / WG)
static_assert(LAPW_PER * WG == 128 * LAPW_SW, "a slab of k <= 128 rows");

// slab s of the raw features (zero past d)
__device__ __forceinline__ void lapw_load(const float* __restrict__ Xe,
                                          const int k, const int d,
                                          const int s, const int tid,
                                          float (&pre)[LAPW_PER]) {
#pragma unroll
  for (int u = 0; u < LAPW_PER; ++u) {
    const int f = tid + u * WG;
    const int a = f / LAPW_SW, j = s * LAPW_SW + f % LAPW_SW;
    pre[u] = (a < k && j < d) ? Xe[(size_t)a * d + j] : 0.f;
  }
}

// slab s of the scaled rows x' = (x - x_0) o scale, centred on the expert's
// first row: q is translation-invariant, and the Gram form below cancels
// against the norms of what it is given, so the rows go in as small as one
// pass makes them.  Clears xfin on a non-finite feature.
__device__ __forceinline__ void lapw_load_scaled(
    const float* __restrict__ Xe, const float* __restrict__ scale,
    const int k, const int d, const int s, const int tid,
    float (&pre)[LAPW_PER], bool& xfin) {
#pragma unroll
  for (int u = 0; u < LAPW_PER; ++u) {
    const int f = tid + u * WG;
    const int a = f / LAPW_SW, j = s * LAPW_SW + f % LAPW_SW;
    float v = 0.f;
    if (a < k && j < d) {
      const float x = Xe[(size_t)a * d + j];
      xfin = xfin && isfinite(x);
      v = (x - Xe[j]) * scale[j];
    }
    pre[u] = v;
  }
}

__device__ __forceinline__ void lapw_store(float* buf, const int k,
                                           const int tid,
                                           const float (&pre)[LAPW_PER]) {
#pragma unroll
  for (int u = 0; u < LAPW_PER; ++u) {
    const int f = tid + u * WG;
    const int a = f / LAPW_SW;
    if (a < k) buf[a * LAPW_SS + f % LAPW_SW] = pre[u];
  }
}

// buffer of slab s
__device__ __forceinline__ float* lapw_buf(float* slab, const int k,
                                           const int s) {
  return slab + (s & 1) * lapw_slab_floats(k);
}

// Kb = exp(-max(q, 0)) into A's STRICT UPPER triangle, where the resident
// kernel puts it, with q_ab = n_a + n_b - 2 x'_a . x'_b from the Gram tiles of
// the scaled rows on v_mfma_f32_16x16x4_f32 (phase B of expert_nll.hip is the
// same form).  The lower triangle's 16 x 16 tiles are dealt round-robin to the
// 8 waves, at most 5 to a wave at k = 128, and every accumulator stays in
// registers over all slabs: X is streamed once.  A lane's fragment is ONE
// 16-B read per slab and row tile: lane (l16, kg) holds columns 4 kg .. 4 kg
// + 3 of row l16, and the slab's four MFMA steps take the k-index 4 kg + v in
// step v for both operands, which only permutes the terms of the dot product.
// Fragment rows past k are clamped onto row k - 1: they feed only D entries
// past k, which the epilogue drops.  The row norms are the diagonal of the
// diagonal tiles (the same rounding as the products they are set against;
// q_aa = 0 exactly) and pass through nrm (k floats).
// All WG threads must call; the caller's barrier publishes the cache.
// Returns false if the expert holds a non-finite feature.
__device__ inline bool lapw_kb_cache(float* A, const int SA, float* slab,
                                     float* nrm,
                                     const float* __restrict__ Xe,
                                     const float* __restrict__ scale,
                                     const int k, const int d,
                                     const int tid) {
  const int lane = tid & 63, wave = tid >> 6;
  const int l16 = lane & 15, kg = lane >> 4;
  const int nt = (k + 15) / 16;
  const int ntri = nt * (nt + 1) / 2;
  const int ns = (d + LAPW_SW - 1) / LAPW_SW;
  constexpr int MAXT = 5;                   // 36 tiles over 8 waves
  mfma_f32x4_t acc[MAXT];                   // compile-time indexed only
#pragma unroll
  for (int u = 0; u < MAXT; ++u) acc[u] = {0.f, 0.f, 0.f, 0.f};
  bool xfin = true;
  float pre[LAPW_PER];
  lapw_load_scaled(Xe, scale, k, d, 0, tid, pre, xfin);
  lapw_store(slab, k, tid, pre);
  __syncthreads();
  for (int s = 0; s < ns; ++s) {
    const float* cur = lapw_buf(slab, k, s);
    if (s + 1 < ns) lapw_load_scaled(Xe, scale, k, d, s + 1, tid, pre, xfin);
#pragma unroll
    for (int u = 0; u < MAXT; ++u) {
      const int t = wave + u * (WG / 64);
      if (t >= ntri) continue;
      int ti, tj;
      tri_decode(t, ti, tj);
      const int ia = min(ti * 16 + l16, k - 1);
      const int jb = min(tj * 16 + l16, k - 1);
      const float4 av = *(const float4*)(cur + ia * LAPW_SS + 4 * kg);
      const float4 bv = *(const float4*)(cur + jb * LAPW_SS + 4 * kg);
      acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, bv.x, acc[u],
                                                    0, 0, 0);
      acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, bv.y, acc[u],
                                                    0, 0, 0);
      acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.z, bv.z, acc[u],
                                                    0, 0, 0);
      acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.w, bv.w, acc[u],
                                                    0, 0, 0);
    }
    // the other buffer was last read before the barrier of slab s - 1
    if (s + 1 < ns) lapw_store(lapw_buf(slab, k, s + 1), k, tid, pre);
    __syncthreads();
  }
  // D map: row = (lane>>4)*4 + r, col = lane&15
#pragma unroll
  for (int u = 0; u < MAXT; ++u) {
    const int t = wave + u * (WG / 64);
    if (t >= ntri) continue;
    int ti, tj;
    tri_decode(t, ti, tj);
    if (ti != tj) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (kg * 4 + r == l16 && ti * 16 + l16 < k)
        nrm[ti * 16 + l16] = acc[u][r];
  }
  __syncthreads();
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
      if (gi >= k || gj >= k || gj >= gi) continue;
      const float q = nrm[gi] + nrm[gj] - 2.0f * acc[u][r];
      A[(size_t)gj * SA + gi] = __expf(-fmaxf(q, 0.f));   // upper: gj < gi
    }
  }
  return xfin;
}

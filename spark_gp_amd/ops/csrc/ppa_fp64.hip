// Fused fp64 PPA accumulation: KK += K^T K and Ky += K^T y with fp32 kernel
// values, fp64 products and fp64 accumulation on v_mfma_f64_16x16x4_f64
// (MI355X, gfx950).  Replaces, for setPpaPrecision("fp64") with
// setFusedPpaFp64(True), the chunk.double() copy and the two torch (rocBLAS)
// products of hip_backend.kmn_knm_and_kmny.
//
// Work split.  A block of 256 threads (2 x 2 waves) owns one 128 x 128 tile
// (ti >= tj) of the lower triangle of KK and one of split_k slices of the
// chunk's rows; the grid is 1-D, slice-major over tiles.  A wave owns 64 x 64
// outputs as 4 x 4 MFMA accumulators: 128 registers per lane.  Fragment and
// D maps are the ones measured for big_chol.hip: A lane l -> A[i = l & 15]
// [k = l >> 4], B lane l -> B[k = l >> 4][j = l & 15], D lane l reg r ->
// D[(l >> 4) + 4 r][l & 15].
//
// K-step.  32 rows at a time.  The two operand windows W_I, W_J [32, 128]
// (rows of the chunk x columns of the tile's row / column window) sit in LDS
// as doubles, 2 x 32 KB, row k stored with its column index XOR 16 (k & 1):
// a 32-lane group of a fragment read is two rows of 16 consecutive doubles,
// and the swap puts the odd row on the other 32 banks.  A diagonal tile
// builds W_I alone and feeds it to both operands.  Per step a wave issues
// 8 x 16 MFMAs on 8 + 8 ds_read_b64.
//
// Feeders.
//   GEN = true (d <= 32): the block keeps the fp32 rows of its two active-set
//     windows in LDS for the whole k loop, stages the step's 32 rows of X and
//     computes K = amp Kb(sum_j s2_j (x_j - a_j)^2) by direct differences in
//     fp32, cross_kernel_tile_kernel's arithmetic, into the windows: no K_nm
//     array exists.  A thread makes a 4 x 4 patch (rows rg + 8 i, columns
//     cg + 32 j) per window: its A reads hit bank cg + q, its X reads are
//     broadcasts, its window stores are 32 consecutive doubles per row.
//   GEN = false (any d): the windows are read from the fp32 [c, m] chunk
//     cross_kernel_tile wrote, widened at the staging write.
// Rows >= c and columns >= m are loaded from the clamped index and replaced
// by exact zeros, so no load diverges and the padding adds nothing.
//
// Buffering.  The next step's global loads (X rows or chunk values, and y)
// are issued into registers before the current step's MFMAs and written to
// LDS after them.  The windows themselves are single-buffered: two more
// 32 KB windows next to the generating feeder's 33 KB of A rows pass the
// 160 KB of LDS, so generation and the MFMAs of one block do not overlap.
//
// Ky.  A diagonal tile's block also sums K_ri y_r in fp64 from the window it
// holds: thread t takes column t & 127 over rows 16 (t >> 7) .. + 16.
//
// Reproducibility.  No atomics.  split_k = 1: the block adds its tile, and an
// off-diagonal tile's mirror, into KK and its column sums into Ky; every
// element has one owner.  split_k > 1: every slice stores its fp64 tile (an
// empty slice stores zeros) and column sums to the caller's scratch, and
// ppa_fp64_reduce_kernel adds them per element in ascending slice order into
// both triangles of KK and into Ky.  The same inputs give the same bits.
//
// Resources on gfx950 (hipcc -O3, -Rpass-analysis=kernel-resource-usage):
//   <RBF | M32 | M52, GEN = true>: 256 VGPRs, 168 AGPRs, 0 B scratch,
//     105,984 B LDS, 1 wave/SIMD (one block per compute unit);
//   <RBF, GEN = false>: 254 VGPRs, 128 AGPRs, 0 B scratch, 67,840 B LDS,
//     1 wave/SIMD;
//   ppa_fp64_reduce_kernel: 22 VGPRs, no LDS.
// The 128 accumulator registers live in AGPRs and do not spill; the
// generating feeder parks 40 more values there between its phases.

#include <hip/hip_runtime.h>
#include <math.h>

#include "kernel_geom.h"
#include "launchers.h"

typedef __attribute__((ext_vector_type(4))) double f64x4;

static_assert(PF_THREADS == 256 && PF_TILE == 128 && PF_BK == 32,
              "the lane maps below are written for this geometry");

// element (k, col) of an operand window
__device__ __forceinline__ int pf_widx(const int k, const int col) {
  return k * PF_TILE + (col ^ ((k & 1) << 4));
}

// lower-triangle tile f -> (ti >= tj)
__device__ __forceinline__ void pf_tri_decode(const int f, int& ti, int& tj) {
  int a = (int)((sqrtf(8.f * (float)f + 1.f) - 1.f) * 0.5f);
  while ((a + 1) * (a + 2) / 2 <= f) ++a;
  while (a * (a + 1) / 2 > f) --a;
  ti = a;
  tj = f - a * (a + 1) / 2;
}

// the next k-step's global values, held in registers across the MFMAs
template <bool GEN> struct PfRegs;
template <> struct PfRegs<true> {
  float x[PF_BK * PF_DMAX / PF_THREADS];     // 32 rows of X, d <= 32
  float y;
};
template <> struct PfRegs<false> {
  float ki[PF_BK * PF_TILE / PF_THREADS];    // chunk values of window I
  float kj[PF_BK * PF_TILE / PF_THREADS];    // and J (off-diagonal tiles)
  float y;
};

__device__ __forceinline__ float pf_load_y(const float* __restrict__ yv,
                                           const int c, const int k0,
                                           const int tid) {
  const int gr = k0 + (tid & (PF_BK - 1));
  const float v = yv[gr < c ? gr : c - 1];
  return gr < c ? v : 0.f;
}

// GEN: rows k0 .. k0 + 32 of X, element f = r d + q of the step per thread
__device__ __forceinline__ void pf_load(PfRegs<true>& R,
                                        const float* __restrict__ X,
                                        const float* __restrict__ yv,
                                        const int c, const int d,
                                        const int k0, const int tid) {
#pragma unroll
  for (int u = 0; u < PF_BK * PF_DMAX / PF_THREADS; ++u) {
    const int f = tid + PF_THREADS * u;
    const int r = f / d, q = f - r * d;
    const int gr = k0 + r < c ? k0 + r : c - 1;
    R.x[u] = (f < PF_BK * d) ? X[(size_t)gr * d + q] : 0.f;
  }
  R.y = pf_load_y(yv, c, k0, tid);
}

__device__ __forceinline__ void pf_stage_x(const PfRegs<true>& R,
                                           float* __restrict__ xs,
                                           double* __restrict__ ys,
                                           const int d, const int tid) {
#pragma unroll
  for (int u = 0; u < PF_BK * PF_DMAX / PF_THREADS; ++u) {
    const int f = tid + PF_THREADS * u;
    const int r = f / d, q = f - r * d;
    if (f < PF_BK * d) xs[r * PF_XSTR + q] = R.x[u];
  }
  if (tid < PF_BK) ys[tid] = (double)R.y;
}

// staged: element (r, col) = (tid >> 7) + 2 u, tid & 127 of each window
__device__ __forceinline__ float pf_load_k(const float* __restrict__ K,
                                           const int c, const int m,
                                           const int gr, const int gc) {
  const float v = K[(size_t)(gr < c ? gr : c - 1) * m + (gc < m ? gc : m - 1)];
  return (gr < c && gc < m) ? v : 0.f;
}

__device__ __forceinline__ void pf_load(PfRegs<false>& R,
                                        const float* __restrict__ K,
                                        const float* __restrict__ yv,
                                        const int c, const int m,
                                        const int k0, const int i0,
                                        const int j0, const bool diag,
                                        const int tid) {
  const int col = tid & (PF_TILE - 1), r0 = tid >> 7;
#pragma unroll
  for (int u = 0; u < PF_BK * PF_TILE / PF_THREADS; ++u)
    R.ki[u] = pf_load_k(K, c, m, k0 + r0 + 2 * u, i0 + col);
  if (!diag) {
#pragma unroll
    for (int u = 0; u < PF_BK * PF_TILE / PF_THREADS; ++u)
      R.kj[u] = pf_load_k(K, c, m, k0 + r0 + 2 * u, j0 + col);
  }
  R.y = pf_load_y(yv, c, k0, tid);
}

__device__ __forceinline__ void pf_stage_k(const PfRegs<false>& R,
                                           double* __restrict__ wi,
                                           double* __restrict__ wj,
                                           double* __restrict__ ys,
                                           const bool diag, const int tid) {
  const int col = tid & (PF_TILE - 1), r0 = tid >> 7;
#pragma unroll
  for (int u = 0; u < PF_BK * PF_TILE / PF_THREADS; ++u)
    wi[pf_widx(r0 + 2 * u, col)] = (double)R.ki[u];
  if (!diag) {
#pragma unroll
    for (int u = 0; u < PF_BK * PF_TILE / PF_THREADS; ++u)
      wj[pf_widx(r0 + 2 * u, col)] = (double)R.kj[u];
  }
  if (tid < PF_BK) ys[tid] = (double)R.y;
}

// the fp32 rows of one active-set window, clamped at m - 1
__device__ __forceinline__ void pf_stage_a(const float* __restrict__ A,
                                           float* __restrict__ aw,
                                           const int m, const int d,
                                           const int c0, const int tid) {
  for (int f = tid; f < PF_TILE * d; f += PF_THREADS) {
    const int r = f / d, q = f - r * d;
    const int gc = c0 + r < m ? c0 + r : m - 1;
    aw[r * PF_XSTR + q] = A[(size_t)gc * d + q];
  }
}

template <int FAM>
__device__ __forceinline__ void pf_emit(const float (&q)[4][4],
                                        double* __restrict__ w,
                                        const float amp, const int c,
                                        const int m, const int k0,
                                        const int c0, const int rg,
                                        const int cg) {
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int row = rg + 8 * i, col = cg + 32 * j;
      // q is a sum of squares: no clamp
      const float v = amp * (FAM == GEOM_FAM_RBF ? __expf(-q[i][j])
                                                 : family_kb<FAM>(q[i][j]));
      w[pf_widx(row, col)] =
          (k0 + row < c && c0 + col < m) ? (double)v : 0.0;
    }
}

// K values of the step's 32 rows against window I (and J): q by direct
// differences, as cross_kernel_tile_kernel forms it
template <int FAM, bool DIAG>
__device__ __forceinline__ void pf_generate(
    const float* __restrict__ xs, const float* __restrict__ aw,
    const float* __restrict__ s2s, double* __restrict__ wi,
    double* __restrict__ wj, const float amp, const int c, const int m,
    const int d, const int k0, const int i0, const int j0, const int tid) {
  const int rg = tid >> 5, cg = tid & 31;
  const float* awj = aw + PF_TILE * PF_XSTR;
  float qi[4][4], qj[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) qi[i][j] = qj[i][j] = 0.f;

#pragma unroll 4
  for (int q = 0; q < d; ++q) {
    const float w = s2s[q];
    float xf[4], ai[4], aj[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) xf[i] = xs[(rg + 8 * i) * PF_XSTR + q];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      ai[j] = aw[(cg + 32 * j) * PF_XSTR + q];
      if (!DIAG) aj[j] = awj[(cg + 32 * j) * PF_XSTR + q];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float t = xf[i] - ai[j];
        qi[i][j] += w * t * t;
        if (!DIAG) {
          const float tj = xf[i] - aj[j];
          qj[i][j] += w * tj * tj;
        }
      }
  }
  pf_emit<FAM>(qi, wi, amp, c, m, k0, i0, rg, cg);
  if (!DIAG) pf_emit<FAM>(qj, wj, amp, c, m, k0, j0, rg, cg);
}

template <int FAM, bool GEN>
__global__ void __launch_bounds__(PF_THREADS)
ppa_fp64_kernel(const float* __restrict__ X,     // GEN: rows [c, d];
                                                 // else the chunk K [c, m]
                const float* __restrict__ A,     // GEN: active set [m, d]
                const float* __restrict__ s2v,   // GEN: [d] scale^2
                const float amp,
                const float* __restrict__ yv,    // [c]
                const int c, const int m, const int d, const int split_k,
                double* __restrict__ Ky,         // [m] accumulated
                double* __restrict__ KK,         // [m, m] accumulated
                double* __restrict__ partials) { // split_k > 1: the slices'
                                                 // tiles and column sums
  __shared__ __align__(16) double wi[PF_BK * PF_TILE];
  __shared__ __align__(16) double wj[PF_BK * PF_TILE];
  __shared__ double ys[PF_BK];
  __shared__ double kyred[PF_THREADS];
  __shared__ float aw[GEN ? 2 * PF_TILE * PF_XSTR : 1];
  __shared__ float xs[GEN ? PF_BK * PF_XSTR : 1];
  __shared__ float s2s[GEN ? PF_DMAX : 1];

  const int ntiles = (int)pf_tiles(m);
  const int tile = blockIdx.x % ntiles, slice = blockIdx.x / ntiles;
  int ti, tj;
  pf_tri_decode(tile, ti, tj);
  const int i0 = ti * PF_TILE, j0 = tj * PF_TILE;
  const bool diag = ti == tj;

  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int wr = (wave >> 1) * 64, wc = (wave & 1) * 64;
  const int l16 = lane & 15, kg = lane >> 4;

  // this slice's k-steps; the last slices of a short chunk may have none
  const int ksteps = (c + PF_BK - 1) / PF_BK;
  const int per = (ksteps + split_k - 1) / split_k;
  const int ks0 = slice * per;
  const int ks1 = ks0 + per < ksteps ? ks0 + per : ksteps;

  if (GEN) {
    pf_stage_a(A, aw, m, d, i0, tid);
    if (!diag) pf_stage_a(A, aw + PF_TILE * PF_XSTR, m, d, j0, tid);
    if (tid < d) s2s[tid] = s2v[tid];
  }

  f64x4 acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = {0.0, 0.0, 0.0, 0.0};
  double kyacc = 0.0;

  PfRegs<GEN> R;
  if (ks0 < ks1) {
    if constexpr (GEN) pf_load(R, X, yv, c, d, ks0 * PF_BK, tid);
    else pf_load(R, X, yv, c, m, ks0 * PF_BK, i0, j0, diag, tid);
  }

  for (int ks = ks0; ks < ks1; ++ks) {
    const int k0 = ks * PF_BK;
    if constexpr (GEN) {
      pf_stage_x(R, xs, ys, d, tid);
      __syncthreads();       // also orders the A windows before their use
      if (diag)
        pf_generate<FAM, true>(xs, aw, s2s, wi, wj, amp, c, m, d, k0, i0, j0,
                               tid);
      else
        pf_generate<FAM, false>(xs, aw, s2s, wi, wj, amp, c, m, d, k0, i0,
                                j0, tid);
    } else {
      pf_stage_k(R, wi, wj, ys, diag, tid);
    }
    if (ks + 1 < ks1) {
      if constexpr (GEN) pf_load(R, X, yv, c, d, k0 + PF_BK, tid);
      else pf_load(R, X, yv, c, m, k0 + PF_BK, i0, j0, diag, tid);
    }
    __syncthreads();

    const double* bw = diag ? wi : wj;
#pragma unroll
    for (int kc = 0; kc < PF_BK / 4; ++kc) {
      const int k = kc * 4 + kg;
      double af[4], bf[4];
#pragma unroll
      for (int a = 0; a < 4; ++a) af[a] = wi[pf_widx(k, wr + 16 * a + l16)];
#pragma unroll
      for (int b = 0; b < 4; ++b) bf[b] = bw[pf_widx(k, wc + 16 * b + l16)];
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b)
          acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[a], bf[b],
                                                           acc[a][b], 0, 0, 0);
    }
    if (diag) {
      const int col = tid & (PF_TILE - 1), kh = (tid >> 7) * (PF_BK / 2);
#pragma unroll
      for (int kk = 0; kk < PF_BK / 2; ++kk)
        kyacc += wi[pf_widx(kh + kk, col)] * ys[kh + kk];
    }
    __syncthreads();
  }

  // ---- epilogue ----------------------------------------------------------
  double* part = nullptr;
  if (split_k > 1)
    part = partials + (size_t)slice * pf_slice_doubles(m);
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int li = wr + 16 * a + kg + 4 * r, lj = wc + 16 * b + l16;
        const double v = acc[a][b][r];
        if (split_k > 1) {
          part[(size_t)tile * (PF_TILE * PF_TILE) + li * PF_TILE + lj] = v;
        } else {
          const int gi = i0 + li, gj = j0 + lj;
          if (gi < m && gj < m) {
            KK[(size_t)gi * m + gj] += v;
            if (!diag) KK[(size_t)gj * m + gi] += v;
          }
        }
      }
  if (diag) {
    kyred[tid] = kyacc;
    __syncthreads();
    if (tid < PF_TILE) {
      const double t = kyred[tid] + kyred[tid + PF_TILE];
      if (split_k > 1)
        part[(size_t)ntiles * (PF_TILE * PF_TILE) + i0 + tid] = t;
      else if (i0 + tid < m)
        Ky[i0 + tid] += t;
    }
  }
}

// KK and Ky += the slices' partials, per element in ascending slice order;
// an off-diagonal tile's element and its mirror get sums of the same terms
// in the same order.  Grid (tiles, 16 strips of 8 tile rows): thread t takes
// elements t + 256 u of its strip, rows of 128 consecutive doubles, for the
// tile and again (reading the transposed element) for the mirror tile.
__global__ void __launch_bounds__(PF_THREADS)
ppa_fp64_reduce_kernel(const double* __restrict__ partials, const int m,
                       const int split_k, double* __restrict__ Ky,
                       double* __restrict__ KK) {
  const int tile = blockIdx.x, strip = blockIdx.y, tid = threadIdx.x;
  int ti, tj;
  pf_tri_decode(tile, ti, tj);
  const int i0 = ti * PF_TILE, j0 = tj * PF_TILE;
  const size_t sstr = pf_slice_doubles(m);
  const double* pt = partials + (size_t)tile * (PF_TILE * PF_TILE);
#pragma unroll
  for (int u = 0; u < 8 * PF_TILE / PF_THREADS; ++u) {
    const int e = tid + PF_THREADS * u;
    const int a = strip * 8 + (e >> 7), b = e & (PF_TILE - 1);
    double sum = 0.0, mir = 0.0;
    for (int s = 0; s < split_k; ++s) {
      sum += pt[s * sstr + a * PF_TILE + b];
      if (ti != tj) mir += pt[s * sstr + b * PF_TILE + a];
    }
    if (i0 + a < m && j0 + b < m) KK[(size_t)(i0 + a) * m + j0 + b] += sum;
    if (ti != tj && j0 + a < m && i0 + b < m)
      KK[(size_t)(j0 + a) * m + i0 + b] += mir;
  }
  if (ti == tj && strip == 0 && tid < PF_TILE) {
    const double* pk = partials + (size_t)gridDim.x * (PF_TILE * PF_TILE) +
                       i0 + tid;
    double sum = 0.0;
    for (int s = 0; s < split_k; ++s) sum += pk[s * sstr];
    if (i0 + tid < m) Ky[i0 + tid] += sum;
  }
}

// ---------------------------------------------------------------------------
// launcher
// ---------------------------------------------------------------------------
// A == nullptr selects the staged feeder: X is then the fp32 chunk [c, m]
// and s2v, amp, family and d are not used.  partials: pf_partial_doubles(m,
// split_k) doubles, not touched when split_k is 1.

extern "C" hipError_t launch_ppa_fp64(
    const float* X, const float* A, const float* s2v, float amp,
    const float* yv, int c, int m, int d, int split_k, double* Ky, double* KK,
    double* partials, int family, hipStream_t stream) {
  if (!geom_family_ok(family) || c < 1 || split_k < 1 ||
      !ppa_fp64_supported_md(m, d) || (A && d > PF_DMAX))
    return hipErrorInvalidValue;
  void (*kern)(const float*, const float*, const float*, float, const float*,
               int, int, int, int, double*, double*, double*) =
      !A                       ? ppa_fp64_kernel<GEOM_FAM_RBF, false>
      : family == GEOM_FAM_RBF ? ppa_fp64_kernel<GEOM_FAM_RBF, true>
      : family == GEOM_FAM_M32 ? ppa_fp64_kernel<GEOM_FAM_M32, true>
                               : ppa_fp64_kernel<GEOM_FAM_M52, true>;
  const int ntiles = (int)pf_tiles(m);
  hipLaunchKernelGGL(kern, dim3(ntiles * split_k), dim3(PF_THREADS), 0,
                     stream, X, A, s2v, amp, yv, c, m, d, split_k, Ky, KK,
                     partials);
  if (split_k > 1)   // same stream: after every slice's partials are written
    hipLaunchKernelGGL(ppa_fp64_reduce_kernel, dim3(ntiles, PF_TILE / 8),
                       dim3(PF_THREADS), 0, stream, partials, m, split_k, Ky,
                       KK);
  return hipGetLastError();
}

// K16 — one Lloyd step of k-means for MI355X (gfx950, CDNA4): every row's
// nearest centroid, then the per-centroid sums and counts, in two launches
// joined by assign[n_pad] (int32).  No [n, m] array exists anywhere, nothing
// is atomic, and every sum has a fixed order: two runs, and two cards, give
// the same bits.
//
// The two reductions want different ownership, a row tile needs all
// centroids and a centroid slab needs all rows, hence two kernels.  Both run
// on v_mfma_f32_16x16x4_f32 (exact fp32 products, fp32 accumulation).
//
// 1. kmeans_assign_kernel.  A block owns KM_ROWS = 256 rows, wave w the 64
//    rows [64 w, 64 w + 64) as four 16-row tiles (below KM_SMALL_N rows, where
//    that tiling would leave compute units idle: 64 rows, one tile per wave).  Centroids come in panels
//    of KM_PANEL = 64 (four column tiles), staged KM_DBLK = 32 dims at a time
//    through LDS and shared by the four waves; the 4 x 4 accumulator tiles of
//    a panel live in registers, so d never enters the LDS plan.  The X tile
//    stays in LDS across panels while d <= KM_XRES_DMAX and is staged again
//    per panel above.  A panel ends with s_j = ||c_j||^2 - 2 x.c_j (norms
//    from kmeans_norms_kernel, +inf for the columns past m; padded dims are
//    zero) and each lane's running (best, argbest) for its 16 rows: strict <
//    in increasing j.  After the last panel the 16 lanes that hold one row's
//    columns are reduced by butterfly, the lower index winning among equal
//    scores.  Rows past n get assign = -1.
//
// 2. kmeans_accumulate_kernel.  sums = O^T X and counts = O^T 1 for the
//    one-hot O [rows, m] of assign: a block owns KM_SLAB = 128 centroids (32
//    per wave, two row tiles of the product), one panel of the d + 1 columns
//    [X | 1] (NDT <= 8 column tiles) and one slice of KM_SLICE rows.  Rows
//    are staged KM_RCH = 128 at a time; an A fragment is one compare and
//    select on the staged assign value, a B fragment one LDS read.  A product
//    1 * x or 0 * x is exact, so only the fp32 accumulation rounds, and the
//    ones column counts exactly (a slice has fewer than 2^24 rows).  The
//    accumulators go out as the fp64 partial [slice, m, d + 1];
//    kmeans_reduce_kernel adds the partials in slice order into fp64
//    sums [m, d] and counts [m].
//
// Non-finite features.  A NaN score never wins the strict <, so a row whose
// scores are all NaN goes to centroid 0.  In the accumulate kernel 0 * x is
// NaN for a non-finite x, so such a value poisons its column of every
// centroid of the slabs that see the row, not only of its own cluster as an
// index_add would; either way the step's centres are not finite, which is
// what the caller sees.
//
// Geometry, LDS strides with their bank arguments, and the gate:
// kernel_geom.h.

#include <hip/hip_runtime.h>
#include <math.h>

// gfx950's packed fp32 arithmetic stays off for all device code of this file
#ifdef __HIP_DEVICE_COMPILE__
#pragma clang attribute push(                                      \
    __attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

#include "kernel_geom.h"
#include "launchers.h"

typedef __attribute__((ext_vector_type(4))) float km_f32x4;

// f32 16x16x4 fragments: A[i][k] and B[k][j] at lane l are i = j = l & 15,
// k = l >> 4; D[row][col] at lane l, reg r is col = l & 15,
// row = 4 (l >> 4) + r.

// c2[j] = ||c_j||^2 for j < m, +inf for m <= j < mp; a wave per centroid
__global__ void __launch_bounds__(64)
kmeans_norms_kernel(const float* __restrict__ C, const int m, const int d,
                    float* __restrict__ c2) {
  const int j = blockIdx.x, lane = threadIdx.x;
  float s = 0.f;
  if (j < m)
    for (int k = lane; k < d; k += 64) {
      const float v = C[(size_t)j * d + k];
      s = fmaf(v, v, s);
    }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
  if (lane == 0) c2[j] = j < m ? s : HUGE_VALF;
}

// (v, i) against lane ^ o's: the lower score, the lower index among equal ones
__device__ __forceinline__ void km_lower(float& v, int& i, const int o) {
  const float ov = __shfl_xor(v, o, 64);
  const int oi = __shfl_xor(i, o, 64);
  if (ov < v || (ov == v && oi < i)) {
    v = ov;
    i = oi;
  }
}

template <int RT>   // 16-row tiles per wave: 4, or 1 below KM_SMALL_N rows
__global__ void __launch_bounds__(KM_THREADS)
kmeans_assign_kernel(const float* __restrict__ X,    // [n, d]
                     const float* __restrict__ C,    // [m, d]
                     const float* __restrict__ c2,   // [km_mpad(m)]
                     const long n, const int m, const int d,
                     int* __restrict__ assign) {     // [km_npad(n)]
  extern __shared__ char lds_raw[];
  constexpr int ROWS = 64 * RT;                   // of the block
  const int XS = KM_STR(km_xdims(d)), CS = KM_STR(KM_DBLK);
  // carve: the order of km_assign_lds_bytes
  float* const xs = (float*)lds_raw;
  float* const cs =
      (float*)(lds_raw + a16(sizeof(float) * ROWS * (size_t)XS));
  const bool resident = d <= KM_XRES_DMAX;

  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int l16 = lane & 15, kg = lane >> 4;
  const int wr = wave * 16 * RT;
  const long row0 = (long)blockIdx.x * ROWS;
  const int mp = km_mpad(m);

  float best[4 * RT];   // of row 16 a + 4 kg + r of the wave, at [4 a + r]
  int arg[4 * RT];
#pragma unroll
  for (int i = 0; i < 4 * RT; ++i) {
    best[i] = HUGE_VALF;
    arg[i] = 0;
  }

  for (int p0 = 0; p0 < mp; p0 += KM_PANEL) {
    km_f32x4 acc[RT][4];
#pragma unroll
    for (int a = 0; a < RT; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) acc[a][b] = {0.f, 0.f, 0.f, 0.f};

    for (int d0 = 0; d0 < d; d0 += KM_DBLK) {
      const int dl = min(KM_DBLK, d - d0);
      const int xoff = resident ? d0 : 0;
      if (!resident || p0 == 0) {
        for (int f = tid; f < ROWS * KM_DBLK; f += KM_THREADS) {
          const int r = f >> 5, q = f & 31;       // coalesced along a row
          const long gr = row0 + r;
          xs[r * XS + xoff + q] =
              (gr < n && q < dl) ? X[(size_t)gr * d + d0 + q] : 0.f;
        }
      }
      for (int f = tid; f < KM_PANEL * KM_DBLK; f += KM_THREADS) {
        const int r = f >> 5, q = f & 31;
        const int gc = p0 + r;
        cs[r * CS + q] = (gc < m && q < dl) ? C[(size_t)gc * d + d0 + q] : 0.f;
      }
      __syncthreads();
#pragma unroll
      for (int kc = 0; kc < KM_DBLK / 4; ++kc) {
        const int fk = kg + kc * 4;
        float xa[RT], cb[4];
#pragma unroll
        for (int a = 0; a < RT; ++a)
          xa[a] = xs[(wr + a * 16 + l16) * XS + xoff + fk];
#pragma unroll
        for (int b = 0; b < 4; ++b) cb[b] = cs[(b * 16 + l16) * CS + fk];
#pragma unroll
        for (int a = 0; a < RT; ++a)
#pragma unroll
          for (int b = 0; b < 4; ++b)
            acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                xa[a], cb[b], acc[a][b], 0, 0, 0);
      }
      __syncthreads();
    }

    // the panel's scores against the running best: b, then the panels, run
    // through a lane's columns in increasing j
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int col = p0 + b * 16 + l16;
      const float nrm = c2[col];
#pragma unroll
      for (int a = 0; a < RT; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float s = fmaf(-2.0f, acc[a][b][r], nrm);
          if (s < best[4 * a + r]) {
            best[4 * a + r] = s;
            arg[4 * a + r] = col;
          }
        }
    }
  }

  // a row's columns sit in the 16 lanes of equal lane >> 4
#pragma unroll
  for (int i = 0; i < 4 * RT; ++i) {
    km_lower(best[i], arg[i], 1);
    km_lower(best[i], arg[i], 2);
    km_lower(best[i], arg[i], 4);
    km_lower(best[i], arg[i], 8);
  }
#pragma unroll
  for (int a = 0; a < RT; ++a) {
    if (l16 == 0) {
      const long gr = row0 + wr + a * 16 + kg * 4;    // < km_npad(n)
      int4 out;
      out.x = gr + 0 < n ? arg[4 * a + 0] : -1;
      out.y = gr + 1 < n ? arg[4 * a + 1] : -1;
      out.z = gr + 2 < n ? arg[4 * a + 2] : -1;
      out.w = gr + 3 < n ? arg[4 * a + 3] : -1;
      *(int4*)(assign + gr) = out;
    }
  }
}

template <int NDT>
__global__ void __launch_bounds__(KM_THREADS)
kmeans_accumulate_kernel(const float* __restrict__ X,      // [n, d]
                         const int* __restrict__ assign,   // [km_npad(n)]
                         const long n, const int m, const int d,
                         double* __restrict__ partials) {  // [slices, m, d+1]
  constexpr int W = 16 * NDT;
  constexpr int XS = ((W + 31) & ~31) + 16;                // km_acc_str(NDT)
  __shared__ float xs[KM_RCH * XS];
  __shared__ int as[KM_RCH];

  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int l16 = lane & 15, kg = lane >> 4;
  const long slice = blockIdx.x;
  const int cw = blockIdx.y * KM_SLAB + wave * 32;   // the wave's centroids
  const int col0 = blockIdx.z * W;
  const long rbeg = slice * KM_SLICE;
  const long rend = min(n, rbeg + KM_SLICE);

  km_f32x4 acc[2][NDT];
#pragma unroll
  for (int t = 0; t < NDT; ++t) {
    acc[0][t] = {0.f, 0.f, 0.f, 0.f};
    acc[1][t] = {0.f, 0.f, 0.f, 0.f};
  }

  for (long rc = rbeg; rc < rend; rc += KM_RCH) {
    for (int f = tid; f < KM_RCH * W; f += KM_THREADS) {
      const int r = f / W, q = f - r * W;
      const long gr = rc + r;
      const int gcol = col0 + q;
      float v = 0.f;
      if (gr < rend) {
        if (gcol < d) v = X[(size_t)gr * d + gcol];
        else if (gcol == d) v = 1.0f;                // the column that counts
      }
      xs[r * XS + q] = v;
    }
    if (tid < KM_RCH) as[tid] = rc + tid < rend ? assign[rc + tid] : -1;
    __syncthreads();
    if (cw < m) {                                    // wave-uniform
#pragma unroll 4
      for (int ks = 0; ks < KM_RCH / 4; ++ks) {
        const int row = 4 * ks + kg;
        const int c = as[row] - cw - l16;
        const float a0 = c == 0 ? 1.0f : 0.f;
        const float a1 = c == 16 ? 1.0f : 0.f;
        float b[NDT];
#pragma unroll
        for (int t = 0; t < NDT; ++t) b[t] = xs[row * XS + 16 * t + l16];
#pragma unroll
        for (int t = 0; t < NDT; ++t) {
          acc[0][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b[t],
                                                           acc[0][t], 0, 0, 0);
          acc[1][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b[t],
                                                           acc[1][t], 0, 0, 0);
        }
      }
    }
    __syncthreads();
  }

  const int cols = d + 1;
#pragma unroll
  for (int ct = 0; ct < 2; ++ct)
#pragma unroll
    for (int t = 0; t < NDT; ++t) {
      const int col = col0 + 16 * t + l16;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int c = cw + ct * 16 + kg * 4 + r;
        if (c < m && col < cols)
          partials[((size_t)slice * m + c) * cols + col] =
              (double)acc[ct][t][r];
      }
    }
}

// sums[c, j] (j < d) and counts[c] (j = d) = sum over slices, in slice order
__global__ void __launch_bounds__(KM_THREADS)
kmeans_reduce_kernel(const double* __restrict__ partials, const long slices,
                     const int m, const int d, double* __restrict__ sums,
                     double* __restrict__ counts) {
  const size_t total = (size_t)m * (d + 1);
  const size_t idx = (size_t)blockIdx.x * KM_THREADS + threadIdx.x;
  if (idx >= total) return;
  double s = 0.0;
  long b = 0;
  for (; b + 8 <= slices; b += 8) {
    double v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = partials[(size_t)(b + k) * total + idx];
#pragma unroll
    for (int k = 0; k < 8; ++k) s += v[k];
  }
  for (; b < slices; ++b) s += partials[(size_t)b * total + idx];
  const size_t c = idx / (d + 1);
  const int j = (int)(idx - c * (d + 1));
  if (j < d) sums[c * d + j] = s;
  else counts[c] = s;
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------

extern "C" hipError_t launch_kmeans_assign(const float* X, const float* C,
                                           long n, int m, int d, float* c2,
                                           int* assign, hipStream_t stream) {
  if (!kmeans_supported_nmd(n, m, d)) return hipErrorInvalidConfiguration;
  hipLaunchKernelGGL(kmeans_norms_kernel, dim3((unsigned)km_mpad(m)),
                     dim3(64), 0, stream, C, m, d, c2);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return err;
  const int rt = km_row_tiles(n);
  const dim3 grid((unsigned)(km_npad(n) / (64 * rt))), blk(KM_THREADS);
  const size_t lds = km_assign_lds_bytes(64 * rt, d);
  if (rt == 1)
    hipLaunchKernelGGL(kmeans_assign_kernel<1>, grid, blk, lds, stream, X, C,
                       c2, n, m, d, assign);
  else
    hipLaunchKernelGGL(kmeans_assign_kernel<4>, grid, blk, lds, stream, X, C,
                       c2, n, m, d, assign);
  return hipGetLastError();
}

extern "C" hipError_t launch_kmeans_accumulate(const float* X,
                                               const int* assign, long n,
                                               int m, int d, double* partials,
                                               double* sums, double* counts,
                                               hipStream_t stream) {
  if (!kmeans_supported_nmd(n, m, d)) return hipErrorInvalidConfiguration;
  const long slices = km_slices(n);
  const dim3 grid((unsigned)slices, (unsigned)((m + KM_SLAB - 1) / KM_SLAB),
                  (unsigned)km_panels(d));
  const dim3 blk(KM_THREADS);
#define KM_CASE(NDT_)                                                      \
  case NDT_:                                                               \
    hipLaunchKernelGGL((kmeans_accumulate_kernel<NDT_>), grid, blk, 0,     \
                       stream, X, assign, n, m, d, partials);              \
    break
  switch (km_panel_tiles(d)) {
    KM_CASE(1); KM_CASE(2); KM_CASE(3); KM_CASE(4);
    KM_CASE(5); KM_CASE(6); KM_CASE(7); KM_CASE(8);
    default: return hipErrorInvalidConfiguration;
  }
#undef KM_CASE
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return err;
  const size_t total = (size_t)m * (d + 1);
  hipLaunchKernelGGL(kmeans_reduce_kernel,
                     dim3((unsigned)((total + KM_THREADS - 1) / KM_THREADS)),
                     blk, 0, stream, partials, slices, m, d, sums, counts);
  return hipGetLastError();
}

#ifdef __HIP_DEVICE_COMPILE__
#pragma clang attribute pop
#endif

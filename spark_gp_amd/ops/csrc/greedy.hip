// K15 — incremental greedy forward selection (Seeger et al. 2003) for MI355X
// (gfx950, CDNA4): the two device passes of one round.
//
// With mc points selected, every candidate row i carries the columns
//   U[j, i] = (Lmm^-1 c_i)_j  (fp32)      V[j, i] = (Lpd^-1 c_i)_j  (fp64)
// for j < mc, laid out [m, n_pad] so that a round's column is contiguous over
// rows, and the fp64 accumulators p_i = sum_j U^2, q_i = sum_j V^2,
// mu_i = sum_j V[j, i] beta_j.  When x* joins as index mc the host grows the
// two Cholesky factors by one row (a, a_nn of Lmm; l, l_nn of Lpd) and
//
//   pass 1   c_i = amp Kb(q(x_i, x*))            generated here, fp32
//            u_i = (c_i - sum_j U[j, i] a_j) / a_nn  -> U[mc, i],  p_i += u_i^2
//            w_j = sum_i V[j, i] c_i,  cc = sum c_i^2,  cy = sum c_i y_i
//   pass 2   v_i = (c_i - sum_j V[j, i] l_j) / l_nn  -> V[mc, i],  q_i += v_i^2,
//            mu_i += v_i beta_new,  the score delta_i, and its argmax
//
// Both passes are matrix-vector products with a single right-hand side, so
// the matrix cores have nothing to do here: the yardstick is HBM bandwidth,
// n mc (4 + 8 + 8) bytes per round (U once, V twice).
//
// Work split: a block owns GR_ROWS = 512 rows, each lane GR_RPL = 2
// consecutive ones, so a U column is read with 8-byte and a V column with
// 16-byte loads, coalesced across the wave.
//  * Generator: the block's X rows are staged GR_DBLK dims at a time
//    (coalesced) and a thread sums q by differences for one row, the form of
//    cross_kernel_tile_kernel; c goes to LDS for its owner lane and to
//    global [n_pad] for pass 2.
//  * GEMV side (u, v): lanes run along rows; a_j / l_j is wave-uniform and
//    comes from scalar loads; eight columns are loaded ahead of the FMAs that
//    use them, into four independent fp64 accumulators per row.
//  * Transposed side (w): per lane the products of a tile of GR_JT = 8
//    columns with its own rows; one folding butterfly reduces the eight
//    values over the wave (10 shuffles for 8 columns: each of the first three
//    steps halves the values a lane holds); the waves meet in LDS, GR_JCH
//    columns at a time, and are summed in wave order.
// Every sum has a fixed order: per-block partials [blocks, m + 2] are added
// by block index in a second small kernel, the argmax takes the lowest index
// among equal maxima.  No atomics; two runs give the same bits.
//
// Tails are safe by construction: n_pad is a whole number of blocks, rows
// past n carry c = 0 (hence u = v = 0, by induction over rounds, without any
// initialisation of U or V) and never enter the argmax; columns past mc are
// predicated off with a wave-uniform bound and never read.
//
// Geometry and the gate: kernel_geom.h.

#include <hip/hip_runtime.h>
#include <math.h>

// gfx950's packed fp32 arithmetic stays off for all device code of this file
#ifdef __HIP_DEVICE_COMPILE__
#pragma clang attribute push(                                      \
    __attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

#include "kernel_geom.h"
#include "launchers.h"

#define GR_WAVES (GR_THREADS / 64)
#define GR_KU 8   // columns loaded ahead on the GEMV side
static_assert(GR_RPL == 2, "rows of a lane are one float2 / double2");
static_assert(GR_JT == 8, "the folding butterfly is written for 8 columns");

__device__ __forceinline__ double gr_wave_sum(double s) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
  return s;
}

// Sum t[0..8) over the wave; lane L < 8 returns the sum of t[gr_fold_col(L)].
// Step s = 0, 1, 2 pairs lanes that differ in bit s: the lane with the bit
// clear keeps the lower half of its values, its partner the upper half, each
// adding the other's copy.  Three plain steps over bits 3..5 finish.
__device__ __forceinline__ double gr_fold_sum(double (&t)[GR_JT],
                                              const int lane) {
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    const int h = 4 >> s;
    const bool up = (lane >> s) & 1;
#pragma unroll
    for (int k = 0; k < h; ++k) {
      const double mine = up ? t[k + h] : t[k];
      const double theirs = up ? t[k] : t[k + h];
      t[k] = mine + __shfl_xor(theirs, 1 << s, 64);
    }
  }
  double r = t[0];
#pragma unroll
  for (int o = 8; o <= 32; o <<= 1) r += __shfl_xor(r, o, 64);
  return r;
}

__device__ __forceinline__ int gr_fold_col(const int lane) {
  return ((lane & 1) << 2) | (lane & 2) | ((lane >> 2) & 1);
}

// c - sum_{j < mc} S[j, i] b_j for the two rows at Sp = S + i0; T2 is float2
// (U) or double2 (V).  b_j is uniform: scalar loads.
template <typename T2>
__device__ __forceinline__ void gr_gemv(const T2* __restrict__ Sp,
                                        const double* __restrict__ b,
                                        const int mc, const size_t n_pad2,
                                        const double c0, const double c1,
                                        double& r0, double& r1) {
  double acc0[4] = {0.0, 0.0, 0.0, 0.0}, acc1[4] = {0.0, 0.0, 0.0, 0.0};
  int j = 0;
  for (; j + GR_KU <= mc; j += GR_KU) {
    T2 sv[GR_KU];
#pragma unroll
    for (int k = 0; k < GR_KU; ++k) sv[k] = Sp[(size_t)(j + k) * n_pad2];
#pragma unroll
    for (int k = 0; k < GR_KU; ++k) {
      const double bj = b[j + k];
      acc0[k & 3] = fma((double)sv[k].x, bj, acc0[k & 3]);
      acc1[k & 3] = fma((double)sv[k].y, bj, acc1[k & 3]);
    }
  }
  for (; j < mc; ++j) {
    const T2 sv = Sp[(size_t)j * n_pad2];
    const double bj = b[j];
    acc0[0] = fma((double)sv.x, bj, acc0[0]);
    acc1[0] = fma((double)sv.y, bj, acc1[0]);
  }
  r0 = c0 - ((acc0[0] + acc0[1]) + (acc0[2] + acc0[3]));
  r1 = c1 - ((acc1[0] + acc1[1]) + (acc1[2] + acc1[3]));
}

template <int FAM>
__global__ void __launch_bounds__(GR_THREADS)
greedy_pass1_kernel(const float* __restrict__ X,       // [n, d]
                    const float* __restrict__ xstar,   // [d]
                    const float* __restrict__ s2v,     // [d] scale^2
                    const float amp,
                    const double* __restrict__ y,      // [n_pad], 0 past n
                    const double* __restrict__ a,      // [mc]
                    const double a_nn,
                    const long n, const long n_pad, const int d, const int mc,
                    const long pstride,
                    float* U,                          // [m, n_pad]
                    const double* __restrict__ V,      // [m, n_pad]
                    float* __restrict__ c,             // [n_pad]
                    double* __restrict__ p,            // [n_pad]
                    double* __restrict__ partials) {   // [blocks, pstride]
  __shared__ float xs[GR_THREADS][GR_DBLK + 1];
  __shared__ float xss[GR_DBLK], s2s[GR_DBLK];
  __shared__ float cs[GR_ROWS];
  __shared__ double red[GR_WAVES][GR_JCH];

  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const long row0 = (long)blockIdx.x * GR_ROWS;

  // ---- c for the block's rows: a thread per row, GR_THREADS rows a turn ---
  for (int sub = 0; sub < GR_RPL; ++sub) {
    const long r0 = row0 + (long)sub * GR_THREADS;
    float qa = 0.f;
    for (int d0 = 0; d0 < d; d0 += GR_DBLK) {
      const int dl = min(GR_DBLK, d - d0);
      for (int f = tid; f < GR_THREADS * dl; f += GR_THREADS) {
        const int r = f / dl, k = f - r * dl;
        const long gr = r0 + r;
        xs[r][k] = (gr < n) ? X[(size_t)gr * d + d0 + k] : 0.f;
      }
      if (tid < dl) {
        xss[tid] = xstar[d0 + tid];
        s2s[tid] = s2v[d0 + tid];
      }
      __syncthreads();
      for (int k = 0; k < dl; ++k) {
        const float df = xs[tid][k] - xss[k];
        qa += s2s[k] * df * df;
      }
      __syncthreads();
    }
    cs[sub * GR_THREADS + tid] =
        (r0 + tid < n) ? amp * family_kb<FAM>(qa) : 0.f;
  }
  __syncthreads();

  const long i0 = row0 + GR_RPL * tid;
  const float2 cf = *(const float2*)&cs[GR_RPL * tid];
  *(float2*)(c + i0) = cf;
  const double c0 = cf.x, c1 = cf.y;

  // ---- u = (c - U^T a) / a_nn ---------------------------------------------
  {
    double u0, u1;
    gr_gemv<float2>((const float2*)(U + i0), a, mc, (size_t)(n_pad / 2), c0,
                    c1, u0, u1);
    u0 /= a_nn;
    u1 /= a_nn;
    *(float2*)(U + (size_t)mc * n_pad + i0) = make_float2((float)u0, (float)u1);
    double2 pv = *(const double2*)(p + i0);
    pv.x += u0 * u0;
    pv.y += u1 * u1;
    *(double2*)(p + i0) = pv;
  }

  // ---- w_j = sum_i V[j, i] c_i over the block's rows ------------------------
  double* const pout = partials + (size_t)blockIdx.x * pstride;
  const double2* const Vp = (const double2*)(V + i0);
  const size_t vstr = (size_t)(n_pad / 2);
  const int fc = gr_fold_col(lane);
  for (int jc = 0; jc < mc; jc += GR_JCH) {
    const int jend = min(mc, jc + GR_JCH);
    for (int j0 = jc; j0 < jend; j0 += GR_JT) {
      double t[GR_JT];
#pragma unroll
      for (int k = 0; k < GR_JT; ++k) {
        t[k] = 0.0;
        if (j0 + k < jend) {                       // wave-uniform
          const double2 vv = Vp[(size_t)(j0 + k) * vstr];
          t[k] = vv.x * c0 + vv.y * c1;
        }
      }
      const double s = gr_fold_sum(t, lane);
      if (lane < GR_JT && j0 + fc < jend) red[wave][j0 - jc + fc] = s;
    }
    __syncthreads();
    if (tid < jend - jc) {
      double s = red[0][tid];
#pragma unroll
      for (int w = 1; w < GR_WAVES; ++w) s += red[w][tid];
      pout[jc + tid] = s;
    }
    __syncthreads();
  }

  // ---- cc = sum c^2, cy = sum c y -------------------------------------------
  const double2 yv = *(const double2*)(y + i0);
  const double scc = gr_wave_sum(c0 * c0 + c1 * c1);
  const double scy = gr_wave_sum(c0 * yv.x + c1 * yv.y);
  if (lane == 0) {
    red[wave][0] = scc;
    red[wave][1] = scy;
  }
  __syncthreads();
  if (tid < 2) {
    double s = red[0][tid];
#pragma unroll
    for (int w = 1; w < GR_WAVES; ++w) s += red[w][tid];
    pout[mc + tid] = s;
  }
}

// out[j] = sum_b partials[b, j], j < cols, in block order
__global__ void __launch_bounds__(GR_THREADS)
greedy_sum_partials_kernel(const double* __restrict__ partials,
                           const long blocks, const long pstride,
                           const int cols, double* __restrict__ out) {
  const int j = blockIdx.x * GR_THREADS + threadIdx.x;
  if (j >= cols) return;
  double s = 0.0;
  long b = 0;
  for (; b + 8 <= blocks; b += 8) {
    double v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = partials[(size_t)(b + k) * pstride + j];
#pragma unroll
    for (int k = 0; k < 8; ++k) s += v[k];
  }
  for (; b < blocks; ++b) s += partials[(size_t)b * pstride + j];
  out[j] = s;
}

// the larger score, the lower row among equal ones
__device__ __forceinline__ void gr_better(double& v, long long& i,
                                          const double ov,
                                          const long long oi) {
  if (ov > v || (ov == v && oi < i)) {
    v = ov;
    i = oi;
  }
}

__device__ __forceinline__ void gr_block_argmax(double& v, long long& i,
                                                double* redv,
                                                long long* redi) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const double ov = __shfl_xor(v, o, 64);
    const long long oi = __shfl_xor(i, o, 64);
    gr_better(v, i, ov, oi);
  }
  if (lane == 0) {
    redv[wave] = v;
    redi[wave] = i;
  }
  __syncthreads();
  for (int w = 0; w < GR_WAVES; ++w) gr_better(v, i, redv[w], redi[w]);
}

// The selection score of the provider, term for term; NaN -> -inf and an
// infinite score to the largest finite value of its sign (torch.nan_to_num).
__device__ __forceinline__ double gr_score(const double kxx, const double s,
                                           const double sigma2, const double p,
                                           const double q, const double mu,
                                           const double y) {
  const double li = sqrt(kxx - p);
  const double sl = s / li;
  const double sl2 = sl * sl;
  const double xi = 1.0 / (sl2 + 1.0 - q);
  const double kappa = xi * (1.0 + 2.0 * sl2);
  const double r = y - mu;
  const double delta =
      -log(sl) -
      (log(xi) + xi * (1.0 - kappa) / sigma2 * (r * r) - kappa + 2.0) / 2.0;
  if (isnan(delta)) return -HUGE_VAL;
  if (isinf(delta)) return delta > 0.0 ? 1.7976931348623157e308
                                       : -1.7976931348623157e308;
  return delta;
}

__global__ void __launch_bounds__(GR_THREADS)
greedy_pass2_kernel(const float* __restrict__ c,       // [n_pad]
                    const double* __restrict__ y,      // [n_pad]
                    const double* __restrict__ l,      // [mc]
                    const double l_nn, const double beta_new,
                    const double kxx, const double sigma2,
                    const long n, const long n_pad, const int mc,
                    double* V,                         // [m, n_pad]
                    const double* __restrict__ p,      // [n_pad]
                    double* __restrict__ q,            // [n_pad]
                    double* __restrict__ mu,           // [n_pad]
                    double* __restrict__ delta,        // [n_pad]
                    double* __restrict__ bval,         // [blocks]
                    long long* __restrict__ bidx) {    // [blocks]
  __shared__ double redv[GR_WAVES];
  __shared__ long long redi[GR_WAVES];
  const int tid = threadIdx.x;
  const long i0 = (long)blockIdx.x * GR_ROWS + GR_RPL * tid;
  const float2 cf = *(const float2*)(c + i0);

  double v0, v1;
  gr_gemv<double2>((const double2*)(V + i0), l, mc, (size_t)(n_pad / 2),
                   (double)cf.x, (double)cf.y, v0, v1);
  v0 /= l_nn;
  v1 /= l_nn;
  *(double2*)(V + (size_t)mc * n_pad + i0) = make_double2(v0, v1);
  double2 qv = *(const double2*)(q + i0);
  double2 mv = *(const double2*)(mu + i0);
  qv.x += v0 * v0;
  qv.y += v1 * v1;
  mv.x = fma(v0, beta_new, mv.x);
  mv.y = fma(v1, beta_new, mv.y);
  *(double2*)(q + i0) = qv;
  *(double2*)(mu + i0) = mv;

  const double2 pv = *(const double2*)(p + i0);
  const double2 yv = *(const double2*)(y + i0);
  const double s = sqrt(sigma2);
  const double e0 =
      i0 < n ? gr_score(kxx, s, sigma2, pv.x, qv.x, mv.x, yv.x) : -HUGE_VAL;
  const double e1 = i0 + 1 < n
      ? gr_score(kxx, s, sigma2, pv.y, qv.y, mv.y, yv.y) : -HUGE_VAL;
  *(double2*)(delta + i0) = make_double2(e0, e1);

  // rows past n score -inf at an index above every row: they never win
  double bv = e0;
  long long bi = i0;
  gr_better(bv, bi, e1, i0 + 1);
  gr_block_argmax(bv, bi, redv, redi);
  if (tid == 0) {
    bval[blockIdx.x] = bv;
    bidx[blockIdx.x] = bi;
  }
}

// best = (max score, its lowest row as a double) over the per-block results
__global__ void __launch_bounds__(GR_THREADS)
greedy_argmax_kernel(const double* __restrict__ bval,
                     const long long* __restrict__ bidx, const long blocks,
                     double* __restrict__ best) {
  __shared__ double redv[GR_WAVES];
  __shared__ long long redi[GR_WAVES];
  double v = -HUGE_VAL;
  long long i = 0x7fffffffffffffffLL;
  for (long b = threadIdx.x; b < blocks; b += GR_THREADS)
    gr_better(v, i, bval[b], bidx[b]);
  gr_block_argmax(v, i, redv, redi);
  if (threadIdx.x == 0) {
    best[0] = v;
    best[1] = (double)i;
  }
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------

extern "C" hipError_t launch_greedy_pass1(
    const float* X, const float* xstar, const float* s2v, float amp,
    const double* y, const double* a, double a_nn, long n, int d, int mc,
    int m, float* U, const double* V, float* c, double* p, double* partials,
    double* sums, int family, hipStream_t stream) {
  if (!geom_family_ok(family)) return hipErrorInvalidValue;
  if (!greedy_supported_nmd(n, m, d) || mc < 0 || mc >= m)
    return hipErrorInvalidConfiguration;
  const long blocks = gr_blocks(n), n_pad = gr_npad(n);
  const long pstride = gr_pstride(m);
  const dim3 grid((unsigned)blocks), blk(GR_THREADS);
#define GR_CASE(FAM_)                                                       \
  hipLaunchKernelGGL((greedy_pass1_kernel<FAM_>), grid, blk, 0, stream, X,  \
                     xstar, s2v, amp, y, a, a_nn, n, n_pad, d, mc, pstride, \
                     U, V, c, p, partials)
  switch (family) {
    case GEOM_FAM_RBF: GR_CASE(GEOM_FAM_RBF); break;
    case GEOM_FAM_M32: GR_CASE(GEOM_FAM_M32); break;
    default:           GR_CASE(GEOM_FAM_M52); break;
  }
#undef GR_CASE
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return err;
  const int cols = mc + 2;
  hipLaunchKernelGGL(greedy_sum_partials_kernel,
                     dim3((unsigned)((cols + GR_THREADS - 1) / GR_THREADS)),
                     blk, 0, stream, partials, blocks, pstride, cols, sums);
  return hipGetLastError();
}

extern "C" hipError_t launch_greedy_pass2(
    const float* c, const double* y, const double* l, double l_nn,
    double beta_new, double kxx, double sigma2, long n, int mc, int m,
    double* V, const double* p, double* q, double* mu, double* delta,
    double* bval, long long* bidx, double* best, hipStream_t stream) {
  if (!greedy_supported_nmd(n, m, 1) || mc < 0 || mc >= m)
    return hipErrorInvalidConfiguration;
  const long blocks = gr_blocks(n), n_pad = gr_npad(n);
  hipLaunchKernelGGL(greedy_pass2_kernel, dim3((unsigned)blocks),
                     dim3(GR_THREADS), 0, stream, c, y, l, l_nn, beta_new,
                     kxx, sigma2, n, n_pad, mc, V, p, q, mu, delta, bval,
                     bidx);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return err;
  hipLaunchKernelGGL(greedy_argmax_kernel, dim3(1), dim3(GR_THREADS), 0,
                     stream, bval, bidx, blocks, best);
  return hipGetLastError();
}

#ifdef __HIP_DEVICE_COMPILE__
#pragma clang attribute pop
#endif

// Kernel geometry shared by the device code and the host-side gates: the
// LDS budgets of the fused expert kernels and the SYRK tile constants.
// Included by expert_nll.hip, laplace.hip, cross_syrk.hip, predict.hip (hipcc) and by
// bindings.cpp (host compiler), so a *_supported() answer and the launch it
// guards are computed by the same function.
#pragma once
#include <stddef.h>

#ifdef __HIPCC__
#define GEOM_HD __host__ __device__
#else
#define GEOM_HD
#endif

// ---- covariance families (expert_nll.hip, cross_syrk.hip) -----------------
// A kernel is instantiated per family: Kb(q) over the scaled squared distance
// q = ||x'_a - x'_b||^2, t = sqrt(q) (family_kb, family_kb_kd below):
//   RBF         Kb = e^-q                Kd = -dKb/dq = e^-q
//   Matern 3/2  Kb = (1 + t) e^-t        Kd = e^-t / 2
//   Matern 5/2  Kb = (1 + t + t^2/3) e^-t   Kd = (1 + t) e^-t / 6
#define GEOM_FAM_RBF 0
#define GEOM_FAM_M32 1
#define GEOM_FAM_M52 2

static inline bool geom_family_ok(long family) {
  return family >= GEOM_FAM_RBF && family <= GEOM_FAM_M52;
}

#ifdef __HIPCC__
// Kb at a q that may carry a small negative rounding residue
template <int FAM>
__device__ __forceinline__ float family_kb(const float q) {
  const float qc = q > 0.f ? q : 0.f;
  if (FAM == GEOM_FAM_RBF) return __expf(-qc);
  const float t = sqrtf(qc);
  const float e = __expf(-t);
  if (FAM == GEOM_FAM_M32) return (1.0f + t) * e;
  return (1.0f + t + t * t * (1.0f / 3.0f)) * e;
}

// Matern only (FAM is GEOM_FAM_M32 or GEOM_FAM_M52): Kb and Kd from
// t = sqrt(q), one exp for both
template <int FAM>
__device__ __forceinline__ void family_kb_kd(const float t, float& kb,
                                             float& kd) {
  const float e = __expf(-t);
  if (FAM == GEOM_FAM_M32) {
    kb = (1.0f + t) * e;
    kd = 0.5f * e;
  } else {
    kb = (1.0f + t + t * t * (1.0f / 3.0f)) * e;
    kd = (1.0f + t) * e * (1.0f / 6.0f);
  }
}
#endif

// ---- fused expert kernels (expert_nll.hip, laplace.hip) -------------------
// Every LDS region is padded to 16 B so the vectorized dots can assume
// aligned bases.

// row stride of the k x k working buffer: k+1 up to a multiple of 4
static GEOM_HD inline size_t geom_sa(int k) {
  return (size_t)((k + 4) & ~3);
}

// temp buffer: max(k*36, 32*SA, 448) floats
static GEOM_HD inline size_t geom_tsz(int k) {
  size_t t = (size_t)k * 36;
  if (t < 32 * geom_sa(k)) t = 32 * geom_sa(k);
  if (t < 448) t = 448;
  return t;
}

static GEOM_HD inline size_t a16(size_t n) {
  return (n + 15) & ~(size_t)15;
}

// X row stride: 16-B aligned rows
static GEOM_HD inline size_t geom_dp4(int d) {
  return (size_t)((d + 4) & ~3);
}

// temp buffer of fused_expert_nll_kernel, in floats: only the terms its own
// phases use (geom_tsz's 32*SA term is laplace.hip's).  The 8x8 inverses
// Vq of a diagonal block take 256 of a floor of 448 (the rest was the
// earlier assembly's scratch; the floor stays, and with it the LDS plan
// and chol_invert_lower's contract); the C2 panel copy and D's U: (k-32) rows of stride 36; H's
// per-row-tile partials: ceil(k/16)*d.
static GEOM_HD inline size_t nll_tsz(int k, int d) {
  size_t t = 448;
  if (k > 32 && t < (size_t)(k - 32) * 36) t = (size_t)(k - 32) * 36;
  const size_t h = (size_t)((k + 15) / 16) * (size_t)d;
  if (t < h) t = h;
  return t;
}

// Phase B of fused_expert_nll_kernel stages the scaled features in the
// front of the k x SA working buffer, which nothing has written yet, in
// column slabs: the slab width in columns, a multiple of 16 with rows of
// stride width + 4 <= SA.  0 selects the global-fragment form, for shapes
//  - where not even one 16-column slab fits (k < 16), or
//  - where no wave has more than one tile and no tile more than one
//    16-index chunk: the global form then pays a single load latency, and
//    staging would only add a barrier to it ((32, 8) is such a shape).
static GEOM_HD inline int nll_bslab(int k, int d) {
  const int nt = (k + 15) / 16;
  if (nt * (nt + 1) / 2 <= 8 && d <= 16) return 0;
  const int fit = (((int)geom_sa(k) - 4) / 16) * 16;
  const int all = (d + 15) & ~15;
  return all < fit ? all : fit;
}

// LDS bytes of fused_expert_nll_kernel; region order is NllLds's carve.
// The scaled features have no region of their own: phase B stages them
// inside A before anything else is written there (nll_bslab) and phase H
// reads its MFMA fragments from global X.  That is what lets three experts
// share a CU at k = 100: 53 344 B against floor(160 KiB / 3) = 54 613 B.
static GEOM_HD inline size_t nll_lds_bytes(int k, int d) {
  size_t off = 0;
  off += a16(sizeof(double) * 10);                      // red + misc
  off += a16(sizeof(float) * (size_t)k * geom_sa(k));   // A
  off += a16(sizeof(float) * nll_tsz(k, d));            // T
  off += 4 * a16(sizeof(float) * k);                    // yb alpha tvec rrow
  off += 2 * a16(sizeof(float) * d);                    // s2 sc
  off += 16;                                            // bad (+pad)
  return off;
}

// LDS bytes of fused_laplace_kernel<ev>; region order is lap_carve's
static GEOM_HD inline size_t lap_lds_bytes(int k, int d, int ev = 0) {
  size_t off = a16(sizeof(double) * 10);
  off += a16(sizeof(float) * (size_t)k * geom_sa(k));   // A
  off += a16(sizeof(float) * (size_t)k * geom_dp4(d));  // X
  off += a16(sizeof(float) * geom_tsz(k));
  off += 8 * a16(sizeof(float) * k);
  off += a16(sizeof(float) * d);
  if (ev) {
    off += 2 * a16(sizeof(float) * k);        // vv + s2v
    off += a16(sizeof(float) * d);            // betav
    off += a16(sizeof(double) * (d + 2));     // gout
  }
  off += 16;
  return off;
}

#define GEOM_LDS_MAX (160 * 1024)   // LDS per workgroup on gfx950

// ---- fused prediction (predict.hip) ---------------------------------------
// One block owns a tile of TR test rows and keeps their whole fp32 cross
// row c[TR][m] in LDS; TR is the largest of 64 / 32 / 16 whose plan fits.
#define PP_THREADS 512   // 8 waves
#define PP_DBLK 32       // feature dims staged per pass
#define PP_CB 128        // active-set rows staged per pass

// m up to the 16-column MFMA tile; columns [m, mp) of c are zero
static GEOM_HD inline int pp_mp(int m) {
  return (m + 15) & ~15;
}

// row stride of the c tile in floats.  = 2 (mod 4): the A-fragment read
// c[i][k0 + (l>>4)], i = l&15, then touches bank 2 i u + (l>>4) (mod 32)
// with u odd: 32 distinct banks in each 32-lane group.
static GEOM_HD inline int pp_cstr(int m) {
  return pp_mp(m) + 2;
}

// LDS bytes of ppa_predict_kernel<., ., TR>; region order is its carve
static GEOM_HD inline size_t pp_lds_bytes(int tr, int m) {
  size_t off = 0;
  off += a16(sizeof(double) * (PP_THREADS / 64) * (size_t)tr);   // red
  off += a16(sizeof(float) * (size_t)tr * pp_cstr(m));           // c
  off += a16(sizeof(float) * PP_CB * (PP_DBLK + 1));             // as
  off += a16(sizeof(float) * (size_t)tr * (PP_DBLK + 1));        // xs
  off += a16(sizeof(float) * PP_DBLK);                           // s2
  return off;
}

#define PP_M_MAX 4096   // keeps every size above far inside int range

// rows per block for an active set of m points: 64, 32 or 16; 0 if even
// 16 rows do not fit.  d never enters: the features are staged PP_DBLK at
// a time and the running q lives in the c tile.
static GEOM_HD inline int pp_tile_rows(long m) {
  if (m < 1 || m > PP_M_MAX) return 0;
  for (int tr = 64; tr >= 16; tr >>= 1)
    if (pp_lds_bytes(tr, (int)m) <= GEOM_LDS_MAX) return tr;
  return 0;
}

static GEOM_HD inline bool ppa_predict_supported_md(long m, long d) {
  return d >= 1 && d <= 65536 && pp_tile_rows(m) != 0;
}

// ---- SYRK kernels (cross_syrk.hip) ----------------------------------------
#define SY_CT 256     // output tile edge (per block)
#define SY_BK 32      // k rows per staged block
#define SF_DMAX 32    // syrk_fused_gen: d-slots per row that fit its LDS
// syrk_fused_gen's f16 generator takes scaled coordinates below this bound
// (half the f16 range, 65504); above it the fp32 generator runs
#define SF_F16_ABS_LIMIT 32768.0

// syrk_fused_gen's partial tiles: one SY_CT x SY_CT fp32 tile per (k-slice
// with rows, upper-triangle tile), slice-major
static GEOM_HD inline size_t sf_partial_offset(int slice, int tile,
                                               int tiles) {
  return ((size_t)slice * tiles + tile) * (SY_CT * SY_CT);
}

// floats of that buffer for a chunk of c rows: the slices with rows are the
// first ceil(kblocks / per) of split_k, per = ceil(kblocks / split_k)
static GEOM_HD inline size_t sf_partial_floats(long c, long m, long split_k) {
  const long kblocks = (c + SY_BK - 1) / SY_BK;
  if (kblocks < 1 || split_k < 1) return 0;
  const long per = (kblocks + split_k - 1) / split_k;
  const long ntile = (m + SY_CT - 1) / SY_CT;
  return sf_partial_offset((int)((kblocks + per - 1) / per), 0,
                           (int)(ntile * (ntile + 1) / 2));
}

// largest lower-triangle tile set the split-k family (syrk_bf16,
// syrk_fused_gen) takes; larger sets go to the k-synchronized kernel
#define SY_SPLITK_MAX_TILES 256

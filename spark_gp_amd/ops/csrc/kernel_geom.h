// Kernel geometry shared by the device code and the host-side gates: the
// LDS budgets of the fused expert kernels and the SYRK tile constants.
// Included by expert_nll.hip, expert_nll_panel.hip, expert_nll_f64.hip,
// laplace.hip,
// cross_syrk.hip, predict.hip,
// predict_wide.hip, greedy.hip, kmeans.hip, ppa_fp64.hip (hipcc) and by
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

// ---- response links of the fused Laplace kernels (laplace_link.h) ---------
#define LAP_LINK_LOGISTIC 0
#define LAP_LINK_PROBIT 1

static inline bool lap_link_ok(long link) {
  return link == LAP_LINK_LOGISTIC || link == LAP_LINK_PROBIT;
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

// ---- streamed-feature Laplace kernel (laplace_wide.hip) -------------------
// fused_laplace_kernel<ev, RBF, WIDE>: lap_lds_bytes without the k x dp4 block
// of X and without a per-dimension region other than betav.  X passes
// through two slab buffers of k rows by LAPW_SW columns (row stride
// LAPW_SS = width + 4 floats: 16-B aligned rows, conflict-free fragment
// reads); s2 is folded into the staging of the Kb cache (the scale is read
// with the slab), and the d beta entries of gout accumulate in the output row
// itself, so gout keeps only the amplitude and noise slots.
//   (k, d) = (100, 784), ev: 79 248 B  -> two workgroups per CU (<= 80 KiB)
//   (k, d) = (128, 1024), ev: 115 824 B -> one workgroup per CU
#define LAPW_SW 16
#define LAPW_SS (LAPW_SW + 4)
#define LAPW_D_MAX 1024

// floats of one slab buffer
static GEOM_HD inline size_t lapw_slab_floats(int k) {
  return a16(sizeof(float) * (size_t)k * LAPW_SS) / sizeof(float);
}

// region order is lap_carve<ev, true>'s
static GEOM_HD inline size_t lapw_lds_bytes(int k, int d, int ev = 0) {
  size_t off = a16(sizeof(double) * 10);
  off += a16(sizeof(float) * (size_t)k * geom_sa(k));   // A
  off += 2 * sizeof(float) * lapw_slab_floats(k);       // slabs
  off += a16(sizeof(float) * geom_tsz(k));
  off += 8 * a16(sizeof(float) * k);
  if (ev) {
    off += 2 * a16(sizeof(float) * k);        // vv + s2v
    off += a16(sizeof(float) * d);            // betav
    off += a16(sizeof(double) * 2);           // gout: amp, noise
  }
  off += 16;
  return off;
}

static GEOM_HD inline bool lapw_supported(long k, long d, int ev) {
  return k >= 1 && k <= 128 && d >= 1 && d <= LAPW_D_MAX &&
         lapw_lds_bytes((int)k, (int)d, ev) <= GEOM_LDS_MAX;
}

// ---- fp64 expert kernel (expert_nll_f64.hip) ------------------------------
// The whole kp x kp fp64 matrix of an expert in LDS (kp: k up to whole
// 16-row MFMA tiles, the padding an identity), factored by 16-column blocks.
#define NLF_K_MAX 128
#define NLF_D_MAX 128
#define NLF_TB 16                 // block width = the 16x16x4 f64 MFMA tile
#define NLF_XC 16                 // feature columns of a staged slab of x'
// slab row stride in doubles, = 2 (mod 4) like nllf64_sa: the 16-row by
// 2-column fragment read of a 32-lane group covers the 64 banks once
#define NLF_XS (NLF_XC + 2)

static GEOM_HD inline int nllf64_kp(int k) {
  return (k + NLF_TB - 1) / NLF_TB * NLF_TB;
}

// row stride of the matrix in doubles: kp + 2 = 2 (mod 4)
static GEOM_HD inline int nllf64_sa(int k) {
  return nllf64_kp(k) + 2;
}

// LDS bytes of fused_expert_nll_f64_kernel; region order is f64_carve's.
// 102 KB at (100, 32), 159 840 B at (128, 128): every k <= 128, d <= 128
// fits (the kernel's registers keep it at one workgroup per CU anyway).
static GEOM_HD inline size_t nllf64_lds_bytes(int k, int d) {
  const size_t kp = (size_t)nllf64_kp(k);
  size_t off = 0;
  off += a16(sizeof(double) * 10);                          // red
  off += a16(sizeof(double) * kp * (size_t)nllf64_sa(k));   // A
  off += a16(sizeof(double) * kp * NLF_XS);                 // T
  off += a16(sizeof(double) * (NLF_K_MAX / NLF_TB) * NLF_XC);   // Hp
  off += a16(sizeof(double) * d);                           // hs
  off += 5 * a16(sizeof(double) * kp);         // yb alpha tvec rrow nrm
  off += a16(sizeof(double) * d);                           // sc
  off += 16;                                                // bad (+pad)
  return off;
}

static GEOM_HD inline bool nllf64_supported(long k, long d) {
  return k >= 1 && k <= NLF_K_MAX && d >= 1 && d <= NLF_D_MAX &&
         nllf64_lds_bytes((int)k, (int)d) <= GEOM_LDS_MAX;
}

// ---- panel expert kernel (expert_nll_panel.hip) ---------------------------
// For experts past the resident kernel's LDS plan: persistent workgroups, the
// kp x kp matrix of the expert a workgroup is on in its slab of a global
// scratch [grid, kp, kp] (kp: k up to whole super-blocks of sb rows, the
// padding an identity), every phase a sequence of sb x sb block products
// whose operands pass through LDS NLP_KC contraction indices at a time.
#define NLP_K_MIN 129
#define NLP_K_MAX 1024
#define NLP_D_MAX 128
#define NLP_KC 32                 // contraction depth of a staged chunk
// chunk row stride, = 2 (mod 4): 32 distinct banks per 32-lane group of a
// fragment read (pp_cstr's argument)
#define NLP_KS (NLP_KC + 2)
#define NLP_WT 64                 // tile edge of the elementwise phase W
// the scratch of one launch stays under this many bytes (the grid is cut to
// fit): 256 slabs at k = 1024
#define NLP_SCRATCH_MAX_BYTES ((size_t)1 << 30)

static GEOM_HD inline bool nlp_sb_ok(long sb) { return sb == 64 || sb == 128; }

// super-block rows where the caller names none.  Measured at d = 32 over 1M
// rows (profiles/PROFILES.md round 17): 64 is 4 % faster at k = 256, 128 is
// 8 % faster at k = 512 and 17 % at k = 1000 (half the staged bytes per
// flop).  Between 256 and 512 the rule is not measured.
static GEOM_HD inline int nlp_sb_default(long k) { return k <= 256 ? 64 : 128; }

static GEOM_HD inline bool nlp_supported_kd(long k, long d) {
  return k >= NLP_K_MIN && k <= NLP_K_MAX && d >= 1 && d <= NLP_D_MAX;
}

static GEOM_HD inline int nlp_kp(int k, int sb) {
  return (k + sb - 1) / sb * sb;
}

// floats of the block buffer: the leaf's sb x (sb + 4) diagonal block, or
// phase W's transposed tile
static GEOM_HD inline size_t nlp_pbuf_floats(int sb) {
  const size_t p = (size_t)sb * geom_sa(sb), w = NLP_WT * (NLP_WT + 1);
  return p > w ? p : w;
}

// chol_invert_lower's temp for an sb-row block
static GEOM_HD inline size_t nlp_tsz(int sb) {
  const size_t t = (size_t)(sb - 32) * 36;
  return t > 448 ? t : 448;
}

// LDS bytes of fused_expert_nll_panel_kernel; region order is its carve
static GEOM_HD inline size_t nlp_lds_bytes(int sb, int k, int d) {
  const int kp = nlp_kp(k, sb);
  size_t off = 0;
  off += a16(sizeof(double) * 10);                       // red + misc
  off += a16(sizeof(double) * NLP_D_MAX);                // hs
  off += a16(sizeof(float) * nlp_pbuf_floats(sb));       // P
  off += a16(sizeof(float) * nlp_tsz(sb));               // T
  off += 2 * a16(sizeof(float) * (size_t)sb * NLP_KS);   // As Bs
  off += a16(sizeof(float) * (size_t)(sb / 16) * sb);    // Hp
  off += 5 * a16(sizeof(float) * kp);          // yb alpha tvec rrow nrm
  off += 2 * a16(sizeof(float) * d);                     // sc s2
  off += 16;                                             // bad (+pad)
  return off;
}

static GEOM_HD inline size_t nlp_slab_floats(int k, int sb) {
  return (size_t)nlp_kp(k, sb) * (size_t)nlp_kp(k, sb);
}

// workgroups of one launch over E experts: at most what the device keeps
// resident, what NLP_SCRATCH_MAX_BYTES holds, and max_blocks if > 0
static GEOM_HD inline long nlp_grid(long E, long resident, long max_blocks,
                                    int k, int sb) {
  long g = E;
  if (g > resident) g = resident;
  const long fit = (long)(NLP_SCRATCH_MAX_BYTES /
                          (nlp_slab_floats(k, sb) * sizeof(float)));
  if (g > fit) g = fit;
  if (max_blocks > 0 && g > max_blocks) g = max_blocks;
  return g;
}

// floats of the scratch of a launch of `grid` workgroups: never grows with E
static GEOM_HD inline size_t nlp_scratch_floats(long grid, int k, int sb) {
  return (size_t)grid * nlp_slab_floats(k, sb);
}

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

// ---- wide fused prediction (predict_wide.hip) -----------------------------
// For active sets past the narrow kernel's LDS plan: persistent blocks take
// row tiles of PPW_R rows, a tile's fp32 cross rows c[PPW_R][mp] live in the
// block's slab of a global scratch buffer [grid, PPW_R, mp], and LDS holds
// the double-buffered PPW_P x PPW_W panels of M that the block's waves share.
#define PPW_R 128        // rows per tile: a 16-row MFMA slab per wave
#define PPW_P 64         // k depth of a staged M panel (4 k blocks of 16)
#define PPW_W 64         // its columns: 4 MFMA column tiles per wave
// panel row stride in doubles, = 4 (mod 8): the B-fragment read
// Ms[4 (l>>4) + s][16 b + (l&15)] of a wave is 4 rows of 16 contiguous
// doubles; rows 4 apart then start 32 words apart modulo 64, so the two rows
// of a 32-lane group fall on disjoint halves of 64 banks
#define PPW_MSTR (PPW_W + 4)
#define PPW_M_MAX 8192
static_assert(PPW_R == 16 * (PP_THREADS / 64), "a 16-row slab per wave");
static_assert(PPW_P == PPW_W, "a column panel's first k panel is its diagonal");
static_assert(PPW_P * PPW_W % PP_THREADS == 0, "panel staged in whole passes");

// LDS bytes of ppa_predict_wide_kernel; region order is its carve.  No term
// depends on m or d.
static GEOM_HD inline size_t ppw_lds_bytes() {
  size_t off = 0;
  off += a16(sizeof(double) * 2 * PPW_P * PPW_MSTR);              // M panels
  off += a16(sizeof(float) * PP_CB * (PP_DBLK + 1));              // as
  off += a16(sizeof(float) * PPW_R * (PP_DBLK + 1));              // xs
  off += a16(sizeof(float) * PP_DBLK);                            // s2
  return off;
}

static GEOM_HD inline bool ppa_predict_wide_supported_md(long m, long d) {
  return d >= 1 && d <= 65536 && m >= 1 && m <= PPW_M_MAX &&
         ppw_lds_bytes() <= GEOM_LDS_MAX;
}

// blocks of one launch over t rows on a device of `cus` compute units (one
// block per unit: its LDS plan and 512 threads leave room for no second);
// max_blocks > 0 caps it.  0 for t = 0.
static GEOM_HD inline long ppw_grid(long t, long cus, long max_blocks) {
  long g = (t + PPW_R - 1) / PPW_R;
  if (g > cus) g = cus;
  if (max_blocks > 0 && g > max_blocks) g = max_blocks;
  return g;
}

// floats of the scratch buffer of a launch of `grid` blocks: bounded by the
// grid, never by t
static GEOM_HD inline size_t ppw_scratch_floats(long grid, int m) {
  return (size_t)grid * PPW_R * (size_t)pp_mp(m);
}

// ---- greedy forward selection (greedy.hip) --------------------------------
// A block owns GR_ROWS candidate rows, GR_RPL consecutive ones per lane; the
// per-candidate state is laid out [m, n_pad] (a round's column contiguous
// over rows) with n_pad a whole number of blocks, so the streaming loops
// carry no row bound.
#define GR_THREADS 256   // 4 waves
#define GR_RPL 2         // rows per lane: 8-byte U loads, 16-byte V loads
#define GR_ROWS (GR_THREADS * GR_RPL)
#define GR_DBLK 16       // feature dims staged per pass of the generator
#define GR_JT 8          // V columns per cross-lane reduction
#define GR_JCH 256       // V columns whose per-wave sums LDS holds at a time
#define GR_M_MAX 8192
static_assert(GR_JCH % GR_JT == 0 && GR_JCH <= GR_THREADS,
              "a chunk is whole tiles, and one thread sums a column");

static GEOM_HD inline long gr_blocks(long n) {
  return (n + GR_ROWS - 1) / GR_ROWS;
}

static GEOM_HD inline long gr_npad(long n) {
  return gr_blocks(n) * GR_ROWS;
}

// doubles per block of the pass-1 partials: w [m], then sum c^2 and sum c y
static GEOM_HD inline long gr_pstride(long m) {
  return m + 2;
}

static GEOM_HD inline bool greedy_supported_nmd(long n, long m, long d) {
  return n >= 1 && n <= 0x7fffffffL - GR_ROWS && m >= 1 && m <= GR_M_MAX &&
         d >= 1 && d <= 65536;
}

// device bytes of the state of a selection of m points among n rows: U fp32
// and V fp64 [m, n_pad], the row vectors c (fp32) and y, p, q, mu, delta
// (fp64), the pass-1 partials and the per-block argmax
static GEOM_HD inline size_t gr_state_bytes(long n, long m) {
  const size_t np = (size_t)gr_npad(n), nb = (size_t)gr_blocks(n);
  return np * (size_t)m * (sizeof(float) + sizeof(double)) +
         np * (sizeof(float) + 5 * sizeof(double)) +
         nb * (size_t)gr_pstride(m) * sizeof(double) +
         nb * (sizeof(double) + sizeof(long long));
}

// ---- k-means Lloyd step (kmeans.hip) --------------------------------------
// Assign: a block owns KM_ROWS rows (a 64-row group of four 16-row MFMA
// tiles per wave) and walks the centroids in panels of KM_PANEL, KM_DBLK
// dims at a time.  Accumulate: a block owns KM_SLAB centroids (32 per wave),
// a panel of up to KM_DPANEL of the d + 1 columns (the dims, then the ones
// column that counts) and one slice of KM_SLICE rows, staged KM_RCH rows at
// a time.  Every grid depends on (n, m, d) and these constants only.
#define KM_THREADS 256   // 4 waves
#define KM_ROWS 256
#define KM_PANEL 64
#define KM_DBLK PP_DBLK
// The assign kernel keeps its X tile in LDS across panels up to this many
// (KM_DBLK-padded) dims: 256 x 66 x 4 B + the panel = 76 KiB, two blocks per
// CU.  Above it the tile is staged again for every panel.
#define KM_XRES_DMAX 64
// LDS row stride of the assign kernel's X tile (dp dims wide) and centroid
// panel.  = 2 (mod 4): a fragment read t[i][k0 + (l>>4)], i = l&15, touches
// bank 2 i u + (l>>4) (mod 32) with u odd, 32 distinct banks in each 32-lane
// group (pp_cstr's argument).
#define KM_STR(dp) ((dp) + 2)
#define KM_SLAB 128
#define KM_DPANEL 128
#define KM_RCH 128
#define KM_SLICE 2048    // rows of one fp32 accumulation: exact counts < 2^24
#define KM_M_MAX 8192
static_assert(KM_ROWS == 64 * (KM_THREADS / 64), "a 64-row group per wave");
static_assert(KM_SLAB == 32 * (KM_THREADS / 64), "32 centroids per wave");
static_assert(KM_SLICE % KM_RCH == 0 && KM_RCH % 4 == 0, "whole k steps");

static GEOM_HD inline long km_blocks(long n) {
  return (n + KM_ROWS - 1) / KM_ROWS;
}

// elements of assign: n up to whole row tiles, -1 past n
static GEOM_HD inline long km_npad(long n) {
  return km_blocks(n) * KM_ROWS;
}

// elements of the centroid norms: m up to whole panels, +inf past m
static GEOM_HD inline int km_mpad(int m) {
  return (m + KM_PANEL - 1) / KM_PANEL * KM_PANEL;
}

// dims of the assign kernel's LDS X tile: all of d (padded) while resident
static GEOM_HD inline int km_xdims(int d) {
  const int dp = (d + KM_DBLK - 1) / KM_DBLK * KM_DBLK;
  return dp <= KM_XRES_DMAX ? dp : KM_DBLK;
}

// 16-row tiles per wave of the assign kernel: below KM_SMALL_N rows 256-row
// tiles make fewer than 256 blocks, so a block takes 64 rows.  A function of
// n alone, and a row's scores do not depend on the tiling.
#define KM_SMALL_N 65536
static GEOM_HD inline int km_row_tiles(long n) {
  return n <= KM_SMALL_N ? 1 : 4;
}

// LDS bytes of kmeans_assign_kernel on `rows` rows; region order is its carve
static GEOM_HD inline size_t km_assign_lds_bytes(int rows, int d) {
  return a16(sizeof(float) * rows * KM_STR(km_xdims(d))) +
         a16(sizeof(float) * KM_PANEL * KM_STR(KM_DBLK));
}

static GEOM_HD inline long km_slices(long n) {
  return (n + KM_SLICE - 1) / KM_SLICE;
}

// the d + 1 columns of the accumulate kernel in 16-column MFMA tiles, split
// evenly over the fewest panels of at most KM_DPANEL columns
static GEOM_HD inline int km_panels(int d) {
  return (d + 1 + KM_DPANEL - 1) / KM_DPANEL;
}

static GEOM_HD inline int km_panel_tiles(int d) {
  const int tiles = (d + 1 + 15) / 16, panels = km_panels(d);
  return (tiles + panels - 1) / panels;
}

// LDS row stride of the accumulate kernel's X chunk of ndt column tiles.
// = 16 (mod 32): the B-fragment read xs[k0 + (l>>4)][j0 + (l&15)] of a
// 32-lane group is two rows of 16 contiguous floats that start 16 banks
// apart, 32 distinct banks.
static GEOM_HD inline int km_acc_str(int ndt) {
  return ((16 * ndt + 31) & ~31) + 16;
}

// doubles of the accumulate kernel's partials: [slices, m, d + 1]
static GEOM_HD inline size_t km_partial_doubles(long n, long m, long d) {
  return (size_t)km_slices(n) * (size_t)m * (size_t)(d + 1);
}

// d: no register or LDS plan depends on it (the assign kernel walks it in
// chunks, the accumulate kernel in panels over the grid's z), so the bound
// is the 65535 panels of a grid, cut to the 65536 of the other gates
static GEOM_HD inline bool kmeans_supported_nmd(long n, long m, long d) {
  return n >= 1 && n <= 0x7fffffffL - KM_ROWS && m >= 1 && m <= KM_M_MAX &&
         d >= 1 && d <= 65536;
}

// ---- SYRK kernels (cross_syrk.hip) ----------------------------------------
#define SY_CT 256    // output tile edge (per block)
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

// ---- fp64 PPA accumulation (ppa_fp64.hip) ---------------------------------
// KK += K^T K on the f64 matrix cores: a block owns one PF_TILE x PF_TILE
// tile of the lower triangle and one of split_k row slices, and walks its
// rows PF_BK at a time through two [PF_BK, PF_TILE] fp64 operand windows.
#define PF_THREADS 256   // 2 x 2 waves, 64 x 64 outputs each
#define PF_TILE 128
#define PF_BK 32
#define PF_DMAX 32       // generating feeder: dims of the A windows in LDS
#define PF_XSTR (PF_DMAX + 1)   // their row stride: bank = row + q (mod 32)
#define PF_M_MAX 8192    // the bound of big_chol, which consumes KK

static GEOM_HD inline long pf_windows(long m) {
  return (m + PF_TILE - 1) / PF_TILE;
}

// lower-triangle tiles, diagonal included
static GEOM_HD inline long pf_tiles(long m) {
  return pf_windows(m) * (pf_windows(m) + 1) / 2;
}

// doubles one row slice leaves in the partials: a full tile per output tile,
// then PF_TILE column sums (Ky) per window
static GEOM_HD inline size_t pf_slice_doubles(long m) {
  return (size_t)pf_tiles(m) * PF_TILE * PF_TILE +
         (size_t)pf_windows(m) * PF_TILE;
}

// doubles of the partials of a launch; split_k = 1 adds into KK itself
static GEOM_HD inline size_t pf_partial_doubles(long m, long split_k) {
  return split_k > 1 ? (size_t)split_k * pf_slice_doubles(m) : 0;
}

static GEOM_HD inline bool ppa_fp64_supported_md(long m, long d) {
  return m >= 1 && m <= PF_M_MAX && d >= 1 && d <= 65536;
}

// The host-callable launcher of every kernel, declared once.  Included by
// bindings.cpp (the only caller) and by each .hip file that defines one, so
// a launcher whose parameters drift from its declaration fails to compile
// ("conflicting types") instead of linking silently through C linkage.
// Host-safe: no device code, no HIP language extensions.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

// `family`: a GEOM_FAM_* code of kernel_geom.h; a launcher given an unknown
// one returns hipErrorInvalidValue.

// ---- expert_nll.hip -------------------------------------------------------
hipError_t launch_fused_expert_nll(
    const float* X, const float* y, const float* scale, float amp,
    float noise, int E, int k, int d, double* out_nll, double* out_sumW0,
    double* out_trG, double* out_contr, int* out_bad,
    unsigned long long* out_clk, int family, hipStream_t stream);

hipError_t fused_expert_nll_resident_wgs(int k, int d, int family, int* out);

// ---- expert_nll_panel.hip -------------------------------------------------
// 128 < k <= 1024 (nlp_supported_kd).  scratch: nlp_scratch_floats(grid, k,
// sb) floats for 1 <= grid <= E persistent workgroups; sb: the super-block,
// 64 or 128.  An unknown sb is answered like an unknown family.
hipError_t launch_fused_expert_nll_panel(
    const float* X, const float* y, const float* scale, float amp,
    float noise, int E, int k, int d, float* scratch, int grid, int sb,
    double* out_nll, double* out_sumW0, double* out_trG, double* out_contr,
    int* out_bad, int family, hipStream_t stream);

hipError_t fused_expert_nll_panel_resident_wgs(int k, int d, int family,
                                               int sb, int* out);

// ---- expert_nll_f64.hip ---------------------------------------------------
// The outputs of launch_fused_expert_nll in full fp64, k <= 128 and d <= 128
// (nllf64_supported).  X: [E, k, d] floats, or doubles with x_is_f64.
hipError_t launch_fused_expert_nll_f64(
    const void* X, int x_is_f64, const double* y, const double* scale,
    double amp, double noise, int E, int k, int d, double* out_nll,
    double* out_sumW0, double* out_trG, double* out_contr, int* out_bad,
    int family, hipStream_t stream);

// ---- laplace.hip ----------------------------------------------------------
// `link`: a LAP_LINK_* code of kernel_geom.h.  (These two answer an unknown
// family or link, and a Matern family under the probit link, like an
// unsupported (k, d): with hipErrorInvalidConfiguration.)
hipError_t launch_fused_laplace_newton(
    const float* X, const float* y, float* f, const float* scale, float amp,
    float noise, int E, int k, int d, double tol, int max_newton,
    double* out_psi, double* out_sumlogl, int* out_iters, int* out_bad,
    int family, int link, hipStream_t stream);

hipError_t launch_fused_laplace_evidence(
    const float* X, const float* y, float* f, const float* scale, float amp,
    float noise, int E, int k, int d, double tol, int max_newton,
    double* out_psi, double* out_sumlogl, int* out_iters, int* out_bad,
    double* out_logz, double* out_grad, int family, int link,
    hipStream_t stream);

// ---- laplace_wide.hip -----------------------------------------------------
// The two above for the RBF family with X streamed: 1 <= k <= 128 and
// 1 <= d <= 1024 (lapw_supported); hipErrorInvalidConfiguration otherwise,
// and for an unknown link.
hipError_t launch_fused_laplace_newton_wide(
    const float* X, const float* y, float* f, const float* scale, float amp,
    float noise, int E, int k, int d, double tol, int max_newton,
    double* out_psi, double* out_sumlogl, int* out_iters, int* out_bad,
    int link, hipStream_t stream);

hipError_t launch_fused_laplace_evidence_wide(
    const float* X, const float* y, float* f, const float* scale, float amp,
    float noise, int E, int k, int d, double tol, int max_newton,
    double* out_psi, double* out_sumlogl, int* out_iters, int* out_bad,
    double* out_logz, double* out_grad, int link, hipStream_t stream);

hipError_t fused_laplace_wide_resident_wgs(int k, int d, int* out);

// ---- cross_syrk.hip -------------------------------------------------------
hipError_t launch_cross_kernel_tile(
    const float* X, const float* A, const float* s2v, float amp, int c,
    int m, int d, void* out, void* out_lo, void* out_t, void* out_lo_t,
    int out_is_bf16, const float* yv, double* Ky, int family,
    hipStream_t stream);

hipError_t launch_cross_mfma(const float* Xs, const float* As,
                             const float* nx, const float* na, float amp,
                             int c, int m, int d, void* out_bfT,
                             void* out_loT, const float* yv, double* Ky,
                             int family, hipStream_t stream);

hipError_t launch_syrk_bf16(const void* KcT, const void* KlT, int c, int m,
                            int cpitch, int split_k, float* KK,
                            hipStream_t stream);

hipError_t launch_syrk_bf16_sync(const void* KcT, const void* KlT, int c,
                                 int m, int cpitch, const int* tiles, int nb,
                                 int kpb, int* phase_ctr, int nactive,
                                 float* KK, hipStream_t stream);

hipError_t launch_syrk_fused_gen(
    const float* Xs, const float* As, const float* nx, const float* na,
    float amp, const float* yv, int c, int m, int d, int split_k,
    double* Ky, float* KK, float* partials, int family, int gen_f16,
    hipStream_t stream);   // partials: sf_partial_floats(c, m, split_k)

hipError_t launch_colsum_gemv(const void* Kc, const float* y, int c, int m,
                              double* Ky, hipStream_t stream);

// ---- ppa_fp64.hip ---------------------------------------------------------
// KK [m, m] += K^T K and Ky [m] += K^T y in fp64, m <= PF_M_MAX.  A given:
// K is generated from the rows X [c, d], d <= PF_DMAX; A == nullptr: X is
// the fp32 chunk K [c, m] itself.  partials: pf_partial_doubles(m, split_k)
// doubles of scratch (none at split_k = 1).
hipError_t launch_ppa_fp64(
    const float* X, const float* A, const float* s2v, float amp,
    const float* yv, int c, int m, int d, int split_k, double* Ky, double* KK,
    double* partials, int family, hipStream_t stream);

// ---- predict.hip ----------------------------------------------------------
// var == nullptr: mean only (M is then not read)
hipError_t launch_ppa_predict(
    const float* X, const float* A, const float* s2v, float amp,
    const double* mv, const double* M, double kxx, long t, int m, int d,
    double* mean, double* var, int family, hipStream_t stream);

// ---- predict_wide.hip -----------------------------------------------------
// scratch: ppw_scratch_floats(grid, m) floats, grid <= ceil(t / PPW_R)
// blocks; var == nullptr: mean only (M and scratch are then not touched)
hipError_t launch_ppa_predict_wide(
    const float* X, const float* A, const float* s2v, float amp,
    const double* mv, const double* M, double kxx, long t, int m, int d,
    float* scratch, int grid, double* mean, double* var, int family,
    hipStream_t stream);

// ---- greedy.hip -----------------------------------------------------------
// One round of the incremental forward selection, with mc < m points in.
// Row vectors hold gr_npad(n) elements, U and V [m, gr_npad(n)], partials
// gr_blocks(n) * gr_pstride(m) doubles.  sums: [mc + 2] = (w, cc, cy).
hipError_t launch_greedy_pass1(
    const float* X, const float* xstar, const float* s2v, float amp,
    const double* y, const double* a, double a_nn, long n, int d, int mc,
    int m, float* U, const double* V, float* c, double* p, double* partials,
    double* sums, int family, hipStream_t stream);

// bval, bidx: [gr_blocks(n)]; best: (max score, its lowest row as a double)
hipError_t launch_greedy_pass2(
    const float* c, const double* y, const double* l, double l_nn,
    double beta_new, double kxx, double sigma2, long n, int mc, int m,
    double* V, const double* p, double* q, double* mu, double* delta,
    double* bval, long long* bidx, double* best, hipStream_t stream);

// ---- kmeans.hip -----------------------------------------------------------
// One Lloyd step in two launches joined by assign [km_npad(n)]: the nearest
// centroid of every row (-1 past n; lowest index among equal scores), then
// fp64 sums [m, d] and counts [m] of the rows of each centroid.
// c2: km_mpad(m) floats of scratch (the centroid norms)
hipError_t launch_kmeans_assign(const float* X, const float* C, long n, int m,
                                int d, float* c2, int* assign,
                                hipStream_t stream);

// partials: km_partial_doubles(n, m, d) doubles of scratch
hipError_t launch_kmeans_accumulate(const float* X, const int* assign, long n,
                                    int m, int d, double* partials,
                                    double* sums, double* counts,
                                    hipStream_t stream);

// ---- big_chol.hip ---------------------------------------------------------
hipError_t launch_dpotrf_diag(double* A, long m, int jb, double* Vout,
                              int* bad, hipStream_t stream);

hipError_t launch_dgemm64(int ta, int tb, int sub, int syrk, const double* A,
                          const double* B, double* C, int M, int N, int K,
                          long lda, long ldb, long ldc, hipStream_t stream);

// ---- synth.hip ------------------------------------------------------------
hipError_t launch_synth_regression(float* X, float* y, long n, int d,
                                   unsigned long long seed, float noise_sd,
                                   hipStream_t stream);

#ifdef __cplusplus
}
#endif

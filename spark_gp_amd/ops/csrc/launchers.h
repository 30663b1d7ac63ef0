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

// ---- laplace.hip ----------------------------------------------------------
hipError_t launch_fused_laplace_newton(
    const float* X, const float* y, float* f, const float* scale, float amp,
    float noise, int E, int k, int d, double tol, int max_newton,
    double* out_psi, double* out_sumlogl, int* out_iters, int* out_bad,
    hipStream_t stream);

hipError_t launch_fused_laplace_evidence(
    const float* X, const float* y, float* f, const float* scale, float amp,
    float noise, int E, int k, int d, double tol, int max_newton,
    double* out_psi, double* out_sumlogl, int* out_iters, int* out_bad,
    double* out_logz, double* out_grad, hipStream_t stream);

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

// ---- predict.hip ----------------------------------------------------------
// var == nullptr: mean only (M is then not read)
hipError_t launch_ppa_predict(
    const float* X, const float* A, const float* s2v, float amp,
    const double* mv, const double* M, double kxx, long t, int m, int d,
    double* mean, double* var, int family, hipStream_t stream);

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

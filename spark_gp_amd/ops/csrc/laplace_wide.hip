// The streamed-feature (WIDE) instantiations of the fused Laplace kernel and
// their launchers: RBF and ARD-RBF bases, the logistic link (the probit
// instantiations come from laplace_wide_probit.hip), 1 <= k <= 128
// rows and 1 <= d <= LAPW_D_MAX feature dimensions — the experts whose
// [k, d] block of X the resident kernel cannot hold in LDS (d > k; MNIST's
// 100 x 784 is 313 KB).  The template is laplace.hip's, compiled here in a
// translation unit of its own as the Matern families are; what the WIDE
// instantiations do differently is in laplace_wide.h, and their LDS plan is
// lapw_lds_bytes (kernel_geom.h): 79 248 B at (100, 784), two workgroups
// per CU, and 115 824 B at (128, 1024).
#include <hip/hip_runtime.h>

#define LAP_FAMILY GEOM_FAM_RBF
#define LAP_WIDE
#include "laplace.hip"

extern "C" const void* lap_kernel_wide_probit(int ev);   // laplace_wide_probit.hip

// the WIDE instantiation of a link code; null for an unknown one
static lap_kernel_t lapw_kernel_of(int link, int ev) {
  switch (link) {
    case LAP_LINK_LOGISTIC:
      return ev ? fused_laplace_kernel<true, GEOM_FAM_RBF, true>
                : fused_laplace_kernel<false, GEOM_FAM_RBF, true>;
    case LAP_LINK_PROBIT: return (lap_kernel_t)lap_kernel_wide_probit(ev);
  }
  return nullptr;
}

extern "C" hipError_t launch_fused_laplace_newton_wide(
    const float* X, const float* y, float* f, const float* scale, float amp,
    float noise, int E, int k, int d, double tol, int max_newton,
    double* out_psi, double* out_sumlogl, int* out_iters, int* out_bad,
    int link, hipStream_t stream) {
  const lap_kernel_t kern = lapw_kernel_of(link, 0);
  if (!kern || !lapw_supported(k, d, 0)) return hipErrorInvalidConfiguration;
  hipLaunchKernelGGL(kern, dim3(E), dim3(WG), lapw_lds_bytes(k, d, 0),
                     stream, X, y, f, scale, amp, noise, k, d, tol,
                     max_newton, out_psi, out_sumlogl, out_iters, out_bad,
                     (double*)nullptr, (double*)nullptr);
  return hipGetLastError();
}

extern "C" hipError_t launch_fused_laplace_evidence_wide(
    const float* X, const float* y, float* f, const float* scale, float amp,
    float noise, int E, int k, int d, double tol, int max_newton,
    double* out_psi, double* out_sumlogl, int* out_iters, int* out_bad,
    double* out_logz, double* out_grad, int link, hipStream_t stream) {
  const lap_kernel_t kern = lapw_kernel_of(link, 1);
  if (!kern || !lapw_supported(k, d, 1)) return hipErrorInvalidConfiguration;
  hipLaunchKernelGGL(kern, dim3(E), dim3(WG), lapw_lds_bytes(k, d, 1),
                     stream, X, y, f, scale, amp, noise, k, d, tol,
                     max_newton, out_psi, out_sumlogl, out_iters, out_bad,
                     out_logz, out_grad);
  return hipGetLastError();
}

// resident workgroups per CU of the evidence kernel at (k, d), as the runtime
// counts them
extern "C" hipError_t fused_laplace_wide_resident_wgs(int k, int d, int* out) {
  if (!lapw_supported(k, d, 1)) return hipErrorInvalidConfiguration;
  const lap_kernel_t kern = fused_laplace_kernel<true, GEOM_FAM_RBF, true>;
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(
      out, kern, WG, lapw_lds_bytes(k, d, 1));
}

// The probit-link instantiations of the streamed-feature (WIDE) fused Laplace
// kernel: the template of laplace.hip compiled for LAP_LINK_PROBIT, handed to
// the launchers of laplace_wide.hip.  Same LDS plan (lapw_lds_bytes) and
// slab pipeline as the logistic ones; laplace_link.h has the link.
#define LAP_FAMILY GEOM_FAM_RBF
#define LAP_LINK LAP_LINK_PROBIT
#define LAP_WIDE
#include "laplace.hip"

extern "C" const void* lap_kernel_wide_probit(int ev) {
  return ev ? (const void*)fused_laplace_kernel<true, GEOM_FAM_RBF, true,
                                                LAP_LINK_PROBIT>
            : (const void*)fused_laplace_kernel<false, GEOM_FAM_RBF, true,
                                                LAP_LINK_PROBIT>;
}

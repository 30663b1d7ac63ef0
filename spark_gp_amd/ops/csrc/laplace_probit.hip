// The probit-link instantiations of the resident fused Laplace kernel (RBF
// family, Newton-only and evidence): the template of laplace.hip compiled for
// LAP_LINK_PROBIT in a translation unit of its own, as the Matern families
// are (see the header comment there, and laplace_link.h for the link).
#define LAP_FAMILY GEOM_FAM_RBF
#define LAP_LINK LAP_LINK_PROBIT
#define LAP_KERNEL_GETTER lap_kernel_probit
#include "laplace.hip"

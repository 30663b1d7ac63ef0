// The Matern 5/2 instantiations of the fused Laplace kernel: the template of
// laplace.hip compiled for GEOM_FAM_M52, in a translation unit of its own
// (see the header comment there).
#define LAP_FAMILY GEOM_FAM_M52
#define LAP_KERNEL_GETTER lap_kernel_m52
#include "laplace.hip"

// The Matern 3/2 instantiations of the fused Laplace kernel: the template of
// laplace.hip compiled for GEOM_FAM_M32, in a translation unit of its own
// (see the header comment there).
#define LAP_FAMILY GEOM_FAM_M32
#define LAP_KERNEL_GETTER lap_kernel_m32
#include "laplace.hip"

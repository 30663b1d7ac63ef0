// The Matern 3/2 front of the fused per-expert NLL kernel: the kernel of
// expert_nll.hip compiled for GEOM_FAM_M32, in a translation unit of its
// own (see the note above the kernel there).
#define NLL_FAMILY GEOM_FAM_M32
#define NLL_KERNEL fused_expert_nll_m32_kernel
#define NLL_KERNEL_GETTER nll_kernel_m32
#include "expert_nll.hip"

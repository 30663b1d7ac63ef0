// The Matern 5/2 front of the fused per-expert NLL kernel: the kernel of
// expert_nll.hip compiled for GEOM_FAM_M52, in a translation unit of its
// own (see the note above the kernel there).
#define NLL_FAMILY GEOM_FAM_M52
#define NLL_KERNEL fused_expert_nll_m52_kernel
#define NLL_KERNEL_GETTER nll_kernel_m52
#include "expert_nll.hip"

// fh_spmulti_part.hip -- the kernels for a matrix unknown over a sparse operator (csrc/fh_spmulti.h) as a translation unit of their own: the
// explicit instantiations the launchers in fh_host_launch.h declare `extern`; compiles in parallel with the host unit.
#include <hip/hip_runtime.h>
#include "fh_spmulti.h"

#define SPMC_INSTANTIATE_LB(LB) SPMC_LB_KERNELS(template, LB)
SPMC_FOR_EACH_LB(SPMC_INSTANTIATE_LB)
#define SPMC_INSTANTIATE(G, LB) SPMC_KERNELS(template, G, LB)
SPMC_FOR_EACH(SPMC_INSTANTIATE)

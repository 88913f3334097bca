// fh_multi_part.hip -- the multi-column dense kernels (csrc/fh_multi.h) as a translation unit of their own: the explicit instantiations the
// launchers in fh_host_launch.h declare `extern`; compiles in parallel with the host unit.
#include <hip/hip_runtime.h>
#include "fh_multi.h"

#define MC_INSTANTIATE(LB, CH, R) MC_KERNELS(template, LB, CH, R)
MC_FOR_EACH(MC_INSTANTIATE)

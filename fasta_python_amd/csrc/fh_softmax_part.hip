// fh_softmax_part.hip -- the row kernel of the softmax loss (csrc/fh_softmax.h) as a translation unit of its own: the explicit instantiations
// the launchers in fh_host_launch.h declare `extern`; compiles in parallel with the host unit.
#include <hip/hip_runtime.h>
#include "fh_softmax.h"

#define SM_INSTANTIATE(LB) SM_KERNELS(template, LB)
SM_FOR_EACH_LB(SM_INSTANTIATE)

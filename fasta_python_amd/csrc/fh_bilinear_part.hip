// fh_bilinear_part.hip -- the kernels of the bilinear smooth term (csrc/fh_bilinear.h) as a translation unit of their own: the explicit
// instantiations the launchers in fh_host_launch.h declare `extern`; compiles in parallel with the host unit.
#include <hip/hip_runtime.h>
#include "fh_bilinear.h"

#define BL_INSTANTIATE(LB) BL_KERNELS(template, LB)
BL_FOR_EACH(BL_INSTANTIATE)

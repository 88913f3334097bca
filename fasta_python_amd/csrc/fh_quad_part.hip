// fh_quad_part.hip -- the kernels of the quadratic smooth term (csrc/fh_quad.h) as a translation unit of their own: the explicit instantiations
// the launchers in fh_host_launch.h declare `extern`; compiles in parallel with the host unit.
#include <hip/hip_runtime.h>
#include "fh_quad.h"

#define QD_INSTANTIATE(LB, CH, R) QD_KERNELS(template, LB, CH, R)
MC_FOR_EACH(QD_INSTANTIATE)

// fh_tv3d_part.hip -- the kernels of the 3-D stencil operator (csrc/fh_tv3d.h) as a translation unit of their own: the explicit
// instantiations the launchers in fh_host_launch.h declare `extern`; compiles in parallel with the host unit.
#include <hip/hip_runtime.h>
#include "fh_tv3d.h"

TV3_KERNELS(template)

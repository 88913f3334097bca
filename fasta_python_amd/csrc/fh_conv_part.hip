// fh_conv_part.hip -- the kernels of the periodic convolution operator (csrc/fh_conv.h) as a translation unit of their own: the explicit
// instantiations the launchers in fh_host_launch.h declare `extern`; compiles in parallel with the host unit.
#include <hip/hip_runtime.h>
#include "fh_conv.h"

CONV_KERNELS(template)

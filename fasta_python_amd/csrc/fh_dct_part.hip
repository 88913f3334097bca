// fh_dct_part.hip -- the kernels of the subsampled DCT operator (csrc/fh_dct.h) as a translation unit of their own: the explicit
// instantiations the launchers in fh_host_launch.h declare `extern`; compiles in parallel with the host unit.
#include <hip/hip_runtime.h>
#include "fh_dct.h"

#define DCT_INSTANTIATE(LDSN) DCT_KERNELS(template, LDSN)
DCT_FOR_EACH(DCT_INSTANTIATE)
#undef DCT_INSTANTIATE
DCT_TILE_KERNELS(template)

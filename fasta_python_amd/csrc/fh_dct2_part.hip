// fh_dct2_part.hip -- the kernels of the subsampled 2-D DCT operator (csrc/fh_dct2.h) as a translation unit of their own: the explicit
// instantiations the launchers in fh_host_launch.h declare `extern`; compiles in parallel with the host unit.
#include <hip/hip_runtime.h>
#include "fh_dct2.h"

#define DCT2_INSTANTIATE(LDSN) DCT2_KERNELS(template, LDSN)
DCT_FOR_EACH(DCT2_INSTANTIATE)
#undef DCT2_INSTANTIATE
DCT2_TILE_KERNELS(template)

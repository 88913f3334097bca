// fh_sparse_part.hip -- the sparse-operator kernels (csrc/fh_sparse.h) as a translation unit of their own: the explicit instantiations the
// launchers in fh_host_launch.h declare `extern`; compiles in parallel with the host unit.
#include <hip/hip_runtime.h>
#include "fh_sparse.h"

#define SP_INSTANTIATE(G) SP_KERNELS(template, G)
SP_FOR_EACH(SP_INSTANTIATE)

// fh_screen_part.hip -- the kernels of gap-safe screening (csrc/fh_screen.h) as a translation unit of their own: the explicit instantiations
// the entry points in fasta_hip.hip declare `extern`, and the three kernels that are no templates; compiles in parallel with the host unit.
#include <hip/hip_runtime.h>
#define FH_SCREEN_DEFINE
#include "fh_screen.h"

SCREEN_KERNELS(template)

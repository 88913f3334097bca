// fh_gap_part.hip -- the kernels of the duality-gap certificate (csrc/fh_gap.h) as a translation unit of their own: the explicit
// instantiations the entry point in fasta_hip.hip declares `extern`; compiles in parallel with the host unit.
#include <hip/hip_runtime.h>
#include "fh_gap.h"

GAP_KERNELS(template)

// fh_standardize_part.hip -- the kernels of fh_standardize (csrc/fh_standardize.h) as a translation unit of their own: the explicit instantiations
// the entry point in fasta_hip.hip declares `extern`, and the three kernels that are no templates; compiles in parallel with the host unit.
#include <hip/hip_runtime.h>
#define FH_STANDARDIZE_DEFINE
#include "fh_standardize.h"

STD_KERNELS(template)

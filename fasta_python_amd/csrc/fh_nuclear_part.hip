// fh_nuclear_part.hip -- the instantiations of the block-Jacobi step kernel (csrc/fh_nuclear.h): one object of the library.
#include "fh_nuclear.h"
#define NUC_INSTANTIATE template
NUC_KERNELS(NUC_INSTANTIATE)

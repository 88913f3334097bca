// controller_shim.cpp -- the loop's controller as it ships (fasta_python_amd/csrc/fh_controller.h), instantiated with the host's square
// (libm's pow through a volatile pointer, as csrc/fh_host_iterate.h) for the CPU test tier: built and loaded by tests/controller_shim.py.
#include <math.h>
#include "fh_loop.h"
#include "fh_controller.h"
static double (*volatile shim_pow)(double, double) = pow;
struct ShimSq { double operator()(double x) const { return shim_pow(x, 2.0); } };
extern "C" void fc_shim_sizes(unsigned long long sizes[3]) { sizes[0] = sizeof(RunOpts); sizes[1] = sizeof(RunState); sizes[2] = sizeof(FcDecision); }
extern "C" int fc_shim_backtrack(const RunOpts* o, const RunState* st, int lsq, const double* s, double tau, int bt) {
  return fc_backtrack(*o, st->f_window, st->iteration, fc_f(lsq != 0, s[FC_FSQ], ShimSq()), s[FC_DXG0], s[FC_DX2], tau, bt, ShimSq()) ? 1 : 0;
}
extern "C" void fc_shim_decide(const RunOpts* o, RunState* st, int lsq, int g_kind, double mu, const double* s, double tau, int bt, double* record, FcDecision* d) {
  *d = fc_decide(*o, lsq != 0, g_kind, mu, s, tau, bt, st->alpha1, st->max_residual, st->best_quality, record, ShimSq());
  fc_advance(*st, *d, bt);
}

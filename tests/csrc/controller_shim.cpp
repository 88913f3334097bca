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
// ... and instantiated as the DEVICE instantiates it (FcSqMul: a square is a product), for the exact-arithmetic tier of the persistent launch
// (tests/run_paths.py restates the controller in Python; tests/test_run_paths_cpu.py proves the restatement equal to these)
extern "C" int fc_shim_backtrack_mul(const RunOpts* o, const RunState* st, int lsq, const double* s, double tau, int bt) {
  return fc_backtrack(*o, st->f_window, st->iteration, fc_f(lsq != 0, s[FC_FSQ], FcSqMul()), s[FC_DXG0], s[FC_DX2], tau, bt, FcSqMul()) ? 1 : 0;
}
extern "C" void fc_shim_decide_mul(const RunOpts* o, RunState* st, int lsq, int g_kind, double mu, const double* s, double tau, int bt, double* record, FcDecision* d) {
  *d = fc_decide(*o, lsq != 0, g_kind, mu, s, tau, bt, st->alpha1, st->max_residual, st->best_quality, record, FcSqMul());
  fc_advance(*st, *d, bt);
}
extern "C" void fc_shim_alpha_mul(const RunOpts* o, double alpha1, double rdot, double* out3) {
  const FcAlpha a = fc_alpha(*o, alpha1, rdot, FcSqMul());
  out3[0] = a.alpha0; out3[1] = a.alpha1; out3[2] = a.coef;
}
// roles = {xi, ti, bi, pc, gc, zc, last_accel}
extern "C" void fc_shim_rotate(int accelerate, int better, int* roles, int* perm) {
  int p[5];
  for (int k = 0; k < 5; ++k) p[k] = perm[k];
  fc_rotate(accelerate != 0, better != 0, roles[0], roles[1], roles[2], roles[3], roles[4], roles[5], roles[6], p);
  for (int k = 0; k < 5; ++k) perm[k] = p[k];
}

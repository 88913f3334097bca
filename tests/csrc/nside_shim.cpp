// nside_shim.cpp -- the n-side arithmetic of one element as it ships (fasta_python_amd/csrc/fh_nside.h: the functions every second-tier kernel
// calls), compiled for the host for the CPU test tier: built and loaded by tests/test_nside_cpu.py.  Elements are taken in index order.
#include "fh_nside.h"

extern "C" {
void ns_shim_fwd_point(int n, const double* x0, const double* g0, double tau, double* xhat) {
  for (int i = 0; i < n; ++i) xhat[i] = fwd_point(x0[i], g0[i], tau);
}
void ns_shim_dgrad(int n, const double* g1, const double* xhat, const double* x0, double tau, double* dg) {
  for (int i = 0; i < n; ++i) dg[i] = bb_dgrad(g1[i], xhat[i], x0[i], tau);
}
// v[8], zero on entry: with_fsq = 1 leaves slot 0 to the caller's loss sum (the scalar block's order), 0 starts at slot 0
void ns_shim_fwd_sums(int n, int with_fsq, const double* x0, const double* g0, const double* xhat, const double* xp, const double* xav, int gsum,
                      double* v_out) {
  double v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int i = 0; i < n; ++i) {
    if (with_fsq) nside_fwd_sums<1>(x0[i], g0[i], xhat[i], xp[i], xav[i], v, gsum != 0);
    else nside_fwd_sums<0>(x0[i], g0[i], xhat[i], xp[i], xav[i], v, gsum != 0);
  }
  for (int k = 0; k < 8; ++k) v_out[k] = v[k];
}
// v[5], zero on entry; x1[n] = what the function returns
void ns_shim_adj_sums(int n, const double* g1, const double* x0, const double* xp, const double* xacc0, const double* xhat, int accel, double coef,
                      double tau, int gsum, double* v_out, double* x1) {
  double v[5] = {0, 0, 0, 0, 0};
  for (int i = 0; i < n; ++i) x1[i] = nside_adj_sums(g1[i], x0[i], xp[i], xacc0[i], xhat[i], accel != 0, coef, tau, v, gsum != 0);
  for (int k = 0; k < 5; ++k) v_out[k] = v[k];
}
}

// fh_nside.h -- the n-side arithmetic of one element, written ONCE for every operator form of the second tier (fh_sparse.h, fh_spmulti.h,
// fh_multi.h, fh_quad.h, fh_bilinear.h, fh_tv3d.h, fh_dct.h, fh_conv.h, fh_nuclear.h, and k_adj_dense / k_bb_epilogue of fh_dense.h).  This is
// the arithmetic that has to keep the reference's evaluation order (fasta/__init__.py:181-270):
//   nside_fwd_sums    the seven forward sums of one element: <Dx,g0>, ||Dx||^2, ||xprox - xhat||^2, ||g0||^2, the g terms, the restart dot
//   nside_adj_sums    the adjoint epilogue of one element: the FISTA extrapolation of x and the Barzilai-Borwein terms
// and the four helpers they are made of.  Everything here compiles for the host as well (tests/csrc/nside_shim.cpp, a plain C++ compiler with
// -ffp-contract=off) and depends on <math.h> only; fh_device.h includes it first.  The cross-workgroup sum of the records these functions fill
// is device code: finish_records, fh_records.h.  Elementwise operations are never contracted: each rounds like the NumPy expression it
// replaces; the sums use explicit fma().  (The tuned one-pass, persistent and stencil kernels keep their own text -- fh_fused_body.inc, fh_run.h,
// fh_tv.h -- and so does k_fwd_dense, for the reason given where it stands.)
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define NS_FN __host__ __device__ __forceinline__
#else
#define NS_FN static inline      // (a non-clang host build passes -ffp-contract=off instead of the pragmas below)
#endif

// forward (gradient) step x0 - tau*g0, two roundings as in fasta/__init__.py:181
NS_FN double fwd_point(double x0, double g0, double tau) {
#pragma clang fp contract(off)
  double s = tau * g0;
  return x0 - s;
}

// z + coef*(z - zprev), fasta/__init__.py:242-243 evaluation order
NS_FN double extrapolate(double v, double vprev, double coef) {
#pragma clang fp contract(off)
  double d = v - vprev;
  double s = coef * d;
  return v + s;
}

// Dg = g1 + (xhat - x0)/tau, fasta/__init__.py:254
NS_FN double bb_dgrad(double g1, double xhat, double x0, double tau) {
#pragma clang fp contract(off)
  double d = xhat - x0;
  double q = d / tau;
  return g1 + q;
}

NS_FN double sub_nofma(double a, double b) {
#pragma clang fp contract(off)
  return a - b;
}

// The forward sums of one element into v[O .. O + 6] = dxg0, dx2, xh2, g02, gsum, gmax, rdot (O = 1 where the caller keeps its loss sum in
// slot 0, the scalar block's order; O = 0 for a prologue of its own).  xav: x_accel0 of the element, 0 where there is none.  gsum = false: the
// caller forms the sum of the g terms itself (a row norm).
template <int O, int K>
NS_FN void nside_fwd_sums(double x0e, double g0e, double xhe, double xpe, double xav, double (&v)[K], bool gsum = true) {
  static_assert(O >= 0 && O + 7 <= K, "seven slots from O");
  const double dx = sub_nofma(xpe, x0e);
  const double dh = sub_nofma(xpe, xhe);
  v[O + 0] = fma(dx, g0e, v[O + 0]);
  v[O + 1] = fma(dx, dx, v[O + 1]);
  v[O + 2] = fma(dh, dh, v[O + 2]);
  v[O + 3] = fma(g0e, g0e, v[O + 3]);
  if (gsum) v[O + 4] += fabs(xpe);
  v[O + 5] = fmax(v[O + 5], fabs(xpe));
  v[O + 6] = fma(sub_nofma(x0e, xpe), sub_nofma(xpe, xav), v[O + 6]);
}

// The adjoint epilogue of one element: x1 = xprox or its extrapolation (returned), then v[0 .. 4] = dxdg, dg2, xh2, gsum, gmax at x1.
// xacc0e is read only when accel is set.  gsum as above.
template <int K>
NS_FN double nside_adj_sums(double g1, double x0e, double xpe, double xacc0e, double xhe, bool accel, double coef, double tau, double (&v)[K],
                            bool gsum = true) {
  static_assert(K >= 5, "five slots");
  double x1 = xpe;
  if (accel) x1 = extrapolate(xpe, xacc0e, coef);
  const double dx = sub_nofma(xpe, x0e);
  const double dg = bb_dgrad(g1, xhe, x0e, tau);
  const double dh = sub_nofma(x1, xhe);
  v[0] = fma(dx, dg, v[0]);
  v[1] = fma(dg, dg, v[1]);
  v[2] = fma(dh, dh, v[2]);
  if (gsum) v[3] += fabs(x1);
  v[4] = fmax(v[4], fabs(x1));
  return x1;
}

// fh_controller.h -- the decisions the reference takes between two launches, written ONCE for everybody who takes them: the library's host-side
// loop (csrc/fh_host_iterate.h: fh_iterate), the persistent launch (csrc/fh_run.h: k_run_dense, one thread per workgroup) and the finaliser of a
// chained one-pass launch (csrc/fh_fused.h: chain_controller) -- and, compiled by a plain host compiler, the CPU test tier
// (tests/csrc/controller_shim.cpp).  Float64, in the reference's order of operations, never contracted:
//   fc_f / fc_g       f from the device sum (losses.py: f_from_device), g from the prox's reductions (proximal.py: g_from_sums)
//   fc_backtrack      the non-monotone backtracking test                       fasta/__init__.py:195-217
//   fc_alpha          FISTA restart and alpha recursion                        :220-238
//   fc_decide         Barzilai-Borwein step (:253-270), residuals, normaliser, best iterate (:272-300), the four stop rules
//                     (fasta/stopping.py:6-51) and the history record of an ACCEPTED attempt
//   fc_advance        ... and what it changes in the solver state
//   fc_rotate         fh_commit's rotation of the buffer roles, for the two loops that keep the roles on the device
// Sums come in as plain doubles in the order of the scalar block (FC_* below = FH_S_* of include/fasta_hip.h), whichever launch or reduction
// produced them.  The one thing the callers legitimately differ in is HOW A SCALAR IS SQUARED, and that is the functor `sq`: the host squares
// as NumPy's `float64 ** 2` does (libm's pow -- what keeps driver="library" equal to driver="python" bit for bit, see fh_host_iterate.h), the
// device multiplies (FcSqMul).  max(a, b) is Python's everywhere (a unless b > a), the window maximum ndarray.max's (a NaN anywhere wins).
// Depends on <math.h> and fh_loop.h only.  (`fp contract(off)` sits inside every body, not at file scope: kernels that include this header
// must compile exactly as without it.)
#pragma once
#include <math.h>
#include "fh_loop.h"

#if defined(__HIPCC__)
#define FC_FN __host__ __device__ __forceinline__
#define FC_MEMBER __host__ __device__ __forceinline__
#else
#define FC_FN static inline      // (a non-clang host build passes -ffp-contract=off instead of the pragmas below)
#define FC_MEMBER inline
#endif

enum { FC_FSQ = 0, FC_DXG0, FC_DX2, FC_XH2, FC_G02, FC_GSUM, FC_GMAX, FC_RDOT,           // the forward half of an attempt's sums
       FC_DXDG, FC_DG2, FC_FSQ_ADJ, FC_XH2_ADJ, FC_GSUM_ADJ, FC_GMAX_ADJ, FC_NSUMS };    // the adjoint half (*_ADJ: at the extrapolated point)
enum { FC_G_NONE = 0, FC_G_SUM = 1, FC_G_MAX = 2 };      // g(x) for the objective: 0, mu * sum|x_i| (Shrink), mu * max|x_i| (LinfProx)

struct FcSqMul { FC_MEMBER double operator()(double x) const {
#pragma clang fp contract(off)
  return x * x; } };

struct FcAlpha { double alpha0, alpha1, coef; bool restarted; };
struct FcDecision {
  bool better, stop, restarted;
  double tau_next, alpha0, alpha1, coef, f1, max_residual, best_quality;
};

template <class Sq> FC_FN double fc_f(bool lsq, double sum, Sq sq) {
#pragma clang fp contract(off)
  return lsq ? .5 * sq(sqrt(sum)) : sum;
}
FC_FN double fc_g(int g_kind, double mu, double gsum, double gmax) {
#pragma clang fp contract(off)
  return g_kind == FC_G_SUM ? mu * gsum : (g_kind == FC_G_MAX ? mu * gmax : 0.0);
}

// :195-217 -- true = this attempt (the iteration's `bt`-th retry, step `tau`) is rejected: shrink the step and try again.
// f_window[j % FR_WINDOW_MAX] = f_hist[j]; `iteration` is the number of completed iterations.
template <class Sq>
FC_FN bool fc_backtrack(const RunOpts& o, const double* f_window, unsigned long long iteration, double f1, double dxg0, double dx2, double tau,
                        int bt, Sq sq) {
#pragma clang fp contract(off)
  if (!o.backtrack) return false;
  const unsigned long long i = iteration, lo = i + 1ull > (unsigned long long)o.window ? i + 1ull - (unsigned long long)o.window : 0ull;
  double M = f_window[lo % FR_WINDOW_MAX];                 // f_hist[lo : i + 1].max()
  for (unsigned long long j = lo + 1ull; j <= i; ++j) {
    const double v = f_window[j % FR_WINDOW_MAX];
    if (M != M) break;
    if (v != v || v > M) M = v;
  }
  return f1 - (M + dxg0 + sq(sqrt(dx2)) / (2.0 * tau)) > 1E-12 && bt < o.max_backtracks;
}

// alpha1 from alpha0 (:235); the extrapolation coefficient is (alpha0 - 1) / alpha1 (:237)
template <class Sq> FC_FN double fc_alpha_next(double alpha0, Sq sq) {
#pragma clang fp contract(off)
  return (1.0 + sqrt(1.0 + 4.0 * sq(alpha0))) / 2.0;
}
// :220-238 -- `alpha1` as the last iteration left it, `rdot` the restart dot of this attempt
template <class Sq> FC_FN FcAlpha fc_alpha(const RunOpts& o, double alpha1, double rdot, Sq sq) {
#pragma clang fp contract(off)
  FcAlpha a = {0.0, alpha1, 0.0, false};
  if (!o.accelerate) return a;
  a.alpha0 = alpha1;
  if (o.restart && rdot > 1E-30) { a.alpha0 = 1.0; a.restarted = true; }
  a.alpha1 = fc_alpha_next(a.alpha0, sq);
  a.coef = (a.alpha0 - 1.0) / a.alpha1;
  return a;
}

// :220-300 and the stop rule for an accepted attempt: `s` its sums (FC_*), `tau` its step, `bt` the retries before it; alpha1 / max_residual /
// best_quality as the last iteration left them.  Writes the history record to `h` (FR_HIST doubles) unless h is null.  Changes no state.
template <class Sq>
FC_FN FcDecision fc_decide(const RunOpts& o, bool lsq, int g_kind, double mu, const double* s, double tau, int bt, double alpha1,
                           double max_residual, double best_quality, double* h, Sq sq) {
#pragma clang fp contract(off)
  const FcAlpha al = fc_alpha(o, alpha1, s[FC_RDOT], sq);
  FcDecision d;
  d.restarted = al.restarted; d.alpha0 = al.alpha0; d.alpha1 = al.alpha1; d.coef = al.coef;
  d.f1 = fc_f(lsq, o.accelerate ? s[FC_FSQ_ADJ] : s[FC_FSQ], sq);                 // :188, :245
  const double xh2 = o.accelerate ? s[FC_XH2_ADJ] : s[FC_XH2], gsum = o.accelerate ? s[FC_GSUM_ADJ] : s[FC_GSUM];
  const double gmax = o.accelerate ? s[FC_GMAX_ADJ] : s[FC_GMAX];
  d.tau_next = tau;                                                               // :249
  const double dx_norm = sqrt(s[FC_DX2]);
  if (o.adaptive) {                                                               // :253-270
    const double dot = s[FC_DXDG];
    const double tau_s = sq(dx_norm) / dot;
    const double q = dot / sq(sqrt(s[FC_DG2]));
    const double tau_m = 0.0 > q ? 0.0 : q;                                       // max(q, 0)
    d.tau_next = (2.0 * tau_m > tau_s) ? tau_m : tau_s - .5 * tau_m;
    if (d.tau_next <= 0.0 || isinf(d.tau_next) || isnan(d.tau_next)) d.tau_next = tau * 1.5;
  }
  const double resid = dx_norm / tau;                                             // :272
  const double na = sqrt(s[FC_G02]), nb = sqrt(xh2) / tau;
  const double normalizer = (nb > na ? nb : na) + 1E-12;                          // max(a, b) + EPSILON  (:274)
  const double norm_resid = resid / normalizer;
  d.max_residual = resid > max_residual ? resid : max_residual;                   // :281
  double objective = 0.0, quality = resid;
  if (o.evaluate_objective) {                                                     // :284-289
    objective = d.f1 + fc_g(g_kind, mu, gsum, gmax);
    quality = objective;
  }
  d.better = quality < best_quality;                                              // :298-300
  d.best_quality = d.better ? quality : best_quality;
  const bool ratio = resid / d.max_residual < o.tolerance, normed = norm_resid < o.tolerance;      // stopping.py:6-51
  d.stop = o.stop_rule == 0 ? resid < o.tolerance : (o.stop_rule == 1 ? normed : (o.stop_rule == 2 ? ratio : ratio || normed));
  if (h) {
    h[0] = resid; h[1] = norm_resid; h[2] = tau; h[3] = d.f1; h[4] = objective; h[5] = (double)bt; h[6] = d.alpha0;
    h[7] = (d.better ? 1.0 : 0.0) + (d.restarted ? 2.0 : 0.0);
  }
  return d;
}

// the iteration is complete: what it leaves in the solver state (St: RunState, or the public fh_run_state)
template <class St> FC_FN void fc_advance(St& st, const FcDecision& d, int bt) {
  st.f_window[(st.iteration + 1ull) % FR_WINDOW_MAX] = d.f1;
  st.tau_next = d.tau_next; st.alpha1 = d.alpha1; st.max_residual = d.max_residual; st.best_quality = d.best_quality;
  st.backtracks += (unsigned long long)bt;
  st.iteration += 1ull;
  if (d.stop) st.stopped = 1;
}

// x0 <- x1, g0 <- g1 as fh_commit does it: on the ROLES (which buffer of the X pool is x0 / the target / the best iterate, which of the P, G
// and Z pairs is current) and, without acceleration, on `perm` (which physical n-side buffer sits in X[0..2], P[0..1]: std::swap(X[ti], P[pc ^ 1]))
FC_FN void fc_rotate(bool accelerate, bool better, int& xi, int& ti, int& bi, int& pc, int& gc, int& zc, int& last_accel, int (&perm)[5]) {
  if (accelerate) { pc ^= 1; last_accel = 1; }
  else { const int a = perm[ti], b = perm[3 + (pc ^ 1)]; perm[ti] = b; perm[3 + (pc ^ 1)] = a; last_accel = 0; }
  xi = ti;
  if (better) bi = xi;
  for (int k = 0; k < 3; ++k) if (k != xi && k != bi) { ti = k; break; }
  zc ^= 1; gc ^= 1;
}

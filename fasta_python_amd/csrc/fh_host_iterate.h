// fh_host_iterate.h -- fh_iterate: the FBS loop (fasta/__init__.py:171-312) driven from the HOST SIDE OF THE LIBRARY (round 6).
//
// fh_run (csrc/fh_run.h) keeps the loop on the device, for the shapes where a workgroup can own whole rows.  Every other operator -- a dense
// matrix of any width, the l-infinity / l1-ball prox kinds with their level search, the stencil, float32 storage, row blocks in this process
// or one rank of a row-sharded run -- still advances one launch (or two) per iteration, and between two launches somebody has to take the
// reference's branch decisions from the 16 scalars the launch returns.  Until round 5 that somebody was Python (fasta_python_amd/solver.py:
// FBSolver.step): 17-19 us per iteration of interpreter time, 14 % of an 8192^2 step and most of a 512 x 512 stencil sweep.  fh_iterate
// is that same driver in C++: it issues the same launches through the same entry points (fh_step / fh_step_accel / fh_fwd / fh_adj /
// fh_fwd_adj / fh_commit), reads the same scalar block after the same single synchronisation and takes the same decisions with the
// same float64 arithmetic -- the backtracking test (:195-217), FISTA restart and alpha recursion (:220-238), the Barzilai-Borwein rule
// (:253-270), residuals, best iterate (:272-300), the four built-in stop rules (fasta/stopping.py:6-51) -- and returns the histories of
// the iterations in fh_run's record format.  Same signature, same options / state / history structs as fh_run, so a caller picks per
// context: fh_run where it exists and wins, fh_iterate everywhere else.
//
// The decisions themselves are csrc/fh_controller.h, shared with the two device-side loops; what stays here is the launch policy and the calls.
// Bit for bit the Python driver: every expression there is the expression of solver.py in the same order, and where Python squares a
// NumPy float64 scalar (`x ** 2`) it calls the C library's pow(x, 2.0) exactly as NumPy's scalar power does -- which is NOT always x * x
// (glibc's pow is within 0.52 ulp, not correctly rounded: ~0.08 % of squares differ in the last bit); the call goes through a volatile
// function pointer because clang would otherwise fold pow(x, 2.0) into x * x.  tests/test_gpu_iterate.py compares the two drivers
// with `==` on every history of every fixture.
//
// The launch POLICY (which kernel serves a forward launch: the one-pass kernel always / speculatively / a K-fwd + K-adj pair under one
// synchronisation / separate launches) arrives in opts->launch_mode -- the caller has settled it, over the ranks if need be
// (fh_fused_agree) -- and the policy's memory (cool-down after a backtrack, back-off after a hand-off timeout) travels in the state, so
// the solve does not depend on where the calls are cut.  Policy never changes results, only which launches produce them.
#pragma once
#include <math.h>
#include "fh_controller.h"

static double (*volatile fh_libm_pow)(double, double) = pow;
struct ItSq { double operator()(double x) const { return fh_libm_pow(x, 2.0); } };          // NumPy's float64_scalar ** 2
static_assert(FC_FSQ == FH_S_FSQ && FC_RDOT == FH_S_RDOT && FC_DXDG == FH_S_DXDG && FC_GMAX_ADJ == FH_S_GMAX_ADJ && FC_NSUMS <= FH_NSCALARS,
              "fh_controller.h reads the scalar block in place");
static_assert(FR_HIST == FH_RUN_HIST && FR_WINDOW_MAX == FH_RUN_WINDOW_MAX, "history record / window of fh_loop.h and include/fasta_hip.h");

struct IterCtl {
  fh_ctx* c; const fh_run_opts* o; fh_run_state* st;
  double s[FH_NSCALARS];       // the scalar block of the latest forward launch (both halves after a one-pass / pair launch)
  bool have_adj;               // ... and it already carries this tau's K-adj half
};

// solver.py:_forward -- the one-pass kernel when the policy has it and `one_pass` asks for it, else K-fwd alone
static int it_forward(IterCtl& k, double tau, bool one_pass, double alpha1) {
#pragma clang fp contract(off)
  fh_run_state* st = k.st;
  const int mode = k.o->launch_mode;
  k.have_adj = false;
  if (mode == FH_LAUNCH_PAIR && one_pass) {
    FH_TRY(fh_fwd_adj(k.c, tau, k.s));
    st->pair_launches += 1;
    k.have_adj = true;
    return 0;
  }
  const bool fused_on = (mode == FH_LAUNCH_ONEPASS_ALWAYS || mode == FH_LAUNCH_ONEPASS_SPECULATIVE) && st->onepass_off_until < 0;
  if (fused_on && one_pass) {
    int rc;
    if (k.o->accelerate) {      // the launch decides the restart itself (:231); the loop mirrors it afterwards
      rc = fh_step_accel(k.c, tau, (alpha1 - 1.0) / fc_alpha_next(alpha1, ItSq()), k.o->restart ? 1 : 0, k.s);
    } else rc = fh_step(k.c, tau, k.s);
    if (rc == 0 && k.s[15] == 0.0) { st->onepass_launches += 1; k.have_adj = true; return 0; }
    if (rc != 0 && rc != FH_E_TIMEOUT) return rc;      // bounded-spin timeouts ONLY: any other status propagates
    // the hand-off between the launch's workgroups timed out (a co-tenant on the GPU?): K-fwd / K-adj now, the one-pass kernel again after
    // `onepass_backoff` iterations, doubling the wait per failure.  (Row-sharded runs all-reduce the timeout word with g1: every rank gets
    // here in the same iteration, the ranks' collective sequences stay aligned.)
    st->onepass_off_until = (long long)st->iteration + st->onepass_backoff;
    st->onepass_backoff *= 2;
    st->onepass_timeouts += 1;
  }
  return fh_fwd(k.c, tau, k.s);
}

extern "C" int fh_iterate(fh_ctx* c, int max_steps, const fh_run_opts* o, fh_run_state* st, double* history, int* steps_done) {
#pragma clang fp contract(off)
  FH_TRY(check_ready(c, true));
  if (!o || !st || !history || !steps_done) return fail(FH_E_ARG, "fh_iterate: null argument");
  *steps_done = 0;
  if (max_steps < 0) return fail(FH_E_ARG, "fh_iterate: max_steps must be >= 0");
  if (o->window < 1 || o->window > FH_RUN_WINDOW_MAX) return fail(FH_E_ARG, "fh_iterate: window must be in [1, %d]", FH_RUN_WINDOW_MAX);
  if (o->stop_rule < 0 || o->stop_rule > 3) return fail(FH_E_ARG, "fh_iterate: stop_rule must be 0..3 (the four rules of fasta/stopping.py)");
  if (o->launch_mode < FH_LAUNCH_SEPARATE || o->launch_mode > FH_LAUNCH_PAIR) return fail(FH_E_ARG, "fh_iterate: unknown launch_mode %d", o->launch_mode);
  if (o->launch_mode == FH_LAUNCH_PAIR && o->accelerate) return fail(FH_E_ARG, "fh_iterate: the K-fwd + K-adj pair has no accelerated form");
  if (st->onepass_backoff <= 0) st->onepass_backoff = 64;
  IterCtl k;
  k.c = c; k.o = o; k.st = st; k.have_adj = false;
  RunOpts ro;
  run_opts_in(o, &ro);
  const fh_ctx* s0 = shard_of(c, 0);
  const bool lsq = s0->loss_kind == LOSS_LSQ;            // (losses.py: LeastSquares.f_from_device / LogisticLoss.f_from_device)
  const int g_kind = g_kind_of(s0);
  const ItSq sq;
  const bool always = o->launch_mode == FH_LAUNCH_ONEPASS_ALWAYS;
  st->stopped = 0;
  for (int step = 0; step < max_steps; ++step) {
    double tau = st->tau_next;                                                    // :178
    if (st->onepass_off_until >= 0 && (long long)st->iteration >= st->onepass_off_until) st->onepass_off_until = -1;      // (every rank holds the same counters: same decision)
    const bool speculate = always || st->spec_cooldown == 0;
    FH_TRY(it_forward(k, tau, speculate, st->alpha1));                            // :181-188  (K-fwd, or K-fwd + K-adj in one pass)
    if (!speculate) st->spec_cooldown -= 1;
    int bt = 0;
    while (fc_backtrack(ro, st->f_window, st->iteration, fc_f(lsq, k.s[FH_S_FSQ], sq), k.s[FH_S_DXG0], k.s[FH_S_DX2], tau, bt, sq)) {   // :195-217
      tau *= o->stepsize_shrink;
      // :207-213: K-fwd again (a speculative K-adj, if any, is void) -- or the one-pass kernel again where it costs what K-fwd costs
      FH_TRY(it_forward(k, tau, always, st->alpha1));
      bt += 1;
    }
    if (bt) st->spec_cooldown = 8;
    // the forward half of the block is final now; K-adj (:242-248) overwrites only its own half
    if (!k.have_adj) {
      double a[FH_NSCALARS];
      FH_TRY(fh_adj(c, tau, o->accelerate ? 1 : 0, fc_alpha(ro, st->alpha1, k.s[FH_S_RDOT], sq).coef, a));
      for (int q = FH_S_DXDG; q < FH_NSCALARS; ++q) k.s[q] = a[q];
    }
    const FcDecision d = fc_decide(ro, lsq, g_kind, s0->mu, k.s, tau, bt, st->alpha1, st->max_residual, st->best_quality,
                                   history + (size_t)step * FH_RUN_HIST, sq);
    FH_TRY(fh_commit(c, d.better ? 1 : 0));                                       // x0 <- x1, g0 <- g1 (:176-177)
    fc_advance(*st, d, bt);
    *steps_done = step + 1;
    if (d.stop) break;
  }
  return 0;
}

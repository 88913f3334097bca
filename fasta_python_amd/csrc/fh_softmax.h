// fh_softmax.h -- the softmax (multinomial logistic) loss over a MATRIX unknown: Z = A X is (m, L), one column per class, labels y in {0 .. L-1}^m,
//   f(Z) = sum_i [ logsumexp(Z_i,:) - Z_i,y_i ],   grad f(Z)_i,l = exp(Z_i,l) / sum_k exp(Z_i,k) - [l == y_i].
// The one smooth term here that couples the L columns of a row of Z; the operators (fh_multi.h dense, fh_spmulti.h sparse), the prologues, the
// proxes and the finalisers are the least-squares ones.  B (FH_VEC_B) holds the one-hot matrix Y, (mv, LB) like every m-side matrix.
//
// The arithmetic of a row z, THE SAME on the host (losses.SoftmaxLoss) and here, FMA contraction off:
//   mx = max_l z_l;  d_l = z_l - mx;  e_l = exp(d_l);  s = ((e_0 + e_1) + e_2) + ... + e_{L-1}  (columns in index order)
//   term = (mx + log(s)) - z_y;   grad_l = e_l / s - Y_l.
// The maximum is always subtracted: z = (800, -800) gives (1, 0) and a finite loss.  exp / log are the device library's (no fast-math variants).
//
//   k_sm_rows<LB>   one lane per column PAIR of a row of Z, k_spmc_resid's layout: C = LB / 2 adjacent lanes own a row, a wave reads Z, Z_acc0 and B
//                   as contiguous 16-byte pieces.  With `accel` the row is first extrapolated (extrapolate(z, zacc0, coef), as k_spmc_resid does).
//                   mx: lane maximum of the valid columns, then an xor tree over the row's C lanes (a maximum does not depend on the order).
//                   s: every lane of the row GATHERS the row's LB values of e by xor exchanges (DPP: spmc_xor; after the step with mask M a lane
//                   holds the 4M columns of its aligned block, in column order) and adds them left to right.  Padding columns hold e = +0.0 and come
//                   last, so s is bit for bit the left-to-right sum of the L valid columns.  z_y: the pair's (Y_l == 1 ? z_l : 0), summed over the
//                   row's lanes (all terms but one are zero: exact).
//                   Outputs: the residual R (mv, LB) unless p.r is null (VALUE-ONLY mode); one loss record per workgroup (store_partial; inside the
//                   workgroup: block_reduce's fixed order over the rows' terms, held by the lanes with c = 0).  Padding columns of R are written
//                   as +0.0, padding rows are never touched (they are zero from the allocation).
//                   With p.counter set the last-arriving workgroup adds the records (fh_records.h: finish_records -- lane t takes records t, t + 256,
//                   ... in order, then block_reduce), writes out[p.slot] and publishes p.seq: how a forward launch gets its FH_S_FSQ.
//   k_sm_finish     the same ordered sum as ONE workgroup of its own (sm_sum_records): how the dense adjoint gets its FH_S_FSQ_ADJ after k_mc_adj has run.
// No float atomics, no spin waits: bitwise repeatable.
#pragma once
#include "fh_spmulti.h"

#define LOSS_SOFTMAX 4

// a[0], a[1] = this lane's column pair on entry; a[l] = column l of the row on exit, in every one of the row's LB / 2 lanes.  ALL lanes of the wave
// must be active.  Step MASK pairs lane c with lane c ^ MASK: a lane holds CUR = 2 * MASK values, the columns of its aligned block in order; the
// lane with the bit set holds the upper half of the doubled block.
template <int LB, int MASK>
__device__ __forceinline__ void sm_gather_step(double (&a)[LB], uint32_t c) {
  constexpr int CUR = 2 * MASK;
  if constexpr (CUR < LB) {
    const bool upper = (c & (uint32_t)MASK) != 0u;
#pragma unroll
    for (int i = 0; i < CUR; ++i) {
      const double mine = a[i];
      const double theirs = spmc_xor<MASK>(mine);
      a[i] = upper ? theirs : mine;
      a[i + CUR] = upper ? mine : theirs;
    }
  }
}
template <int LB>
__device__ __forceinline__ void sm_gather_row(double (&a)[LB], uint32_t c) {
  sm_gather_step<LB, 1>(a, c);
  sm_gather_step<LB, 2>(a, c);
  sm_gather_step<LB, 4>(a, c);
}
// maximum over the row's C lanes (C a power of two <= 8): every lane gets it
template <int C>
__device__ __forceinline__ double sm_row_max(double v) {
  if (C > 1) v = fmax(v, spmc_xor<1>(v));
  if (C > 2) v = fmax(v, spmc_xor<2>(v));
  if (C > 4) v = fmax(v, spmc_xor<4>(v));
  return v;
}

// the records of k_sm_rows in a fixed order, by one whole workgroup: thread 0 writes the sum to out[slot] and publishes seq (0: none)
__device__ __forceinline__ void sm_sum_records(const double* red, uint32_t n, double* out, int slot, unsigned seq, double* s_scr) {
#pragma clang fp contract(off)
  double v[1] = {0.0};
  for (uint32_t i = threadIdx.x; i < n; i += FH_WG) v[0] += load_partial(red + i);
  block_reduce<1>(v, s_scr, -1);
  if (threadIdx.x == 0) {
    scal_store(out + slot, v[0]);
    publish_seq(out, seq);
  }
}

struct SmRowsP {
  uint32_t m, L;
  const double* z; const double* zacc0; const double* b;
  double* r;            // (mv, LB), or nullptr: value only
  int accel;
  double coef;
  double* red_f;        // [gridDim.x]
  unsigned* counter;    // nullptr: somebody else adds the records
  double* out; int slot; unsigned seq;
};

template <int LB>
__global__ __launch_bounds__(FH_WG) void k_sm_rows(const SmRowsP p) {
#pragma clang fp contract(off)
  constexpr uint32_t C = LB / 2;
  static_assert(FH_WG % C == 0 && 64 % C == 0, "the lanes of a row share a wave");
  __shared__ __attribute__((aligned(16))) double s_scr[4];
  __shared__ __attribute__((aligned(16))) unsigned s_flag[4];
  const uint64_t i = (uint64_t)blockIdx.x * FH_WG + threadIdx.x;      // column pair i % C of row i / C
  const uint32_t c = threadIdx.x % C;                                  // (= i % C: a workgroup starts on a row)
  const bool live = i < (uint64_t)p.m * C;
  const bool v0 = 2u * c < p.L, v1 = 2u * c + 1u < p.L;
  d2 zv = {0.0, 0.0}, bv = {0.0, 0.0};
  if (live) {
    zv = reinterpret_cast<const d2*>(p.z)[i];
    if (p.accel) {
      const d2 za = reinterpret_cast<const d2*>(p.zacc0)[i];
      zv.x = extrapolate(zv.x, za.x, p.coef);
      zv.y = extrapolate(zv.y, za.y, p.coef);
    }
    bv = reinterpret_cast<const d2*>(p.b)[i];
  }
  // (every lane of the wave takes every exchange below: dead lanes carry zeros)
  const double ninf = -__builtin_huge_val();
  const double mx = sm_row_max<(int)C>(fmax(v0 ? zv.x : ninf, v1 ? zv.y : ninf));
  double e[LB];
#pragma unroll
  for (int l = 0; l < LB; ++l) e[l] = 0.0;
  if (v0) e[0] = exp(zv.x - mx);
  if (v1) e[1] = exp(zv.y - mx);
  const double e0 = e[0], e1 = e[1];
  sm_gather_row<LB>(e, c);
  double s = e[0];
#pragma unroll
  for (int l = 1; l < LB; ++l) s = s + e[l];                           // left to right; the padding columns' +0.0 come last
  double zy = (bv.x == 1.0 ? zv.x : 0.0) + (bv.y == 1.0 ? zv.y : 0.0);
  zy = spmc_tree<1, (int)C>(zy);
  if (live && p.r) {
    d2 rv;
    rv.x = v0 ? e0 / s - bv.x : 0.0;
    rv.y = v1 ? e1 / s - bv.y : 0.0;
    reinterpret_cast<d2*>(p.r)[i] = rv;
  }
  double v[1] = {0.0};
  if (live && c == 0u) v[0] = (mx + log(s)) - zy;
  if (!p.counter) { publish_record<1, -1>(v, p.red_f, blockIdx.x, s_scr); return; }
  finish_records<1, -1>(v, p.red_f, blockIdx.x, gridDim.x, p.counter, p.out, p.seq, s_scr, s_flag, NoRecords(),
                        [&](double (&w)[1]) { scal_store(p.out + p.slot, w[0]); });
}

static __global__ __launch_bounds__(FH_WG) void k_sm_finish(const double* red, uint32_t n, double* out, int slot, unsigned seq) {
  __shared__ __attribute__((aligned(16))) double s_scr[4];
  sm_sum_records(red, n, out, slot, seq, s_scr);
}

// ---- the instantiations (ONE table for fh_softmax_part.hip, the extern declarations and the dispatch) ----
#define SM_FOR_EACH_LB(X) X(2) X(4) X(8) X(16)
#define SM_KERNELS(DO, LB) DO __global__ void k_sm_rows<LB>(const SmRowsP);

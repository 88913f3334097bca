// fh_spmulti.h -- kernels for a MATRIX unknown over a SPARSE operator (fh_set_matrix_csr_rhs): X is (n, L), B and Z are (m, L), A is kept
// as fh_sparse.h keeps it (A by rows and A^T by rows, 64-bit entry offsets, 32-bit indices), the matrices as fh_multi.h keeps them ((nv, LB) /
// (mv, LB) row-major, LB in {2, 4, 8, 16} the smallest >= L, padding rows and columns zero and never counted).
//
// Why a form of its own: the vector gather (k_sp_fwd) uses 8 bytes of every cache line of the operand it touches.  Here the gather for one
// stored entry is a whole row of X -- LB * 8 contiguous bytes -- and the 12 streamed bytes of index and value are paid once for all L columns.
//
// Lanes: C = LB / 2 COLUMN lanes cover one row of X with one 16-byte load each (a lane never holds a whole row of X: fh_multi.h records what
// 16-byte loads at LB * 8 bytes lane stride cost the dense form).  A group of G lanes (G >= C, a power of two) serves one row of A and works
// on E = G / C entries per trip: lane (e, c) = lane e * C + c of the group walks entries k0 + e, k0 + e + E, ..., loads index and value (one
// address for its C column lanes: one request) and the two doubles at X[j * LB + 2c], and keeps two accumulators.
//
//   k_spmc_prologue<LB>    n-side prologue, one lane per row of X: k_mc_prologue's arithmetic (FH_PROX_GROUP's row norm included) without the
//                          streaming copy of xprox -- the gather reads the row-major xprox itself.
//   k_spmc_fwd<G, LB, NT>  Z = A * operand.  Row sum order: lane partials, then an xor tree over the lane bits log2(C) .. log2(G) - 1 (DPP inside
//                          16 lanes, a shuffle across).  Lanes with e = 0 write their two columns of Z and the loss terms of the valid columns.
//                          A long row (SpMatP.longer) gets a workgroup of its own: FH_WG / C entries per trip, the tree inside each wave, then the four
//                          waves in order.  Row ranges, long rows and G are fixed at set-matrix time (they depend on LB).
//   k_spmc_resid<LB>       m-side prologue of the adjoint, one lane per column pair: R = Z' - B (Z' = Z or its FISTA extrapolation) and the loss sum
//                          at Z' over the valid entries (FH_S_FSQ_ADJ).
//   k_spmc_adj<G, LB, NT>  G1 = A^T * R, the same gather over the A^T copy.  Every (j, column pair) of G1 has one owner lane, which runs the n-side
//                          epilogue of k_mc_adj (modes 0 and 1).  FH_PROX_GROUP's row norm of x1 is an xor tree over the row's C column lanes
//                          (the lane bits below log2(C)), valid columns only.
// Finalisers are arrive_last only: no spin waits, no co-residency assumption.  No float atomics, every sum in a fixed order: bitwise repeatable.
// NT = 1 (FH_TUNE_NT_LOADS) streams index and value non-temporally, as in fh_sparse.h; the gathered operand keeps the default policy.
#pragma once
#include "fh_multi.h"
#include "fh_sparse.h"

// lane l's copy of the value in lane l ^ MASK.  ALL lanes of the wave must be active.
template <int MASK>
__device__ __forceinline__ double spmc_xor(double v) {
  if (MASK == 1) return dpp_f64<0xB1>(v);                    // quad_perm [1,0,3,2]
  if (MASK == 2) return dpp_f64<0x4E>(v);                    // quad_perm [2,3,0,1]
  if (MASK == 4) return dpp_f64<0x1B>(dpp_f64<0x141>(v));    // row_half_mirror (l ^ 7), then quad_perm [3,2,1,0] (l ^ 3)
  if (MASK == 8) return dpp_f64<0x128>(v);                   // row_ror:8 -- inside a row of 16 lanes a rotation by 8 is l ^ 8
  return __shfl_xor(v, MASK, 64);
}
// sum over the lanes that differ from this one in the lane bits LO <= bit < HI (both powers of two), lowest bit first; every lane gets its sum
template <int LO, int HI>
__device__ __forceinline__ double spmc_tree(double v) {
  if (LO <= 1 && 1 < HI) v += spmc_xor<1>(v);
  if (LO <= 2 && 2 < HI) v += spmc_xor<2>(v);
  if (LO <= 4 && 4 < HI) v += spmc_xor<4>(v);
  if (LO <= 8 && 8 < HI) v += spmc_xor<8>(v);
  if (LO <= 16 && 16 < HI) v += spmc_xor<16>(v);
  if (LO <= 32 && 32 < HI) v += spmc_xor<32>(v);
  return v;
}

// lane (e, c)'s share of row [k0, k1): entries k0 + e, k0 + e + stride, ..., columns 2c and 2c + 1 of the gathered rows of x
template <int LB, int NT>
__device__ __forceinline__ d2 spmc_lane_dot(const SpMatP& a, const double* x, long long k0, long long k1, uint32_t e, uint32_t c, uint32_t stride) {
  const d2* xc = reinterpret_cast<const d2*>(x) + c;
  d2 acc = {0.0, 0.0};
#pragma unroll 4
  for (long long k = k0 + e; k < k1; k += stride) {
    const int j = sp_idx<NT>(a.idx + k);
    const double av = sp_val<NT>(a.val + k);
    const d2 xv = xc[(size_t)j * (LB / 2)];
    acc.x = fma(av, xv.x, acc.x);
    acc.y = fma(av, xv.y, acc.y);
  }
  return acc;
}

// a long row, the whole workgroup: every lane with tid < C ends up with its column pair's sum.  `s_col` = 4 * LB doubles of LDS.
template <int LB, int NT>
__device__ __forceinline__ d2 spmc_long_row(const SpMatP& a, const double* x, uint32_t row, double* s_col) {
  constexpr int C = LB / 2;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  d2 acc = spmc_lane_dot<LB, NT>(a, x, a.ptr[row], a.ptr[(size_t)row + 1], tid / C, tid % C, FH_WG / C);
  acc.x = spmc_tree<C, 64>(acc.x);
  acc.y = spmc_tree<C, 64>(acc.y);
  if (lane < (uint32_t)C) { s_col[wave * LB + 2 * lane] = acc.x; s_col[wave * LB + 2 * lane + 1] = acc.y; }
  __syncthreads();
  d2 s = {0.0, 0.0};
  if (tid < (uint32_t)C) {                                    // the four waves in order
    s.x = ((s_col[2 * tid] + s_col[LB + 2 * tid]) + s_col[2 * LB + 2 * tid]) + s_col[3 * LB + 2 * tid];
    s.y = ((s_col[2 * tid + 1] + s_col[LB + 2 * tid + 1]) + s_col[2 * LB + 2 * tid + 1]) + s_col[3 * LB + 2 * tid + 1];
  }
  return s;
}

// ---- n-side prologue ----------------------------------------------------------------------------------------------------------------------
struct SpmcProP {
  uint32_t n, L;        // logical rows / columns of X
  uint32_t nv;          // device rows of X
  const double* x0; const double* g0; const double* xacc0;
  double* xhat; double* xp;
  double tau;
  ProxP px;             // kind: IDENTITY / SHRINK / NONNEG / BOX (elementwise, prox_scalar_rt) or PX_GROUP
  double* red_n;        // [gridDim.x][8]
};

template <int LB>
__global__ __launch_bounds__(FH_WG) void k_spmc_prologue(const SpmcProP p) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) double s_scr[4 * 8];
  const uint32_t row = blockIdx.x * FH_WG + threadIdx.x;
  double v[7] = {0, 0, 0, 0, 0, 0, 0};   // dxg0, dx2, xh2, g02, gsum, gmax, rdot
  if (row < p.nv) {
    const uint64_t o = (uint64_t)row * LB;
    double x0v[LB], g0v[LB], xh[LB], xq[LB];
#pragma unroll
    for (int l = 0; l < LB; l += 2) {
      const d2 a = *reinterpret_cast<const d2*>(p.x0 + o + l);
      const d2 b = *reinterpret_cast<const d2*>(p.g0 + o + l);
      x0v[l] = a.x; x0v[l + 1] = a.y; g0v[l] = b.x; g0v[l + 1] = b.y;
    }
    const bool rowok = row < p.n;
    double nu2 = 0.0;
#pragma unroll
    for (int l = 0; l < LB; ++l) {
      const bool valid = rowok && (uint32_t)l < p.L;
      xh[l] = valid ? fwd_point(x0v[l], g0v[l], p.tau) : 0.0;
      nu2 += xh[l] * xh[l];
    }
    double scale = 1.0;
    if (p.px.kind == PX_GROUP) {          // the row-wise l2 shrink: shrink the row norm, never divide by zero
      const double nu = sqrt(nu2);
      scale = fmax(nu - p.px.thr, 0.0) / (nu + (nu == 0.0 ? 1.0 : 0.0));
    }
    double pn2 = 0.0;
#pragma unroll
    for (int l = 0; l < LB; ++l) {
      const bool valid = rowok && (uint32_t)l < p.L;
      double q = p.px.kind == PX_GROUP ? xh[l] * scale : prox_scalar_rt(p.px.kind, xh[l], p.px, 0.0);
      if (!valid) q = 0.0;
      xq[l] = q;
      pn2 += q * q;
    }
    // the n-side sums, a column pair at a time next to its 16 bytes of x_accel0
#pragma unroll
    for (int l = 0; l < LB; l += 2) {
      d2 a = {0.0, 0.0};
      if (p.xacc0) a = *reinterpret_cast<const d2*>(p.xacc0 + o + l);
#pragma unroll
      for (int h = 0; h < 2; ++h)
        if (rowok && (uint32_t)(l + h) < p.L) nside_fwd_sums<0>(x0v[l + h], g0v[l + h], xh[l + h], xq[l + h], a[h], v, p.px.kind != PX_GROUP);
    }
    if (p.px.kind == PX_GROUP) v[4] = sqrt(pn2);
#pragma unroll
    for (int l = 0; l < LB; l += 2) {
      *reinterpret_cast<d2*>(p.xhat + o + l) = (d2){xh[l], xh[l + 1]};
      *reinterpret_cast<d2*>(p.xp + o + l) = (d2){xq[l], xq[l + 1]};
    }
  }
  publish_record<7, 5>(v, p.red_n + 1, blockIdx.x, s_scr);
}

// ---- K-fwd --------------------------------------------------------------------------------------------------------------------------------
struct SpmcFwdP {
  SpMatP a;             // A by rows
  uint32_t m, L;
  uint32_t nred_n;      // records of the prologue (0: none ran, the n-side sums are written as zeros)
  const double* x;      // the operand, (nv, LB): xprox from the prologue, or a plain matrix
  const double* b; double* z;
  int sub_b;
  unsigned seq;
  const double* red_n;  // [nred_n][8]
  double* red_m;        // [gridDim.x]
  unsigned* counter;
  double* out;
};

// row epilogue of the lane that owns columns 2c, 2c + 1 of row `row`
template <int LB>
__device__ __forceinline__ void spmc_fwd_row(const SpmcFwdP& p, uint32_t row, uint32_t c, d2 zv, double& fpart) {
  const uint64_t o = (uint64_t)row * LB + 2u * c;
  *reinterpret_cast<d2*>(p.z + o) = zv;
  d2 bv = {0.0, 0.0};
  if (p.sub_b) bv = *reinterpret_cast<const d2*>(p.b + o);
  if (2u * c < p.L) fpart += p.sub_b ? loss_term(zv.x, bv.x, LOSS_LSQ) : zv.x * zv.x;
  if (2u * c + 1u < p.L) fpart += p.sub_b ? loss_term(zv.y, bv.y, LOSS_LSQ) : zv.y * zv.y;
}

template <int G, int LB, int NT>
__global__ __launch_bounds__(FH_WG) void k_spmc_fwd(const SpmcFwdP p) {
  constexpr int C = LB / 2;
  constexpr uint32_t E = G / C, GROUPS = FH_WG / G;
  static_assert(G >= C && G >= 4 && G <= 64, "a group is at least one row of X wide and at most a wave");
  __shared__ __attribute__((aligned(16))) double s_scr[4 * 8];
  __shared__ __attribute__((aligned(16))) double s_col[4 * LB];
  __shared__ __attribute__((aligned(16))) unsigned s_flag[4];
  const uint32_t tid = threadIdx.x;
  const uint32_t gid = tid / G, gl = tid % G;
  const uint32_t c = gl % C, e = gl / C;
  double fpart = 0.0;
  if (blockIdx.x < p.a.nwg) {
    const uint32_t r0 = p.a.part[blockIdx.x], r1 = p.a.part[blockIdx.x + 1];
    for (uint32_t base = r0; base < r1; base += GROUPS) {           // (uniform trip count: the tree needs every lane of the wave)
      const uint32_t row = base + gid;
      long long k0 = 0, k1 = 0;
      if (row < r1) { k0 = p.a.ptr[row]; k1 = p.a.ptr[(size_t)row + 1]; }
      const bool mine = row < r1 && k1 - k0 <= p.a.longer;
      if (!mine) k1 = k0;
      d2 acc = spmc_lane_dot<LB, NT>(p.a, p.x, k0, k1, e, c, E);
      acc.x = spmc_tree<C, G>(acc.x);
      acc.y = spmc_tree<C, G>(acc.y);
      if (mine && e == 0) spmc_fwd_row<LB>(p, row, c, acc, fpart);
    }
  } else {                                                          // one long row, the whole workgroup
    const uint32_t row = p.a.longrows[blockIdx.x - p.a.nwg];
    const d2 zv = spmc_long_row<LB, NT>(p.a, p.x, row, s_col);
    if (tid < (uint32_t)C) spmc_fwd_row<LB>(p, row, tid, zv, fpart);
  }
  // (This kernel keeps its own text of the finaliser -- what finish_records<1, S_GMAX, 8> does, fh_records.h: routed through it, k_spmc_fwd<64, 16, *>
  // takes 66 VGPRs instead of 64 and loses an occupancy step, 8 -> 7 waves per SIMD; profiles/nside_refactor.txt section 3.)
  {
    double v[1] = {fpart};
    block_reduce<1>(v, s_scr, -1);
    if (tid == 0) store_partial(p.red_m + blockIdx.x, v[0]);
  }
  if (arrive_last(p.counter, gridDim.x, s_flag)) {
    double v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (uint32_t i = tid; i < gridDim.x; i += FH_WG) v[0] += load_partial(p.red_m + i);
    for (uint32_t i = tid; i < p.nred_n; i += FH_WG) {
#pragma unroll
      for (int k = 1; k < 8; ++k) {
        const double t = load_partial(p.red_n + (uint64_t)i * 8 + k);
        if (k == S_GMAX) v[k] = fmax(v[k], t); else v[k] += t;
      }
    }
    block_reduce<8>(v, s_scr, S_GMAX);
    if (tid == 0) {
#pragma unroll
      for (int k = 0; k < 8; ++k) scal_store(p.out + k, v[k]);
      scal_store(p.out + S_ALPHA, 0.0);
      publish_seq(p.out, p.seq);
      __hip_atomic_store(p.counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// ---- m-side prologue of the adjoint -------------------------------------------------------------------------------------------------------
struct SpmcResP {
  uint32_t m, L;
  const double* z; const double* zacc0; const double* b;
  double* r;
  int sub_b, accel;
  double coef;
  double* red_f;        // [gridDim.x]
};

template <int LB>
__global__ __launch_bounds__(FH_WG) void k_spmc_resid(const SpmcResP p) {
  constexpr uint32_t C = LB / 2;
  __shared__ __attribute__((aligned(16))) double s_scr[4];
  const uint64_t i = (uint64_t)blockIdx.x * FH_WG + threadIdx.x;      // column pair i % C of row i / C
  double v[1] = {0.0};
  if (i < (uint64_t)p.m * C) {
    const uint32_t c = (uint32_t)(i % C);
    d2 zv = reinterpret_cast<const d2*>(p.z)[i];
    if (p.accel) {
      const d2 za = reinterpret_cast<const d2*>(p.zacc0)[i];
      zv.x = extrapolate(zv.x, za.x, p.coef);
      zv.y = extrapolate(zv.y, za.y, p.coef);
    }
    d2 bv = {0.0, 0.0};
    if (p.sub_b) bv = reinterpret_cast<const d2*>(p.b)[i];
    d2 rv = zv;
    if (p.sub_b) { rv.x = loss_grad(zv.x, bv.x, LOSS_LSQ); rv.y = loss_grad(zv.y, bv.y, LOSS_LSQ); }
    reinterpret_cast<d2*>(p.r)[i] = rv;                                // (padding columns: zeros in, zeros out)
    if (2u * c < p.L) v[0] += p.sub_b ? loss_term(zv.x, bv.x, LOSS_LSQ) : zv.x * zv.x;
    if (2u * c + 1u < p.L) v[0] += p.sub_b ? loss_term(zv.y, bv.y, LOSS_LSQ) : zv.y * zv.y;
  }
  publish_record<1, -1>(v, p.red_f, blockIdx.x, s_scr);
}

// ---- K-adj --------------------------------------------------------------------------------------------------------------------------------
struct SpmcAdjP {
  SpMatP a;             // A^T by rows
  uint32_t n, L;
  uint32_t nred_f;      // records of k_spmc_resid
  const double* r;      // (mv, LB)
  int accel, mode, group;   // mode 0 = FBS (BB epilogue), 1 = plain gradient (g1 only); group: FH_PROX_GROUP's g terms
  unsigned seq;
  double coef, tau;
  const double* x0; const double* xp; const double* xacc0; const double* xhat;
  double* x1; double* g1;
  const double* red_f;  // [nred_f]
  double* red_bb;       // [gridDim.x][8]
  unsigned* counter;
  double* out;
};

// the n-side epilogue of columns 2c, 2c + 1 of row j of G1, in their owner's lane (nside_adj_sums per column).  Returns the pair's share of
// the squared row norm of x1 (valid columns only), which FH_PROX_GROUP sums over the row's column lanes.
template <int LB>
__device__ __forceinline__ double spmc_adj_pair(const SpmcAdjP& p, uint32_t j, uint32_t c, d2 g, double (&v)[5]) {
  const uint64_t o = (uint64_t)j * LB + 2u * c;
  *reinterpret_cast<d2*>(p.g1 + o) = g;
  if (p.mode != 0) return 0.0;
  const d2 x0v = *reinterpret_cast<const d2*>(p.x0 + o);
  const d2 xpv = *reinterpret_cast<const d2*>(p.xp + o);
  const d2 xhv = *reinterpret_cast<const d2*>(p.xhat + o);
  d2 xav = {0.0, 0.0};
  if (p.accel) xav = *reinterpret_cast<const d2*>(p.xacc0 + o);
  d2 x1v;
  double n2 = 0.0;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const bool valid = 2u * c + (uint32_t)h < p.L;
    double x1 = 0.0;
    if (valid) {
      x1 = nside_adj_sums(g[h], x0v[h], xpv[h], xav[h], xhv[h], p.accel, p.coef, p.tau, v, !p.group);
      n2 = add_nofma(n2, x1 * x1);
    }
    x1v[h] = x1;
  }
  if (p.accel) *reinterpret_cast<d2*>(p.x1 + o) = x1v;
  return n2;
}

template <int G, int LB, int NT>
__global__ __launch_bounds__(FH_WG) void k_spmc_adj(const SpmcAdjP p) {
  constexpr int C = LB / 2;
  constexpr uint32_t E = G / C, GROUPS = FH_WG / G;
  static_assert(G >= C && G >= 4 && G <= 64, "a group is at least one row of X wide and at most a wave");
  __shared__ __attribute__((aligned(16))) double s_scr[4 * 8];
  __shared__ __attribute__((aligned(16))) double s_col[4 * LB];
  __shared__ __attribute__((aligned(16))) unsigned s_flag[4];
  const uint32_t tid = threadIdx.x;
  const uint32_t gid = tid / G, gl = tid % G;
  const uint32_t c = gl % C, e = gl / C;
  double v[5] = {0, 0, 0, 0, 0};      // dxdg, dg2, xh2, gsum, gmax
  if (blockIdx.x < p.a.nwg) {
    const uint32_t r0 = p.a.part[blockIdx.x], r1 = p.a.part[blockIdx.x + 1];
    for (uint32_t base = r0; base < r1; base += GROUPS) {
      const uint32_t row = base + gid;
      long long k0 = 0, k1 = 0;
      if (row < r1) { k0 = p.a.ptr[row]; k1 = p.a.ptr[(size_t)row + 1]; }
      const bool mine = row < r1 && k1 - k0 <= p.a.longer;
      if (!mine) k1 = k0;
      d2 acc = spmc_lane_dot<LB, NT>(p.a, p.r, k0, k1, e, c, E);
      acc.x = spmc_tree<C, G>(acc.x);
      acc.y = spmc_tree<C, G>(acc.y);
      double n2 = 0.0;
      if (mine && e == 0) n2 = spmc_adj_pair<LB>(p, row, c, acc, v);
      if (p.group && p.mode == 0) {                                  // (launch-uniform: every lane of the wave takes the tree)
        n2 = spmc_tree<1, C>(n2);
        if (mine && gl == 0) v[3] += sqrt(n2);
      }
    }
  } else {
    const uint32_t row = p.a.longrows[blockIdx.x - p.a.nwg];
    const d2 g = spmc_long_row<LB, NT>(p.a, p.r, row, s_col);
    double n2 = 0.0;
    if (tid < (uint32_t)C) n2 = spmc_adj_pair<LB>(p, row, tid, g, v);
    if (p.group && p.mode == 0) {
      n2 = spmc_tree<1, C>(n2);
      if (tid == 0) v[3] += sqrt(n2);
    }
  }
  finish_records<5, 4, 6>(v, p.red_bb, blockIdx.x, gridDim.x, p.counter, p.out, p.seq, s_scr, s_flag,
                          [&](double (&w)[6]) { add_column(w[5], p.red_f, p.nred_f); },      // fsq: k_spmc_resid's records
                          [&](double (&w)[6]) { store_adj_scalars(p.out, w); });
}

// ---- the instantiations (ONE table for fh_spmulti_part.hip, the extern declarations and the dispatch) ----
// X(G, LB): G from max(4, LB / 2) to 64
#define SPMC_FOR_EACH_LB(X) X(2) X(4) X(8) X(16)
#define SPMC_FOR_EACH(X)                          \
  X(4, 2) X(8, 2) X(16, 2) X(32, 2) X(64, 2)      \
  X(4, 4) X(8, 4) X(16, 4) X(32, 4) X(64, 4)      \
  X(4, 8) X(8, 8) X(16, 8) X(32, 8) X(64, 8)      \
  X(8, 16) X(16, 16) X(32, 16) X(64, 16)
#define SPMC_LB_KERNELS(DO, LB)                               \
  DO __global__ void k_spmc_prologue<LB>(const SpmcProP);     \
  DO __global__ void k_spmc_resid<LB>(const SpmcResP);
#define SPMC_KERNELS(DO, G, LB)                               \
  DO __global__ void k_spmc_fwd<G, LB, 0>(const SpmcFwdP);    \
  DO __global__ void k_spmc_fwd<G, LB, 1>(const SpmcFwdP);    \
  DO __global__ void k_spmc_adj<G, LB, 0>(const SpmcAdjP);    \
  DO __global__ void k_spmc_adj<G, LB, 1>(const SpmcAdjP);

// fh_sparse.h -- kernels for a SPARSE operator and a VECTOR unknown (fh_set_matrix_csr; a matrix unknown over the same two copies: fh_spmulti.h): the library keeps A by rows (CSR) and A^T by rows (the CSC of A, built by
// a stable counting sort, so every column lists its entries in ascending row order), and BOTH directions are gathers over "rows" of one of the
// two copies.  No atomics, every sum has a fixed order: bitwise repeatable, like every other kernel of the library.
//
// Device layout (private to this header and its launchers): ptr[rows + 1] 64-bit entry offsets, idx[nnz] 32-bit column (row) numbers, val[nnz]
// float64.  Vectors keep the vector form's padded layout; their padding is zero on allocation and no kernel here writes it.
//
//   k_sp_prologue  n-side prologue as its own small launch, one lane per element: xhat = x0 - tau*g0, xprox = prox_scalar(xhat) -- the same
//                  device functions, FMA contraction off, as the vector kernels, so the outputs are bit-exact -- and the seven n-side sums
//                  of k_fwd_dense, one record per workgroup.  Plain operands (fh_init, fh_apply, fh_gradient_at) skip it.
//   k_sp_fwd<G>    z = A * operand.  G in {4, 8, 16, 32, 64} lanes of a wave own one row (chosen on the host from the mean row length); the
//                  rows are dealt to the workgroups in contiguous ranges balanced by their non-zeros (computed once, at set-matrix time).  A row
//                  much longer than the mean (SpMatP.longer: more than 64 * G and more than 16 mean rows) is left out of the ranges and walked
//                  by a whole workgroup of its own (blocks behind the range blocks), so one dense row does not serialise the launch.  Row order of a sum: lane partials (entries k, k + G,
//                  ...), then an xor tree over the group's lanes (DPP inside 16 lanes, a shuffle across).  Row epilogue: z and the loss term.
//   k_sp_resid     m-side prologue of the adjoint: r = grad f(z') with z' = z or its FISTA extrapolation -- whose coefficient is only known
//                  when the adjoint is launched, which is why the residual is formed here and not in K-fwd's row epilogue -- and the loss sum
//                  at z' (FH_S_FSQ_ADJ), one record per workgroup.  One read of z [, zacc0], b and one write of r: 32 bytes per ROW.
//   k_sp_adj<G>    g1 = A^T * r, the same gather over the A^T copy.  Every g1_j has exactly one owner, so the n-side epilogue (Dg, <Dx,Dg>,
//                  ||Dg||^2, the FISTA extrapolation of x, the g terms of x1) runs in the owner's lane: no slab partials.
// Finalisers are arrive_last only: no spin waits, no co-residency assumption.  All entry offsets are 64-bit; idx stays 32-bit.
// Loads: val / idx stream once and were the non-temporal candidates; measured, NT = 1 is never faster than plain loads here (profiles/sparse_rows.txt),
// so NT = 0 is what the launchers pick and NT = 1 stays behind FH_TUNE_NT_LOADS.  The gathered operand keeps the default policy -- it is what the caches are for.
#pragma once
#include "fh_dense.h"

#define SP_LONG_FACTOR 64          // a row of more than max(SP_LONG_FACTOR * G, SP_LONG_MEANS * mean row length) entries gets a workgroup of its own
#define SP_LONG_MEANS 16           // (G stops at 64: without the second term every row of a matrix with more than 4096 entries per row would count as long)

struct SpMatP {
  const long long* ptr;            // [rows + 1]
  const int* idx;                  // [nnz]
  const double* val;               // [nnz]
  const uint32_t* part;            // [nwg + 1]: workgroup w owns rows [part[w], part[w + 1])
  const uint32_t* longrows;        // [nlong]: the rows left to whole workgroups (blocks nwg .. nwg + nlong - 1)
  uint32_t rows, nwg, nlong;
  long long longer;                // the threshold above, fixed at set-matrix time
};

template <int NT> __device__ __forceinline__ double sp_val(const double* p) { return NT ? FH_NT_LOAD(p) : *p; }
template <int NT> __device__ __forceinline__ int sp_idx(const int* p) { return NT ? FH_NT_LOAD(p) : *p; }

// sum over the G lanes of a group (G consecutive lanes, aligned); every lane of the group ends up with the sum.  ALL lanes of the wave must be active.
template <int G>
__device__ __forceinline__ double sp_group_sum(double v) {
  v += dpp_f64<0xB1>(v);                       // quad_perm [1,0,3,2]
  v += dpp_f64<0x4E>(v);                       // quad_perm [2,3,0,1]
  if (G >= 8) v += dpp_f64<0x141>(v);          // row_half_mirror
  if (G >= 16) v += dpp_f64<0x140>(v);         // row_mirror
  if (G >= 32) v += __shfl_xor(v, 16, 64);
  if (G >= 64) v += __shfl_xor(v, 32, 64);
  return v;
}

// this lane's share of row [k0, k1): entries k0 + gl, k0 + gl + STRIDE, ...
template <int NT>
__device__ __forceinline__ double sp_lane_dot(const SpMatP& a, const double* x, long long k0, long long k1, uint32_t gl, uint32_t stride) {
  double acc = 0.0;
#pragma unroll 4
  for (long long k = k0 + gl; k < k1; k += stride) {
    const int j = sp_idx<NT>(a.idx + k);
    const double av = sp_val<NT>(a.val + k);
    acc = fma(av, x[(size_t)j], acc);
  }
  return acc;
}

// ---- n-side prologue ----------------------------------------------------------------------------------------------------------------------
struct SpProP {
  uint32_t n;
  const double* x0; const double* g0; const double* xacc0;
  double* xhat; double* xp;
  double tau;
  ProxP px;             // IDENTITY / SHRINK / NONNEG / BOX
  double* red_n;        // [gridDim.x][8]
};

static __global__ __launch_bounds__(FH_WG) void k_sp_prologue(const SpProP p) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) double s_scr[4 * 8];
  const uint32_t j = blockIdx.x * FH_WG + threadIdx.x;
  double v[7] = {0, 0, 0, 0, 0, 0, 0};   // dxg0, dx2, xh2, g02, gsum, gmax, rdot
  if (j < p.n) {
    const double x0e = p.x0[j], g0e = p.g0[j];
    const double xav = p.xacc0 ? p.xacc0[j] : 0.0;
    const double xhe = fwd_point(x0e, g0e, p.tau);
    const double xpe = prox_scalar_rt(p.px.kind, xhe, p.px, 0.0);
    nside_fwd_sums<0>(x0e, g0e, xhe, xpe, xav, v);
    p.xhat[j] = xhe;
    p.xp[j] = xpe;
  }
  publish_record<7, 5>(v, p.red_n + 1, blockIdx.x, s_scr);
}

// ---- K-fwd --------------------------------------------------------------------------------------------------------------------------------
struct SpFwdP {
  SpMatP a;             // A by rows
  uint32_t m;
  uint32_t nred_n;      // records of the prologue (0: none ran, the n-side sums are written as zeros)
  const double* x;      // the operand: xprox from the prologue, or a plain vector
  const double* b; double* z;
  int sub_b, loss;
  unsigned seq;
  const double* red_n;  // [nred_n][8]
  double* red_m;        // [gridDim.x]
  unsigned* counter;
  double* out;
};

template <int G, int NT>
__global__ __launch_bounds__(FH_WG) void k_sp_fwd(const SpFwdP p) {
  constexpr uint32_t GROUPS = FH_WG / G;
  __shared__ __attribute__((aligned(16))) double s_scr[4 * 8];
  __shared__ __attribute__((aligned(16))) unsigned s_flag[4];
  const uint32_t tid = threadIdx.x;
  const uint32_t gid = tid / G, gl = tid % G;
  double fpart = 0.0;
  if (blockIdx.x < p.a.nwg) {
    const uint32_t r0 = p.a.part[blockIdx.x], r1 = p.a.part[blockIdx.x + 1];
    for (uint32_t base = r0; base < r1; base += GROUPS) {           // (uniform trip count: the group sum needs every lane of the wave)
      const uint32_t row = base + gid;
      long long k0 = 0, k1 = 0;
      if (row < r1) { k0 = p.a.ptr[row]; k1 = p.a.ptr[(size_t)row + 1]; }
      const bool mine = row < r1 && k1 - k0 <= p.a.longer;
      if (!mine) k1 = k0;
      const double zv = sp_group_sum<G>(sp_lane_dot<NT>(p.a, p.x, k0, k1, gl, G));
      if (mine && gl == 0) {
        p.z[row] = zv;
        fpart += p.sub_b ? loss_term(zv, p.b[row], p.loss) : zv * zv;
      }
    }
  } else {                                                          // one long row, the whole workgroup
    const uint32_t row = p.a.longrows[blockIdx.x - p.a.nwg];
    double v[1] = {sp_lane_dot<NT>(p.a, p.x, p.a.ptr[row], p.a.ptr[(size_t)row + 1], tid, FH_WG)};
    block_reduce<1>(v, s_scr, -1);
    if (tid == 0) {
      p.z[row] = v[0];
      fpart += p.sub_b ? loss_term(v[0], p.b[row], p.loss) : v[0] * v[0];
    }
  }
  double v[1] = {fpart};
  finish_records<1, S_GMAX, 8>(v, p.red_m, blockIdx.x, gridDim.x, p.counter, p.out, p.seq, s_scr, s_flag,
                               [&](double (&w)[8]) { add_records<1, 8, S_GMAX>(w, p.red_n, p.nred_n); },
                               [&](double (&w)[8]) { store_fwd_scalars(p.out, w, 0.0); });
}

// ---- m-side prologue of the adjoint -------------------------------------------------------------------------------------------------------
struct SpResP {
  uint32_t m;
  const double* z; const double* zacc0; const double* b;
  double* r;
  int sub_b, loss, accel;
  double coef;
  double* red_f;        // [gridDim.x]
};

static __global__ __launch_bounds__(FH_WG) void k_sp_resid(const SpResP p) {
  __shared__ __attribute__((aligned(16))) double s_scr[4];
  const uint32_t i = blockIdx.x * FH_WG + threadIdx.x;
  double v[1] = {0.0};
  if (i < p.m) {
    double zv = p.z[i];
    if (p.accel) zv = extrapolate(zv, p.zacc0[i], p.coef);
    const double bv = p.sub_b ? p.b[i] : 0.0;
    p.r[i] = p.sub_b ? loss_grad(zv, bv, p.loss) : zv;
    v[0] = p.sub_b ? loss_term(zv, bv, p.loss) : zv * zv;
  }
  block_reduce<1>(v, s_scr, -1);
  if (threadIdx.x == 0) store_partial(p.red_f + blockIdx.x, v[0]);
}

// ---- K-adj --------------------------------------------------------------------------------------------------------------------------------
struct SpAdjP {
  SpMatP a;             // A^T by rows
  uint32_t n;
  uint32_t nred_f;      // records of k_sp_resid
  const double* r;
  int accel, mode;      // mode 0 = FBS (BB epilogue), 1 = plain gradient (g1 only)
  unsigned seq;
  double coef, tau;
  const double* x0; const double* xp; const double* xacc0; const double* xhat;
  double* x1; double* g1;
  const double* red_f;  // [nred_f]
  double* red_bb;       // [gridDim.x][8]
  unsigned* counter;
  double* out;
};

// g1 and the n-side epilogue of one element, in its owner's lane
__device__ __forceinline__ void sp_adj_element(const SpAdjP& p, uint32_t j, double g, double (&v)[5]) {
  p.g1[j] = g;
  if (p.mode != 0) return;
  const double x1 = nside_adj_sums(g, p.x0[j], p.xp[j], p.accel ? p.xacc0[j] : 0.0, p.xhat[j], p.accel, p.coef, p.tau, v);
  if (p.accel) p.x1[j] = x1;
}

template <int G, int NT>
__global__ __launch_bounds__(FH_WG) void k_sp_adj(const SpAdjP p) {
  constexpr uint32_t GROUPS = FH_WG / G;
  __shared__ __attribute__((aligned(16))) double s_scr[4 * 8];
  __shared__ __attribute__((aligned(16))) unsigned s_flag[4];
  const uint32_t tid = threadIdx.x;
  const uint32_t gid = tid / G, gl = tid % G;
  double v[5] = {0, 0, 0, 0, 0};      // dxdg, dg2, xh2, gsum, gmax
  if (blockIdx.x < p.a.nwg) {
    const uint32_t r0 = p.a.part[blockIdx.x], r1 = p.a.part[blockIdx.x + 1];
    for (uint32_t base = r0; base < r1; base += GROUPS) {
      const uint32_t row = base + gid;
      long long k0 = 0, k1 = 0;
      if (row < r1) { k0 = p.a.ptr[row]; k1 = p.a.ptr[(size_t)row + 1]; }
      const bool mine = row < r1 && k1 - k0 <= p.a.longer;
      if (!mine) k1 = k0;
      const double g = sp_group_sum<G>(sp_lane_dot<NT>(p.a, p.r, k0, k1, gl, G));
      if (mine && gl == 0) sp_adj_element(p, row, g, v);
    }
  } else {
    const uint32_t row = p.a.longrows[blockIdx.x - p.a.nwg];
    double w[1] = {sp_lane_dot<NT>(p.a, p.r, p.a.ptr[row], p.a.ptr[(size_t)row + 1], tid, FH_WG)};
    block_reduce<1>(w, s_scr, -1);
    if (tid == 0) sp_adj_element(p, row, w[0], v);
  }
  finish_records<5, 4, 6>(v, p.red_bb, blockIdx.x, gridDim.x, p.counter, p.out, p.seq, s_scr, s_flag,
                          [&](double (&w)[6]) { add_column(w[5], p.red_f, p.nred_f); },      // fsq: k_sp_resid's records
                          [&](double (&w)[6]) { store_adj_scalars(p.out, w); });
}

// ---- the instantiations (ONE table for fh_sparse_part.hip, the extern declarations and the dispatch) ----
#define SP_FOR_EACH(X) X(4) X(8) X(16) X(32) X(64)
#define SP_KERNELS(DO, G)                                  \
  DO __global__ void k_sp_fwd<G, 0>(const SpFwdP);         \
  DO __global__ void k_sp_fwd<G, 1>(const SpFwdP);         \
  DO __global__ void k_sp_adj<G, 0>(const SpAdjP);         \
  DO __global__ void k_sp_adj<G, 1>(const SpAdjP);

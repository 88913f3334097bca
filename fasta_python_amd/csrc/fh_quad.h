// fh_quad.h -- kernels for a QUADRATIC smooth term on an explicit symmetric matrix: f(X) = .5 <X, Q X> + <C, X>, X an (n, L) matrix (L = 1: a vector
// unknown), Q (n, n) symmetric and possibly indefinite, A = identity (fh_set_quadratic; examples/max_norm.py:49-50 with Q = S + S^T, the dual of
// examples/svm.py:68-69 with Q = (l l^T) o (D D^T) and C = -1).
//
// ONE product W = Q X gives both the value .5 <X, W> + <C, X> and the gradient W + C, so an attempt of the step costs one read of Q (n^2 * 8 bytes)
// and the second direction is an elementwise launch that never touches the matrix.  Device layout: the multi-column form's (csrc/fh_multi.h):
// every matrix is rows of LB doubles, LB in {2, 4, 8, 16} the smallest of them >= L, padding rows and padding columns zero; Q is stored like a
// dense A, W lives in the m-side buffers (m = n), C in the buffer of b.
//
//   k_qd_prologue  k_mc_prologue with one more prox: one lane per ROW of X, xhat = x0 - tau*g0, xprox = prox(xhat) -- elementwise kinds through
//                  prox_scalar_rt, FH_PROX_GROUP and FH_PROX_ROWBALL (examples/max_norm.py:53-59) from the row norm, once per row -- the seven
//                  n-side sums, and xprox once more in K-fwd's streaming layout.
//   k_qd_fwd       W = Q * Xprox with k_mc_fwd's streaming loop (a workgroup owns R whole rows per pass, lanes walk the row in 16-byte pieces,
//                  reduce-scatter, the waves in order, columns split at LB = 16).  The row epilogue is its own: it writes W and adds
//                  xprox[i,l] * (.5 * w[i,l] + c[i,l]) over the valid entries, xprox read from the row-major copy.  Last workgroup: the
//                  m-side records, then the prologue's records, in index order.
//   k_qd_grad      the adjoint direction, elementwise, one lane per row: w' = w or its FISTA extrapolation (Q is linear: that IS Q applied to
//                  the extrapolated iterate), g1 = w' + c, the n-side epilogue (fh_nside.h), and FH_S_FSQ_ADJ = sum x1' * (.5 * w' + c).  Never reads Q.
// Finalisers are arrive_last only: no spin waits, no co-residency assumption.  No float atomics: bitwise repeatable.
#pragma once
#include "fh_multi.h"

#define PX_ROWBALL 8
#define LOSS_QUAD 2

// ---- n-side prologue ----------------------------------------------------------------------------------------------------------------------
// (McProP; for PX_ROWBALL px.thr carries mu itself -- the radius does not scale with the step, examples/max_norm.py:57-59)
template <int LB>
__global__ __launch_bounds__(FH_WG) void k_qd_prologue(const McProP p) {
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
    const bool rownorm = p.px.kind == PX_GROUP || p.px.kind == PX_ROWBALL;
    double scale = 1.0, den = 1.0;
    if (rownorm) {
      const double nu = sqrt(nu2);
      const double one = nu == 0.0 ? 1.0 : 0.0;                                  // never divide by zero: a zero row stays zero
      scale = fmax(nu - p.px.thr, 0.0) / (nu + one);                             // examples/mmv.py:53-59
      den = fmax(nu, p.px.thr) + one;                                            // examples/max_norm.py:57
    }
    double pn2 = 0.0;
#pragma unroll
    for (int l = 0; l < LB; ++l) {
      const bool valid = rowok && (uint32_t)l < p.L;
      double q;
      if (p.px.kind == PX_GROUP) q = xh[l] * scale;
      else if (p.px.kind == PX_ROWBALL) q = (p.px.thr * xh[l]) / den;            // examples/max_norm.py:59: mu * X / scale
      else q = prox_scalar_rt(p.px.kind, xh[l], p.px, 0.0);
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
    mc_pack_row<LB>(p.xs, p.ld2, row, xq);
  }
  publish_record<7, 5>(v, p.red_n + 1, blockIdx.x, s_scr);
}

// one entry's share of f: x * (.5 * w + c), three roundings
__device__ __forceinline__ double qd_term(double x, double w, double c) {
#pragma clang fp contract(off)
  const double h = 0.5 * w;
  const double s = h + c;
  return x * s;
}

// ---- K-fwd: W = Q * X, LB columns -----------------------------------------------------------------------------------------------------------
struct QdFwdP {
  const double* Q;
  uint32_t ld2;         // 16-byte pieces per device row of Q
  uint32_t n, L;        // logical rows of Q / columns of X
  uint32_t nrg;         // row groups = mp / R
  uint32_t nred_n;      // records of the prologue (0: no prologue ran, the n-side sums are written as zeros)
  const double* x;      // the operand in the streaming layout (mc_pack_row)
  const double* xrow;   // the same operand row-major, (.., LB): the factor of the loss sum
  const double* c;      // linear term, (.., LB), zeros when none was given
  double* w;
  int with_f;           // 0: the product alone (fh_apply)
  unsigned seq;
  const double* red_n;  // [nred_n][8]
  double* red_m;        // [gridDim.x]
  unsigned* counter;
  double* out;
};

// (k_mc_fwd's loop and its register shapes, csrc/fh_multi.h: the column split at LB = 16 and the occupancy hint are explained there)
template <int LB, int CH, int R, int NT>
__global__ __launch_bounds__(FH_WG) __attribute__((amdgpu_waves_per_eu(1, 2))) void k_qd_fwd(const QdFwdP p) {
  constexpr int NG = LB / CH;          // column groups
  constexpr int GL = FH_WG / NG;       // lanes per group
  constexpr int WPG = 4 / NG;          // waves per group
  constexpr int N = R * CH;            // accumulators per lane
  __shared__ __attribute__((aligned(16))) double s_part[4 * N];
  __shared__ __attribute__((aligned(16))) double s_scr[4 * 8];
  __shared__ __attribute__((aligned(16))) unsigned s_flag[4];
  const uint32_t tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const uint32_t grp = tid / GL, gl = tid % GL;
  const int base = mc_rs_base<N>(lane);
  const d2* xe = reinterpret_cast<const d2*>(p.x) + (uint64_t)(grp * (CH / 2)) * p.ld2;              // this group's planes of the even rows
  const d2* xo = reinterpret_cast<const d2*>(p.x) + (uint64_t)(LB / 2 + grp * (CH / 2)) * p.ld2;     // ... and of the odd rows
  double fpart = 0.0;
  const uint32_t ntrip = (p.ld2 + GL - 1) / GL;
  for (uint32_t rg = blockIdx.x; rg < p.nrg; rg += gridDim.x) {
    const d2* Qb = reinterpret_cast<const d2*>(p.Q) + (uint64_t)rg * R * p.ld2;
    double acc[N];
#pragma unroll
    for (int i = 0; i < N; ++i) acc[i] = 0.0;
    for (uint32_t t = 0; t < ntrip; ++t) {
      const uint32_t c0 = t * GL + gl;
      const bool ok = c0 < p.ld2;
      const uint32_t k0 = ok ? c0 : 0u;                      // clamp: in-bounds redundant loads, zero x
      d2 a[R];
#pragma unroll
      for (int r = 0; r < R; ++r) a[r] = load_stream<NT>(Qb + (uint64_t)r * p.ld2 + k0);
      d2 xa[CH / 2], xb[CH / 2];
#pragma unroll
      for (int l = 0; l < CH / 2; ++l) {
        xa[l] = xe[(uint64_t)l * p.ld2 + k0]; xb[l] = xo[(uint64_t)l * p.ld2 + k0];
        if (!ok) { xa[l] = (d2){0.0, 0.0}; xb[l] = (d2){0.0, 0.0}; }
      }
#pragma unroll
      for (int r = 0; r < R; ++r) {
#pragma unroll
        for (int l = 0; l < CH / 2; ++l) {
          acc[r * CH + 2 * l] = fma(a[r].y, xb[l].x, fma(a[r].x, xa[l].x, acc[r * CH + 2 * l]));
          acc[r * CH + 2 * l + 1] = fma(a[r].y, xb[l].y, fma(a[r].x, xa[l].y, acc[r * CH + 2 * l + 1]));
        }
      }
    }
    mc_reduce_scatter<N>(acc, lane);
    if (N >= 64) {
#pragma unroll
      for (int i = 0; i < (N >= 64 ? N / 64 : 1); ++i) s_part[wave * N + base + i] = acc[i];
    } else if (lane < N) {
      s_part[wave * N + base] = acc[0];                      // (lanes l and l + N hold the same sums)
    }
    __syncthreads();
    if (tid < N * NG) {
      const uint32_t g = tid / N, idx = tid % N;
      double wv = s_part[(g * WPG) * N + idx];
#pragma unroll
      for (int w = 1; w < WPG; ++w) wv += s_part[(g * WPG + w) * N + idx];       // the group's waves in order
      const uint32_t row = rg * R + idx / CH, col = g * CH + idx % CH;
      const uint64_t o = (uint64_t)row * LB + col;
      p.w[o] = wv;
      if (p.with_f && row < p.n && col < p.L) fpart += qd_term(p.xrow[o], wv, p.c[o]);
    }
    __syncthreads();
  }
  // (This kernel keeps its own text of the finaliser -- what finish_records<1, S_GMAX, 8> does, fh_records.h: routed through it, a small K-fwd
  // (n = 512 .. 1024, L = 4) measured 0.25 us slower on the MI355X, below the parent's band; profiles/nside_refactor.txt section 6.)
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

// ---- the adjoint direction: elementwise ---------------------------------------------------------------------------------------------------
struct QdGradP {
  uint32_t n, L;        // logical rows / columns
  uint32_t rows;        // device rows of W (every lane of the grid owns one)
  const double* w; const double* wacc0; const double* c;
  int accel, mode, group;             // mode 0 = FBS (BB epilogue), 1 = plain gradient (g1 only, the sums are published as zeros); group: FH_PROX_GROUP's g terms
  unsigned seq;
  double coef, tau;
  const double* x0; const double* xp; const double* xacc0; const double* xhat;
  double* x1; double* g1;
  double* red;          // [gridDim.x][8]
  unsigned* counter;
  double* out;
};

template <int LB>
__global__ __launch_bounds__(FH_WG) void k_qd_grad(const QdGradP p) {
  __shared__ __attribute__((aligned(16))) double s_scr[4 * 8];
  __shared__ __attribute__((aligned(16))) unsigned s_flag[4];
  const uint32_t tid = threadIdx.x;
  const uint32_t row = blockIdx.x * FH_WG + tid;
  double v[6] = {0, 0, 0, 0, 0, 0};      // dxdg, dg2, xh2, gsum, gmax, f
  if (row < p.rows) {
    const uint64_t o = (uint64_t)row * LB;
    double n2 = 0.0;
#pragma unroll
    for (int l = 0; l < LB / 2; ++l) {
      const d2 wv = *reinterpret_cast<const d2*>(p.w + o + 2 * l);
      const d2 cv = *reinterpret_cast<const d2*>(p.c + o + 2 * l);
      d2 wa = {0.0, 0.0};
      if (p.accel) wa = *reinterpret_cast<const d2*>(p.wacc0 + o + 2 * l);
      d2 x0v = {0.0, 0.0}, xpv = {0.0, 0.0}, xhv = {0.0, 0.0}, xav = {0.0, 0.0};
      if (p.mode == 0) {
        x0v = *reinterpret_cast<const d2*>(p.x0 + o + 2 * l);
        xpv = *reinterpret_cast<const d2*>(p.xp + o + 2 * l);
        xhv = *reinterpret_cast<const d2*>(p.xhat + o + 2 * l);
        if (p.accel) xav = *reinterpret_cast<const d2*>(p.xacc0 + o + 2 * l);
      }
      d2 gv, x1v;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const bool valid = row < p.n && (uint32_t)(2 * l + h) < p.L;
        double we = wv[h];
        if (p.accel) we = extrapolate(wv[h], wa[h], p.coef);
        const double g = valid ? add_nofma(we, cv[h]) : 0.0;
        gv[h] = g;
        double x1 = 0.0;
        if (valid && p.mode == 0) {
          x1 = nside_adj_sums(g, x0v[h], xpv[h], xav[h], xhv[h], p.accel, p.coef, p.tau, v, !p.group);
          n2 = add_nofma(n2, x1 * x1);
          v[5] = add_nofma(v[5], qd_term(x1, we, cv[h]));
        }
        x1v[h] = x1;
      }
      *reinterpret_cast<d2*>(p.g1 + o + 2 * l) = gv;
      if (p.mode == 0 && p.accel) *reinterpret_cast<d2*>(p.x1 + o + 2 * l) = x1v;
    }
    if (p.mode == 0 && p.group) v[3] += sqrt(n2);
  }
  finish_records<6, 4>(v, p.red, blockIdx.x, gridDim.x, p.counter, p.out, p.seq, s_scr, s_flag, NoRecords(),
                       [&](double (&w)[6]) { store_adj_scalars(p.out, w); });
}

// ---- the instantiations: MC_FOR_EACH's shapes (ONE table for fh_quad_part.hip, the extern declarations and the dispatch) ----
#define QD_KERNELS(DO, LB, CH, R)                                         \
  DO __global__ void k_qd_prologue<LB>(const McProP);                     \
  DO __global__ void k_qd_fwd<LB, CH, R, 0>(const QdFwdP);                \
  DO __global__ void k_qd_fwd<LB, CH, R, 1>(const QdFwdP);                \
  DO __global__ void k_qd_grad<LB>(const QdGradP);

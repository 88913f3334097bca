// fh_bilinear.h -- kernels for a BILINEAR smooth term: f(Z) = .5 ||S - X Y^T||_F^2 with Z = [X; Y], X (m, K), Y (n, K), S (m, n) dense float64,
// A = identity (fh_set_factorization; the reference's examples/nn_factorization.py:48-57).  gradf(Z) = [d Y; d^T X] with d = X Y^T - S.
//
// ONE read of S at a point Z gives the value and both halves of the gradient; d is formed piece by piece in registers and never written.
// Device layout: the multi-column form's (csrc/fh_multi.h): Z and everything of its shape is (m + n) rows of LB doubles, LB in {2, 4, 8, 16} the
// smallest of them >= K, padding rows and padding columns zero; S is stored like a dense A (mp rows of ld doubles, zero padding).
//
//   k_bl_prologue  k_mc_prologue without the row-norm kind and without the streaming copy, plus the SPLIT prox (FH_PROX_ROWSPLIT): rows
//                  [0, split) take one elementwise kind with its parameters, rows [split, ..) another, each through prox_scalar_rt; the l1 sum
//                  FH_S_GSUM then runs over the top rows only.  One lane per row, the seven n-side sums, one record per workgroup.
//   k_bl_pass      the pass over S.  A work item is a row panel (PR rows) x a column tile (BL_TC = 512 columns: ONE 16-byte piece of a row of S per
//                  lane); a workgroup strides over the items.  A lane keeps the two rows of Y that belong to its two columns (2 LB doubles) and
//                  their GY sums (2 LB doubles) in registers for the whole panel and walks down the panel RB = bl_ns(LB) / LB rows at a time:
//                  d = X_i . Y_j - S_ij (fma chain over the columns in order, started from -S_ij), f += d^2, GY_j += d X_i, and the RB x LB
//                  products d Y_j of a chunk, summed over the lane's two columns, go through fh_multi.h's wave reduce-scatter and then over the
//                  four waves in order (LDS, double-buffered: one barrier per chunk) into the GX partial of (tile, row).  GRAD = 0 leaves out
//                  everything but d and f: the value alone, with the SAME bits of f (same chain, same order).  No atomics on floats: GX is
//                  written once per (column tile, row), GY once per (row panel, column); k_bl_grad adds them in index order.
//   k_bl_extrap    x1 = xprox + coef (xprox - xacc0): the point of the second pass of an accelerated step (the form is not linear: the
//                  gradient at the extrapolated point is not the extrapolation of two gradients).
//   k_bl_grad      the n-side epilogue, elementwise, one lane per row of Z: g1 = the sum of that row's partials in index order (column tiles
//                  for a row of X, row panels for a row of Y), the n-side sums (fh_nside.h), FH_S_FSQ_ADJ = f of the pass that produced the partials.
// Finalisers are arrive_last only: no spin waits, no co-residency assumption.  Bitwise repeatable run to run.
#pragma once
#include "fh_quad.h"

#define PX_ROWSPLIT 9
#define LOSS_BILINEAR 3
#define BL_TC 512       // columns of S per work item: FH_WG lanes x one 16-byte piece
#define BL_N 32         // GX sums of a chunk that go through the reduce-scatter: RB = bl_ns(LB) / LB rows of S per chunk
// (16 at LB = 16: with 32 the lane's Y rows, GY sums and chunk products are 128 doubles, past the 256 registers multiply-adds can address)
static constexpr int bl_ns(int LB) { return LB == 16 ? 16 : BL_N; }

// ---- n-side prologue ----------------------------------------------------------------------------------------------------------------------
struct BlProP {
  McProP a;             // (a.px: the prox of all rows, or of the top rows; a.xs / a.ld2 unused)
  ProxP bot;            // rowsplit: the prox of rows [split, n)
  uint32_t split;
  int rowsplit;
};

template <int LB>
__global__ __launch_bounds__(FH_WG) void k_bl_prologue(const BlProP p) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) double s_scr[4 * 8];
  const uint32_t row = blockIdx.x * FH_WG + threadIdx.x;
  double v[7] = {0, 0, 0, 0, 0, 0, 0};   // dxg0, dx2, xh2, g02, gsum, gmax, rdot
  if (row < p.a.nv) {
    const uint64_t o = (uint64_t)row * LB;
    double x0v[LB], g0v[LB], xh[LB], xq[LB];
#pragma unroll
    for (int l = 0; l < LB; l += 2) {
      const d2 a = *reinterpret_cast<const d2*>(p.a.x0 + o + l);
      const d2 b = *reinterpret_cast<const d2*>(p.a.g0 + o + l);
      x0v[l] = a.x; x0v[l + 1] = a.y; g0v[l] = b.x; g0v[l + 1] = b.y;
    }
    const bool rowok = row < p.a.n;
    const bool top = !p.rowsplit || row < p.split;
    const ProxP px = top ? p.a.px : p.bot;
#pragma unroll
    for (int l = 0; l < LB; ++l) {
      const bool valid = rowok && (uint32_t)l < p.a.L;
      xh[l] = valid ? fwd_point(x0v[l], g0v[l], p.a.tau) : 0.0;
      double q = prox_scalar_rt(px.kind, xh[l], px, 0.0);
      if (!valid) q = 0.0;
      xq[l] = q;
    }
    // the n-side sums, a column pair at a time next to its 16 bytes of x_accel0
#pragma unroll
    for (int l = 0; l < LB; l += 2) {
      d2 a = {0.0, 0.0};
      if (p.a.xacc0) a = *reinterpret_cast<const d2*>(p.a.xacc0 + o + l);
#pragma unroll
      for (int h = 0; h < 2; ++h)
        if (rowok && (uint32_t)(l + h) < p.a.L) nside_fwd_sums<0>(x0v[l + h], g0v[l + h], xh[l + h], xq[l + h], a[h], v, top);
    }
#pragma unroll
    for (int l = 0; l < LB; l += 2) {
      *reinterpret_cast<d2*>(p.a.xhat + o + l) = (d2){xh[l], xh[l + 1]};
      *reinterpret_cast<d2*>(p.a.xp + o + l) = (d2){xq[l], xq[l + 1]};
    }
  }
  publish_record<7, 5>(v, p.a.red_n + 1, blockIdx.x, s_scr);
}

// ---- the pass over S ----------------------------------------------------------------------------------------------------------------------------
struct BlPassP {
  const double* S;
  uint32_t ld2;         // 16-byte pieces per device row of S
  uint32_t m, n, L;     // logical rows / columns of S, columns of the factors
  uint32_t pr;          // rows of a panel (a multiple of 16)
  uint32_t nrp, nct;    // row panels, column tiles: nrp * nct work items, item = panel * nct + tile
  const double* z;      // the point: rows [0, m) = X, rows [m, m + n) = Y, LB doubles each
  double* px;           // GX partials [nct][m][LB]
  double* py;           // GY partials [nrp][n][LB]
  double* fout;         // f at the point, kept on the device for k_bl_grad (FH_S_FSQ_ADJ)
  int publish;          // 1: the finaliser writes the forward half of the scalar block (f, the prologue's sums) and the sequence number
  uint32_t nred_n;      // records of the prologue (0: none ran, the n-side sums are written as zeros)
  unsigned seq;
  const double* red_n;  // [nred_n][8]
  double* red_m;        // [gridDim.x]
  unsigned* counter;
  double* out;
};

// (amdgpu_waves_per_eu(1, 2) as for k_mc_fwd: the loads of a chunk are issued together, not sunk to their first use)
template <int LB, int GRAD, int NT>
__global__ __launch_bounds__(FH_WG) __attribute__((amdgpu_waves_per_eu(1, 2))) void k_bl_pass(const BlPassP p) {
  constexpr int NS = bl_ns(LB);        // GX sums of a chunk
  constexpr int RB = NS / LB;          // rows of S per chunk
  __shared__ __attribute__((aligned(16))) double s_part[2][4 * NS];
  __shared__ __attribute__((aligned(16))) double s_scr[4 * 8];
  __shared__ __attribute__((aligned(16))) unsigned s_flag[4];
  const uint32_t tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int base = mc_rs_base<NS>(lane);
  const d2* Sd = reinterpret_cast<const d2*>(p.S);
  const uint32_t nitems = p.nrp * p.nct;
  double fpart = 0.0;
  int buf = 0;
  for (uint32_t it = blockIdx.x; it < nitems; it += gridDim.x) {
    const uint32_t pnl = it / p.nct, tile = it % p.nct;
    const uint32_t c0 = tile * (BL_TC / 2) + tid;            // this lane's piece of every row of the panel
    const bool ok = c0 < p.ld2;
    const uint32_t k0 = ok ? c0 : 0u;                        // clamp: an in-bounds redundant load, the piece counts as zero
    const uint32_t j0 = 2u * c0;
    const bool live_a = ok && j0 < p.n, live_b = ok && j0 + 1u < p.n;
    double ya[LB], yb[LB], ga[LB], gb[LB];
#pragma unroll
    for (int l = 0; l < LB; l += 2) {
      d2 a = {0.0, 0.0}, b = {0.0, 0.0};
      if (live_a) a = *reinterpret_cast<const d2*>(p.z + (uint64_t)(p.m + j0) * LB + l);
      if (live_b) b = *reinterpret_cast<const d2*>(p.z + (uint64_t)(p.m + j0 + 1u) * LB + l);
      ya[l] = a.x; ya[l + 1] = a.y; yb[l] = b.x; yb[l + 1] = b.y;
      ga[l] = 0.0; ga[l + 1] = 0.0; gb[l] = 0.0; gb[l + 1] = 0.0;
    }
    const uint32_t r0 = pnl * p.pr;
    const uint32_t r1 = min(r0 + p.pr, p.m);                 // (chunks are aligned to RB | 16: the last one stays inside the mp padded rows)
    for (uint32_t rc = r0; rc < r1; rc += RB) {
      d2 s[RB];
#pragma unroll
      for (int r = 0; r < RB; ++r) s[r] = load_stream<NT>(Sd + (uint64_t)(rc + r) * p.ld2 + k0);
      double c[NS];
#pragma unroll
      for (int r = 0; r < RB; ++r) {
        const uint32_t i = rc + r;
        const bool rowok = i < p.m;                          // (workgroup-uniform; a row past m is padding of S and counts as a zero row of X)
        double x[LB];
#pragma unroll
        for (int l = 0; l < LB; ++l) x[l] = rowok ? p.z[(uint64_t)i * LB + l] : 0.0;
        double da = ok ? -s[r].x : 0.0, db = ok ? -s[r].y : 0.0;
#pragma unroll
        for (int l = 0; l < LB; ++l) { da = fma(x[l], ya[l], da); db = fma(x[l], yb[l], db); }
        fpart = fma(da, da, fpart);
        fpart = fma(db, db, fpart);
        if (GRAD) {
#pragma unroll
          for (int l = 0; l < LB; ++l) {
            ga[l] = fma(da, x[l], ga[l]);
            gb[l] = fma(db, x[l], gb[l]);
            c[r * LB + l] = fma(db, yb[l], da * ya[l]);
          }
        }
      }
      if (GRAD) {
        mc_reduce_scatter<NS>(c, lane);
        if (lane < NS) s_part[buf][wave * NS + base] = c[0];      // (lanes l and l + NS hold the same sums)
        __syncthreads();
        if (tid < NS) {
          const double gx = ((s_part[buf][tid] + s_part[buf][NS + tid]) + s_part[buf][2 * NS + tid]) + s_part[buf][3 * NS + tid];
          const uint32_t row = rc + tid / LB;
          if (row < p.m) p.px[((uint64_t)tile * p.m + row) * LB + tid % LB] = gx;
        }
        buf ^= 1;         // (the next chunk writes the other half: its barrier separates this chunk's reads from the chunk after next's writes)
      }
    }
    if (GRAD) {
#pragma unroll
      for (int l = 0; l < LB; l += 2) {
        if (live_a) *reinterpret_cast<d2*>(p.py + ((uint64_t)pnl * p.n + j0) * LB + l) = (d2){ga[l], ga[l + 1]};
        if (live_b) *reinterpret_cast<d2*>(p.py + ((uint64_t)pnl * p.n + j0 + 1u) * LB + l) = (d2){gb[l], gb[l + 1]};
      }
    }
  }
  double v[1] = {fpart};
  finish_records<1, S_GMAX, 8>(v, p.red_m, blockIdx.x, gridDim.x, p.counter, p.out, p.publish ? p.seq : 0u, s_scr, s_flag,
                               [&](double (&w)[8]) { add_records<1, 8, S_GMAX>(w, p.red_n, p.nred_n); },      // the prologue's n-side sums
                               [&](double (&w)[8]) {
                                 w[S_FSQ] = 0.5 * w[S_FSQ];
                                 *p.fout = w[S_FSQ];
                                 if (p.publish) store_fwd_scalars(p.out, w, 0.0);
                               });
}

// ---- the point of an accelerated step's second pass ------------------------------------------------------------------------------------------
static __global__ __launch_bounds__(FH_WG) void k_bl_extrap(const double* xp, const double* xacc0, double coef, double* x1, uint32_t n, uint32_t L,
                                                           uint32_t LB, uint64_t count) {
  const uint64_t i = (uint64_t)blockIdx.x * FH_WG + threadIdx.x;
  if (i >= count) return;
  const bool valid = i / LB < n && i % LB < L;
  x1[i] = valid ? extrapolate(xp[i], xacc0[i], coef) : 0.0;
}

// ---- the n-side epilogue: partial reduction and the n-side sums ---------------------------------------------------------------------------------
struct BlGradP {
  uint32_t m, n, L;     // rows of X / of Y, columns
  uint32_t rows;        // device rows of Z (every lane of the grid owns one)
  uint32_t nct, nrp;    // partials per row of X / of Y
  uint32_t gtop;        // rows whose |x1| enter FH_S_GSUM_ADJ: m + n, or the split of FH_PROX_ROWSPLIT
  const double* px; const double* py;
  const double* fsrc;   // f of the pass that wrote the partials
  int accel, mode;      // mode 0 = FBS (BB epilogue), 1 = plain gradient (g1 only, the sums are published as zeros)
  unsigned seq;
  double coef, tau;
  const double* x0; const double* xp; const double* xacc0; const double* xhat;
  double* g1;
  double* red;          // [gridDim.x][8]
  unsigned* counter;
  double* out;
};

template <int LB>
__global__ __launch_bounds__(FH_WG) void k_bl_grad(const BlGradP p) {
  __shared__ __attribute__((aligned(16))) double s_scr[4 * 8];
  __shared__ __attribute__((aligned(16))) unsigned s_flag[4];
  const uint32_t tid = threadIdx.x;
  const uint32_t row = blockIdx.x * FH_WG + tid;
  double v[5] = {0, 0, 0, 0, 0};      // dxdg, dg2, xh2, gsum, gmax
  if (row < p.rows) {
    const uint64_t o = (uint64_t)row * LB;
    const bool isx = row < p.m, isy = !isx && row < p.m + p.n;
    const double* part = isx ? p.px + (uint64_t)row * LB : p.py + (uint64_t)(row - p.m) * LB;      // (not dereferenced on a padding row)
    const uint64_t stride = (uint64_t)(isx ? p.m : p.n) * LB;
    const uint32_t np = isx ? p.nct : (isy ? p.nrp : 0u);
#pragma unroll
    for (int l = 0; l < LB / 2; ++l) {
      d2 gv = {0.0, 0.0};
      for (uint32_t q = 0; q < np; ++q) {          // index order: column tiles for a row of X, row panels for a row of Y
        const d2 t = *reinterpret_cast<const d2*>(part + (uint64_t)q * stride + 2 * l);
        gv.x = add_nofma(gv.x, t.x); gv.y = add_nofma(gv.y, t.y);
      }
      d2 x0v = {0.0, 0.0}, xpv = {0.0, 0.0}, xhv = {0.0, 0.0}, xav = {0.0, 0.0};
      if (p.mode == 0) {
        x0v = *reinterpret_cast<const d2*>(p.x0 + o + 2 * l);
        xpv = *reinterpret_cast<const d2*>(p.xp + o + 2 * l);
        xhv = *reinterpret_cast<const d2*>(p.xhat + o + 2 * l);
        if (p.accel) xav = *reinterpret_cast<const d2*>(p.xacc0 + o + 2 * l);
      }
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const bool valid = (isx || isy) && (uint32_t)(2 * l + h) < p.L;
        const double g = valid ? gv[h] : 0.0;
        gv[h] = g;
        // (x1, which is not kept: the bits k_bl_extrap wrote)
        if (valid && p.mode == 0) nside_adj_sums(g, x0v[h], xpv[h], xav[h], xhv[h], p.accel, p.coef, p.tau, v, row < p.gtop);
      }
      *reinterpret_cast<d2*>(p.g1 + o + 2 * l) = gv;
    }
  }
  finish_records<5, 4>(v, p.red, blockIdx.x, gridDim.x, p.counter, p.out, p.seq, s_scr, s_flag, NoRecords(), [&](double (&w)[5]) {
    scal_store(p.out + S_DXDG, w[0]); scal_store(p.out + S_DG2, w[1]); scal_store(p.out + S_XH2_ADJ, w[2]);
    scal_store(p.out + S_GSUM_ADJ, w[3]); scal_store(p.out + S_GMAX_ADJ, w[4]); scal_store(p.out + S_FSQ_ADJ, *p.fsrc);
  });
}

// ---- the instantiations (ONE table for fh_bilinear_part.hip, the extern declarations and the dispatch) ----
#define BL_FOR_EACH(X) X(2) X(4) X(8) X(16)
#define BL_KERNELS(DO, LB)                                   \
  DO __global__ void k_bl_prologue<LB>(const BlProP);        \
  DO __global__ void k_bl_pass<LB, 0, 0>(const BlPassP);     \
  DO __global__ void k_bl_pass<LB, 0, 1>(const BlPassP);     \
  DO __global__ void k_bl_pass<LB, 1, 0>(const BlPassP);     \
  DO __global__ void k_bl_pass<LB, 1, 1>(const BlPassP);     \
  DO __global__ void k_bl_grad<LB>(const BlGradP);

// fh_multi.h -- dense kernels for a MATRIX unknown: X is (n, L), B and Z are (m, L), one A for all L columns (fh_set_rhs; over a sparse A: fh_spmulti.h).
//
// The vector kernels of fh_dense.h are bound by the read of A: m*n*8 bytes per direction whatever the unknown.  Here every 16-byte piece
// of A that a lane loads is used for LB columns, so L right-hand sides cost one read of A -- and the prox may couple the columns of a row
// (FH_PROX_GROUP, the row-wise l2 shrink of the reference's examples/mmv.py:51-59).
//
// Device layout: every n-side matrix is `nv` rows (n padded as the vector form pads it) of LB doubles, every m-side matrix `mv` rows of LB
// doubles, row-major, LB in {2, 4, 8, 16} the smallest of them >= L.  Padding rows and padding columns are ZERO and stay zero through every
// kernel here (the prologue and the epilogue force them; the products of zeros are zeros), and no sum counts them.
//
//   k_mc_prologue  n-side prologue as its own small launch, one lane per ROW of X: xhat = x0 - tau*g0, xprox = prox(xhat) -- the row norm,
//                  its sqrt and the division of FH_PROX_GROUP happen here, once per row, not inside the streaming loop -- and the seven
//                  n-side sums of k_fwd_dense, one record per workgroup.
//   k_mc_fwd       Z = A * Xprox from ONE read of A plus the loss sum over (m, L).  k_fwd_dense's structure: a workgroup owns R whole rows
//                  per pass, lanes walk the row in 16-byte pieces; a lane holds R x CH accumulators (CH = its columns: all LB, or 8 of 16) and reads
//                  the two X rows of its piece (from a copy of X laid out for coalesced loads) once for all R rows: X bytes / A bytes = CH / R.  Reduction: lane pieces, then a
//                  wave tree (a reduce-scatter: every exchange halves what a lane still carries, ~R*LB adds per lane instead of
//                  6 * R*LB), then the four waves in order.  Its last workgroup adds the prologue's records in index order.
//   k_mc_adj       G1 = A^T * R, R = Z' - B.  k_adj_dense's slab scheme: a lane owns CPT 16-byte column pairs = 2*CPT whole rows of G
//                  (2*CPT*LB accumulators); the slab's residual is staged in LDS 2048 / LB rows at a time (16 KiB, what the vector kernel
//                  uses) and read back as wave-wide broadcasts; slab partials are summed in slab order by the last workgroup of a column
//                  chunk, which then runs the n-side epilogue (BB sums, FISTA extrapolation, g terms: the row norms of x1 are in-lane).
// Finalisers are arrive_last only: no spin waits, no co-residency assumption.  No float atomics: bitwise repeatable.
#pragma once
#include "fh_dense.h"

#define PX_GROUP 7
#define MC_LDS_DOUBLES 2048        // residual stage of k_mc_adj: the 16 KiB of k_adj_dense's s_r

// ---- wave-level reduce-scatter of N running sums (N a power of two) -----------------------------------------------------------------------
// Step s pairs lane l with lane l ^ (1 << s): while a lane still carries more than one value it keeps one half of them (bit s of its id
// clear: the lower half) and adds its partner's copy of that half.  Afterwards lane l holds, fully summed over the wave, the
// max(N / 64, 1) consecutive values that start at mc_rs_base<N>(l).  Fixed order, so repeatable.
template <int MASK>
__device__ __forceinline__ double mc_xor(double v) {
  if (MASK == 1) return dpp_f64<0xB1>(v);
  if (MASK == 2) return dpp_f64<0x4E>(v);
  return __shfl_xor(v, MASK, 64);
}
template <int N, int S, int CUR>
__device__ __forceinline__ void mc_rs_step(double (&v)[N], int lane) {
  constexpr int MASK = 1 << S;
  const bool upper = (lane & MASK) != 0;
  if constexpr (CUR > 1) {
    constexpr int H = CUR / 2;
#pragma unroll
    for (int i = 0; i < H; ++i) {
      const double keep = upper ? v[i + H] : v[i];
      const double send = upper ? v[i] : v[i + H];
      v[i] = keep + mc_xor<MASK>(send);
    }
  } else {
    v[0] += mc_xor<MASK>(v[0]);
  }
}
template <int N>
__device__ __forceinline__ void mc_reduce_scatter(double (&v)[N], int lane) {
  mc_rs_step<N, 0, N>(v, lane);
  mc_rs_step<N, 1, (N >= 2 ? N / 2 : 1)>(v, lane);
  mc_rs_step<N, 2, (N >= 4 ? N / 4 : 1)>(v, lane);
  mc_rs_step<N, 3, (N >= 8 ? N / 8 : 1)>(v, lane);
  mc_rs_step<N, 4, (N >= 16 ? N / 16 : 1)>(v, lane);
  mc_rs_step<N, 5, (N >= 32 ? N / 32 : 1)>(v, lane);
}
template <int N>
__device__ __forceinline__ int mc_rs_base(int lane) {
  int base = 0;
#pragma unroll
  for (int s = 0; s < 6; ++s)
    if ((N >> (s + 1)) > 0 && (lane & (1 << s))) base += N >> (s + 1);
  return base;
}

// ---- K-fwd's streaming copy of X ---------------------------------------------------------------------------------------------------------------
// k_mc_fwd's lane of piece c needs rows 2c and 2c + 1 of X.  Read from the (nv, LB) layout that is LB * 16 contiguous bytes per lane, i.e. every
// 16-byte load instruction of a wave touches 64 different cache lines (measured: LB = 8 stuck at 4.6 TB/s).  The streaming copy holds the same
// numbers as LB planes of ld2 pieces: plane j < LB/2 = columns (2j, 2j + 1) of the even rows, plane LB/2 + j = the same columns of the odd rows,
// so that consecutive lanes read consecutive 16 bytes of a plane.  Written by the prologue next to xprox, or by k_mc_pack for a plain operand.
template <int LB>
__device__ __forceinline__ void mc_pack_row(double* xs, uint32_t ld2, uint32_t row, const double (&v)[LB]) {
  const uint32_t c = row >> 1, e = row & 1u;
#pragma unroll
  for (int l = 0; l < LB / 2; ++l)
    reinterpret_cast<d2*>(xs)[(uint64_t)(e * (LB / 2) + l) * ld2 + c] = (d2){v[2 * l], v[2 * l + 1]};
}
template <int LB>
__global__ __launch_bounds__(FH_WG) void k_mc_pack(const double* x, double* xs, uint32_t nv, uint32_t ld2) {
  const uint32_t row = blockIdx.x * FH_WG + threadIdx.x;
  if (row >= nv) return;
  double v[LB];
#pragma unroll
  for (int l = 0; l < LB; l += 2) {
    const d2 a = *reinterpret_cast<const d2*>(x + (uint64_t)row * LB + l);
    v[l] = a.x; v[l + 1] = a.y;
  }
  mc_pack_row<LB>(xs, ld2, row, v);
}

// ---- n-side prologue ----------------------------------------------------------------------------------------------------------------------
struct McProP {
  uint32_t n, L;        // logical rows / columns of X
  uint32_t nv;          // device rows of X
  const double* x0; const double* g0; const double* xacc0;
  double* xhat; double* xp;
  double* xs;           // xprox once more, in K-fwd's streaming layout (mc_pack_row)
  uint32_t ld2;         // row pairs of X = 16-byte pieces per row of A
  double tau;
  ProxP px;             // kind: IDENTITY / SHRINK / NONNEG / BOX (elementwise, prox_scalar) or PX_GROUP
  double* red_n;        // [gridDim.x][8]
};

template <int LB>
__global__ __launch_bounds__(FH_WG) void k_mc_prologue(const McProP p) {
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
    if (p.px.kind == PX_GROUP) {          // examples/mmv.py:53-59: shrink the row norm, never divide by zero
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
    mc_pack_row<LB>(p.xs, p.ld2, row, xq);
  }
  publish_record<7, 5>(v, p.red_n + 1, blockIdx.x, s_scr);
}

// sum of the g terms of an (n, L) matrix held as (nv, LB): out[S_GSUM] = sum |x| (group = 0) or sum of row norms (group = 1), out[S_GMAX] = max |x|
static __global__ __launch_bounds__(FH_WG) void k_mc_gterms(const double* x, uint32_t n, uint32_t L, uint32_t LB, int group, double* red,
                                                            unsigned* counter, double* out) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) double s_scr[8];
  __shared__ __attribute__((aligned(16))) unsigned s_flag[4];
  double v[2] = {0.0, 0.0};
  for (uint32_t row = blockIdx.x * FH_WG + threadIdx.x; row < n; row += gridDim.x * FH_WG) {
    double s2 = 0.0;
    for (uint32_t l = 0; l < L; ++l) {
      const double a = x[(uint64_t)row * LB + l];
      s2 += a * a;
      if (!group) v[0] += fabs(a);
      v[1] = fmax(v[1], fabs(a));
    }
    if (group) v[0] += sqrt(s2);
  }
  block_reduce<2>(v, s_scr, 1);
  if (threadIdx.x == 0) { store_partial(red + 2 * blockIdx.x, v[0]); store_partial(red + 2 * blockIdx.x + 1, v[1]); }
  if (!arrive_last(counter, gridDim.x, s_flag)) return;
  double w[2] = {0.0, 0.0};
  for (uint32_t i = threadIdx.x; i < gridDim.x; i += FH_WG) { w[0] += load_partial(red + 2 * i); w[1] = fmax(w[1], load_partial(red + 2 * i + 1)); }
  block_reduce<2>(w, s_scr, 1);
  if (threadIdx.x == 0) {
    out[S_GSUM] = w[0]; out[S_GMAX] = w[1];
    __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// ---- K-fwd, LB columns --------------------------------------------------------------------------------------------------------------------
struct McFwdP {
  const double* A;
  uint32_t ld2;         // 16-byte pieces per device row of A
  uint32_t m, L;        // logical rows of A / columns of X
  uint32_t nrg;         // row groups = mp / R
  uint32_t nred_n;      // records of the prologue (0: no prologue ran, the n-side sums are written as zeros)
  const double* x;      // the operand in the streaming layout (mc_pack_row): xprox from the prologue, or a plain operand from k_mc_pack
  const double* b; double* z;
  int sub_b;
  unsigned seq;
  const double* red_n;  // [nred_n][8]
  double* red_m;        // [gridDim.x]
  unsigned* counter;
  double* out;
};

// LB = 16: R * LB accumulators per lane at R >= 8 are more than the 256 registers float64 multiply-adds can address (hipcc parks them in AGPRs
// and copies them in and out inside the loop: 1.67 ms at 16384^2; R = 4, X bytes = 4 x A bytes: 1.30 ms).  So the COLUMNS are split instead:
// NG = LB / CH groups of lanes (waves 0-1 and 2-3), each walking the whole row for its CH = 8 columns -- the LB = 8 loop, twice, side by side
// in one workgroup: both groups load the same pieces of A within a trip, HBM delivers them once.
// (amdgpu_waves_per_eu(1, 2): the grid is two workgroups per CU.  Without the hint hipcc chases a higher occupancy for the small shapes by
// sinking every load of a trip to just in front of its first use and waiting for each one alone: LB = 2 ran at 3.8 TB/s that way.)
template <int LB, int CH, int R, int NT>
__global__ __launch_bounds__(FH_WG) __attribute__((amdgpu_waves_per_eu(1, 2))) void k_mc_fwd(const McFwdP p) {
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
    const d2* Ab = reinterpret_cast<const d2*>(p.A) + (uint64_t)rg * R * p.ld2;
    double acc[N];
#pragma unroll
    for (int i = 0; i < N; ++i) acc[i] = 0.0;
    for (uint32_t t = 0; t < ntrip; ++t) {
      const uint32_t c0 = t * GL + gl;
      const bool ok = c0 < p.ld2;
      const uint32_t k0 = ok ? c0 : 0u;                      // clamp: in-bounds redundant loads, zero x
      d2 a[R];
#pragma unroll
      for (int r = 0; r < R; ++r) a[r] = load_stream<NT>(Ab + (uint64_t)r * p.ld2 + k0);
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
      double zv = s_part[(g * WPG) * N + idx];
#pragma unroll
      for (int w = 1; w < WPG; ++w) zv += s_part[(g * WPG + w) * N + idx];       // the group's waves in order
      const uint32_t row = rg * R + idx / CH, col = g * CH + idx % CH;
      const uint64_t o = (uint64_t)row * LB + col;
      p.z[o] = zv;
      if (row < p.m && col < p.L) fpart += p.sub_b ? loss_term(zv, p.b[o], LOSS_LSQ) : zv * zv;
    }
    __syncthreads();
  }
  double v[1] = {fpart};
  finish_records<1, S_GMAX, 8>(v, p.red_m, blockIdx.x, gridDim.x, p.counter, p.out, p.seq, s_scr, s_flag,
                               [&](double (&w)[8]) { add_records<1, 8, S_GMAX>(w, p.red_n, p.nred_n); },      // the prologue's n-side sums
                               [&](double (&w)[8]) { store_fwd_scalars(p.out, w, 0.0); });
}

// ---- K-adj, LB columns --------------------------------------------------------------------------------------------------------------------
struct McAdjP {
  const double* A;
  uint32_t ld2;         // 16-byte pieces per device row of A = row pairs of G
  uint32_t n, L;
  uint32_t mp, m;
  uint32_t slab_rows, nslab, ncc;
  const double* z; const double* zacc0; const double* b;
  int sub_b, accel, mode, group;      // mode 0 = FBS (BB epilogue), 1 = plain gradient (g1 only); group: FH_PROX_GROUP's g terms
  unsigned seq;
  double coef, tau;
  const double* x0; const double* xp; const double* xacc0; const double* xhat;
  double* x1; double* g1;
  double* gpart;        // [nslab][2 * ld2 * LB]
  double* red_bb;       // [ncc][8]
  double* red_f;        // [nslab]
  unsigned* cc_counter; unsigned* fin_counter;
  double* out;
};

template <int LB, int CPT, int NT>
__global__ __launch_bounds__(FH_WG) __attribute__((amdgpu_waves_per_eu(1, 4))) void k_mc_adj(const McAdjP p) {
  constexpr uint32_t SB = MC_LDS_DOUBLES / LB;          // rows of the residual staged at a time
  __shared__ __attribute__((aligned(16))) double s_r[MC_LDS_DOUBLES];
  __shared__ __attribute__((aligned(16))) double s_scr[4 * 8];
  __shared__ __attribute__((aligned(16))) unsigned s_flag[4];
  const uint32_t tid = threadIdx.x;
  const uint32_t cc = blockIdx.x % p.ncc, slab = blockIdx.x / p.ncc;
  const uint32_t row0 = slab * p.slab_rows;
  const uint32_t rows = min(p.slab_rows, p.mp - row0);

  uint32_t col[CPT];
  double acc[CPT][2][LB];
#pragma unroll
  for (int j = 0; j < CPT; ++j) {
    col[j] = min(cc * (FH_WG * CPT) + j * FH_WG + tid, p.ld2 - 1u);   // clamp: redundant but in-bounds
#pragma unroll
    for (int l = 0; l < LB; ++l) { acc[j][0][l] = 0.0; acc[j][1][l] = 0.0; }
  }
  double fs = 0.0;
  for (uint32_t s0 = 0; s0 < rows; s0 += SB) {
    const uint32_t nb = min(SB, rows - s0);
    __syncthreads();                                       // the previous stage has been consumed
    // ---- stage nb rows of the residual R = Z' - B (Z' = extrapolated Z when accelerating) ----
    for (uint32_t i = tid; i < nb * LB; i += FH_WG) {
      const uint32_t gr = row0 + s0 + i / LB, l = i % LB;
      const uint64_t o = (uint64_t)gr * LB + l;
      double zv = p.z[o];
      if (p.accel) zv = extrapolate(zv, p.zacc0[o], p.coef);
      const double bv = p.sub_b ? p.b[o] : 0.0;
      s_r[i] = p.sub_b ? loss_grad(zv, bv, LOSS_LSQ) : zv;
      if (gr < p.m && l < p.L) fs += p.sub_b ? loss_term(zv, bv, LOSS_LSQ) : zv * zv;
    }
    __syncthreads();
    // ---- stream the rows: per-(row of G, column) accumulators ----
    const d2* Ab = reinterpret_cast<const d2*>(p.A) + (uint64_t)(row0 + s0) * p.ld2;
    // RB rows per trip (a stage always holds a multiple of eight): RB * CPT loads in flight per lane ahead of their 2 * RB * CPT * LB
    // multiply-adds.  Four rows up to LB = 8 (16384^2, LB = 8: 0.525 -> 0.447 ms); at LB = 16 the accumulators leave room for two waves per
    // SIMD only and the plain row-by-row loop is the faster one (0.585 against 0.756 ms).
    constexpr int RB = LB >= 16 ? 1 : 4;
#pragma unroll 2
    for (uint32_t i = 0; i < nb; i += RB) {
      d2 a[RB][CPT];
#pragma unroll
      for (int q = 0; q < RB; ++q)
#pragma unroll
        for (int j = 0; j < CPT; ++j) a[q][j] = load_stream<NT>(Ab + (uint64_t)q * p.ld2 + col[j]);
#pragma unroll
      for (int q = 0; q < RB; ++q) {
        const d2* rr = reinterpret_cast<const d2*>(s_r + (i + q) * LB);
#pragma unroll
        for (int l = 0; l < LB / 2; ++l) {
          const d2 rv = rr[l];
#pragma unroll
          for (int j = 0; j < CPT; ++j) {
            acc[j][0][2 * l] = fma(a[q][j].x, rv.x, acc[j][0][2 * l]);
            acc[j][0][2 * l + 1] = fma(a[q][j].x, rv.y, acc[j][0][2 * l + 1]);
            acc[j][1][2 * l] = fma(a[q][j].y, rv.x, acc[j][1][2 * l]);
            acc[j][1][2 * l + 1] = fma(a[q][j].y, rv.y, acc[j][1][2 * l + 1]);
          }
        }
      }
      Ab += RB * (uint64_t)p.ld2;
    }
  }
  const uint32_t pstride = p.ld2 * LB;                    // double pairs per slab partial
#pragma unroll
  for (int j = 0; j < CPT; ++j) {
    const uint32_t c = cc * (FH_WG * CPT) + j * FH_WG + tid;
    if (c < p.ld2) {
#pragma unroll
      for (int e = 0; e < 2; ++e)
#pragma unroll
        for (int l = 0; l < LB / 2; ++l)
          store_partial16(reinterpret_cast<d2*>(p.gpart) + (uint64_t)slab * pstride, c * LB + e * (LB / 2) + l, (d2){acc[j][e][2 * l], acc[j][e][2 * l + 1]});
    }
  }
  if (cc == 0) {
    double v[1] = {fs};
    block_reduce<1>(v, s_scr, -1);
    if (tid == 0) store_partial(p.red_f + slab, v[0]);
  }

  // ---- last workgroup of this column chunk: ordered slab sum + n-side epilogue ---------------------
  if (!arrive_last(p.cc_counter + cc, p.nslab, s_flag)) return;
  if (tid == 0) __hip_atomic_store(p.cc_counter + cc, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);

  double v[5] = {0, 0, 0, 0, 0};      // dxdg, dg2, xh2, gsum, gmax
#pragma unroll 1
  for (int j = 0; j < CPT; ++j) {
    const uint32_t c = cc * (FH_WG * CPT) + j * FH_WG + tid;
    if (c >= p.ld2) continue;
#pragma unroll 1
    for (int e = 0; e < 2; ++e) {
      const uint32_t grow = 2u * c + e;                    // row of G / X
      const uint64_t o = (uint64_t)grow * LB;
      const uint32_t pi = c * LB + e * (LB / 2);           // pair index of the row inside a slab partial
      d2 g[LB / 2];
#pragma unroll
      for (int l = 0; l < LB / 2; ++l) g[l] = (d2){0.0, 0.0};
      for (uint32_t s = 0; s < p.nslab; ++s) {
#pragma unroll
        for (int l = 0; l < LB / 2; ++l) g[l] += load_partial16(reinterpret_cast<const d2*>(p.gpart) + (uint64_t)s * pstride, pi + l);
      }
#pragma unroll
      for (int l = 0; l < LB / 2; ++l) *reinterpret_cast<d2*>(p.g1 + o + 2 * l) = g[l];
      if (p.mode != 0) continue;
      double n2 = 0.0;
#pragma unroll
      for (int l = 0; l < LB / 2; ++l) {
        const d2 x0v = *reinterpret_cast<const d2*>(p.x0 + o + 2 * l);
        const d2 xpv = *reinterpret_cast<const d2*>(p.xp + o + 2 * l);
        const d2 xhv = *reinterpret_cast<const d2*>(p.xhat + o + 2 * l);
        d2 xav = {0.0, 0.0};
        if (p.accel) xav = *reinterpret_cast<const d2*>(p.xacc0 + o + 2 * l);
        d2 x1v;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const bool valid = grow < p.n && (uint32_t)(2 * l + h) < p.L;
          double x1 = 0.0;
          if (valid) {
            x1 = nside_adj_sums(g[l][h], x0v[h], xpv[h], xav[h], xhv[h], p.accel, p.coef, p.tau, v, !p.group);
            n2 = add_nofma(n2, x1 * x1);
          }
          x1v[h] = x1;
        }
        if (p.accel) *reinterpret_cast<d2*>(p.x1 + o + 2 * l) = x1v;
      }
      if (p.group) v[3] += sqrt(n2);
    }
  }
  // ---- one record per column chunk; the last chunk finaliser: ordered scalar sums -------------------
  finish_records<5, 4, 6>(v, p.red_bb, cc, p.ncc, p.fin_counter, p.out, p.seq, s_scr, s_flag,
                          [&](double (&w)[6]) { add_column(w[5], p.red_f, p.nslab); },      // fsq: one loss sum per slab
                          [&](double (&w)[6]) { store_adj_scalars(p.out, w); });
}

// ---- the instantiations (ONE table for the explicit instantiations of fh_multi_part.hip, their extern declarations and the dispatch) ----
// X(LB, CH, R): K-fwd keeps R * CH accumulators per lane -- 32, 64, 64, 64 -- and R >= CH keeps the X bytes a lane reads at or below its A bytes.
#define MC_ADJ_CPT 2
#define MC_FOR_EACH(X) X(2, 2, 16) X(4, 4, 16) X(8, 8, 8) X(16, 8, 8)
#define MC_KERNELS(DO, LB, CH, R)                                         \
  DO __global__ void k_mc_prologue<LB>(const McProP);                     \
  DO __global__ void k_mc_pack<LB>(const double*, double*, uint32_t, uint32_t); \
  DO __global__ void k_mc_fwd<LB, CH, R, 0>(const McFwdP);                \
  DO __global__ void k_mc_fwd<LB, CH, R, 1>(const McFwdP);                \
  DO __global__ void k_mc_adj<LB, MC_ADJ_CPT, 0>(const McAdjP);           \
  DO __global__ void k_mc_adj<LB, MC_ADJ_CPT, 1>(const McAdjP);

// fh_standardize.h -- standardised features on the device (fh_standardize, include/fasta_hip.h; the host statement of the same numbers is
// fasta_python_amd/preprocess.py: standardize).  The matrix the context holds is rewritten in place, column by column:
//   mean_j  = (sum_i a_ij) / m                              (center; else 0)
//   d_ij    = a_ij - mean_j                                 (float32 storage promoted to double first)
//   scale_j = sqrt((sum_i d_ij^2) / m), 1 where that is 0   (scale; else 1)
//   a_ij   <- d_ij / scale_j                                (float32 storage: rounded to nearest on the store)
// every line one rounded operation.  The centred squares are summed as such: ss - m * mean^2 cancels.
// Dense operator, either storage, vector or multi-column form -- the geometry is ScreenShape (fh_screen.h: column tiles x row slabs), the
// structure that of k_colnorm_dense / k_colnorm_final:
//   k_std_pass_dense<F32, 0>  the column sums: one streaming read, 16-byte loads, eight rows in flight: a lane owns one piece of a column tile and adds a
//                             slab of rows in index order; one partial per (slab, column).  The zero padding rows add nothing.
//   k_std_pass_dense<F32, 1>  the centred squares: the same walk with d = a - mean, ss = fma(d, d, ss) -- over rows i < m ONLY: a padding row would add mean^2
//   k_std_final               the slab partials in slab order, then the closing arithmetic of the means (which = 0) or the scales (which = 1), over
//                             all ld columns: a padding column has sum 0 and ss 0, so mean 0 and scale 1
//   k_std_rewrite_dense<F32>  the read-plus-write stream: the same ownership, trips of four rows, non-temporal 16-byte loads and stores (the policy
//                             and the trip length are the best of profiles/r03_mixprobe.txt for a copy: DESIGN.md section 25).  ONLY rows i < m and
//                             columns j < n are written: the padding of the block stays the zeros every dense kernel relies on.
// Sparse operator (float64, both stored copies), scaling only -- centring would fill the matrix:
//   k_colnorm_csr (fh_screen.h) over A^T by rows gives norms2, k_std_final (which = 1) the scales from them
//   k_std_scale_cols          A^T by rows: stored row j divided by scale_j; a long row gets a workgroup (the blocks behind the short ones)
//   k_std_scale_rows          A by rows: val[k] / scale[idx[k]], one entry per lane, grid-stride -- long rows need no care
// The two copies hold identical bits afterwards (the same division of the same operands).
// Ordinary launches only, no grid barrier, no waiting on another workgroup, no atomics: every sum has a fixed order, bitwise repeatable.
// Elementwise operations are never contracted; the sums of squares use fma().
#pragma once
#include "fh_screen.h"

struct StdP {
  double* A;                // mp rows of ld elements (float64 or float32), padding zero
  uint64_t m, n, mp, ld;
  uint32_t slab, nslab, tiles;
  int which;                // k_std_final: 0 = the means from the sums, 1 = the scales from the sums of squares
  int want;                 // k_std_final, which = 1: 0 = every scale is 1 (scale not asked)
  double* part;             // nslab x ld doubles
  double* mean;             // ld doubles
  double* scl;              // ld doubles
};

__device__ __forceinline__ void std_sum_add(d2 a, double (&acc)[2]) {
#pragma clang fp contract(off)
  acc[0] = acc[0] + a.x;
  acc[1] = acc[1] + a.y;
}
__device__ __forceinline__ void std_sum_add(f4 a, double (&acc)[4]) {
#pragma clang fp contract(off)
  acc[0] = acc[0] + (double)a.x;
  acc[1] = acc[1] + (double)a.y;
  acc[2] = acc[2] + (double)a.z;
  acc[3] = acc[3] + (double)a.w;
}
__device__ __forceinline__ void std_css_add(d2 a, const double (&mu)[2], double (&acc)[2]) {
#pragma clang fp contract(off)
  const double d0 = a.x - mu[0], d1 = a.y - mu[1];
  acc[0] = fma(d0, d0, acc[0]);
  acc[1] = fma(d1, d1, acc[1]);
}
__device__ __forceinline__ void std_css_add(f4 a, const double (&mu)[4], double (&acc)[4]) {
#pragma clang fp contract(off)
  const double d0 = (double)a.x - mu[0], d1 = (double)a.y - mu[1], d2_ = (double)a.z - mu[2], d3 = (double)a.w - mu[3];
  acc[0] = fma(d0, d0, acc[0]);
  acc[1] = fma(d1, d1, acc[1]);
  acc[2] = fma(d2_, d2_, acc[2]);
  acc[3] = fma(d3, d3, acc[3]);
}
// (-DFH_STD_AB_MULTIPLY, `make stdmul`: an A/B build whose rewrite multiplies by the reciprocal of the scale -- two roundings, NOT the statement, never
// shipped -- so that scripts/probes/standardize_sizes.py can price the float64 division of the rewrite)
#ifdef FH_STD_AB_MULTIPLY
#define STD_QUOT(d, s) ((d) * (1.0 / (s)))
#else
#define STD_QUOT(d, s) ((d) / (s))
#endif
// one piece rewritten; live: how many of its columns lie below n (the others keep their bits)
__device__ __forceinline__ d2 std_rewrite(d2 a, const double (&mu)[2], const double (&sc)[2], int live) {
#pragma clang fp contract(off)
  const double d0 = a.x - mu[0], d1 = a.y - mu[1];
  d2 w = a;
  if (live > 0) w.x = STD_QUOT(d0, sc[0]);
  if (live > 1) w.y = STD_QUOT(d1, sc[1]);
  return w;
}
__device__ __forceinline__ f4 std_rewrite(f4 a, const double (&mu)[4], const double (&sc)[4], int live) {
#pragma clang fp contract(off)
  const double d0 = (double)a.x - mu[0], d1 = (double)a.y - mu[1], d2_ = (double)a.z - mu[2], d3 = (double)a.w - mu[3];
  f4 w = a;
  if (live > 0) w.x = (float)STD_QUOT(d0, sc[0]);
  if (live > 1) w.y = (float)STD_QUOT(d1, sc[1]);
  if (live > 2) w.z = (float)STD_QUOT(d2_, sc[2]);
  if (live > 3) w.w = (float)STD_QUOT(d3, sc[3]);
  return w;
}

// CSS = 0: the column sums (every row of the padded block: the padding adds zeros); CSS = 1: the centred squares over rows i < m
template <int F32, int CSS>
__global__ __launch_bounds__(FH_WG) void k_std_pass_dense(const StdP p) {
  typedef typename PieceOf<F32>::type Piece;
  constexpr int V = F32 ? 4 : 2;
  const uint32_t tile = blockIdx.x % p.tiles, slab = blockIdx.x / p.tiles;
  const uint64_t c0 = ((uint64_t)tile * FH_WG + threadIdx.x) * V;
  if (c0 + V > p.ld) return;
  const uint64_t r0 = (uint64_t)slab * p.slab;
  const uint64_t r1 = r0 + p.slab < p.mp ? r0 + p.slab : p.mp;      // (mp and the slab are multiples of 16: whole trips of 8 rows, every load inside the block)
  const Piece* col = reinterpret_cast<const Piece*>(p.A) + c0 / V;
  const uint64_t ldp = p.ld / V;
  double acc[V], mu[V];
#pragma unroll
  for (int k = 0; k < V; ++k) { acc[k] = 0.0; mu[k] = CSS ? p.mean[c0 + k] : 0.0; }
  for (uint64_t r = r0; r < r1; r += 8) {
    if (CSS && r >= p.m) break;
    Piece a[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) a[u] = FH_NT_LOAD(col + (r + u) * ldp);      // eight independent loads in flight, then the adds in row order
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      if (CSS) { if (r + u < p.m) std_css_add(a[u], mu, acc); }
      else std_sum_add(a[u], acc);
    }
  }
  double* out = p.part + (uint64_t)slab * p.ld + c0;
#pragma unroll
  for (int k = 0; k < V; k += 2) *reinterpret_cast<d2*>(out + k) = d2{acc[k], acc[k + 1]};
}

template <int F32>
__global__ __launch_bounds__(FH_WG) void k_std_rewrite_dense(const StdP p) {
  typedef typename PieceOf<F32>::type Piece;
  constexpr int V = F32 ? 4 : 2;
  const uint32_t tile = blockIdx.x % p.tiles, slab = blockIdx.x / p.tiles;
  const uint64_t c0 = ((uint64_t)tile * FH_WG + threadIdx.x) * V;
  if (c0 >= p.n) return;                                            // (a piece of padding columns alone: nothing to write)
  const int live = p.n - c0 < (uint64_t)V ? (int)(p.n - c0) : V;
  const uint64_t r0 = (uint64_t)slab * p.slab;
  uint64_t r1 = r0 + p.slab < p.mp ? r0 + p.slab : p.mp;
  if (r1 > p.m) r1 = p.m;                                           // rows i < m only: a padding row must not receive -mean
  Piece* col = reinterpret_cast<Piece*>(p.A) + c0 / V;
  const uint64_t ldp = p.ld / V;
  double mu[V], sc[V];
#pragma unroll
  for (int k = 0; k < V; ++k) { mu[k] = p.mean[c0 + k]; sc[k] = p.scl[c0 + k]; }
  for (uint64_t r = r0; r < r1; r += 4) {
    Piece a[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) a[u] = FH_NT_LOAD(col + (r + u) * ldp);      // (r + u < mp: r is a multiple of 4 below m <= mp, mp a multiple of 16)
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (r + u < r1) __builtin_nontemporal_store(std_rewrite(a[u], mu, sc, live), col + (r + u) * ldp);
  }
}

// (the kernels that are no templates are defined in one translation unit: fh_standardize_part.hip, or the single-unit builds)
__global__ void k_std_final(const StdP p);
__global__ void k_std_scale_cols(const SpMatP a, uint32_t nshort, const double* scale);
__global__ void k_std_scale_rows(const SpMatP a, unsigned long long nnz, const double* scale);
#ifdef FH_STANDARDIZE_DEFINE
// one lane per column j < ld; part = nullptr: the sums lie in p.scl already (the sparse operator: norms2 from k_colnorm_csr), nslab = 0
__global__ __launch_bounds__(FH_WG) void k_std_final(const StdP p) {
#pragma clang fp contract(off)
  const uint64_t j = (uint64_t)blockIdx.x * FH_WG + threadIdx.x;
  if (j >= p.ld) return;
  if (p.which == 1 && !p.want) { p.scl[j] = 1.0; return; }
  double acc = 0.0;
  if (p.part) {
    const double* col = p.part + j;
    uint32_t s = 0;
    for (; s + 8 <= p.nslab; s += 8) {      // eight loads in flight, then the adds in slab order
      double t[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) t[u] = col[(uint64_t)(s + u) * p.ld];
#pragma unroll
      for (int u = 0; u < 8; ++u) acc = acc + t[u];
    }
    for (; s < p.nslab; ++s) acc = acc + col[(uint64_t)s * p.ld];
  } else {
    acc = p.scl[j];
  }
  const double q = acc / (double)p.m;
  if (p.which == 0) { p.mean[j] = q; return; }
  const double r = sqrt(q);
  p.scl[j] = r != 0.0 ? r : 1.0;
}

// a: A^T by rows.  Blocks 0 .. nshort - 1: a lane per feature, the long ones left out; then one block per long row (the split of k_colnorm_csr).
__global__ __launch_bounds__(FH_WG) void k_std_scale_cols(const SpMatP a, uint32_t nshort, const double* scale) {
#pragma clang fp contract(off)
  double* val = const_cast<double*>(a.val);
  if (blockIdx.x < nshort) {
    const uint64_t j = (uint64_t)blockIdx.x * FH_WG + threadIdx.x;
    if (j >= a.rows) return;
    const long long k0 = a.ptr[j], k1 = a.ptr[j + 1];
    if (k1 - k0 > a.longer) return;
    const double s = scale[j];
    for (long long k = k0; k < k1; ++k) val[k] = val[k] / s;
    return;
  }
  const uint32_t j = a.longrows[blockIdx.x - nshort];
  const long long k0 = a.ptr[j], k1 = a.ptr[j + 1];
  const double s = scale[j];
  for (long long k = k0 + threadIdx.x; k < k1; k += FH_WG) val[k] = val[k] / s;
}

// a: A by rows; every stored entry by the scale of its column
__global__ __launch_bounds__(FH_WG) void k_std_scale_rows(const SpMatP a, unsigned long long nnz, const double* scale) {
#pragma clang fp contract(off)
  double* val = const_cast<double*>(a.val);
  const unsigned long long stride = (unsigned long long)gridDim.x * FH_WG;
  for (unsigned long long k = (unsigned long long)blockIdx.x * FH_WG + threadIdx.x; k < nnz; k += stride) val[k] = val[k] / scale[a.idx[k]];
}
#endif

#define STD_KERNELS(DO)                                                   \
  DO __global__ void k_std_pass_dense<0, 0>(const StdP);                  \
  DO __global__ void k_std_pass_dense<0, 1>(const StdP);                  \
  DO __global__ void k_std_pass_dense<1, 0>(const StdP);                  \
  DO __global__ void k_std_pass_dense<1, 1>(const StdP);                  \
  DO __global__ void k_std_rewrite_dense<0>(const StdP);                  \
  DO __global__ void k_std_rewrite_dense<1>(const StdP);

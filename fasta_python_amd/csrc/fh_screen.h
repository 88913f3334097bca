// fh_screen.h -- gap-safe screening on the device (fh_column_norms, fh_screen, fh_gather_columns, include/fasta_hip.h; the host statement of the
// same numbers is fasta_python_amd/certificates.py: screen).  For min_x .5 ||A x - b||^2 + mu * Omega(x), with the certificate of fh_gap.h at the
// committed iterate (gap, the scale s, g0 = A^H (A x0 - b)) and norms2_j = sum_i a_ij^2:
//   gap_safe = gap + kappa * eps * (P + f + 2 sqrt(f * f0)),  rho = sqrt(2 * gap_safe),
//   feature j is discarded when every column l of its row has  (s * |g_jl| + rho * sqrt(norms2_j)) * (1 + 2^-48) < mu
// (FH_PROX_GROUP: s * ||g_j,:||_2 in place of s * |g_jl|, the row norm formed as k_gap_partials forms it).  At x0 = 0 with s = 1 the gap is zero
// as an identity (r = -b: P and D are the same sums), and so is the radius.  kappa is the longest addition chain of the certificate's sums
// (screen_kappa below, from the slab rule of k_gap_partials).
//   k_colnorm_dense<F32>  one streaming read of the mp x ld block, 16-byte loads: a lane owns one piece (2 or 4 columns) of a column tile and adds a
//                         slab of rows in index order with fma, in float64; one partial per (slab, column)
//   k_colnorm_final       adds the slab partials in slab order into n doubles
//   k_colnorm_csr         the same over A^T by rows (fh_sparse.h: every stored row is one feature), entries in stored order; a long row gets a
//                         workgroup: contiguous stretches per lane, then block_reduce
//   k_screen<GROUP>       one lane per feature: the test, one byte per feature, the kept count of the workgroup as one record
//   k_screen_final        the closing workgroup: the kept counts in index order, then the report
//   k_gather_cols<F32>    dst[i, t] = src[i, idx[t]] for t < count, zeros in the padding; a workgroup owns a slab of rows, 16-byte stores of full rows
// Ordinary launches only, no grid barrier, no waiting on another workgroup, no atomics: every sum has a fixed order, bitwise repeatable.
// Elementwise operations are never contracted (each rounds like the NumPy expression of certificates.py); the sums use fma().
#pragma once
#include "fh_sparse.h"

// ---- THE geometry, host functions ---------------------------------------------------------------------------------------------------------
struct ScreenShape { uint32_t slab, nslab, tile_cols, tiles, grid, kappa; };

// the slab rule of k_gap_partials (fasta_hip.hip: gap_slabs), restated where both the certificate's launcher and kappa read it
static inline void screen_gap_slabs(uint64_t rows, uint32_t* nwg, uint64_t* slab) {
  uint64_t k = (rows + 255) / 256;
  k = k < 1 ? 1 : (k > 256 ? 256 : k);
  *nwg = (uint32_t)k;
  *slab = ((rows + k - 1) / k + 63) / 64 * 64;
}
// the longest addition chain of the certificate's sums: terms per lane (rows of its slab dealt 256 apart, L terms each), the depth of block_reduce
// (4 DPP steps, 3 across the rows of a wave, 3 across the waves), records per lane in add_records, the depth of the second block_reduce folded into
// the 8 of the closing arithmetic
static inline uint32_t screen_kappa(uint64_t m, uint64_t n, uint32_t L) {
  uint32_t nwg_n, nwg_m;
  uint64_t slab_n, slab_m;
  screen_gap_slabs(n, &nwg_n, &slab_n);
  screen_gap_slabs(m, &nwg_m, &slab_m);
  const uint64_t lanes = (slab_n > slab_m ? slab_n : slab_m) / 256 + ((slab_n > slab_m ? slab_n : slab_m) % 256 ? 1 : 0);
  const uint64_t terms = lanes * (L ? L : 1);
  const uint64_t recs = ((uint64_t)nwg_n + nwg_m + 255) / 256;
  return (uint32_t)(terms + 10 + recs + 8);
}
// the norms kernel: tiles of 256 pieces across the ld columns, slabs of whole rows (a multiple of 16) so that about 8 workgroups per CU are in flight
static inline ScreenShape screen_shape(uint64_t mp, uint64_t ld, int f32, int ncu, uint64_t m, uint64_t n, uint32_t L) {
  ScreenShape s;
  s.tile_cols = 256u * (f32 ? 4u : 2u);
  s.tiles = (uint32_t)((ld + s.tile_cols - 1) / s.tile_cols);
  const uint64_t target = 8ull * (uint64_t)(ncu > 0 ? ncu : 256);
  uint64_t ns = (target + s.tiles - 1) / s.tiles;
  if (ns > mp / 16) ns = mp / 16;
  if (ns > 1024) ns = 1024;
  if (ns < 1) ns = 1;
  const uint64_t slab = ((mp + ns - 1) / ns + 15) / 16 * 16;
  s.slab = (uint32_t)slab;
  s.nslab = (uint32_t)((mp + slab - 1) / slab);
  s.grid = s.tiles * s.nslab;
  s.kappa = screen_kappa(m, n, L);
  return s;
}

// ---- column norms -------------------------------------------------------------------------------------------------------------------------
struct ColnormP {
  const double* A;          // mp rows of ld elements (float64 or float32), padding zero
  uint64_t mp, ld, n;
  uint32_t slab, nslab, tiles;
  double* part;             // nslab x ld doubles
  double* out;              // n doubles
};

__device__ __forceinline__ void colnorm_add(d2 a, double (&acc)[2]) {
  acc[0] = fma(a.x, a.x, acc[0]);
  acc[1] = fma(a.y, a.y, acc[1]);
}
__device__ __forceinline__ void colnorm_add(f4 a, double (&acc)[4]) {
  acc[0] = fma((double)a.x, (double)a.x, acc[0]);
  acc[1] = fma((double)a.y, (double)a.y, acc[1]);
  acc[2] = fma((double)a.z, (double)a.z, acc[2]);
  acc[3] = fma((double)a.w, (double)a.w, acc[3]);
}

template <int F32>
__global__ __launch_bounds__(FH_WG) void k_colnorm_dense(const ColnormP p) {
  typedef typename PieceOf<F32>::type Piece;
  constexpr int V = F32 ? 4 : 2;
  const uint32_t tile = blockIdx.x % p.tiles, slab = blockIdx.x / p.tiles;
  const uint64_t c0 = ((uint64_t)tile * FH_WG + threadIdx.x) * V;
  if (c0 + V > p.ld) return;
  const uint64_t r0 = (uint64_t)slab * p.slab;
  const uint64_t r1 = r0 + p.slab < p.mp ? r0 + p.slab : p.mp;      // (mp and the slab are multiples of 16: whole trips of 8 rows)
  const Piece* col = reinterpret_cast<const Piece*>(p.A) + c0 / V;
  const uint64_t ldp = p.ld / V;
  double acc[V];
#pragma unroll
  for (int k = 0; k < V; ++k) acc[k] = 0.0;
  for (uint64_t r = r0; r < r1; r += 8) {
    Piece a[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) a[u] = FH_NT_LOAD(col + (r + u) * ldp);      // eight independent loads in flight, then the adds in row order
#pragma unroll
    for (int u = 0; u < 8; ++u) colnorm_add(a[u], acc);
  }
  double* out = p.part + (uint64_t)slab * p.ld + c0;
#pragma unroll
  for (int k = 0; k < V; k += 2) *reinterpret_cast<d2*>(out + k) = d2{acc[k], acc[k + 1]};
}

// (the three kernels that are no templates are defined in one translation unit: fh_screen_part.hip, or the single-unit builds)
__global__ void k_colnorm_final(const ColnormP p);
__global__ void k_colnorm_csr(const SpMatP a, uint32_t nshort, double* out);
#ifdef FH_SCREEN_DEFINE
__global__ __launch_bounds__(FH_WG) void k_colnorm_final(const ColnormP p) {
#pragma clang fp contract(off)
  const uint64_t j = (uint64_t)blockIdx.x * FH_WG + threadIdx.x;
  if (j >= p.n) return;
  const double* col = p.part + j;
  double acc = 0.0;
  uint32_t s = 0;
  for (; s + 8 <= p.nslab; s += 8) {      // eight loads in flight, then the adds in slab order (a load per add would pay the memory latency nslab times)
    double t[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) t[u] = col[(uint64_t)(s + u) * p.ld];
#pragma unroll
    for (int u = 0; u < 8; ++u) acc = acc + t[u];
  }
  for (; s < p.nslab; ++s) acc = acc + col[(uint64_t)s * p.ld];
  p.out[j] = acc;
}

// a: A^T by rows.  Blocks 0 .. ceil(rows / 256) - 1: a lane per feature, the long ones left out; then one block per long row.
__global__ __launch_bounds__(FH_WG) void k_colnorm_csr(const SpMatP a, uint32_t nshort, double* out) {
  __shared__ double scr[4];
  if (blockIdx.x < nshort) {
    const uint64_t j = (uint64_t)blockIdx.x * FH_WG + threadIdx.x;
    if (j >= a.rows) return;
    const long long k0 = a.ptr[j], k1 = a.ptr[j + 1];
    if (k1 - k0 > a.longer) return;
    double acc = 0.0;
    for (long long k = k0; k < k1; ++k) { const double v = a.val[k]; acc = fma(v, v, acc); }
    out[j] = acc;
    return;
  }
  const uint32_t j = a.longrows[blockIdx.x - nshort];
  const long long k0 = a.ptr[j], k1 = a.ptr[j + 1];
  const long long per = (k1 - k0 + FH_WG - 1) / FH_WG;
  const long long b0 = k0 + per * threadIdx.x;
  const long long b1 = b0 + per < k1 ? b0 + per : k1;
  double acc[1] = {0.0};
  for (long long k = b0; k < b1; ++k) { const double v = a.val[k]; acc[0] = fma(v, v, acc[0]); }
  block_reduce<1>(acc, scr, -1);
  if (threadIdx.x == 0) out[j] = acc[0];
}
#endif

// ---- the test -----------------------------------------------------------------------------------------------------------------------------
#define FH_SCREEN_ONE_PLUS 0x1.000000000001p+0      // 1 + 2^-48
#define FH_SCREEN_EPS 0x1p-52                       // 2^-52

struct ScreenP {
  const double* g;          // n rows of LB doubles
  const double* norms2;     // n doubles
  const double* cert;       // FH_GAP_NOUT doubles, as k_gap_final wrote them
  uint64_t n;
  uint32_t L, LB, nwg, kappa;
  double mu;
  uint8_t* keep;            // n bytes
  uint32_t* counts;         // nwg kept counts
  double* report;           // rho, kept features, gap_safe, mu
};

// gap_safe from the certificate: one rounded operation per line, as certificates.py spells it
__device__ __forceinline__ double screen_gap_safe(const double* cert, uint32_t kappa) {
#pragma clang fp contract(off)
  const double primal = cert[0], gap = cert[2], f = cert[3], omega = cert[4], s = cert[6], f0 = cert[7];
  if (omega == 0.0 && s == 1.0) return 0.0;      // x0 = 0 inside the dual ball: P - D = 0 as an identity
  const double t1 = f * f0;
  const double t2 = sqrt(t1);
  const double t3 = 2.0 * t2;
  const double t4 = primal + f;
  const double t5 = t4 + t3;
  const double ke = (double)kappa * FH_SCREEN_EPS;
  const double t6 = ke * t5;
  const double t7 = gap + t6;
  return fmax(t7, 0.0);
}

template <int GROUP>
__global__ __launch_bounds__(FH_WG) void k_screen(const ScreenP p) {
#pragma clang fp contract(off)
  __shared__ uint32_t cnt[4];
  const double s = p.cert[6];
  const double gs = screen_gap_safe(p.cert, p.kappa);
  const double g2 = 2.0 * gs;
  const double rho = sqrt(g2);
  const uint64_t j = (uint64_t)blockIdx.x * FH_WG + threadIdx.x;
  uint32_t kept = 0;
  if (j < p.n) {
    const double* gr = p.g + j * p.LB;
    const double c = sqrt(p.norms2[j]);
    const double d = rho * c;
    bool discard = true;
    if (GROUP) {
      double sg = 0.0;
      for (uint32_t l = 0; l < p.L; ++l) { const double gg = gr[l] * gr[l]; sg = sg + gg; }
      const double a = s * sqrt(sg);
      const double e = a + d;
      const double t = e * FH_SCREEN_ONE_PLUS;
      discard = t < p.mu;
    } else {
      for (uint32_t l = 0; l < p.L; ++l) {
        const double a = s * fabs(gr[l]);
        const double e = a + d;
        const double t = e * FH_SCREEN_ONE_PLUS;
        discard = discard && (t < p.mu);
      }
    }
    kept = discard ? 0u : 1u;
    p.keep[j] = (uint8_t)kept;
  }
  const uint32_t wave_kept = (uint32_t)__popcll(__ballot(kept != 0u));
  if ((threadIdx.x & 63) == 0) cnt[threadIdx.x >> 6] = wave_kept;
  __syncthreads();
  if (threadIdx.x == 0) p.counts[blockIdx.x] = ((cnt[0] + cnt[1]) + cnt[2]) + cnt[3];
}

// one workgroup, launched behind k_screen: the counts in index order (integers: any order gives the same), then the report
__global__ void k_screen_final(const ScreenP p);
#ifdef FH_SCREEN_DEFINE
__global__ __launch_bounds__(FH_WG) void k_screen_final(const ScreenP p) {
#pragma clang fp contract(off)
  __shared__ double scr[4];
  double w[1] = {0.0};
  for (uint32_t i = threadIdx.x; i < p.nwg; i += FH_WG) w[0] += (double)p.counts[i];      // (exact: at most 2^31 features)
  block_reduce<1>(w, scr, -1);
  if (threadIdx.x != 0) return;
  const double gs = screen_gap_safe(p.cert, p.kappa);
  const double g2 = 2.0 * gs;
  p.report[0] = sqrt(g2); p.report[1] = w[0]; p.report[2] = gs; p.report[3] = p.mu;
}
#endif

// ---- the copy of the kept columns ---------------------------------------------------------------------------------------------------------
struct GatherP {
  const double* src; double* dst;      // float64 or float32 elements, as the two contexts store A
  const int* idx;                      // count source columns, strictly increasing
  uint64_t m, mp, ld_src, ld_dst, count;
  uint64_t slab;                       // rows per workgroup
};

template <int F32> struct ElemOf { typedef double type; };
template <> struct ElemOf<1> { typedef float type; };

template <int F32>
__global__ __launch_bounds__(FH_WG) void k_gather_cols(const GatherP p) {
  typedef typename PieceOf<F32>::type Piece;
  typedef typename ElemOf<F32>::type Elem;
  constexpr int V = F32 ? 4 : 2;
  const Elem* src = reinterpret_cast<const Elem*>(p.src);
  Piece* dst = reinterpret_cast<Piece*>(p.dst);
  const uint64_t r0 = (uint64_t)blockIdx.x * p.slab;
  const uint64_t r1 = r0 + p.slab < p.mp ? r0 + p.slab : p.mp;
  const uint64_t npieces = p.ld_dst / V;
  for (uint64_t q = threadIdx.x; q < npieces; q += FH_WG) {      // this lane's pieces of every row of the slab: its source columns are read once
    int col[V];
#pragma unroll
    for (int k = 0; k < V; ++k) col[k] = q * V + k < p.count ? p.idx[q * V + k] : -1;
    for (uint64_t i = r0; i < r1; ++i) {
      Elem v[V];
#pragma unroll
      for (int k = 0; k < V; ++k) v[k] = (col[k] >= 0 && i < p.m) ? src[i * p.ld_src + (uint64_t)col[k]] : (Elem)0;
      Piece w;
      if constexpr (F32) w = Piece{v[0], v[1], v[2], v[3]}; else w = Piece{v[0], v[1]};
      dst[i * npieces + q] = w;
    }
  }
}

#define SCREEN_KERNELS(DO)                                                \
  DO __global__ void k_colnorm_dense<0>(const ColnormP);                  \
  DO __global__ void k_colnorm_dense<1>(const ColnormP);                  \
  DO __global__ void k_screen<0>(const ScreenP);                          \
  DO __global__ void k_screen<1>(const ScreenP);                          \
  DO __global__ void k_gather_cols<0>(const GatherP);                     \
  DO __global__ void k_gather_cols<1>(const GatherP);

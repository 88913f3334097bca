// fh_gap.h -- the duality-gap certificate of the committed iterate (fh_dual_gap, include/fasta_hip.h; the host statement of the same numbers is
// fasta_python_amd/certificates.py).  For min_x f(A x) + mu * Omega(x), from x0, g0 = A^H grad f(A x0), z = A x0 and b as they lie in device memory:
//   Omega(x0), the dual norm Omega°(g0), s = 1 if Omega° <= mu else mu / Omega°, P = f(z) + mu * Omega, D = -f*(s * grad f(z)), gap = P - D.
// Ordinary launches only: k_gap_partials (one grid: the first nwg_n workgroups own slabs of rows of x0 / g0, the next nwg_m slabs of rows of z / b;
// one 8-double record each), for the logistic loss k_gap_logistic_dual (one grid over the m side, once s is known: every workgroup forms s from the
// same records in the same order), then the one-workgroup k_gap_final.  No grid barrier, no waiting on another workgroup, no atomics on floats; a
// lane adds its rows in index order, block_reduce and add_records (fh_records.h) fix the rest of the order: bitwise repeatable.  Nothing but the
// workspace is written.  Elementwise operations are never contracted (each rounds like the NumPy expression of certificates.py); the sums use fma().
#pragma once
#include "fh_records.h"

enum { GAP_OMEGA = 0, GAP_DNORM = 1, GAP_F = 2, GAP_RB = 3, GAP_BB = 4, GAP_K = 5 };      // slots of a record; GAP_DNORM is a maximum
#define FH_GAP_LN2 0.6931471805599453      // log(2) rounded to nearest, as certificates.py spells it

struct GapP {
  const double* x; const double* g;      // n-side: rows of LB doubles (the vector form: LB = L = 1)
  const double* z; const double* b;      // m-side, the same layout
  uint64_t n, m;                         // rows on either side
  uint32_t L, LB;
  uint32_t nwg_n, nwg_m;                 // workgroups (= records) of either side in k_gap_partials; a slab may be empty
  uint64_t slab_n, slab_m;               // rows per slab
  int group;                             // 1: Omega = sum of row norms (FH_PROX_GROUP), 0: sum of |x| (FH_PROX_SHRINK)
  double mu;
  double* red;                           // (nwg_n + nwg_m) records of 8 doubles
  double* red2;                          // logistic: nwg_m doubles, the dual sums
  double* out;                           // FH_GAP_NOUT doubles
};

// a * log_a with 0 * log 0 = 0
__device__ __forceinline__ double gap_xlog(double a, double log_a) {
#pragma clang fp contract(off)
  return a == 0.0 ? 0.0 : a * log_a;
}
// h(y + s * (sigma(z) - y)) of one row, h(p) = p log p + (1 - p) log(1 - p), without cancellation: the smaller of p and 1 - p is formed directly
__device__ __forceinline__ double gap_logistic_h(double z, double b, double s) {
#pragma clang fp contract(off)
  const double e = exp(b == 1.0 ? z : -z);      // y = 1: q = s * sigma(-z), h = (1 - q) log1p(-q) + q log q;  y = 0: p = s * sigma(z), the same in p
  const double q = s * (1.0 / (1.0 + e));
  const double r = 1.0 - q;
  return gap_xlog(r, log1p(-q)) + gap_xlog(q, log(q));
}
// the step back into the dual ball
__device__ __forceinline__ double gap_scale(double dnorm, double mu) {
#pragma clang fp contract(off)
  return dnorm <= mu ? 1.0 : mu / dnorm;
}

template <int LOSS>
__global__ __launch_bounds__(FH_WG) void k_gap_partials(const GapP p) {
#pragma clang fp contract(off)
  __shared__ double scr[4 * GAP_K];
  double v[GAP_K];
#pragma unroll
  for (int k = 0; k < GAP_K; ++k) v[k] = 0.0;
  if (blockIdx.x < p.nwg_n) {
    const uint64_t j0 = (uint64_t)blockIdx.x * p.slab_n;
    const uint64_t j1 = j0 + p.slab_n < p.n ? j0 + p.slab_n : p.n;
    for (uint64_t j = j0 + threadIdx.x; j < j1; j += FH_WG) {      // a lane owns whole rows
      const double* xr = p.x + j * p.LB;
      const double* gr = p.g + j * p.LB;
      if (p.group) {
        double sx = 0.0, sg = 0.0;
        for (uint32_t l = 0; l < p.L; ++l) {      // column index order, a rounded product and a rounded sum per column
          const double xx = xr[l] * xr[l], gg = gr[l] * gr[l];
          sx = sx + xx;
          sg = sg + gg;
        }
        v[GAP_OMEGA] += sqrt(sx);
        v[GAP_DNORM] = fmax(v[GAP_DNORM], sqrt(sg));
      } else {
        for (uint32_t l = 0; l < p.L; ++l) {
          v[GAP_OMEGA] += fabs(xr[l]);
          v[GAP_DNORM] = fmax(v[GAP_DNORM], fabs(gr[l]));
        }
      }
    }
  } else {
    const uint64_t i0 = (uint64_t)(blockIdx.x - p.nwg_n) * p.slab_m;
    const uint64_t i1 = i0 + p.slab_m < p.m ? i0 + p.slab_m : p.m;
    for (uint64_t i = i0 + threadIdx.x; i < i1; i += FH_WG) {
      const double* zr = p.z + i * p.LB;
      const double* br = p.b + i * p.LB;
      for (uint32_t l = 0; l < p.L; ++l) {
        if (LOSS == LOSS_LOGISTIC) {
          v[GAP_F] += loss_term(zr[l], br[l], LOSS_LOGISTIC);
        } else {
          const double r = zr[l] - br[l];
          v[GAP_F] = fma(r, r, v[GAP_F]);
          v[GAP_RB] = fma(r, br[l], v[GAP_RB]);
          v[GAP_BB] = fma(br[l], br[l], v[GAP_BB]);
        }
      }
    }
  }
  publish_record<GAP_K, GAP_DNORM>(v, p.red, blockIdx.x, scr);
}

// the logistic dual sum over the m side: sum h(y_i + s * (sigma(z_i) - y_i)) per slab, s from the n-side records of k_gap_partials
template <int LOSS>
__global__ __launch_bounds__(FH_WG) void k_gap_logistic_dual(const GapP p) {
  static_assert(LOSS == LOSS_LOGISTIC, "the least-squares dual needs no second pass");
  __shared__ double scr[4 * 2];
  __shared__ double s_sh;
  double w[2] = {0.0, 0.0};
  add_records<GAP_DNORM, GAP_DNORM + 1, GAP_DNORM>(w, p.red, p.nwg_n);
  block_reduce<2>(w, scr, GAP_DNORM);
  if (threadIdx.x == 0) s_sh = gap_scale(w[GAP_DNORM], p.mu);
  __syncthreads();
  const double s = s_sh;
  double h[1] = {0.0};
  const uint64_t i0 = (uint64_t)blockIdx.x * p.slab_m;
  const uint64_t i1 = i0 + p.slab_m < p.m ? i0 + p.slab_m : p.m;
  for (uint64_t i = i0 + threadIdx.x; i < i1; i += FH_WG) h[0] += gap_logistic_h(p.z[i], p.b[i], s);      // (vector form only: LB = 1)
  publish_record<1, -1>(h, p.red2, blockIdx.x, scr);
}

// one workgroup: the records in index order, then the eight outputs in the order of include/fasta_hip.h
template <int LOSS>
__global__ __launch_bounds__(FH_WG) void k_gap_final(const GapP p) {
#pragma clang fp contract(off)
  __shared__ double scr[4 * (GAP_K + 1)];
  double w[GAP_K + 1];
#pragma unroll
  for (int k = 0; k <= GAP_K; ++k) w[k] = 0.0;
  add_records<0, GAP_K, GAP_DNORM>(w, p.red, p.nwg_n + p.nwg_m);
  if (LOSS == LOSS_LOGISTIC) add_column(w[GAP_K], p.red2, p.nwg_m);
  block_reduce<GAP_K + 1>(w, scr, GAP_DNORM);
  if (threadIdx.x != 0) return;
  const double omega = w[GAP_OMEGA], dnorm = w[GAP_DNORM];
  const double s = gap_scale(dnorm, p.mu);
  double f, dual, f0;
  if (LOSS == LOSS_LOGISTIC) {
    f = w[GAP_F];
    dual = -w[GAP_K];
    f0 = (double)p.m * FH_GAP_LN2;
  } else {
    f = 0.5 * w[GAP_F];
    const double a = (0.5 * (s * s)) * w[GAP_F];      // D = -.5 s^2 ||r||^2 - s <r, b>
    const double c = s * w[GAP_RB];
    dual = -a - c;
    f0 = 0.5 * w[GAP_BB];
  }
  const double reg = p.mu * omega;
  const double primal = f + reg;
  p.out[0] = primal; p.out[1] = dual; p.out[2] = primal - dual; p.out[3] = f;
  p.out[4] = omega; p.out[5] = dnorm; p.out[6] = s; p.out[7] = f0;
}

#define GAP_KERNELS(DO)                                              \
  DO __global__ void k_gap_partials<LOSS_LSQ>(const GapP);           \
  DO __global__ void k_gap_partials<LOSS_LOGISTIC>(const GapP);      \
  DO __global__ void k_gap_logistic_dual<LOSS_LOGISTIC>(const GapP); \
  DO __global__ void k_gap_final<LOSS_LSQ>(const GapP);              \
  DO __global__ void k_gap_final<LOSS_LOGISTIC>(const GapP);

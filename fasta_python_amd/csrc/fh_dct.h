// fh_dct.h -- kernels for the subsampled DCT operator (fh_set_dct): A = diag(d) * C, A^H = C^T * diag(d), C the orthonormal DCT-II of length N
// (scipy.fftpack.dct(x, norm='ortho'); examples/democratic_representation.py:80-82 is the 0/1 case of d).  m = n = N.  An implicit operator: no
// matrix is stored, both directions are ONE complex FFT of length N (Makhoul) done in LDS, in the mould of the other K-fwd + K-adj pairs:
// arrive_last finalisers, no spin waits, no co-residency assumption, no atomics on floats, every sum in a fixed order: bitwise repeatable.
//
//   forward   v[j] = x[2j] (j < ceil(N/2)), v[N-1-j] = x[2j+1];  V = FFT_N(v);  y[k] = s_k * Re(e^{-i pi k / 2N} V[k]),  s_0 = sqrt(1/N), s_k = sqrt(2/N)
//   adjoint   u[0] = w[0] s_0, u[k] = w[k] s_k / 2, u[N] = 0;  V[k] = e^{+i pi k / 2N} (u[k] - i u[N-k]);  v = Re(sum_k V[k] e^{+2 pi i n k / N});
//             x[2j] = v[j], x[2j+1] = v[N-1-j]                                                   (the 1/N of the inverse transform is inside u's scale)
//
// Row FFT: Stockham autosort in two ping-pong LDS buffers, mixed radix {5, 3, 4, 2}, one generic radix-R butterfly (the direct R-point DFT from
// constant roots); a pass of current length n and stride s (n * s = L) maps x[q + s (p + j n/R)], j < R, to y[q + s (R p + k)] = w_n^{p k} sum_j
// x_j w_R^{j k}.  Twiddles come from two device tables built on the host in long double: tw[j] = e^{-2 pi i j / N} (it serves N, N1 and N2: both
// divide N) and pw[k] = e^{-i pi k / 2N}; no sincos in a kernel.  The inverse transform is the same code with conjugated roots (CONJ).
//
//   N <= row cap: ONE launch per direction, one workgroup, one row            (k_dct1_fwd / k_dct1_adj<LDSN>)
//   N  > row cap: N = N1 * N2, n = N2 a1 + a2, k = b1 + N1 b2:  V[b1 + N1 b2] = sum_a2 w_N2^{a2 b2} ( w_N^{a2 b1} sum_a1 v[N2 a1 + a2] w_N1^{a1 b1} )
//                 five launches per direction, every global access contiguous along a row, transposes through padded LDS tiles:
//     k_dct_pre_fwd / k_dct_pre_adj    the n-side prologue (the m-side residual), the Makhoul gather, transpose (a1, a2) -> rows a2 of length N1
//     k_dct_rows<LDSN, CONJ>           N2 row transforms of length N1, times w_N^{a2 b1}
//     k_dct_tr                         transpose (a2, b1) -> rows b1 of length N2
//     k_dct_rows<LDSN, CONJ>           N1 row transforms of length N2
//     k_dct_post_fwd / k_dct_post_adj  transpose (b1, b2) -> k = b1 + N1 b2, the post-twiddle and z = d y with the loss sum (the Makhoul scatter
//                                      and the n-side epilogue (fh_nside.h) in g1's one owner), the finaliser
// LDSN in {128, 512, 2048} is the row-length class: two buffers of LDSN double2 (4 / 16 / 64 KiB), so that short rows do not pay 64 KiB of
// occupancy; a workgroup takes LDSN / L rows (at most DCT_MAX_ROWS).  The geometry is ONE rule on the host (csrc/fh_host_launch.h:dct_shape_for).
// No kernel reads or writes beyond N: every tile access is guarded by the matrix extent, ragged tiles included.  N <= 2^22, so every index
// fits 32 bits; byte offsets are formed by pointer arithmetic in 64 bits.  Elementwise solver arithmetic runs with FMA contraction off
// (fwd_point, prox_scalar, sub_nofma, bb_dgrad: fh_device.h); the transform's own arithmetic may contract.
#pragma once
#include "fh_records.h"

#define DCT_ROW_CAP 2048                           // longest row transform: two ping-pong buffers of 2048 double2 = 64 KiB of LDS
#define DCT_MAXRAD 12                              // radices of a row (2048 = 4^5 * 2: 6; all twos would be 11)
#define DCT_TT 32                                  // transpose tile: DCT_TT x DCT_TT elements, rows padded by one
#define DCT_MAX_ROWS 16                            // rows a workgroup of k_dct_rows takes at most

struct DctRad { uint32_t n; uint8_t r[DCT_MAXRAD]; };      // radix sequence of a row length, in pass order

__device__ __forceinline__ d2 dct_cmul(d2 a, d2 b) { d2 r; r.x = a.x * b.x - a.y * b.y; r.y = a.x * b.y + a.y * b.x; return r; }

// a * e^{-2 pi i T / R} (CONJ: e^{+...}) for compile-time R and T: the exact roots (1, -1, -+i) cost no multiplication
template <int R, int T, int CONJ>
__device__ __forceinline__ d2 dct_root_mul(d2 a) {
  constexpr double H3 = 0.86602540378443864676;                                       // sin(2 pi / 3)
  constexpr double C51 = 0.30901699437494742410, S51 = 0.95105651629515357212;        // cos, sin(2 pi / 5)
  constexpr double C52 = -0.80901699437494742410, S52 = 0.58778525229247312917;       // cos, sin(4 pi / 5)
  double c = 1.0, s = 0.0;                                                            // the root is c - i s
  if (R == 2) { c = T ? -1.0 : 1.0; }
  if (R == 4) { c = T == 0 ? 1.0 : (T == 2 ? -1.0 : 0.0); s = T == 1 ? 1.0 : (T == 3 ? -1.0 : 0.0); }
  if (R == 3) { c = T == 0 ? 1.0 : -0.5; s = T == 0 ? 0.0 : (T == 1 ? H3 : -H3); }
  if (R == 5) { c = T == 0 ? 1.0 : ((T == 1 || T == 4) ? C51 : C52); s = T == 0 ? 0.0 : (T == 1 ? S51 : (T == 2 ? S52 : (T == 3 ? -S52 : -S51))); }
  if (CONJ) s = -s;
  d2 r;
  if (s == 0.0 && c == 1.0) return a;
  if (s == 0.0 && c == -1.0) { r.x = -a.x; r.y = -a.y; return r; }
  if (c == 0.0 && s == 1.0) { r.x = a.y; r.y = -a.x; return r; }                      // a * (-i)
  if (c == 0.0 && s == -1.0) { r.x = -a.y; r.y = a.x; return r; }                     // a * (+i)
  r.x = a.x * c + a.y * s; r.y = a.y * c - a.x * s;
  return r;
}

template <int R, int K, int J, int CONJ>
struct DctSum {                                    // sum_{j <= J} a_j w_R^{j K}, added in ascending j
  static __device__ __forceinline__ d2 run(const d2 (&a)[R]) {
    const d2 lo = DctSum<R, K, J - 1, CONJ>::run(a);
    const d2 t = dct_root_mul<R, (J * K) % R, CONJ>(a[J]);
    d2 r; r.x = lo.x + t.x; r.y = lo.y + t.y;
    return r;
  }
};
template <int R, int K, int CONJ>
struct DctSum<R, K, 0, CONJ> { static __device__ __forceinline__ d2 run(const d2 (&a)[R]) { return a[0]; } };

template <int R, int K, int CONJ>
struct DctOut {                                    // outputs K, K - 1, ..., 0 of one butterfly
  static __device__ __forceinline__ void run(const d2 (&a)[R], d2* y, uint32_t s, const d2* tw, uint32_t tstep) {
    d2 b = DctSum<R, K, R - 1, CONJ>::run(a);
    if (K > 0) {
      d2 w = tw[(uint32_t)K * tstep];              // w_n^{p K}: index p * K * (N / n) < N
      if (CONJ) w.y = -w.y;
      b = dct_cmul(b, w);
    }
    y[(uint32_t)K * s] = b;
    DctOut<R, K - 1, CONJ>::run(a, y, s, tw, tstep);
  }
};
template <int R, int CONJ>
struct DctOut<R, -1, CONJ> { static __device__ __forceinline__ void run(const d2 (&)[R], d2*, uint32_t, const d2*, uint32_t) {} };

// one Stockham pass of radix R over `rows` rows of length L held back to back in src (current length n, stride s, n * s = L); twn = N / n
template <int R, int CONJ>
__device__ __forceinline__ void dct_pass(const d2* src, d2* dst, uint32_t L, uint32_t s, uint32_t rows, const d2* tw, uint32_t twn) {
  const uint32_t per = L / R;                      // butterflies of a row
  for (uint32_t t = threadIdx.x; t < rows * per; t += FH_WG) {
    const uint32_t row = t / per, u = t - row * per;
    const uint32_t p = u / s, q = u - p * s;
    const d2* x = src + row * L + u;
    d2 a[R];
#pragma unroll
    for (int j = 0; j < R; ++j) a[j] = x[(uint32_t)j * per];
    DctOut<R, R - 1, CONJ>::run(a, dst + row * L + q + s * R * p, s, tw, p * twn);
  }
}

// the whole transform of `rows` rows of length L (radices rd) that sit in `a`; returns the buffer that holds the result.  The caller has
// synchronised after filling `a`; the routine ends on a barrier.
template <int CONJ>
__device__ __forceinline__ d2* dct_fft_lds(d2* a, d2* b, uint32_t L, uint32_t rows, const DctRad& rd, const d2* tw, uint32_t N) {
  uint32_t n = L, s = 1u;
  for (uint32_t i = 0; i < rd.n; ++i) {
    const uint32_t r = rd.r[i], twn = N / n;
    if (r == 2u) dct_pass<2, CONJ>(a, b, L, s, rows, tw, twn);
    else if (r == 4u) dct_pass<4, CONJ>(a, b, L, s, rows, tw, twn);
    else if (r == 3u) dct_pass<3, CONJ>(a, b, L, s, rows, tw, twn);
    else dct_pass<5, CONJ>(a, b, L, s, rows, tw, twn);
    __syncthreads();
    d2* t = a; a = b; b = t;
    n /= r; s *= r;
  }
  return a;
}

// the Makhoul permutation: position j of v holds x[dct_src(j)]; element i of x sits at v[dct_pos(i)]
__device__ __forceinline__ uint32_t dct_src(uint32_t j, uint32_t N) { return j < (N + 1u) / 2u ? 2u * j : 2u * (N - 1u - j) + 1u; }
__device__ __forceinline__ uint32_t dct_pos(uint32_t i, uint32_t N) { return (i & 1u) ? N - 1u - (i >> 1) : (i >> 1); }

// ---- parameters ---------------------------------------------------------------------------------------------------------------------------
struct DctOpP {                                    // the operator: sizes, radices, tables, work buffers
  uint32_t N, N1, N2;
  DctRad r1, r2;
  const d2* tw; const d2* pw; const double* diag;  // diag = nullptr: all ones
  double sc0, sck;                                 // sqrt(1/N), sqrt(2/N)
  d2* w0; d2* w1;                                  // two-level form: N double2 each
};

struct DctFwdP {
  DctOpP op;
  int mode;             // 0 = forward point + prox of the solver state, 1 = a plain operand in x0
  int sub_b;
  const double* x0; const double* g0; const double* xacc0;
  double* xhat; double* xp;
  const double* b; double* z;
  double tau;
  ProxP px;             // IDENTITY / SHRINK / NONNEG / BOX / LINF / L1BALL (the level at *px.level)
  unsigned seq;
  uint32_t nred_n;      // two-level: records of k_dct_pre_fwd the finaliser adds (0 in the one-row form and for a plain operand)
  const double* red_n;  // [nred_n][8]
  double* red;          // [gridDim.x][8] of the launch that finalises
  unsigned* counter;
  double* out;
};

struct DctAdjP {
  DctOpP op;
  const double* z; const double* zacc0; const double* b;
  int sub_b, accel, mode;      // mode 0 = FBS (BB epilogue), 1 = plain gradient (g1 only)
  unsigned seq;
  double coef, tau;
  const double* x0; const double* xp; const double* xacc0; const double* xhat;
  double* x1; double* g1;
  uint32_t nred_f;      // two-level: records of k_dct_pre_adj (the loss sum at z')
  const double* red_f;  // [nred_f]
  double* red;          // [gridDim.x][8]: dxdg, dg2, xh2, gsum, gmax, fsq
  unsigned* counter;
  double* out;
};

// ---- shared pieces ------------------------------------------------------------------------------------------------------------------------
// the n-side prologue of element i (the other forms' prologue): returns the transform's operand; v = fsq, dxg0, dx2, xh2, g02, gsum, gmax, rdot
__device__ __forceinline__ double dct_fwd_element(const DctFwdP& p, uint32_t i, double level, double (&v)[8]) {
#pragma clang fp contract(off)
  const double x0e = p.x0[i];
  if (p.mode != 0) return x0e;
  const double g0e = p.g0[i];
  const double xav = p.xacc0 ? p.xacc0[i] : 0.0;
  const double xhe = fwd_point(x0e, g0e, p.tau);
  const double xpe = prox_scalar_rt(p.px.kind, xhe, p.px, level);
  nside_fwd_sums<1>(x0e, g0e, xhe, xpe, xav, v);
  p.xhat[i] = xhe;
  p.xp[i] = xpe;
  return xpe;
}
__device__ __forceinline__ double dct_level(const DctFwdP& p) {
  return (p.mode == 0 && (p.px.kind == PX_LINF || p.px.kind == PX_L1BALL)) ? *p.px.level : 0.0;
}

// z[k] = d[k] * s_k * Re(pw[k] V[k]) and its loss term
__device__ __forceinline__ void dct_fwd_out(const DctFwdP& p, uint32_t k, d2 V, double (&v)[8]) {
  const d2 w = p.op.pw[k];
  const double y = (V.x * w.x - V.y * w.y) * (k ? p.op.sck : p.op.sc0);
  const double d = p.op.diag ? p.op.diag[k] : 1.0;
  const double zv = d == 0.0 ? 0.0 : d * y;
  p.z[k] = zv;
  v[0] += p.sub_b ? loss_term(zv, p.b[k], LOSS_LSQ) : zv * zv;
}

// records in index order, the scalar block and the sequence number: the last workgroup of the launch that ends K-fwd
__device__ __forceinline__ void dct_fwd_finish(const DctFwdP& p, double (&v)[8], double* s_scr, unsigned* s_flag) {
  finish_records<8, S_GMAX>(v, p.red, blockIdx.x, gridDim.x, p.counter, p.out, p.seq, s_scr, s_flag,
                            [&](double (&w)[8]) { add_records<1, 8, S_GMAX>(w, p.red_n, p.nred_n); },      // two-level: k_dct_pre_fwd's n-side sums
                            [&](double (&w)[8]) { store_fwd_scalars(p.out, w, 0.0); });
}

// the m-side residual of row k: r = z' - b (z' = z or its FISTA extrapolation) and the loss term at z'
__device__ __forceinline__ double dct_resid(const DctAdjP& p, uint32_t k, double* term) {
  double zv = p.z[k];
  if (p.accel) zv = extrapolate(zv, p.zacc0[k], p.coef);
  const double bv = p.sub_b ? p.b[k] : 0.0;
  *term = p.sub_b ? loss_term(zv, bv, LOSS_LSQ) : zv * zv;
  return p.sub_b ? loss_grad(zv, bv, LOSS_LSQ) : zv;
}
// V[k] = e^{+i pi k / 2N} (u[k] - i u[N-k]) of the adjoint; the loss term of row k is added to *fsq (row N - k is only read)
__device__ __forceinline__ d2 dct_adj_in(const DctAdjP& p, uint32_t k, double* fsq) {
  const uint32_t N = p.op.N;
  const double half = 0.5 * p.op.sck;
  double term, dummy;
  const double rk = dct_resid(p, k, &term);
  *fsq += term;
  const double uk = rk * (p.op.diag ? p.op.diag[k] : 1.0) * (k ? half : p.op.sc0);
  double um = 0.0;
  if (k) um = dct_resid(p, N - k, &dummy) * (p.op.diag ? p.op.diag[N - k] : 1.0) * half;
  const d2 w = p.op.pw[k];                         // c - i s; its conjugate is c + i s
  d2 V;
  V.x = w.x * uk - w.y * um;
  V.y = -w.y * uk - w.x * um;
  return V;
}

// g1[i] = g and the n-side epilogue of element i, in its one owner; v = dxdg, dg2, xh2, gsum, gmax, fsq
__device__ __forceinline__ void dct_adj_element(const DctAdjP& p, uint32_t i, double g, double (&v)[6]) {
  p.g1[i] = g;
  if (p.mode != 0) return;
  const double x1 = nside_adj_sums(g, p.x0[i], p.xp[i], p.accel ? p.xacc0[i] : 0.0, p.xhat[i], p.accel, p.coef, p.tau, v);
  if (p.accel) p.x1[i] = x1;
}

__device__ __forceinline__ void dct_adj_finish(const DctAdjP& p, double (&v)[6], double* s_scr, unsigned* s_flag) {
  finish_records<6, 4>(v, p.red, blockIdx.x, gridDim.x, p.counter, p.out, p.seq, s_scr, s_flag,
                       [&](double (&w)[6]) { add_column(w[5], p.red_f, p.nred_f); },                      // two-level: k_dct_pre_adj's loss sums
                       [&](double (&w)[6]) { store_adj_scalars(p.out, w); });
}

// ---- N <= row cap: one launch per direction, one workgroup -----------------------------------------------------------------------------------
template <int LDSN>
__global__ __launch_bounds__(FH_WG) void k_dct1_fwd(const DctFwdP p) {
  __shared__ __attribute__((aligned(16))) d2 s_a[LDSN];
  __shared__ __attribute__((aligned(16))) d2 s_b[LDSN];
  __shared__ __attribute__((aligned(16))) double s_scr[4 * 8];
  __shared__ __attribute__((aligned(16))) unsigned s_flag[4];
  const uint32_t tid = threadIdx.x, N = p.op.N;
  const double level = dct_level(p);
  double v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (uint32_t i = tid; i < N; i += FH_WG) {
    d2 e; e.x = dct_fwd_element(p, i, level, v); e.y = 0.0;
    s_a[dct_pos(i, N)] = e;
  }
  __syncthreads();
  const d2* res = dct_fft_lds<0>(s_a, s_b, N, 1u, p.op.r1, p.op.tw, N);
  for (uint32_t k = tid; k < N; k += FH_WG) dct_fwd_out(p, k, res[k], v);
  dct_fwd_finish(p, v, s_scr, s_flag);
}

template <int LDSN>
__global__ __launch_bounds__(FH_WG) void k_dct1_adj(const DctAdjP p) {
  __shared__ __attribute__((aligned(16))) d2 s_a[LDSN];
  __shared__ __attribute__((aligned(16))) d2 s_b[LDSN];
  __shared__ __attribute__((aligned(16))) double s_scr[4 * 8];
  __shared__ __attribute__((aligned(16))) unsigned s_flag[4];
  const uint32_t tid = threadIdx.x, N = p.op.N;
  double v[6] = {0, 0, 0, 0, 0, 0};
  for (uint32_t k = tid; k < N; k += FH_WG) s_a[k] = dct_adj_in(p, k, &v[5]);
  __syncthreads();
  const d2* res = dct_fft_lds<1>(s_a, s_b, N, 1u, p.op.r1, p.op.tw, N);
  for (uint32_t i = tid; i < N; i += FH_WG) dct_adj_element(p, i, res[dct_pos(i, N)].x, v);
  dct_adj_finish(p, v, s_scr, s_flag);
}

// ---- N > row cap -----------------------------------------------------------------------------------------------------------------------------
// a tile of a rows x cols matrix: origin and the threads' (column, first row) inside it; 256 threads = 32 columns x 8 rows, four trips
struct DctTile { uint32_t r0, c0, tx, ty; };
template <int TT>
__device__ __forceinline__ DctTile dct_tile(uint32_t cols) {
  const uint32_t tiles_c = (cols + TT - 1) / TT;
  DctTile t;
  t.r0 = (blockIdx.x / tiles_c) * TT; t.c0 = (blockIdx.x % tiles_c) * TT;
  t.tx = threadIdx.x % TT; t.ty = threadIdx.x / TT;
  return t;
}

// `nrows` row transforms of length L: workgroup w takes rows [w * rpw, ...).  real_in: the rows are doubles (K-fwd's first pass).  tw6: the
// result of row a2 is multiplied by w_N^{a2 b1} (the six-step twiddle; a2 * b1 < N)
struct DctRowsP {
  uint32_t N, L, nrows, rpw;
  DctRad rd;
  const d2* tw;
  const void* in; d2* out;
  int real_in, tw6;
};
template <int LDSN, int CONJ>
__global__ __launch_bounds__(FH_WG) void k_dct_rows(const DctRowsP p) {
  __shared__ __attribute__((aligned(16))) d2 s_a[LDSN];
  __shared__ __attribute__((aligned(16))) d2 s_b[LDSN];
  const uint32_t row0 = blockIdx.x * p.rpw;
  const uint32_t rows = p.nrows - row0 < p.rpw ? p.nrows - row0 : p.rpw;
  const uint32_t cnt = rows * p.L;                 // <= LDSN (dct_shape_for)
  const uint64_t base = (uint64_t)row0 * p.L;
  if (p.real_in) {
    const double* in = static_cast<const double*>(p.in) + base;
    for (uint32_t t = threadIdx.x; t < cnt; t += FH_WG) { d2 e; e.x = in[t]; e.y = 0.0; s_a[t] = e; }
  } else {
    const d2* in = static_cast<const d2*>(p.in) + base;
    for (uint32_t t = threadIdx.x; t < cnt; t += FH_WG) s_a[t] = in[t];
  }
  __syncthreads();
  const d2* res = dct_fft_lds<CONJ>(s_a, s_b, p.L, rows, p.rd, p.tw, p.N);
  d2* out = p.out + base;
  for (uint32_t t = threadIdx.x; t < cnt; t += FH_WG) {
    d2 e = res[t];
    if (p.tw6) {
      const uint32_t row = t / p.L, col = t - row * p.L;
      d2 w = p.tw[(row0 + row) * col];
      if (CONJ) w.y = -w.y;
      e = dct_cmul(e, w);
    }
    out[t] = e;
  }
}

// first launch of K-fwd: v as the N1 x N2 matrix (a1, a2), j = N2 a1 + a2, gathered from x through the prologue; written as REAL rows a2 of length N1
template <int TT>
__global__ __launch_bounds__(FH_WG) void k_dct_pre_fwd(const DctFwdP p) {
  __shared__ double s_t[TT][TT + 1];
  __shared__ __attribute__((aligned(16))) double s_scr[4 * 8];
  const uint32_t N = p.op.N, N1 = p.op.N1, N2 = p.op.N2;
  const DctTile t = dct_tile<TT>(N2);
  const double level = dct_level(p);
  double v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (uint32_t rr = t.ty; rr < TT; rr += FH_WG / TT) {
    const uint32_t a1 = t.r0 + rr, a2 = t.c0 + t.tx;
    if (a1 < N1 && a2 < N2) s_t[rr][t.tx] = dct_fwd_element(p, dct_src(N2 * a1 + a2, N), level, v);
  }
  __syncthreads();
  double* out = reinterpret_cast<double*>(p.op.w0);
  for (uint32_t cc = t.ty; cc < TT; cc += FH_WG / TT) {
    const uint32_t a2 = t.c0 + cc, a1 = t.r0 + t.tx;
    if (a1 < N1 && a2 < N2) out[a2 * N1 + a1] = s_t[t.tx][cc];
  }
  if (p.mode != 0) return;                          // a plain operand has no n-side sums
  publish_record<8, S_GMAX>(v, const_cast<double*>(p.red_n), blockIdx.x, s_scr);
}

// out (cols x rows) = in (rows x cols) transposed, complex
template <int TT>
__global__ __launch_bounds__(FH_WG) void k_dct_tr(const d2* in, d2* out, uint32_t rows, uint32_t cols) {
  __shared__ __attribute__((aligned(16))) d2 s_t[TT][TT + 1];
  const DctTile t = dct_tile<TT>(cols);
  for (uint32_t rr = t.ty; rr < TT; rr += FH_WG / TT) {
    const uint32_t r = t.r0 + rr, c = t.c0 + t.tx;
    if (r < rows && c < cols) s_t[rr][t.tx] = in[r * cols + c];
  }
  __syncthreads();
  for (uint32_t cc = t.ty; cc < TT; cc += FH_WG / TT) {
    const uint32_t c = t.c0 + cc, r = t.r0 + t.tx;
    if (r < rows && c < cols) out[c * rows + r] = s_t[t.tx][cc];
  }
}

// last launch of K-fwd: V as the N1 x N2 matrix (b1, b2) in w0 -> k = b1 + N1 b2, z = d y, the loss sum, the finaliser
template <int TT>
__global__ __launch_bounds__(FH_WG) void k_dct_post_fwd(const DctFwdP p) {
  __shared__ __attribute__((aligned(16))) d2 s_t[TT][TT + 1];
  __shared__ __attribute__((aligned(16))) double s_scr[4 * 8];
  __shared__ __attribute__((aligned(16))) unsigned s_flag[4];
  const uint32_t N1 = p.op.N1, N2 = p.op.N2;
  const DctTile t = dct_tile<TT>(N2);
  double v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (uint32_t rr = t.ty; rr < TT; rr += FH_WG / TT) {
    const uint32_t b1 = t.r0 + rr, b2 = t.c0 + t.tx;
    if (b1 < N1 && b2 < N2) s_t[rr][t.tx] = p.op.w0[b1 * N2 + b2];
  }
  __syncthreads();
  for (uint32_t cc = t.ty; cc < TT; cc += FH_WG / TT) {
    const uint32_t b2 = t.c0 + cc, b1 = t.r0 + t.tx;
    if (b1 < N1 && b2 < N2) dct_fwd_out(p, b1 + N1 * b2, s_t[t.tx][cc], v);
  }
  dct_fwd_finish(p, v, s_scr, s_flag);
}

// first launch of K-adj: V[k], k = N2 a1 + a2, from the residual; written as complex rows a2 of length N1; the loss sum at z', one record per workgroup
template <int TT>
__global__ __launch_bounds__(FH_WG) void k_dct_pre_adj(const DctAdjP p) {
  __shared__ __attribute__((aligned(16))) d2 s_t[TT][TT + 1];
  __shared__ __attribute__((aligned(16))) double s_scr[4];
  const uint32_t N1 = p.op.N1, N2 = p.op.N2;
  const DctTile t = dct_tile<TT>(N2);
  double v[1] = {0.0};
  for (uint32_t rr = t.ty; rr < TT; rr += FH_WG / TT) {
    const uint32_t a1 = t.r0 + rr, a2 = t.c0 + t.tx;
    if (a1 < N1 && a2 < N2) s_t[rr][t.tx] = dct_adj_in(p, N2 * a1 + a2, &v[0]);
  }
  __syncthreads();
  for (uint32_t cc = t.ty; cc < TT; cc += FH_WG / TT) {
    const uint32_t a2 = t.c0 + cc, a1 = t.r0 + t.tx;
    if (a1 < N1 && a2 < N2) p.op.w0[a2 * N1 + a1] = s_t[t.tx][cc];
  }
  publish_record<1, -1>(v, const_cast<double*>(p.red_f), blockIdx.x, s_scr);
}

// last launch of K-adj: v[n], n = b1 + N1 b2, from the N1 x N2 matrix (b1, b2) in w0; g1[dct_src(n)] = Re v[n] and the n-side epilogue, the finaliser
template <int TT>
__global__ __launch_bounds__(FH_WG) void k_dct_post_adj(const DctAdjP p) {
  __shared__ double s_t[TT][TT + 1];
  __shared__ __attribute__((aligned(16))) double s_scr[4 * 8];
  __shared__ __attribute__((aligned(16))) unsigned s_flag[4];
  const uint32_t N = p.op.N, N1 = p.op.N1, N2 = p.op.N2;
  const DctTile t = dct_tile<TT>(N2);
  double v[6] = {0, 0, 0, 0, 0, 0};
  for (uint32_t rr = t.ty; rr < TT; rr += FH_WG / TT) {
    const uint32_t b1 = t.r0 + rr, b2 = t.c0 + t.tx;
    if (b1 < N1 && b2 < N2) s_t[rr][t.tx] = p.op.w0[b1 * N2 + b2].x;
  }
  __syncthreads();
  for (uint32_t cc = t.ty; cc < TT; cc += FH_WG / TT) {
    const uint32_t b2 = t.c0 + cc, b1 = t.r0 + t.tx;
    if (b1 < N1 && b2 < N2) dct_adj_element(p, dct_src(b1 + N1 * b2, N), s_t[t.tx][cc], v);
  }
  dct_adj_finish(p, v, s_scr, s_flag);
}

// ---- the instantiations (ONE table for fh_dct_part.hip, the extern declarations and the dispatch) ----
#define DCT_FOR_EACH(X) X(128) X(512) X(2048)
#define DCT_KERNELS(DO, LDSN)                                   \
  DO __global__ void k_dct1_fwd<LDSN>(const DctFwdP);           \
  DO __global__ void k_dct1_adj<LDSN>(const DctAdjP);           \
  DO __global__ void k_dct_rows<LDSN, 0>(const DctRowsP);       \
  DO __global__ void k_dct_rows<LDSN, 1>(const DctRowsP);
#define DCT_TILE_KERNELS(DO)                                                          \
  DO __global__ void k_dct_pre_fwd<DCT_TT>(const DctFwdP);                           \
  DO __global__ void k_dct_post_fwd<DCT_TT>(const DctFwdP);                          \
  DO __global__ void k_dct_pre_adj<DCT_TT>(const DctAdjP);                           \
  DO __global__ void k_dct_post_adj<DCT_TT>(const DctAdjP);                          \
  DO __global__ void k_dct_tr<DCT_TT>(const d2*, d2*, uint32_t, uint32_t);

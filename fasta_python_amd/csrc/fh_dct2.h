// fh_dct2.h -- kernels for the subsampled 2-D DCT operator on an H x W image (fh_set_dct2): A x = d * (C_H X C_W^T), A^H w = C_H^T (d * w) C_W, C_L the
// orthonormal DCT-II of length L (fh_dct.h; scipy.fftpack.dctn / idctn with norm='ortho').  m = n = H * W, images row-major.  The separable transform is
// fh_dct.h's row transform along the two axes: the Makhoul permutation, one complex Stockham FFT of the row's length in LDS (dct_fft_lds), the post-twiddle
// to a REAL row -- so everything that travels between the launches is a real H * W image (8 bytes an element, not the 1-D two-level form's 16).  Four
// ordinary launches per direction, in the mould of the 1-D operator's two-level form: arrive_last finalisers, no spin waits, no co-residency assumption, no
// atomics on floats, every sum in a fixed order: bitwise repeatable.
//
//   K-fwd   k_dct2_fwd_rows<LDSN, 1>   rows i of length W: the n-side prologue of element (i, j) (dct_fwd_element: forward point, prox, the eight n-side sums,
//                                      xhat / xp written once), Makhoul gather, row FFT, post-twiddle; w0 (H x W) = X C_W^T, one n-side record per workgroup
//           k_dct2_tr                  w1 (W x H) = w0^T, through padded 32 x 32 LDS tiles
//           k_dct2_fwd_rows<LDSN, 0>   rows j of length H, in place: w1 (W x H) = (C_H X C_W^T)^T
//           k_dct2_post_fwd            transpose back: z[i, j] = d y with the loss sum, the finaliser
//   K-adj   k_dct2_pre_adj             the m-side residual r = z' - b (z' = z or its FISTA extrapolation), the loss term at z'; w0 (W x H) = (d r)^T, one loss record per workgroup
//           k_dct2_adj_rows<LDSN, 0>   rows j of length H, in place: the DCT-III (pre-twiddle, inverse row FFT, Makhoul scatter)
//           k_dct2_tr                  w1 (H x W) = w0^T
//           k_dct2_adj_rows<LDSN, 1>   rows i of length W: the DCT-III, g1 and the n-side epilogue (fh_nside.h) in g1's one owner, the finaliser
// An axis of length 1 is the identity (no radix pass, pw[0] = 1, s_0 = 1) and takes the same chain.  Each axis has its own twiddle tables, built on the host
// in long double: tw[j] = e^{-2 pi i j / L}, pw[k] = e^{-i pi k / 2L}; no sincos in a kernel.  LDSN in {128, 512, 2048} is the row-length class of an axis; a
// workgroup takes whole rows, as many as the host rule gives it (csrc/fh_host_launch.h:dct2_shape_for), so a row launch may write where it read.  Every
// global access is contiguous along a row; no kernel reads or writes beyond H * W: ragged tiles and a ragged last row group are guarded by the extent.
// H, W <= 2048, so every index fits 32 bits.  Elementwise solver arithmetic runs with FMA contraction off (fh_dct.h's shared pieces); the transform's own
// arithmetic may contract.  Rows are transformed one real row per complex FFT (no two-rows-in-one packing): the error bound is the 1-D operator's per axis.
#pragma once
#include "fh_dct.h"

struct Dct2AxisP {                                 // one axis: length, radices, tables, scales
  uint32_t L;
  DctRad rd;
  const d2* tw; const d2* pw;
  double sc0, sck;                                 // sqrt(1/L), sqrt(2/L)
};
struct Dct2OpP {
  uint32_t H, W;
  Dct2AxisP ah, aw;
  uint32_t rpw_h, rpw_w;                           // rows a workgroup takes along H (W rows of length H) and along W (H rows of length W)
  const double* diag;                              // nullptr: all ones
  double* w0; double* w1;                          // H * W doubles each
};
struct Dct2FwdP { DctFwdP f; Dct2OpP o; };         // f: the solver side (f.op is not read); f.red_n / f.nred_n: the first row launch's records
struct Dct2AdjP { DctAdjP a; Dct2OpP o; };         // a.red_f / a.nred_f: k_dct2_pre_adj's loss records

// rows [row0, row0 + rows) of workgroup blockIdx.x
__device__ __forceinline__ uint32_t dct2_rows_of(uint32_t nrows, uint32_t rpw, uint32_t* row0) {
  *row0 = blockIdx.x * rpw;
  return nrows - *row0 < rpw ? nrows - *row0 : rpw;
}

// DCT-II of `nrows` rows of length ax.L.  FIRST: the rows are the solver's unknown through the prologue, the result goes to o.w0 and the n-side sums to
// record blockIdx.x of f.red_n; otherwise the rows of o.w1 in place.
template <int LDSN, int FIRST>
__global__ __launch_bounds__(FH_WG) void k_dct2_fwd_rows(const Dct2FwdP p) {
  __shared__ __attribute__((aligned(16))) d2 s_a[LDSN];
  __shared__ __attribute__((aligned(16))) d2 s_b[LDSN];
  __shared__ __attribute__((aligned(16))) double s_scr[4 * 8];
  const Dct2AxisP& ax = FIRST ? p.o.aw : p.o.ah;
  const uint32_t L = ax.L;
  uint32_t row0;
  const uint32_t rows = dct2_rows_of(FIRST ? p.o.H : p.o.W, FIRST ? p.o.rpw_w : p.o.rpw_h, &row0);
  const uint32_t cnt = rows * L, base = row0 * L;  // cnt <= LDSN (dct2_shape_for)
  double v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const double level = FIRST ? dct_level(p.f) : 0.0;
  for (uint32_t t = threadIdx.x; t < cnt; t += FH_WG) {
    const uint32_t row = t / L, col = t - row * L;
    d2 e; e.y = 0.0;
    if (FIRST) e.x = dct_fwd_element(p.f, base + t, level, v); else e.x = p.o.w1[base + t];
    s_a[row * L + dct_pos(col, L)] = e;
  }
  __syncthreads();
  const d2* res = dct_fft_lds<0>(s_a, s_b, L, rows, ax.rd, ax.tw, L);
  double* out = (FIRST ? p.o.w0 : p.o.w1) + base;
  for (uint32_t t = threadIdx.x; t < cnt; t += FH_WG) {
    const uint32_t row = t / L, k = t - row * L;
    const d2 V = res[t], w = ax.pw[k];
    out[t] = (V.x * w.x - V.y * w.y) * (k ? ax.sck : ax.sc0);
  }
  if (FIRST && p.f.mode == 0) publish_record<8, S_GMAX>(v, const_cast<double*>(p.f.red_n), blockIdx.x, s_scr);      // (a plain operand has no n-side sums)
}

// out (cols x rows) = in (rows x cols) transposed, real
template <int TT>
__global__ __launch_bounds__(FH_WG) void k_dct2_tr(const double* in, double* out, uint32_t rows, uint32_t cols) {
  __shared__ double s_t[TT][TT + 1];
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

// last launch of K-fwd: w1 (W x H) holds the transform transposed -> z[i, j] = d y, the loss sum, the finaliser
template <int TT>
__global__ __launch_bounds__(FH_WG) void k_dct2_post_fwd(const Dct2FwdP p) {
#pragma clang fp contract(off)
  __shared__ double s_t[TT][TT + 1];
  __shared__ __attribute__((aligned(16))) double s_scr[4 * 8];
  __shared__ __attribute__((aligned(16))) unsigned s_flag[4];
  const uint32_t H = p.o.H, W = p.o.W;
  const DctTile t = dct_tile<TT>(H);               // tiles of the W x H matrix
  double v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (uint32_t rr = t.ty; rr < TT; rr += FH_WG / TT) {
    const uint32_t j = t.r0 + rr, i = t.c0 + t.tx;
    if (j < W && i < H) s_t[rr][t.tx] = p.o.w1[j * H + i];
  }
  __syncthreads();
  for (uint32_t cc = t.ty; cc < TT; cc += FH_WG / TT) {
    const uint32_t i = t.c0 + cc, j = t.r0 + t.tx;
    if (j < W && i < H) {
      const uint32_t k = i * W + j;
      const double y = s_t[t.tx][cc];
      const double d = p.o.diag ? p.o.diag[k] : 1.0;
      const double zv = d == 0.0 ? 0.0 : d * y;
      p.f.z[k] = zv;
      v[0] += p.f.sub_b ? loss_term(zv, p.f.b[k], LOSS_LSQ) : zv * zv;
    }
  }
  dct_fwd_finish(p.f, v, s_scr, s_flag);
}

// first launch of K-adj: w0 (W x H) = (d * r)^T, r the m-side residual; the loss sum at z', one record per workgroup
template <int TT>
__global__ __launch_bounds__(FH_WG) void k_dct2_pre_adj(const Dct2AdjP p) {
#pragma clang fp contract(off)
  __shared__ double s_t[TT][TT + 1];
  __shared__ __attribute__((aligned(16))) double s_scr[4];
  const uint32_t H = p.o.H, W = p.o.W;
  const DctTile t = dct_tile<TT>(W);               // tiles of the H x W matrix
  double v[1] = {0.0};
  for (uint32_t rr = t.ty; rr < TT; rr += FH_WG / TT) {
    const uint32_t i = t.r0 + rr, j = t.c0 + t.tx;
    if (i < H && j < W) {
      const uint32_t k = i * W + j;
      double term;
      const double r = dct_resid(p.a, k, &term);
      v[0] += term;
      s_t[rr][t.tx] = r * (p.o.diag ? p.o.diag[k] : 1.0);
    }
  }
  __syncthreads();
  for (uint32_t cc = t.ty; cc < TT; cc += FH_WG / TT) {
    const uint32_t j = t.c0 + cc, i = t.r0 + t.tx;
    if (i < H && j < W) p.o.w0[j * H + i] = s_t[t.tx][cc];
  }
  publish_record<1, -1>(v, const_cast<double*>(p.a.red_f), blockIdx.x, s_scr);
}

// DCT-III of `nrows` real rows of length ax.L: u[0] = w[0] s_0, u[k] = w[k] s_k / 2; V[k] = e^{+i pi k / 2L} (u[k] - i u[L-k]); v = Re(inverse FFT); x[2j] =
// v[j], x[2j+1] = v[L-1-j].  LAST = 0: the rows of o.w0 (W rows of length H) in place; LAST = 1: the rows of o.w1 (H rows of length W) into g1 with the
// n-side epilogue and the finaliser.
template <int LDSN, int LAST>
__global__ __launch_bounds__(FH_WG) void k_dct2_adj_rows(const Dct2AdjP p) {
  __shared__ __attribute__((aligned(16))) d2 s_a[LDSN];
  __shared__ __attribute__((aligned(16))) d2 s_b[LDSN];
  __shared__ __attribute__((aligned(16))) double s_scr[4 * 8];
  __shared__ __attribute__((aligned(16))) unsigned s_flag[4];
  const Dct2AxisP& ax = LAST ? p.o.aw : p.o.ah;
  const uint32_t L = ax.L;
  uint32_t row0;
  const uint32_t rows = dct2_rows_of(LAST ? p.o.H : p.o.W, LAST ? p.o.rpw_w : p.o.rpw_h, &row0);
  const uint32_t cnt = rows * L, base = row0 * L;  // cnt <= LDSN (dct2_shape_for)
  const double* in = (LAST ? p.o.w1 : p.o.w0) + base;
  double* s_r = reinterpret_cast<double*>(s_b);    // the real rows, staged so that u[k] and u[L-k] are read from LDS
  for (uint32_t t = threadIdx.x; t < cnt; t += FH_WG) s_r[t] = in[t];
  __syncthreads();
  const double half = 0.5 * ax.sck;
  for (uint32_t t = threadIdx.x; t < cnt; t += FH_WG) {
    const uint32_t row = t / L, k = t - row * L;
    const double uk = s_r[t] * (k ? half : ax.sc0);
    const double um = k ? s_r[row * L + L - k] * half : 0.0;
    const d2 w = ax.pw[k];                         // c - i s; its conjugate is c + i s
    d2 V;
    V.x = w.x * uk - w.y * um;
    V.y = -w.y * uk - w.x * um;
    s_a[t] = V;
  }
  __syncthreads();
  const d2* res = dct_fft_lds<1>(s_a, s_b, L, rows, ax.rd, ax.tw, L);
  if (!LAST) {
    double* out = p.o.w0 + base;
    for (uint32_t t = threadIdx.x; t < cnt; t += FH_WG) {
      const uint32_t row = t / L, i = t - row * L;
      out[t] = res[row * L + dct_pos(i, L)].x;
    }
    return;
  }
  double v[6] = {0, 0, 0, 0, 0, 0};
  for (uint32_t t = threadIdx.x; t < cnt; t += FH_WG) {
    const uint32_t row = t / L, i = t - row * L;
    dct_adj_element(p.a, base + t, res[row * L + dct_pos(i, L)].x, v);
  }
  dct_adj_finish(p.a, v, s_scr, s_flag);
}

// ---- the instantiations (ONE table for fh_dct2_part.hip, the extern declarations and the dispatch) ----
#define DCT2_KERNELS(DO, LDSN)                                       \
  DO __global__ void k_dct2_fwd_rows<LDSN, 0>(const Dct2FwdP);       \
  DO __global__ void k_dct2_fwd_rows<LDSN, 1>(const Dct2FwdP);       \
  DO __global__ void k_dct2_adj_rows<LDSN, 0>(const Dct2AdjP);       \
  DO __global__ void k_dct2_adj_rows<LDSN, 1>(const Dct2AdjP);
#define DCT2_TILE_KERNELS(DO)                                                             \
  DO __global__ void k_dct2_post_fwd<DCT_TT>(const Dct2FwdP);                            \
  DO __global__ void k_dct2_pre_adj<DCT_TT>(const Dct2AdjP);                             \
  DO __global__ void k_dct2_tr<DCT_TT>(const double*, double*, uint32_t, uint32_t);

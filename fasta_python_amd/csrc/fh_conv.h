// fh_conv.h -- kernels for the small-kernel periodic convolution operator (fh_set_conv2d): an image x of shape (H, W), taps K of shape
// (kh, kw) with 1 <= kh, kw <= 16, origin (oh, ow), optional diagonal d; m = n = H * W, all indices modulo the dimension.
//
//   (A x)[i,j]   = d[i,j] * sum_{a,b} K[a,b] * x[i-(a-oh), j-(b-ow)]           true convolution
//   (A^T w)[i,j] =          sum_{a,b} K[a,b] * (d*w)[i+(a-oh), j+(b-ow)]       correlation
//
// The arithmetic is the contract: the accumulator starts at +0.0, taps are visited a outer, b inner, both ascending, every term is a rounded
// product followed by a rounded sum (fp contract(off): no FMA), no tap is skipped, d is applied last in A and first in A^T, and d == 0.0
// gives z == 0.0 exactly.  That is `out = zeros; for a: for b: out += K[a,b] * np.roll(x, (a-oh, b-ow), axis=(0,1))`, so the device is held
// to the host closures with ==.
//
// A plain K-fwd + K-adj pair in the mould of fh_tv3d.h: one launch per direction, arrive_last finalisers, no spin waits, no atomics on
// floats, every sum in a fixed order: bitwise repeatable.  Vectors are the C order of (H, W) in the vector form's padded buffers.
//
// A workgroup owns a tile of th x tw output pixels (ConvGeo, chosen on the host by ONE rule: csrc/fh_host_launch.h:conv_shape_for) and
// stages the operand of the tile WITH its halo -- kh - 1 rows and kw - 1 columns, split between the two sides by the origin -- in LDS.
//   k_conv_fwd<MODE>  mode 0: xhat = x0 - tau * g0 and xprox = prox(xhat), both written by the owner, z = A xprox written, the loss sum and the
//               seven n-side sums of the other forms' prologues; mode 1: z = A x0 of a plain operand.  Halo values are RECOMPUTED from
//               x0 / g0, never read back from a stored xprox; the sums count a pixel in its owner only.  Prox kinds: IDENTITY, SHRINK,
//               NONNEG, BOX, and LINF / L1BALL with the level the search in front of the launch left at *px.level.
//   k_conv_adj<MODE>  r = z' - b (z' = z or its FISTA extrapolation; the loss at z' is FH_S_FSQ_ADJ), d * r staged with its halo,
//               g1 = correlation written, and the n-side epilogue (fh_nside.h) in the owner's lane (every g1 entry has one owner); modes 0, 1.
// The tap loop: a lane computes CONV_RUN = 8 consecutive outputs along w.  Per kernel row it reads the CONV_RUN + kw - 1 operands of that
// row from LDS ONCE into registers and slides over them for the kw taps: (8 + kw - 1) / (8 kw) LDS reads per tap instead of 1.  kh is a
// run-time trip count; kw selects one of 16 unrolled bodies (conv_taps<KW>) by a grid-uniform switch, so the window is indexed by constants
// and stays in registers.  The taps travel in the kernel's argument block: uniform, read through the scalar cache, no address arithmetic
// per lane.  LDS columns are skewed by one double every 8 (index c + c / 8) and the row pitch is 8 mod 32 doubles, so the 32 lanes of a
// half wave -- 4 rows x 8 runs, starts 9 doubles apart -- read 32 different 8-byte banks at every window position.
// After the tap loop the outputs go back through LDS so that z / g1 and everything the epilogues read and write are wave-contiguous.
// Wraps are a conditional correction where the kernel is no larger than the image along that axis, a true modulo otherwise.
#pragma once
#include "fh_records.h"

#define CONV_RUN 8                                 // consecutive outputs along w per lane
#define CONV_MAXK 16                               // taps per axis, at most
#define CONV_TILE_PIX (CONV_RUN * FH_WG)           // output pixels of a tile: 32 x 64, or 1 x 2048 for a signal (H == 1, kh == 1)
#define CONV_LDS_DOUBLES 4888                      // (32 + 15) rows x pitch 104; the flat tile needs one row of 2344
#define CONV_SKEW(c) ((c) + ((c) >> 3))

struct ConvGeo {
  uint32_t H, W, kh, kw, oh, ow;
  uint32_t th, tw, tw_log2, pitch, tiles_w;        // tile, log2 of its width, LDS row pitch in doubles, tiles along w
};

// where a workgroup works: tile origin and its clipped extent
struct ConvTile { uint32_t h0, w0, the, twe; };
__device__ __forceinline__ ConvTile conv_tile(const ConvGeo& g) {
  ConvTile t;
  t.w0 = (blockIdx.x % g.tiles_w) * g.tw; t.h0 = (blockIdx.x / g.tiles_w) * g.th;
  t.twe = g.W - t.w0 < g.tw ? g.W - t.w0 : g.tw;
  t.the = g.H - t.h0 < g.th ? g.H - t.h0 : g.th;
  return t;
}
__device__ __forceinline__ uint32_t conv_wrap(int32_t v, uint32_t n, bool mod) {
  if (mod) { const int32_t r = v % (int32_t)n; return (uint32_t)(r < 0 ? r + (int32_t)n : r); }
  if (v < 0) v += (int32_t)n; else if (v >= (int32_t)n) v -= (int32_t)n;
  return (uint32_t)v;
}

// the taps of all kernel rows on this lane's run: ADJ = 0 convolution (LDS row r + kh-1 - a, column c + kw-1 - b), 1 correlation (r + a, c + b)
template <int KW, int ADJ>
__device__ __forceinline__ void conv_taps(const double* s, uint32_t base, uint32_t pitch, uint32_t kh, const double (&taps)[CONV_MAXK * CONV_MAXK],
                                          double (&acc)[CONV_RUN]) {
#pragma clang fp contract(off)
  for (uint32_t a = 0; a < kh; ++a) {
    const double* row = s + base + (ADJ ? a : kh - 1u - a) * pitch;
    double win[CONV_RUN + KW - 1];
#pragma unroll
    for (int j = 0; j < CONV_RUN + KW - 1; ++j) win[j] = row[CONV_SKEW(j)];
#pragma unroll
    for (int b = 0; b < KW; ++b) {
      const double kv = taps[a * KW + b];
#pragma unroll
      for (int j = 0; j < CONV_RUN; ++j) {
        const double t = kv * win[ADJ ? j + b : j + KW - 1 - b];
        acc[j] = acc[j] + t;
      }
    }
  }
}
template <int ADJ>
__device__ __forceinline__ void conv_taps_kw(const double* s, uint32_t base, const ConvGeo& g, const double (&taps)[CONV_MAXK * CONV_MAXK],
                                             double (&acc)[CONV_RUN]) {
  switch (g.kw) {                                  // grid-uniform
#define CONV_CASE(KW) case KW: conv_taps<KW, ADJ>(s, base, g.pitch, g.kh, taps, acc); break;
    CONV_CASE(1) CONV_CASE(2) CONV_CASE(3) CONV_CASE(4) CONV_CASE(5) CONV_CASE(6) CONV_CASE(7) CONV_CASE(8)
    CONV_CASE(9) CONV_CASE(10) CONV_CASE(11) CONV_CASE(12) CONV_CASE(13) CONV_CASE(14) CONV_CASE(15) CONV_CASE(16)
#undef CONV_CASE
    default: break;
  }
}

// the tap loop of a whole tile, LDS to LDS: on entry `s` holds the staged operand (rows the + kh - 1, columns twe + kw - 1, skewed), on
// return the tile's outputs at s[r * pitch + CONV_SKEW(c)]
template <int ADJ>
__device__ __forceinline__ void conv_tile_taps(double* s, const ConvGeo& g, const double (&taps)[CONV_MAXK * CONV_MAXK]) {
  const uint32_t runs = g.tw / CONV_RUN;           // runs of a tile row: 8, or 256 for the flat tile
  const uint32_t r = threadIdx.x / runs, cr = threadIdx.x % runs;
  const uint32_t base = r * g.pitch + 9u * cr;     // CONV_SKEW(8 cr)
  double acc[CONV_RUN];
#pragma unroll
  for (int j = 0; j < CONV_RUN; ++j) acc[j] = 0.0;
  __syncthreads();                                 // the operand is staged
  conv_taps_kw<ADJ>(s, base, g, taps, acc);
  __syncthreads();                                 // every lane has read its windows: the tile is free
#pragma unroll
  for (int j = 0; j < CONV_RUN; ++j) s[base + j] = acc[j];
  __syncthreads();
}

// ---- K-fwd --------------------------------------------------------------------------------------------------------------------------------
struct ConvFwdP {
  ConvGeo g;
  int sub_b;            // (the mode is the template parameter: 0 = forward point + prox of the solver state, 1 = a plain operand in x0)
  const double* x0; const double* g0; const double* xacc0;
  double* xhat; double* xp;
  const double* b; double* z;
  const double* diag;   // H * W, or nullptr: all ones
  double tau;
  ProxP px;             // IDENTITY / SHRINK / NONNEG / BOX / LINF / L1BALL (the level at *px.level)
  unsigned seq;
  double* red;          // [gridDim.x][8]: the loss sum, then the seven n-side sums
  unsigned* counter;
  double* out;
  double taps[CONV_MAXK * CONV_MAXK];              // kh * kw, C order
};

template <int MODE>
__global__ __launch_bounds__(FH_WG) void k_conv_fwd(const ConvFwdP p) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) double s_t[CONV_LDS_DOUBLES];
  __shared__ __attribute__((aligned(16))) double s_scr[4 * 8];
  __shared__ __attribute__((aligned(16))) unsigned s_flag[4];
  const uint32_t tid = threadIdx.x;
  const ConvGeo& g = p.g;
  const ConvTile t = conv_tile(g);
  const uint32_t top = g.kh - 1u - g.oh, left = g.kw - 1u - g.ow;       // the halo in front of the tile: x[i - (a - oh)] reaches back kh-1-oh rows
  const uint32_t cols = t.twe + g.kw - 1u, nel = (t.the + g.kh - 1u) * cols;
  const bool modh = g.kh > g.H, modw = g.kw > g.W;
  const double level = (MODE == 0 && (p.px.kind == PX_LINF || p.px.kind == PX_L1BALL)) ? *p.px.level : 0.0;
  double v[8] = {0, 0, 0, 0, 0, 0, 0, 0};        // fsq, dxg0, dx2, xh2, g02, gsum, gmax, rdot
  {
    const uint32_t dq = FH_WG / cols, dr = FH_WG % cols;
    uint32_t lr = tid / cols, lc = tid % cols;
    for (uint32_t lin = tid; lin < nel; lin += FH_WG) {
      const uint32_t h = conv_wrap((int32_t)(t.h0 + lr) - (int32_t)top, g.H, modh);
      const uint32_t w = conv_wrap((int32_t)(t.w0 + lc) - (int32_t)left, g.W, modw);
      const uint32_t gi = h * g.W + w;
      const double x0e = p.x0[gi];
      double y = x0e;
      if (MODE == 0) {
        const double g0e = p.g0[gi];
        const double xhe = fwd_point(x0e, g0e, p.tau);
        y = prox_scalar_rt(p.px.kind, xhe, p.px, level);
        if (lr >= top && lr < top + t.the && lc >= left && lc < left + t.twe) {        // the owner's copy (not a halo copy)
          const double xav = p.xacc0 ? p.xacc0[gi] : 0.0;
          nside_fwd_sums<1>(x0e, g0e, xhe, y, xav, v);
          p.xhat[gi] = xhe;
          p.xp[gi] = y;
        }
      }
      s_t[lr * g.pitch + CONV_SKEW(lc)] = y;
      lc += dr; lr += dq;
      if (lc >= cols) { lc -= cols; ++lr; }
    }
  }
  conv_tile_taps<0>(s_t, g, p.taps);
  for (uint32_t k = tid; k < CONV_TILE_PIX; k += FH_WG) {
    const uint32_t r = k >> g.tw_log2, c = k & (g.tw - 1u);
    if (r < t.the && c < t.twe) {
      const uint32_t zi = (t.h0 + r) * g.W + (t.w0 + c);
      const double y = s_t[r * g.pitch + CONV_SKEW(c)];
      const double d = p.diag ? p.diag[zi] : 1.0;
      const double zv = d == 0.0 ? 0.0 : d * y;
      p.z[zi] = zv;
      v[0] += p.sub_b ? loss_term(zv, p.b[zi], LOSS_LSQ) : zv * zv;
    }
  }
  finish_records<8, S_GMAX>(v, p.red, blockIdx.x, gridDim.x, p.counter, p.out, p.seq, s_scr, s_flag, NoRecords(),
                            [&](double (&w)[8]) { store_fwd_scalars(p.out, w, 0.0); });
}

// ---- K-adj --------------------------------------------------------------------------------------------------------------------------------
struct ConvAdjP {
  ConvGeo g;
  const double* z; const double* zacc0; const double* b;
  const double* diag;
  int sub_b, accel;            // (the mode is the template parameter: 0 = FBS (BB epilogue), 1 = plain gradient (g1 only))
  unsigned seq;
  double coef, tau;
  const double* x0; const double* xp; const double* xacc0; const double* xhat;
  double* x1; double* g1;
  double* red;          // [gridDim.x][8]: dxdg, dg2, xh2, gsum, gmax, fsq
  unsigned* counter;
  double* out;
  double taps[CONV_MAXK * CONV_MAXK];
};

template <int MODE>
__global__ __launch_bounds__(FH_WG) void k_conv_adj(const ConvAdjP p) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) double s_t[CONV_LDS_DOUBLES];
  __shared__ __attribute__((aligned(16))) double s_scr[4 * 8];
  __shared__ __attribute__((aligned(16))) unsigned s_flag[4];
  const uint32_t tid = threadIdx.x;
  const ConvGeo& g = p.g;
  const ConvTile t = conv_tile(g);
  const uint32_t top = g.oh, left = g.ow;                               // (d w)[i + (a - oh)] reaches back oh rows
  const uint32_t cols = t.twe + g.kw - 1u, nel = (t.the + g.kh - 1u) * cols;
  const bool modh = g.kh > g.H, modw = g.kw > g.W;
  double v[6] = {0, 0, 0, 0, 0, 0};            // dxdg, dg2, xh2, gsum, gmax, fsq
  {
    const uint32_t dq = FH_WG / cols, dr = FH_WG % cols;
    uint32_t lr = tid / cols, lc = tid % cols;
    for (uint32_t lin = tid; lin < nel; lin += FH_WG) {
      const uint32_t h = conv_wrap((int32_t)(t.h0 + lr) - (int32_t)top, g.H, modh);
      const uint32_t w = conv_wrap((int32_t)(t.w0 + lc) - (int32_t)left, g.W, modw);
      const uint32_t zi = h * g.W + w;
      double zv = p.z[zi];
      if (p.accel) zv = extrapolate(zv, p.zacc0[zi], p.coef);
      const double bv = p.sub_b ? p.b[zi] : 0.0;
      const double rv = p.sub_b ? loss_grad(zv, bv, LOSS_LSQ) : zv;
      const double d = p.diag ? p.diag[zi] : 1.0;
      s_t[lr * g.pitch + CONV_SKEW(lc)] = d * rv;
      if (lr >= top && lr < top + t.the && lc >= left && lc < left + t.twe)
        v[5] += p.sub_b ? loss_term(zv, bv, LOSS_LSQ) : zv * zv;
      lc += dr; lr += dq;
      if (lc >= cols) { lc -= cols; ++lr; }
    }
  }
  conv_tile_taps<1>(s_t, g, p.taps);
  for (uint32_t k = tid; k < CONV_TILE_PIX; k += FH_WG) {
    const uint32_t r = k >> g.tw_log2, c = k & (g.tw - 1u);
    if (r < t.the && c < t.twe) {
      const uint32_t gi = (t.h0 + r) * g.W + (t.w0 + c);
      const double gv = s_t[r * g.pitch + CONV_SKEW(c)];
      p.g1[gi] = gv;
      if (MODE == 0) {
        const double x1 = nside_adj_sums(gv, p.x0[gi], p.xp[gi], p.accel ? p.xacc0[gi] : 0.0, p.xhat[gi], p.accel, p.coef, p.tau, v);
        if (p.accel) p.x1[gi] = x1;
      }
    }
  }
  finish_records<6, 4>(v, p.red, blockIdx.x, gridDim.x, p.counter, p.out, p.seq, s_scr, s_flag, NoRecords(),
                       [&](double (&w)[6]) { store_adj_scalars(p.out, w); });
}

// ---- the instantiations (ONE table for fh_conv_part.hip, the extern declarations and the dispatch) ----
#define CONV_KERNELS(DO)                                      \
  DO __global__ void k_conv_fwd<0>(const ConvFwdP);           \
  DO __global__ void k_conv_fwd<1>(const ConvFwdP);           \
  DO __global__ void k_conv_adj<0>(const ConvAdjP);           \
  DO __global__ void k_conv_adj<1>(const ConvAdjP);

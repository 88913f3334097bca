// fh_tv3d.h -- kernels for the 3-D periodic difference stencil (fh_set_stencil3d): A = div : (D, H, W, 3) -> (D, H, W), A^H = grad, the N = 3
// case of examples/tv_denoising.py:26-63.  A plain K-fwd + K-adj pair in the mould of fh_sparse.h: one launch per direction, arrive_last
// finalisers, no spin waits, no co-residency assumption, no atomics on floats, every sum in a fixed order: bitwise repeatable.
//
// Layout: n-side vectors are the C order of (D, H, W, 3) -- flat index 3 * p + c, p = (d * H + h) * W + w -- m-side vectors the C order of
// (D, H, W); both in the vector form's padded buffers, whose padding no kernel here writes.  G0 / G1 / XHAT are stored like any other
// operator's (the 2-D path of fh_tv.h recomputes them; this one does not).
//
//   div(Y)[p]    = ((Y[d+1,h,w,0] - Y[p,0]) + (Y[d,h+1,w,1] - Y[p,1])) + (Y[d,h,w+1,2] - Y[p,2])      NumPy's `out += ...` per axis, in this order
//   grad(X)[p,c] = X[p - e_c] - X[p]                                                               indices modulo the dimension
//
// A workgroup owns a tile of TV3_TH x TV3_TW (h, w) positions and marches along d over `planes` planes (Tv3Shape, chosen on the host by ONE
// rule: csrc/fh_host_launch.h:tv3_shape_for).  Everything that touches the n-side walks the FLAT doubles of a tile row -- 3 * tile width
// contiguous doubles, lane k the k-th of them -- so a wave's loads and stores are contiguous whatever the 24-byte voxel does to alignment;
// voxels are put together through LDS.
//
//   k_tv3_fwd<IDENT, NT>  mode 0: xhat = x0 - tau * g0, xprox = prox(xhat), both written, z = div(xprox) written, the loss sum and the seven
//                         n-side sums of the other forms' prologues; mode 1: z = div(x0) of a plain operand.  x0 / g0 are read once: a plane's
//                         tile with its h+1 row and w+1 column (halo voxels RECOMPUTED from x0 / g0, never read back from a stored xprox) goes
//                         through LDS, two planes deep, so the d+1 neighbour is the plane the march computes next.  IDENT = 1: an elementwise
//                         prox (IDENTITY / SHRINK / NONNEG / BOX through prox_scalar) or the plain operand; IDENT = 0: FH_PROX_TVBALL, the
//                         projection of each voxel's 3-vector, nr = sqrt((y0*y0 + y1*y1) + y2*y2), y / fmax(nr, 1) -- la.norm(Y, axis=-1) and
//                         np.maximum.  n-side sums count a voxel in its owner only (not in a halo copy, not in the halo plane).
//   k_tv3_adj<NT>         r = z' - b (z' = z or its FISTA extrapolation; the loss at z' is FH_S_FSQ_ADJ), g1 = grad(r) written, and the
//                         n-side epilogue (fh_nside.h) in the owner's lane (every g1 entry has one owner: no partials); modes 0 and 1.  The r tile with its
//                         h-1 row and w-1 column sits in LDS two planes deep; the march starts one plane early (d0 - 1).
// Wraps are conditional corrections (as tv_wrap_row), flat offsets 64-bit, elementwise arithmetic under fp contract(off).
// NT = 1 (FH_TUNE_NT_LOADS): non-temporal stores of xhat / xprox / g1; measured within 1.4 % of plain stores from 256^3 on
// (profiles/tv3d_sizes.txt), so plain stores are the default.
#pragma once
#include "fh_records.h"

#define TV3_TH 8                                   // tile: rows (h) ...
#define TV3_TW 64                                  // ... and columns (w); TV3_TH * TV3_TW voxels = 2 per lane
#define TV3_SEG (3 * (TV3_TW + 1))                 // doubles of a tile row in LDS: its own voxels and the halo voxel behind them
#define TV3_ROWS (TV3_TH + 1)                      // own rows and the halo row
#define TV3_EPT ((TV3_ROWS * TV3_SEG + FH_WG - 1) / FH_WG)          // flat n-side elements per lane and plane, halo included (7)
#define TV3_VPT (TV3_TH * TV3_TW / FH_WG)                           // own voxels per lane and plane (2)
#define TV3_RS (TV3_TW + 1)                        // K-adj: residuals of a tile row in LDS (the w-1 halo first)
#define TV3_RPT ((TV3_ROWS * TV3_RS + FH_WG - 1) / FH_WG)           // K-adj: residuals per lane and plane, halo included (3)
#define TV3_GPT (TV3_TH * 3 * TV3_TW / FH_WG)                       // K-adj: own g1 elements per lane and plane (6)

template <int NT> __device__ __forceinline__ void tv3_store(double* p, double v) {
  if (NT) __builtin_nontemporal_store(v, p); else *p = v;
}

// where a workgroup works: tile origin, its clipped extent, the planes it owns
struct Tv3Tile { uint32_t w0, h0, d0, twe, the, npl; };
__device__ __forceinline__ Tv3Tile tv3_tile(uint32_t D, uint32_t H, uint32_t W, uint32_t planes, uint32_t tiles_h, uint32_t tiles_w) {
  const uint32_t tw = blockIdx.x % tiles_w, rest = blockIdx.x / tiles_w;
  const uint32_t th = rest % tiles_h, ch = rest / tiles_h;
  Tv3Tile t;
  t.w0 = tw * TV3_TW; t.h0 = th * TV3_TH; t.d0 = ch * planes;
  t.twe = W - t.w0 < TV3_TW ? W - t.w0 : TV3_TW;
  t.the = H - t.h0 < TV3_TH ? H - t.h0 : TV3_TH;
  t.npl = D - t.d0 < planes ? D - t.d0 : planes;
  return t;
}

// ---- K-fwd --------------------------------------------------------------------------------------------------------------------------------
struct Tv3FwdP {
  uint32_t D, H, W, planes, tiles_h, tiles_w;
  int mode;             // 0 = forward point + prox of the solver state, 1 = a plain operand in x0
  int sub_b;
  const double* x0; const double* g0; const double* xacc0;
  double* xhat; double* xp;
  const double* b; double* z;
  double tau;
  ProxP px;             // IDENTITY / SHRINK / NONNEG / BOX (IDENT = 1); unused by the TV-ball instantiation
  unsigned seq;
  double* red;          // [gridDim.x][8]: the loss sum, then the seven n-side sums
  unsigned* counter;
  double* out;
};

template <int IDENT, int NT>
__global__ __launch_bounds__(FH_WG) void k_tv3_fwd(const Tv3FwdP p) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) double s_y[2][TV3_ROWS * TV3_SEG];
  __shared__ __attribute__((aligned(16))) double s_scr[4 * 8];
  __shared__ __attribute__((aligned(16))) unsigned s_flag[4];
  const uint32_t tid = threadIdx.x;
  const Tv3Tile t = tv3_tile(p.D, p.H, p.W, p.planes, p.tiles_h, p.tiles_w);
  const uint32_t seg_own = 3u * t.twe, seg = seg_own + 3u, nelem = (t.the + 1u) * seg;
  const uint32_t wh = t.w0 + t.twe == p.W ? 0u : t.w0 + t.twe;          // the w+1 halo column and the h+1 halo row, wrapped
  const uint32_t hh = t.h0 + t.the == p.H ? 0u : t.h0 + t.the;
  const uint64_t plane_n = 3ull * (uint64_t)p.H * p.W, plane_m = (uint64_t)p.H * p.W;
  // this lane's flat elements of a plane (the same for every plane): LDS offset | component << 16, offset inside the plane, owner bit
  uint32_t e_lds[TV3_EPT], e_off[TV3_EPT], e_valid = 0u, e_own = 0u;
#pragma unroll
  for (int j = 0; j < TV3_EPT; ++j) {
    const uint32_t lin = tid + (uint32_t)j * FH_WG;
    e_lds[j] = 0u; e_off[j] = 0u;
    if (lin < nelem) {
      const uint32_t r = lin / seg, e = lin - r * seg;
      const bool halo_w = e >= seg_own;
      const uint32_t h = r < t.the ? t.h0 + r : hh;
      const uint32_t col = halo_w ? e - seg_own : e;                    // doubles past the first voxel of the run this element lies in
      e_lds[j] = (r * TV3_SEG + e) | ((col % 3u) << 16);
      e_off[j] = 3u * (h * p.W + (halo_w ? wh : t.w0)) + col;           // (3 * H * W < 2^31)
      e_valid |= 1u << j;
      if (r < t.the && !halo_w) e_own |= 1u << j;
    }
  }
  double v[8] = {0, 0, 0, 0, 0, 0, 0, 0};      // fsq, dxg0, dx2, xh2, g02, gsum, gmax, rdot
  // the forward point's outputs and sums of one element, in its owner
  auto account = [&](uint64_t gi, double x0e, double g0e, double xhe, double xpe) {
    const double xav = p.xacc0 ? p.xacc0[gi] : 0.0;
    nside_fwd_sums<1>(x0e, g0e, xhe, xpe, xav, v);
    tv3_store<NT>(p.xhat + gi, xhe);
    tv3_store<NT>(p.xp + gi, xpe);
  };
  for (uint32_t i = 0; i <= t.npl; ++i) {                               // plane npl is the d+1 halo of the last own plane
    const bool own_plane = i < t.npl;
    uint32_t d = t.d0 + i;
    if (d == p.D) d = 0u;
    double* cur = s_y[i & 1u];
    const double* prev = s_y[(i & 1u) ^ 1u];
    const uint64_t base_n = (uint64_t)d * plane_n;
    double x0r[TV3_EPT], g0r[TV3_EPT];
#pragma unroll
    for (int j = 0; j < TV3_EPT; ++j) {
      x0r[j] = 0.0; g0r[j] = 0.0;
      if (e_valid >> j & 1u) {
        const uint64_t gi = base_n + e_off[j];
        const double x0e = p.x0[gi];
        double y = x0e;
        if (p.mode == 0) {
          const double g0e = p.g0[gi];
          y = fwd_point(x0e, g0e, p.tau);
          x0r[j] = x0e; g0r[j] = g0e;
          if (IDENT) {
            const double xhe = y;
            y = prox_scalar_rt(p.px.kind, xhe, p.px, 0.0);
            if (own_plane && (e_own >> j & 1u)) account(gi, x0e, g0e, xhe, y);
          }
        }
        cur[e_lds[j] & 0xFFFFu] = y;
      }
    }
    __syncthreads();
    if (!IDENT && p.mode == 0) {                                        // TV ball: the voxel's three forward points are in LDS now
      double ypr[TV3_EPT];
#pragma unroll
      for (int j = 0; j < TV3_EPT; ++j) {
        ypr[j] = 0.0;
        if (e_valid >> j & 1u) {
          const uint32_t lo = e_lds[j] & 0xFFFFu, vb = lo - (e_lds[j] >> 16);
          const double y0 = cur[vb], y1 = cur[vb + 1u], y2 = cur[vb + 2u];
          const double q0 = y0 * y0, q1 = y1 * y1, q2 = y2 * y2;
          const double nr = sqrt((q0 + q1) + q2);
          const double xhe = cur[lo];
          ypr[j] = xhe / fmax(nr, 1.0);
          if (own_plane && (e_own >> j & 1u)) account(base_n + e_off[j], x0r[j], g0r[j], xhe, ypr[j]);
        }
      }
      __syncthreads();
#pragma unroll
      for (int j = 0; j < TV3_EPT; ++j)
        if (e_valid >> j & 1u) cur[e_lds[j] & 0xFFFFu] = ypr[j];
      __syncthreads();
    }
    if (i >= 1u) {                                                      // z of the plane before: its d+1 neighbour is `cur`
      const uint32_t dz = t.d0 + i - 1u;
#pragma unroll
      for (int j = 0; j < TV3_VPT; ++j) {
        const uint32_t k = tid + (uint32_t)j * FH_WG;
        const uint32_t r = k / TV3_TW, c = k % TV3_TW;
        if (r < t.the && c < t.twe) {
          const uint32_t o = r * TV3_SEG + 3u * c;
          const double a0 = cur[o] - prev[o];
          const double a1 = prev[o + TV3_SEG + 1u] - prev[o + 1u];
          const double a2 = prev[o + 3u + 2u] - prev[o + 2u];
          const double zv = (a0 + a1) + a2;
          const uint64_t zi = (uint64_t)dz * plane_m + (uint64_t)(t.h0 + r) * p.W + (t.w0 + c);
          p.z[zi] = zv;
          v[0] += p.sub_b ? loss_term(zv, p.b[zi], LOSS_LSQ) : zv * zv;
        }
      }
    }
    __syncthreads();                                                    // `prev` is the next plane's target
  }
  finish_records<8, S_GMAX>(v, p.red, blockIdx.x, gridDim.x, p.counter, p.out, p.seq, s_scr, s_flag, NoRecords(),
                            [&](double (&w)[8]) { store_fwd_scalars(p.out, w, 0.0); });
}

// ---- K-adj --------------------------------------------------------------------------------------------------------------------------------
struct Tv3AdjP {
  uint32_t D, H, W, planes, tiles_h, tiles_w;
  const double* z; const double* zacc0; const double* b;
  int sub_b, accel, mode;      // mode 0 = FBS (BB epilogue), 1 = plain gradient (g1 only)
  unsigned seq;
  double coef, tau;
  const double* x0; const double* xp; const double* xacc0; const double* xhat;
  double* x1; double* g1;
  double* red;          // [gridDim.x][8]: dxdg, dg2, xh2, gsum, gmax, fsq
  unsigned* counter;
  double* out;
};

template <int NT>
__global__ __launch_bounds__(FH_WG) void k_tv3_adj(const Tv3AdjP p) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) double s_r[2][TV3_ROWS * TV3_RS];
  __shared__ __attribute__((aligned(16))) double s_scr[4 * 8];
  __shared__ __attribute__((aligned(16))) unsigned s_flag[4];
  const uint32_t tid = threadIdx.x;
  const Tv3Tile t = tv3_tile(p.D, p.H, p.W, p.planes, p.tiles_h, p.tiles_w);
  const uint32_t rs = t.twe + 1u, nres = (t.the + 1u) * rs;
  const uint32_t wl = t.w0 == 0u ? p.W - 1u : t.w0 - 1u;                // the w-1 halo column and the h-1 halo row, wrapped
  const uint32_t hl = t.h0 == 0u ? p.H - 1u : t.h0 - 1u;
  const uint64_t plane_n = 3ull * (uint64_t)p.H * p.W, plane_m = (uint64_t)p.H * p.W;
  // this lane's residuals of a plane (row 0 / column 0 of the LDS tile are the halo) ...
  uint32_t r_lds[TV3_RPT], r_off[TV3_RPT], r_valid = 0u, r_own = 0u;
#pragma unroll
  for (int j = 0; j < TV3_RPT; ++j) {
    const uint32_t lin = tid + (uint32_t)j * FH_WG;
    r_lds[j] = 0u; r_off[j] = 0u;
    if (lin < nres) {
      const uint32_t rr = lin / rs, cc = lin - rr * rs;
      const uint32_t h = rr == 0u ? hl : t.h0 + rr - 1u;
      const uint32_t w = cc == 0u ? wl : t.w0 + cc - 1u;
      r_lds[j] = rr * TV3_RS + cc;
      r_off[j] = h * p.W + w;
      r_valid |= 1u << j;
      if (rr >= 1u && cc >= 1u) r_own |= 1u << j;
    }
  }
  // ... and its own g1 elements: LDS offset of the voxel | component << 16, flat offset inside the plane
  const uint32_t seg = 3u * t.twe, ngel = t.the * seg;
  uint32_t g_lds[TV3_GPT], g_off[TV3_GPT], g_valid = 0u;
#pragma unroll
  for (int j = 0; j < TV3_GPT; ++j) {
    const uint32_t lin = tid + (uint32_t)j * FH_WG;
    g_lds[j] = 0u; g_off[j] = 0u;
    if (lin < ngel) {
      const uint32_t r = lin / seg, e = lin - r * seg;
      g_lds[j] = ((r + 1u) * TV3_RS + e / 3u + 1u) | ((e % 3u) << 16);
      g_off[j] = 3u * ((t.h0 + r) * p.W + t.w0) + e;
      g_valid |= 1u << j;
    }
  }
  double v[6] = {0, 0, 0, 0, 0, 0};            // dxdg, dg2, xh2, gsum, gmax, fsq
  for (uint32_t i = 0; i <= t.npl; ++i) {                               // trip 0 loads the d-1 halo of the first own plane
    const uint32_t d = i == 0u ? (t.d0 == 0u ? p.D - 1u : t.d0 - 1u) : t.d0 + i - 1u;
    double* cur = s_r[i & 1u];
    const double* prev = s_r[(i & 1u) ^ 1u];
    const uint64_t base_m = (uint64_t)d * plane_m;
#pragma unroll
    for (int j = 0; j < TV3_RPT; ++j) {
      if (r_valid >> j & 1u) {
        const uint64_t zi = base_m + r_off[j];
        double zv = p.z[zi];
        if (p.accel) zv = extrapolate(zv, p.zacc0[zi], p.coef);
        const double bv = p.sub_b ? p.b[zi] : 0.0;
        cur[r_lds[j]] = p.sub_b ? loss_grad(zv, bv, LOSS_LSQ) : zv;
        if (i >= 1u && (r_own >> j & 1u)) v[5] += p.sub_b ? loss_term(zv, bv, LOSS_LSQ) : zv * zv;
      }
    }
    __syncthreads();
    if (i >= 1u) {
      const uint64_t base_n = (uint64_t)d * plane_n;
#pragma unroll
      for (int j = 0; j < TV3_GPT; ++j) {
        if (g_valid >> j & 1u) {
          const uint32_t o = g_lds[j] & 0xFFFFu, c = g_lds[j] >> 16;
          const double rp = cur[o];
          const double nb = c == 0u ? prev[o] : (c == 1u ? cur[o - TV3_RS] : cur[o - 1u]);
          const double g = nb - rp;
          const uint64_t gi = base_n + g_off[j];
          tv3_store<NT>(p.g1 + gi, g);
          if (p.mode == 0) {
            const double x1 = nside_adj_sums(g, p.x0[gi], p.xp[gi], p.accel ? p.xacc0[gi] : 0.0, p.xhat[gi], p.accel, p.coef, p.tau, v);
            if (p.accel) p.x1[gi] = x1;
          }
        }
      }
    }
    __syncthreads();                                                    // `prev` is the next plane's target
  }
  finish_records<6, 4>(v, p.red, blockIdx.x, gridDim.x, p.counter, p.out, p.seq, s_scr, s_flag, NoRecords(),
                       [&](double (&w)[6]) { store_adj_scalars(p.out, w); });
}

// ---- the instantiations (ONE table for fh_tv3d_part.hip, the extern declarations and the dispatch) ----
#define TV3_KERNELS(DO)                                          \
  DO __global__ void k_tv3_fwd<0, 0>(const Tv3FwdP);             \
  DO __global__ void k_tv3_fwd<0, 1>(const Tv3FwdP);             \
  DO __global__ void k_tv3_fwd<1, 0>(const Tv3FwdP);             \
  DO __global__ void k_tv3_fwd<1, 1>(const Tv3FwdP);             \
  DO __global__ void k_tv3_adj<0>(const Tv3AdjP);                \
  DO __global__ void k_tv3_adj<1>(const Tv3AdjP);

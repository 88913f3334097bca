// fh_dense.h -- fused dense-matrix FBS kernels for gfx950.
//
// Device layout of A: row-major float64, `mp` rows (m padded with zero rows to a multiple of 16) of
// `ld` doubles (n padded with zero columns to a multiple of 16, plus an optional anti-aliasing pad),
// so every row starts 128-byte aligned and every lane issues 16-byte loads with no tail logic.
// n-side vectors are `ld` long with zero padding; m-side vectors are `mp` long with zero padding.
//
//   K-fwd  (k_fwd_dense):  one launch =  xhat = x0 - tau*g0 ; xprox = prox(xhat) ; z1 = A xprox ;
//                          ||z1-b||^2, <Dx,g0>, ||Dx||^2, ||xprox-xhat||^2, ||g0||^2, g terms, restart dot.
//       Each workgroup owns R whole rows per pass: lanes stride the row in 16-byte pieces
//       (4 KiB contiguous per workgroup per row), recompute the prox'd x chunk on the fly from
//       x0/g0 (1 MiB, L2 resident), keep R accumulators, then wave-__shfl + LDS reduce.
//       Algorithmic HBM bytes: m*n*8 (A) + (2n + m) reads + (2n + m) writes.
//   K-adj  (k_adj_dense):  one launch =  r = z1' - b ; g1 = A^T r ; Dg, <Dx,Dg>, ||Dg||^2 (+ FISTA
//                          extrapolation of x and z).
//       Workgroup (slab, column chunk): lanes own 16-byte column pairs, walk down the slab's rows
//       with per-column register accumulators (coalesced row pieces of the same row-major bytes),
//       r staged in LDS.  Slab partials go to a workspace; the LAST workgroup to finish a column
//       chunk sums the slabs in index order and does the n-side epilogue; the last chunk finaliser
//       sums the scalars.  No float atomics => bitwise repeatable.
//       Algorithmic HBM bytes: m*n*8 (A) + (2m [+m]) + 4n reads + n [+n] writes (+ partials, <0.2 %).
#pragma once
#include "fh_device.h"
#include "fh_records.h"

struct FwdP {
  const double* A;
  uint64_t ld;          // elements per device row
  uint32_t ld2;         // 16-byte pieces per device row (ld / 2 for float64 storage, ld / 4 for float32 storage)
  uint32_t nv2;         // double pairs per n-side vector (= ld / 2)
  uint32_t n;           // logical columns
  uint32_t m;           // logical rows (padding rows carry no loss term)
  uint32_t nrg;         // row groups = mp / R
  uint32_t nchunks;     // ceil(nv2 / 256)
  const double* x0; const double* g0; const double* xacc0;
  double* xhat; double* xp;
  const double* b; double* z;
  double tau;
  int sub_b;            // residual r = z - b (1) or r = z (0, fh_apply)
  int loss;             // LOSS_LSQ / LOSS_LOGISTIC
  ProxP px;
  double* red_n;        // [nchunks][8]
  double* red_m;        // [gridDim.x]
  unsigned* counter;
  double* out;          // device scalar block (FH_S_* layout)
};

// xprox pair for 16-byte piece c.  KIND = PX_PLAIN: xprox := x0 (fh_init / fh_apply / Lipschitz probes).
template <int KIND>
__device__ __forceinline__ d2 xprox_pair(const FwdP& p, uint32_t c, double level) {
  d2 xv = reinterpret_cast<const d2*>(p.x0)[c];
  if (KIND != PX_PLAIN) {
    const d2 gv = reinterpret_cast<const d2*>(p.g0)[c];
    xv.x = prox_scalar<KIND>(fwd_point(xv.x, gv.x, p.tau), p.px, level);
    xv.y = prox_scalar<KIND>(fwd_point(xv.y, gv.y, p.tau), p.px, level);
  }
  return xv;
}

// (k_fwd_dense keeps its own text of the n-side sums and of the finaliser: routed through fh_nside.h / fh_records.h it computes the same values but is not
// byte-identical to its measured form -- instruction order and register numbers move -- and this kernel is held to byte identity,
// profiles/nside_refactor.txt section 2.  The same goes for k_diff_sq below.)
template <int R, int NT, int KIND, int F32 = 0>
__global__ __launch_bounds__(FH_WG) void k_fwd_dense(const FwdP p) {
  typedef typename PieceOf<F32>::type PT;
  constexpr int XD = xd2<F32>();
  __shared__ __attribute__((aligned(16))) double s_scr[4 * 16];
  __shared__ __attribute__((aligned(16))) unsigned s_flag[4];
  const uint32_t tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const double level = (KIND == PX_LINF || KIND == PX_L1BALL) ? *p.px.level : 0.0;

  // ---------------- n-side: forward point, prox, line-search reductions (once per column) --------
  if (KIND != PX_PLAIN) {
    for (uint32_t chunk = blockIdx.x; chunk < p.nchunks; chunk += gridDim.x) {
      const uint32_t c = chunk * FH_WG + tid;
      double v[7] = {0, 0, 0, 0, 0, 0, 0};   // dxg0, dx2, xh2, g02, gsum, gmax, rdot
      if (c < p.nv2) {
        const d2 x0v = reinterpret_cast<const d2*>(p.x0)[c];
        const d2 g0v = reinterpret_cast<const d2*>(p.g0)[c];
        d2 xav = {0.0, 0.0};
        if (p.xacc0) xav = reinterpret_cast<const d2*>(p.xacc0)[c];
        d2 xh, xp;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          const bool valid = (2u * c + e) < p.n;
          const double x0e = x0v[e], g0e = g0v[e];
          double xhe = fwd_point(x0e, g0e, p.tau);
          double xpe = prox_scalar<KIND>(xhe, p.px, level);
          if (!valid) { xhe = 0.0; xpe = 0.0; }
          xh[e] = xhe; xp[e] = xpe;
          if (valid) {
            const double dx = sub_nofma(xpe, x0e);
            const double dh = sub_nofma(xpe, xhe);
            v[0] = fma(dx, g0e, v[0]);
            v[1] = fma(dx, dx, v[1]);
            v[2] = fma(dh, dh, v[2]);
            v[3] = fma(g0e, g0e, v[3]);
            v[4] += fabs(xpe);
            v[5] = fmax(v[5], fabs(xpe));
            v[6] = fma(sub_nofma(x0e, xpe), sub_nofma(xpe, xav[e]), v[6]);
          }
        }
        reinterpret_cast<d2*>(p.xhat)[c] = xh;
        reinterpret_cast<d2*>(p.xp)[c] = xp;
      }
      block_reduce<7>(v, s_scr, 5);
      if (tid == 0) {
#pragma unroll
        for (int k = 0; k < 7; ++k) store_partial(p.red_n + (uint64_t)chunk * 8 + 1 + k, v[k]);
      }
    }
  }

  // ---------------- m-side: z1 = A xprox for R rows per pass ----------------------------------
  // Two 16-byte pieces per lane per trip: the 2R row loads are issued first, the (L2-resident)
  // x0/g0 loads and the prox recompute overlap their latency.
  double fpart = 0.0;
  const uint32_t ntrip = (p.ld2 + 2 * FH_WG - 1) / (2 * FH_WG);
  for (uint32_t rg = blockIdx.x; rg < p.nrg; rg += gridDim.x) {
    const PT* Ab = reinterpret_cast<const PT*>(p.A) + (uint64_t)rg * R * p.ld2;
    double acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = 0.0;
    for (uint32_t t = 0; t < ntrip; ++t) {
      const uint32_t c0 = t * (2 * FH_WG) + tid;          // always < ld2 except possibly in the last trip
      const uint32_t c1 = c0 + FH_WG;
      const bool ok0 = c0 < p.ld2, ok1 = c1 < p.ld2;
      const uint32_t k0 = ok0 ? c0 : 0u, k1 = ok1 ? c1 : 0u;   // clamp: in-bounds redundant loads
      PT a0[R], a1[R];
#pragma unroll
      for (int r = 0; r < R; ++r) a0[r] = load_stream<NT>(Ab + (uint64_t)r * p.ld2 + k0);
#pragma unroll
      for (int r = 0; r < R; ++r) a1[r] = load_stream<NT>(Ab + (uint64_t)r * p.ld2 + k1);
      d2 x0v[XD], x1v[XD];
#pragma unroll
      for (int e = 0; e < XD; ++e) {
        x0v[e] = xprox_pair<KIND>(p, k0 * XD + e, level);
        x1v[e] = xprox_pair<KIND>(p, k1 * XD + e, level);
        if (!ok0) x0v[e] = (d2){0.0, 0.0};
        if (!ok1) x1v[e] = (d2){0.0, 0.0};
      }
#pragma unroll
      for (int r = 0; r < R; ++r) acc[r] = piece_dot(a0[r], x0v, acc[r]);
#pragma unroll
      for (int r = 0; r < R; ++r) acc[r] = piece_dot(a1[r], x1v, acc[r]);
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      acc[r] = wave_sum(acc[r]);
      if (lane == 0) s_scr[wave * 16 + r] = acc[r];
    }
    __syncthreads();
    if (tid < R) {
      const double zv = ((s_scr[tid] + s_scr[16 + tid]) + s_scr[32 + tid]) + s_scr[48 + tid];
      const uint32_t row = rg * R + tid;
      p.z[row] = zv;
      if (row < p.m) fpart += p.sub_b ? loss_term(zv, p.b[row], p.loss) : zv * zv;
    }
    __syncthreads();
  }
  {
    double v[1] = {fpart};
    block_reduce<1>(v, s_scr, -1);
    if (tid == 0) store_partial(p.red_m + blockIdx.x, v[0]);
  }

  // ---------------- last workgroup: ordered final sums ------------------------------------------
  if (arrive_last(p.counter, gridDim.x, s_flag)) {
    double v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (uint32_t i = tid; i < gridDim.x; i += FH_WG) v[0] += load_partial(p.red_m + i);
    if (KIND != PX_PLAIN) {
      for (uint32_t i = tid; i < p.nchunks; i += FH_WG) {
#pragma unroll
        for (int k = 1; k < 8; ++k) {
          const double t = load_partial(p.red_n + (uint64_t)i * 8 + k);
          if (k == S_GMAX) v[k] = fmax(v[k], t); else v[k] += t;
        }
      }
    }
    block_reduce<8>(v, s_scr, S_GMAX);
    if (tid == 0) {
#pragma unroll
      for (int k = 0; k < 8; ++k) scal_store(p.out + k, v[k]);
      scal_store(p.out + S_ALPHA, level);
      publish_seq(p.out, p.px.seq);
      __hip_atomic_store(p.counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// ------------------------------------------------------------------------------------------------
struct AdjP {
  const double* A;
  uint64_t ld;
  uint32_t ld2;         // 16-byte pieces per device row
  uint32_t nv2;         // double pairs per n-side vector
  uint32_t n;
  uint32_t mp;          // padded rows
  uint32_t m;           // logical rows
  uint32_t slab_rows;   // rows per slab (multiple of 8, <= ADJ_MAX_SLAB)
  uint32_t nslab, ncc;
  uint32_t cyclic;      // != 0: slab s takes rows s, s + nslab, s + 2 nslab, ... (all slabs stream ONE window of the matrix); 0: rows [s * slab_rows, + slab_rows)
  const double* z; const double* zacc0; const double* b;
  int sub_b;            // r = grad f(z) (z - b for least squares), else r = z
  int loss;             // LOSS_LSQ / LOSS_LOGISTIC
  int accel;            // extrapolate z and x with `coef`
  double coef;
  int mode;             // 0 = FBS (BB epilogue), 1 = plain gradient (g1 only), 2 = sharded (g1 partial + local fsq only)
  unsigned seq;         // (in the struct's padding) != 0: published behind the scalar block by the finaliser (fh_device.h:publish_seq)
  double tau;
  const double* x0; const double* xp; const double* xacc0; const double* xhat;
  double* x1;           // extrapolated iterate (accel only; else == xp and not written)
  double* g1;
  double* gpart;        // [nslab][ld]
  double* red_bb;       // [ncc][8]
  double* red_f;        // [nslab]
  unsigned* cc_counter; // [ncc]
  unsigned* fin_counter;
  double* out;
};

#define ADJ_MAX_SLAB 2048

// n-side epilogue for one element (nside_adj_sums); a padding element has no share in the sums and its x1 is zero.
// v: dxdg, dg2, xh2, gsum, gmax
__device__ __forceinline__ double bb_element(const AdjP& p, double g1, double x0, double xp, double xacc0,
                                             double xhat, bool valid, double (&v)[5]) {
  return valid ? nside_adj_sums(g1, x0, xp, xacc0, xhat, p.accel, p.coef, p.tau, v) : 0.0;
}

template <int CPT, int NT, int F32 = 0>
__global__ __launch_bounds__(FH_WG) void k_adj_dense(const AdjP p) {
  typedef typename PieceOf<F32>::type PT;
  constexpr int XD = xd2<F32>();
  __shared__ __attribute__((aligned(16))) double s_r[ADJ_MAX_SLAB];
  __shared__ __attribute__((aligned(16))) double s_scr[4 * 8];
  __shared__ __attribute__((aligned(16))) unsigned s_flag[4];
  const uint32_t tid = threadIdx.x;
  const uint32_t cc = blockIdx.x % p.ncc, slab = blockIdx.x / p.ncc;
  // rows of this slab: a contiguous block (default), or dealt cyclically over the slabs (FH_TUNE_ADJ_CYCLIC; what the one-pass kernel does by default since
  // round 6 -- here measured mixed: profiles/r06_placement.txt)
  const uint32_t row0 = p.cyclic ? slab : slab * p.slab_rows;
  const uint32_t rstep = p.cyclic ? p.nslab : 1u;
  const uint32_t rows = p.cyclic ? (slab < p.mp ? (p.mp - slab + p.nslab - 1u) / p.nslab : 0u) : min(p.slab_rows, p.mp - row0);

  // ---- stage the slab's residual r = z1' - b in LDS (z1' = extrapolated z when accelerating) ----
  double fs = 0.0;
  for (uint32_t i = tid; i < rows; i += FH_WG) {
    const uint32_t gr = row0 + i * rstep;
    double zv = p.z[gr];
    if (p.accel) zv = extrapolate(zv, p.zacc0[gr], p.coef);
    const double rv = p.sub_b ? loss_grad(zv, p.b[gr], p.loss) : zv;
    s_r[i] = rv;
    if (gr < p.m) fs += p.sub_b ? loss_term(zv, p.b[gr], p.loss) : zv * zv;
  }
  __syncthreads();

  // ---- stream the slab: per-column accumulators, rows walked top to bottom ------------------------
  uint32_t col[CPT];
  d2 acc[CPT][XD];
#pragma unroll
  for (int j = 0; j < CPT; ++j) {
    col[j] = min(cc * (FH_WG * CPT) + j * FH_WG + tid, p.ld2 - 1u);   // clamp: redundant but in-bounds
#pragma unroll
    for (int e = 0; e < XD; ++e) acc[j][e] = (d2){0.0, 0.0};
  }
  const PT* Ab = reinterpret_cast<const PT*>(p.A) + (uint64_t)row0 * p.ld2;
  const uint64_t astep = (uint64_t)rstep * p.ld2;
#pragma unroll 4
  for (uint32_t i = 0; i < rows; ++i) {
    const double rv = s_r[i];
#pragma unroll
    for (int j = 0; j < CPT; ++j) piece_axpy(load_stream<NT>(Ab + col[j]), rv, acc[j]);
    Ab += astep;
  }
#pragma unroll
  for (int j = 0; j < CPT; ++j) {
    const uint32_t c = cc * (FH_WG * CPT) + j * FH_WG + tid;
    if (c < p.ld2) {
#pragma unroll
      for (int e = 0; e < XD; ++e) store_partial16(reinterpret_cast<d2*>(p.gpart) + (uint64_t)slab * p.nv2, c * XD + e, acc[j][e]);
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

  double v[5] = {0, 0, 0, 0, 0};
#pragma unroll
  for (int j = 0; j < CPT * XD; ++j) {
    const uint32_t piece = cc * (FH_WG * CPT) + (j / XD) * FH_WG + tid;
    if (piece >= p.ld2) continue;
    const uint32_t c = piece * XD + (j % XD);                      // double-pair index into the n-side vectors
    d2 g = {0.0, 0.0};
#pragma unroll 16
    for (uint32_t s = 0; s < p.nslab; ++s) g += load_partial16(reinterpret_cast<const d2*>(p.gpart), s * p.nv2 + c);
    reinterpret_cast<d2*>(p.g1)[c] = g;
    if (p.mode == 0) {
      const d2 x0v = reinterpret_cast<const d2*>(p.x0)[c];
      const d2 xpv = reinterpret_cast<const d2*>(p.xp)[c];
      const d2 xhv = reinterpret_cast<const d2*>(p.xhat)[c];
      d2 xav = {0.0, 0.0};
      if (p.accel) xav = reinterpret_cast<const d2*>(p.xacc0)[c];
      d2 x1v;
      x1v.x = bb_element(p, g.x, x0v.x, xpv.x, xav.x, xhv.x, 2u * c < p.n, v);
      x1v.y = bb_element(p, g.y, x0v.y, xpv.y, xav.y, xhv.y, 2u * c + 1u < p.n, v);
      if (p.accel) reinterpret_cast<d2*>(p.x1)[c] = x1v;
    }
  }
  // ---- one record per column chunk; the last chunk finaliser: ordered scalar sums -------------------
  finish_records<5, 4, 6>(v, p.red_bb, cc, p.ncc, p.fin_counter, p.out, p.seq, s_scr, s_flag,
                          [&](double (&w)[6]) { add_column(w[5], p.red_f, p.nslab); },      // fsq: one loss sum per slab
                          [&](double (&w)[6]) { store_adj_scalars(p.out, w); });
}

// n-side epilogue as its own launch: used after the RCCL all-reduce when A is row-sharded
// (g1 already holds the global sum).  grid = nchunks workgroups of 256 column pairs.
// `pack` (optional): the 3 doubles a one-pass launch appended to g1 and the all-reduce summed over the ranks (loss sum, timeout
// word, loss sum at the extrapolated point).  `mirror` (optional): host-mapped copy of the complete scalar block, written by the
// finalising thread so that the caller needs no further launch to see it.
static __global__ __launch_bounds__(FH_WG) void k_bb_epilogue(const AdjP p_in, uint32_t nchunks, const double* fsq_src, const double* coef_src,
                                                       const double* pack, double* mirror) {
  AdjP p = p_in;
  if (coef_src) p.coef = *coef_src;      // FISTA coefficient decided on the device by the one-pass kernel (restart rule)
  __shared__ __attribute__((aligned(16))) double s_scr[4 * 8];
  __shared__ __attribute__((aligned(16))) unsigned s_flag[4];
  const uint32_t tid = threadIdx.x;
  const uint32_t c = blockIdx.x * FH_WG + tid;
  double v[5] = {0, 0, 0, 0, 0};
  if (c < p.ld2) {
    const d2 g = reinterpret_cast<const d2*>(p.g1)[c];
    const d2 x0v = reinterpret_cast<const d2*>(p.x0)[c];
    const d2 xpv = reinterpret_cast<const d2*>(p.xp)[c];
    const d2 xhv = reinterpret_cast<const d2*>(p.xhat)[c];
    d2 xav = {0.0, 0.0};
    if (p.accel) xav = reinterpret_cast<const d2*>(p.xacc0)[c];
    d2 x1v;
    x1v.x = bb_element(p, g.x, x0v.x, xpv.x, xav.x, xhv.x, 2u * c < p.n, v);
    x1v.y = bb_element(p, g.y, x0v.y, xpv.y, xav.y, xhv.y, 2u * c + 1u < p.n, v);
    if (p.accel) reinterpret_cast<d2*>(p.x1)[c] = x1v;
  }
  // (seq = 0: the caller learns of the block from the end of the launch, no sequence number)
  finish_records<5, 4>(v, p.red_bb, blockIdx.x, nchunks, p.fin_counter, p.out, 0u, s_scr, s_flag, NoRecords(), [&](double (&w)[5]) {
    p.out[S_DXDG] = w[0]; p.out[S_DG2] = w[1]; p.out[S_XH2_ADJ] = w[2];
    p.out[S_GSUM_ADJ] = w[3]; p.out[S_GMAX_ADJ] = w[4];
    p.out[S_FSQ_ADJ] = *fsq_src;
    if (pack) { p.out[S_FSQ] = pack[0]; p.out[15] = pack[1]; }
    if (mirror) {
#pragma unroll
      for (int k = 0; k < 16; ++k) mirror[k] = p.out[k];
    }
  });
}

// ---- utility kernels (non-template kernels are `static`: this header is included by several translation units) ------------
template <int F32>
__global__ __launch_bounds__(FH_WG) void k_gen_matrix(double* A, uint32_t ld2, uint32_t m, uint32_t mp,
                                                      uint32_t n, uint64_t row0, uint64_t key, double coef) {
  typedef typename PieceOf<F32>::type PT;
  constexpr uint32_t E = F32 ? 4u : 2u;                         // columns per 16-byte piece
  const uint64_t total = (uint64_t)mp * ld2;
  for (uint64_t t = (uint64_t)blockIdx.x * FH_WG + threadIdx.x; t < total; t += (uint64_t)gridDim.x * FH_WG) {
    const uint32_t row = (uint32_t)(t / ld2), c = (uint32_t)(t % ld2);
    double e[4] = {0.0, 0.0, 0.0, 0.0};
    if (row < m) {
      const uint64_t base = (row0 + row) * (uint64_t)n;
#pragma unroll
      for (uint32_t k = 0; k < E; ++k)
        if (E * c + k < n) e[k] = fh_ihall(key, base + E * c + k, coef);
    }
    PT v;
    if constexpr (F32) { v.x = (float)e[0]; v.y = (float)e[1]; v.z = (float)e[2]; v.w = (float)e[3]; }   // round to nearest even, as ndarray.astype(float32)
    else { v.x = e[0]; v.y = e[1]; }
    reinterpret_cast<PT*>(A)[t] = v;
  }
}

// float64 rows <-> float32 storage (fh_set_matrix / fh_get_matrix_rows in float32-storage mode), `rows` x `n` elements
static __global__ __launch_bounds__(FH_WG) void k_rows_to_f32(const double* src, uint64_t src_ld, float* dst, uint64_t dst_ld, uint32_t rows, uint32_t n) {
  for (uint64_t t = (uint64_t)blockIdx.x * FH_WG + threadIdx.x; t < (uint64_t)rows * n; t += (uint64_t)gridDim.x * FH_WG) {
    const uint64_t r = t / n, c = t % n;
    dst[r * dst_ld + c] = (float)src[r * src_ld + c];
  }
}
static __global__ __launch_bounds__(FH_WG) void k_rows_from_f32(const float* src, uint64_t src_ld, double* dst, uint64_t dst_ld, uint32_t rows, uint32_t n) {
  for (uint64_t t = (uint64_t)blockIdx.x * FH_WG + threadIdx.x; t < (uint64_t)rows * n; t += (uint64_t)gridDim.x * FH_WG) {
    const uint64_t r = t / n, c = t % n;
    dst[r * dst_ld + c] = (double)src[r * src_ld + c];
  }
}

// sum of (a-b)^2 over len elements -> out[0]; single-workgroup-final pattern
static __global__ __launch_bounds__(FH_WG) void k_diff_sq(const double* a, const double* b, uint32_t len, double* red,
                                                   unsigned* counter, double* out) {
  __shared__ __attribute__((aligned(16))) double s_scr[4];
  __shared__ __attribute__((aligned(16))) unsigned s_flag[4];
  double v[1] = {0.0};
  for (uint32_t i = blockIdx.x * FH_WG + threadIdx.x; i < len; i += gridDim.x * FH_WG) {
    const double d = sub_nofma(a[i], b[i]);
    v[0] = fma(d, d, v[0]);
  }
  block_reduce<1>(v, s_scr, -1);
  if (threadIdx.x == 0) store_partial(red + blockIdx.x, v[0]);
  if (!arrive_last(counter, gridDim.x, s_flag)) return;
  double w[1] = {0.0};
  for (uint32_t i = threadIdx.x; i < gridDim.x; i += FH_WG) w[0] += load_partial(red + i);
  block_reduce<1>(w, s_scr, -1);
  if (threadIdx.x == 0) {
    out[0] = w[0];
    __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// sum|x| and max|x| over len elements -> out[S_GSUM], out[S_GMAX]
static __global__ __launch_bounds__(FH_WG) void k_gterms(const double* x, uint32_t len, double* red, unsigned* counter, double* out) {
  __shared__ __attribute__((aligned(16))) double s_scr[8];
  __shared__ __attribute__((aligned(16))) unsigned s_flag[4];
  double v[2] = {0.0, 0.0};
  for (uint32_t i = blockIdx.x * FH_WG + threadIdx.x; i < len; i += gridDim.x * FH_WG) {
    const double a = fabs(x[i]);
    v[0] += a;
    v[1] = fmax(v[1], a);
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

// Read-only streaming pass over A, the "achievable ceiling" printed next to the 8 TB/s spec peak.  Shaped like the
// product's fastest stream (the one-pass kernel) so that it bounds the product: persistent workgroups (1-2 per CU), every
// lane keeps THREE rotating register buffers of U non-temporal 16-byte loads (U = 16: 128-192 KiB in flight per workgroup), the
// next tile's loads are issued before the current tile is consumed, branch-free clamped addressing so the compiler keeps
// counted `vmcnt` waits, and nothing but one add per element.  (Round 1's probe -- plain loads from 8192 transient
// workgroups -- and a K-fwd-shaped loop that drains `vmcnt(0)` every trip both topped out BELOW the product kernels.)
template <int U, int NT>
__global__ __launch_bounds__(FH_WG) void k_stream_probe(const double* A, uint64_t npieces, double* sink) {
  const d2* p = reinterpret_cast<const d2*>(A);
  const uint64_t tile = (uint64_t)U * FH_WG;                       // 16-byte pieces per workgroup per trip
  const uint64_t ntiles = (npieces + tile - 1) / tile;
  const uint64_t last = npieces - 1;
  d2 b0[U], b1[U], b2[U];
  double acc = 0.0, acc2 = 0.0;
  // (the empty asm statements pin the issue order: without them hipcc sinks each load to just behind the add that frees
  // its register and ends every trip on `vmcnt(0)`, i.e. with nothing in flight)
  auto load = [&](d2 (&buf)[U], uint64_t t) {                       // tiles past the end re-read the last one (clamped)
    const uint64_t base = (t < ntiles ? t : ntiles - 1) * tile + threadIdx.x;
#pragma unroll
    for (int j = 0; j < U; ++j) { const uint64_t i = base + (uint64_t)j * FH_WG; buf[j] = load_stream<NT>(p + (i < last ? i : last)); }
    asm volatile("" ::: "memory");
  };
  auto eat = [&](const d2 (&buf)[U]) {
#pragma unroll
    for (int j = 0; j < U; ++j) { acc += buf[j].x; acc2 += buf[j].y; }   // serial chains: the adds cannot be hoisted above the loads of later tiles
    asm volatile("" ::: "memory");
  };
  const uint64_t g = gridDim.x;
  uint64_t t = blockIdx.x;
  load(b0, t);
  load(b1, t + g);
  for (; t < ntiles; t += 3ull * g) {          // two tiles (2*U loads per lane) stay in flight behind the one being consumed
    load(b2, t + 2ull * g); eat(b0);
    load(b0, t + 3ull * g); eat(b1);
    load(b1, t + 4ull * g); eat(b2);
  }
  if (acc + acc2 == 1.2345e300) sink[0] = acc;   // never true; keeps the loads alive
}

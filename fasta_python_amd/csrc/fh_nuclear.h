// fh_nuclear.h -- the IDENTITY operator with an elementwise loss (fh_set_identity) and the prox of the nuclear norm (FH_PROX_NUCLEAR):
// examples/logistic_matrix_completion.py, min_X mu ||X||_* + sum log(1 + e^X) - (B == 1) X with fasta(None, None, f, gradf, g, proxg, X0).
//
// The unknown is an (M, N) matrix kept in the VECTOR form's buffers, length M * N in C order; m = n = M * N, z = x, FH_VEC_B holds B.
//
//   k_id_fwd       K-fwd, elementwise: xhat = x0 - tau*g0, xprox = prox(xhat) for the kinds IDENTITY / SHRINK / NONNEG / BOX (the same device
//                  functions, FMA contraction off, as every vector kernel: bit-exact outputs) -- or, for FH_PROX_NUCLEAR, xhat and xprox as the
//                  thresholding below left them --, z1 = xprox, the loss sum and the seven n-side sums.  Mode 1: z = x0 and the loss sum alone.
//   k_id_adj       K-adj, elementwise: x1 = xprox + coef*(xprox - x_accel0), g1 = loss_grad(x1), the loss at x1 and the n-side epilogue
//                  (its own text of nside_adj_sums, see below).  Mode 1: g1 = loss_grad(z) (or z itself, fh_apply).
//   Both are grid-stride launches, a lane's elements in index order, workgroup records summed in index order by the last workgroup to arrive:
//   no float atomics, bitwise repeatable.
//   OBSERVATION WEIGHTS (fh_set_loss_weights): f(X) = sum_j w_j loss(x_j, b_j).  Both kernels are templates on WEIGHTED; the weighted form takes
//   the unweighted argument block followed by the pointer to w (IdFwdWP / IdAdjWP), so the unweighted instantiation is the code it always was.
//   A term is w == 0 ? 0 : w * loss_term, a gradient entry w == 0 ? 0 : w * loss_grad: the SELECT keeps an unobserved entry at exactly 0.0
//   whatever x is (log(1 + exp(800)) is inf, and 0 * inf is NaN); w == 1 gives the unweighted bits.
//
// FH_PROX_NUCLEAR: singular-value thresholding by BLOCK ONE-SIDED JACOBI (Hestenes).  With p = min(M, N), q = max(M, N): the working buffer
// holds P rows (p padded with zero rows to a multiple of the block size Bk) of ld doubles, [ W | J^T ]: W = xhat, transposed when M > N, in
// q columns padded to an even count, then a P x P block that starts as the identity -- every rotation of rows is applied to both alike, so at
// the end the rows of W are mutually orthogonal (w_i = sigma_i v_i^T) and xhat = J W.  No Gram matrix of the whole xhat, no LAPACK.
//
//   k_nuc_load     xhat (from x0, g0, tau, or a plain operand) into W, the identity into J^T, ||xhat||_F^2 by a fixed-order reduction.
//   k_nuc_step<BK> ONE STEP of a sweep, an ordinary launch: workgroup k owns pair k of a round-robin tournament over the nb = P / Bk blocks
//                  (nuc_pair below; an odd nb gives one block a bye, nb = 1 a single self-pair), 2 Bk rows nobody else touches in this step.
//                    1. the rows stream through LDS in chunks of NUC_CC columns; a lane owns one entry of their 2Bk x 2Bk Gram matrix G (for
//                       Bk < 8 several lanes share an entry, each a fixed residue class of the column pairs, combined in lane order);
//                    2. wave 0 diagonalises G in LDS by cyclic Jacobi, accumulating the rotations in V (nuc_diagonalise: the rules are there);
//                    3. if anything rotated, all waves write V^T rows back, a lane per 16-byte column pair, and the step's rotation count is
//                       added to this sweep's INTEGER counter.  A workgroup that rotated nothing writes nothing.
//   k_nuc_sigma    sigma_i = ||w_i||, phi_i = max(sigma_i - thr, 0) / (sigma_i + (sigma_i == 0)), and the sum and the largest of the kept values
//                  max(sigma_i - thr, 0) and #{sigma_i > thr}, in index order: the nuclear norm of xprox (FH_S_GSUM), its spectral norm
//                  (FH_S_GMAX) and the rank kept (FH_S_ALPHA) come for free.
//   k_nuc_recon    xprox = J diag(phi) W, plain FMA in index order, rows with phi_i = 0 skipped; written back transposed when M > N.
//
// FH_PROX_NUCBALL: the Euclidean projection onto { ||X||_* <= radius }, the same decomposition with another map of the singular values:
//   k_nuc_ball     ONE workgroup, behind k_nuc_sigma at thr = 0 (whose per-row records hold sigma_i): the sigma are ordered descending by
//                  counting (rank_i = #{j : sigma_j > sigma_i, or equal and j < i}: deterministic, no padding), ONE lane forms the running
//                  sums c_k in that order (np.cumsum's order), alpha = max_k (c_k - radius) / k over the lanes (max is exact in any order),
//                  theta = max(alpha, 0): proximal.project_L1_ball of the singular values.  Then phi_i = max(sigma_i - theta, 0) /
//                  (sigma_i + (sigma_i == 0)) and the three scalars exactly as k_nuc_sigma forms them at thr = theta.
//
// A SWEEP is all steps of the schedule; the host reads the sweep's counter once (csrc/fh_host_launch.h: nuc_decompose) and stops after the first
// sweep that rotated nothing.  No spin wait, no grid barrier, no persistent launch: steps are dependent launches on the context's stream.
#pragma once
#include <type_traits>
#include "fh_dense.h"

#define PX_NUCLEAR 10
#define NUC_CC 256                 // columns of a chunk of the Gram pass
#define NUC_LDT (NUC_CC + 2)       // doubles per row of the LDS tile: 16 bytes of padding, 2Bk rows on distinct banks for 16-byte reads
#define NUC_MAX_SWEEPS 30          // outer sweeps of a decomposition and inner sweeps of a step alike
#define NUC_MAX_P 1024
// FH_TUNE_NUC_BLOCK_ROWS = 0: the pairwise rotation.  Measured (profiles/nuclear_sizes.txt): with this step kernel, whose diagonalisation is the work of ONE wave,
// blocks of 8 rows take 2.6 - 5.7 times as long per prox as blocks of 1 at every shape measured; blocks pay once that phase is spread over the workgroup.
#define NUC_AUTO_BLOCK_ROWS 1u
#define NUC_EPS 2.220446049250313e-16

// ---- the identity operator -------------------------------------------------------------------------------------------------------------------
struct IdFwdP {
  uint64_t n;
  int mode;             // 0 = FBS forward step, 1 = plain operand (z = x0)
  int given;            // mode 0: xhat and xp hold the thresholding's results (FH_PROX_NUCLEAR)
  int sub_b, loss;
  const double* x0; const double* g0; const double* xacc0;
  double* xhat; double* xp; double* z;
  const double* b;
  double tau;
  ProxP px;             // IDENTITY / SHRINK / NONNEG / BOX
  const double* nuc;    // given: [0] the nuclear norm of xprox, [1] the rank kept, [2] its largest singular value
  unsigned seq;
  double* red;          // [gridDim.x][8]
  unsigned* counter;
  double* out;
};

struct IdFwdWP { IdFwdP p; const double* w; };      // the weighted form's argument block: the unweighted one, then the weights (length n)
__device__ __forceinline__ const IdFwdP& id_args(const IdFwdP& a) { return a; }
__device__ __forceinline__ const IdFwdP& id_args(const IdFwdWP& a) { return a.p; }
__device__ __forceinline__ const double* id_weights(const IdFwdP&) { return nullptr; }
__device__ __forceinline__ const double* id_weights(const IdFwdWP& a) { return a.w; }
// w == 0 ? 0 : w * t -- the select, not the product: an unobserved entry contributes exactly 0.0 even where t is inf
__device__ __forceinline__ double id_weighted(double w, double t) {
#pragma clang fp contract(off)
  return w == 0.0 ? 0.0 : w * t;
}

template <bool WEIGHTED>
static __global__ __launch_bounds__(FH_WG) void k_id_fwd(const typename std::conditional<WEIGHTED, IdFwdWP, IdFwdP>::type args) {
#pragma clang fp contract(off)
  const IdFwdP& p = id_args(args);
  const double* wt = id_weights(args);
  __shared__ __attribute__((aligned(16))) double s_scr[4 * 8];
  __shared__ __attribute__((aligned(16))) unsigned s_flag[4];
  const uint32_t tid = threadIdx.x;
  double v[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // fsq, dxg0, dx2, xh2, g02, gsum, gmax, rdot
  for (uint64_t j = (uint64_t)blockIdx.x * FH_WG + tid; j < p.n; j += (uint64_t)gridDim.x * FH_WG) {
    if (p.mode != 0) {
      const double zv = p.x0[j];
      p.z[j] = zv;
      if (WEIGHTED) v[0] += p.sub_b ? id_weighted(wt[j], loss_term(zv, p.b[j], p.loss)) : zv * zv;
      else v[0] += p.sub_b ? loss_term(zv, p.b[j], p.loss) : zv * zv;
      continue;
    }
    const double x0e = p.x0[j], g0e = p.g0[j];
    const double xav = p.xacc0 ? p.xacc0[j] : 0.0;
    double xhe, xpe;
    if (p.given) { xhe = p.xhat[j]; xpe = p.xp[j]; }
    else {
      xhe = fwd_point(x0e, g0e, p.tau);
      xpe = prox_scalar_rt(p.px.kind, xhe, p.px, 0.0);
      p.xhat[j] = xhe;
      p.xp[j] = xpe;
    }
    p.z[j] = xpe;
    if (WEIGHTED) v[0] += id_weighted(wt[j], loss_term(xpe, p.b[j], p.loss));
    else v[0] += loss_term(xpe, p.b[j], p.loss);
    nside_fwd_sums<1>(x0e, g0e, xhe, xpe, xav, v);
  }
  finish_records<8, S_GMAX>(v, p.red, blockIdx.x, gridDim.x, p.counter, p.out, p.seq, s_scr, s_flag, NoRecords(), [&](double (&w)[8]) {
    double alpha = 0.0;                      // the thresholding's g terms and the rank it kept stand in for the elementwise ones
    if (p.mode == 0 && p.given) { w[S_GSUM] = p.nuc[0]; alpha = p.nuc[1]; w[S_GMAX] = p.nuc[2]; }
    store_fwd_scalars(p.out, w, alpha);
  });
}

struct IdAdjP {
  uint64_t n;
  int mode;             // 0 = FBS (x1, g1, the BB epilogue), 1 = plain gradient of z (g1 only; the sums are published as zeros)
  int accel, sub_b, loss;
  int gsum_mode;        // FH_S_GSUM_ADJ / FH_S_GMAX_ADJ: 0 = sum / max |x1|, 1 = gsum_src[0] / [2] (the thresholding's: x1 is xprox), 2 = NaN / 0 (not evaluated), 3 = left to a later launch
  unsigned seq;
  double coef, tau;
  const double* z; const double* b;
  const double* x0; const double* xp; const double* xacc0; const double* xhat;
  double* x1; double* g1;
  const double* gsum_src;
  double* red;          // [gridDim.x][8]
  unsigned* counter;
  double* out;
};

// (k_id_adj keeps its own text of the n-side epilogue and of the finaliser: the gradient is taken AT x1, so the extrapolation has to be formed before
// nside_adj_sums would form it, and through the shared code the small launch (64 x 64) measured 0.27 us slower; profiles/nside_refactor.txt section 6.)
struct IdAdjWP { IdAdjP p; const double* w; };
__device__ __forceinline__ const IdAdjP& id_args(const IdAdjP& a) { return a; }
__device__ __forceinline__ const IdAdjP& id_args(const IdAdjWP& a) { return a.p; }
__device__ __forceinline__ const double* id_weights(const IdAdjP&) { return nullptr; }
__device__ __forceinline__ const double* id_weights(const IdAdjWP& a) { return a.w; }

template <bool WEIGHTED>
static __global__ __launch_bounds__(FH_WG) void k_id_adj(const typename std::conditional<WEIGHTED, IdAdjWP, IdAdjP>::type args) {
#pragma clang fp contract(off)
  const IdAdjP& p = id_args(args);
  const double* wt = id_weights(args);
  __shared__ __attribute__((aligned(16))) double s_scr[4 * 8];
  __shared__ __attribute__((aligned(16))) unsigned s_flag[4];
  const uint32_t tid = threadIdx.x;
  double v[6] = {0, 0, 0, 0, 0, 0};      // dxdg, dg2, xh2, gsum, gmax, f
  for (uint64_t j = (uint64_t)blockIdx.x * FH_WG + tid; j < p.n; j += (uint64_t)gridDim.x * FH_WG) {
    if (p.mode != 0) {
      const double zv = p.z[j];
      const double bv = p.sub_b ? p.b[j] : 0.0;
      if (WEIGHTED && p.sub_b) {
        const double wv = wt[j];
        p.g1[j] = id_weighted(wv, loss_grad(zv, bv, p.loss));
        v[5] += id_weighted(wv, loss_term(zv, bv, p.loss));
        continue;
      }
      p.g1[j] = p.sub_b ? loss_grad(zv, bv, p.loss) : zv;
      v[5] += p.sub_b ? loss_term(zv, bv, p.loss) : zv * zv;
      continue;
    }
    const double x0e = p.x0[j], xpe = p.xp[j], xhe = p.xhat[j], bv = p.b[j];
    double x1 = xpe;
    if (p.accel) x1 = extrapolate(xpe, p.xacc0[j], p.coef);
    double g = loss_grad(x1, bv, p.loss), ft = loss_term(x1, bv, p.loss);
    if (WEIGHTED) { const double wv = wt[j]; g = id_weighted(wv, g); ft = id_weighted(wv, ft); }
    p.g1[j] = g;
    v[5] += ft;
    const double dx = sub_nofma(xpe, x0e);
    const double dg = bb_dgrad(g, xhe, x0e, p.tau);
    const double dh = sub_nofma(x1, xhe);
    v[0] = fma(dx, dg, v[0]);
    v[1] = fma(dg, dg, v[1]);
    v[2] = fma(dh, dh, v[2]);
    v[3] += fabs(x1);
    v[4] = fmax(v[4], fabs(x1));
    if (p.accel) p.x1[j] = x1;
  }
  block_reduce<6>(v, s_scr, 4);
  if (tid == 0) {
#pragma unroll
    for (int k = 0; k < 6; ++k) store_partial(p.red + (uint64_t)blockIdx.x * 8 + k, v[k]);
  }
  if (!arrive_last(p.counter, gridDim.x, s_flag)) return;
  double w[6] = {0, 0, 0, 0, 0, 0};
  for (uint32_t i = tid; i < gridDim.x; i += FH_WG) {
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const double t = load_partial(p.red + (uint64_t)i * 8 + k);
      if (k == 4) w[k] = fmax(w[k], t); else w[k] += t;
    }
  }
  block_reduce<6>(w, s_scr, 4);
  if (tid == 0) {
    if (p.gsum_mode == 1) { w[3] = p.gsum_src[0]; w[4] = p.gsum_src[2]; }
    if (p.gsum_mode == 2) { w[3] = __builtin_nan(""); w[4] = 0.0; }
    scal_store(p.out + S_DXDG, w[0]); scal_store(p.out + S_DG2, w[1]); scal_store(p.out + S_XH2_ADJ, w[2]);
    if (p.gsum_mode != 3) { scal_store(p.out + S_GSUM_ADJ, w[3]); scal_store(p.out + S_GMAX_ADJ, w[4]); }
    scal_store(p.out + S_FSQ_ADJ, w[5]);
    publish_seq(p.out, p.seq);
    __hip_atomic_store(p.counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// ---- singular-value thresholding ---------------------------------------------------------------------------------------------------------------
struct NucGeo {
  uint32_t M, N;        // the unknown
  uint32_t p, q;        // min / max of them: W has p rows of q columns
  uint32_t P, nb;       // rows of the working buffer (p padded to a multiple of Bk), blocks
  uint32_t qpad, ld;    // q padded to an even count; doubles per row of [ W | J^T ]
  int transposed;       // M > N: W = xhat^T
};

struct NucLoadP {
  NucGeo g;
  const double* x0; const double* g0;      // g0 = nullptr: the operand is x0 itself
  double tau;
  double* xhat;                            // where x0 - tau*g0 is kept (nullptr: nowhere)
  double* W;
  int with_j;
  double* red;          // [gridDim.x]
  unsigned* counter;
  double* fro2;         // ||xhat||_F^2
};

static __global__ __launch_bounds__(FH_WG) void k_nuc_load(const NucLoadP p) {
  __shared__ __attribute__((aligned(16))) double s_scr[4];
  __shared__ __attribute__((aligned(16))) unsigned s_flag[4];
  const uint32_t tid = threadIdx.x;
  const uint64_t total = (uint64_t)p.g.P * p.g.ld;
  double v[1] = {0.0};
  for (uint64_t e = (uint64_t)blockIdx.x * FH_WG + tid; e < total; e += (uint64_t)gridDim.x * FH_WG) {
    const uint32_t r = (uint32_t)(e / p.g.ld), c = (uint32_t)(e % p.g.ld);
    if (c >= p.g.qpad) {
      if (p.with_j) p.W[e] = (c - p.g.qpad == r) ? 1.0 : 0.0;
      continue;
    }
    double val = 0.0;
    if (r < p.g.p && c < p.g.q) {
      const uint64_t src = p.g.transposed ? (uint64_t)c * p.g.N + r : (uint64_t)r * p.g.N + c;
      val = p.x0[src];
      if (p.g0) val = fwd_point(val, p.g0[src], p.tau);
      if (p.xhat) p.xhat[src] = val;
      v[0] = fma(val, val, v[0]);
    }
    p.W[e] = val;
  }
  finish_records<1, -1>(v, p.red, blockIdx.x, gridDim.x, p.counter, nullptr, 0u, s_scr, s_flag, NoRecords(),      // (no scalar block, no sequence number)
                        [&](double (&w)[1]) { store_partial(p.fro2, w[0]); });
}

// Pair k of step r of a sweep over nb blocks: the round-robin tournament by the circle method over nbe = nb rounded up to even (the last
// of them stays put, the others turn).  false: a bye (the partner is the block an odd nb lacks).  nb = 1: the one self-pair, *b = nb.
__host__ __device__ __forceinline__ bool nuc_pair(uint32_t nb, uint32_t r, uint32_t k, uint32_t* a, uint32_t* b) {
  if (nb == 1) { *a = 0; *b = nb; return true; }
  const uint32_t nbe = nb + (nb & 1u);
  uint32_t x, y;
  if (k == 0) { x = nbe - 1; y = r; }
  else { x = (r + k) % (nbe - 1); y = (r + nbe - 1 - k) % (nbe - 1); }
  if (x >= nb || y >= nb) return false;
  *a = x < y ? x : y; *b = x < y ? y : x;
  return true;
}

// what one wave shares through LDS between two phases of a rotation: every lane's writes before every lane's reads
__device__ __forceinline__ void nuc_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Cyclic Jacobi on the symmetric R x R matrix G in LDS, by ONE wave (all 64 lanes call it; lane k < R owns row / column k of an update); V
// starts as the identity and collects the rotations (V <- V J), G <- J^T G J.  The rules:
//   * index k is DEAD when G_kk <= dead_thr = (eps ||xhat||_F)^2 (written so that a NaN is dead too): its row and column of G are zeroed;
//   * the pair (i, j), i < j in row-cyclic order, rotates iff |G_ij| > tol * sqrt(G_ii * G_jj), tol = eps * sqrt(q), with
//     zeta = (G_jj - G_ii) / (2 G_ij), t = sign(zeta) / (|zeta| + sqrt(1 + zeta^2)) (sign(0) = 1), c = 1 / sqrt(1 + t^2), s = c t;
//     G_ij and G_ji are then set to zero;
//   * inner sweeps until one rotates nothing, at most NUC_MAX_SWEEPS.
// Returns the number of rotations (the same in every lane).
template <int R>
__device__ __forceinline__ unsigned nuc_diagonalise(volatile double* G, volatile double* V, double dead_thr, double tol, int lane) {
  for (int e = lane; e < R * R; e += 64) V[e] = (e / R == e % R) ? 1.0 : 0.0;
  // (a dead index: first its row, then its column -- no lane zeroes another lane's diagonal before that lane has read it)
  const bool dead_k = lane < R && !(G[(lane < R ? lane : 0) * (R + 1)] > dead_thr);
  nuc_wave_sync();
  if (dead_k) for (int c = 0; c < R; ++c) G[lane * R + c] = 0.0;
  nuc_wave_sync();
  if (dead_k) for (int c = 0; c < R; ++c) G[c * R + lane] = 0.0;
  nuc_wave_sync();
  unsigned total = 0;
  for (int sweep = 0; sweep < NUC_MAX_SWEEPS; ++sweep) {
    unsigned rot = 0;
    for (int i = 0; i < R - 1; ++i) {
      for (int j = i + 1; j < R; ++j) {
        // (every lane reads the same three words; readlane makes the branch below a scalar one)
        const double gij = readlane_f64(G[i * R + j], 0);
        if (gij == 0.0) continue;                                   // (cannot pass the test below; spares the diagonal reads)
        const double gii = readlane_f64(G[i * R + i], 0), gjj = readlane_f64(G[j * R + j], 0);
        if (!(fabs(gij) > tol * sqrt(gii * gjj))) continue;
        const double zeta = (gjj - gii) / (2.0 * gij);
        const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
        const double c = 1.0 / sqrt(1.0 + t * t);
        const double s = c * t;
        nuc_wave_sync();
        if (lane < R) {                                             // columns i and j of G and of V
          const double a = G[lane * R + i], b = G[lane * R + j];
          G[lane * R + i] = c * a - s * b; G[lane * R + j] = s * a + c * b;
          const double va = V[lane * R + i], vb = V[lane * R + j];
          V[lane * R + i] = c * va - s * vb; V[lane * R + j] = s * va + c * vb;
        }
        nuc_wave_sync();
        if (lane < R) {                                             // rows i and j of G
          const double a = G[i * R + lane], b = G[j * R + lane];
          double ni = c * a - s * b, nj = s * a + c * b;
          if (lane == j) ni = 0.0;
          if (lane == i) nj = 0.0;
          G[i * R + lane] = ni; G[j * R + lane] = nj;
        }
        nuc_wave_sync();
        rot += 1u;
      }
    }
    total += rot;
    if (rot == 0u) break;
  }
  return total;
}

struct NucStepP {
  NucGeo g;
  double* W;
  uint32_t step;        // of the sweep's schedule
  uint32_t cols;        // columns the rotations are applied to: ld with J, qpad for a values-only decomposition
  const double* fro2;
  unsigned* rotations;  // this sweep's counter
};

template <int BK>
__global__ __launch_bounds__(FH_WG) void k_nuc_step(const NucStepP p) {
  constexpr int R = 2 * BK;
  constexpr int NG = FH_WG / (R * R);          // lanes that share an entry of G (1 for BK = 8)
  __shared__ __attribute__((aligned(16))) double s_tile[R * NUC_LDT];
  __shared__ __attribute__((aligned(16))) double s_G[R * R];
  __shared__ __attribute__((aligned(16))) double s_V[R * R];
  __shared__ __attribute__((aligned(16))) double s_part[FH_WG];
  __shared__ unsigned s_rot;
  const uint32_t tid = threadIdx.x;
  uint32_t ba = 0, bb = 0;
  if (!nuc_pair(p.g.nb, p.step, blockIdx.x, &ba, &bb)) return;                     // the bye (the whole workgroup)
  // row a < R of the pair -> row of the working buffer, or P ("absent": the second half of a self-pair)
  auto row_of = [&](int a) -> uint32_t { return a < BK ? ba * BK + a : (bb < p.g.nb ? bb * BK + (a - BK) : p.g.P); };
  const uint32_t q2 = p.g.qpad / 2;                                                 // 16-byte pieces of a row of W
  // 1. the Gram matrix of the R rows
  const int ent = tid % (R * R), grp = tid / (R * R);
  const int ea = ent / R, eb = ent % R;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (uint32_t c0 = 0; c0 < q2; c0 += NUC_CC / 2) {
    for (uint32_t t = tid; t < (uint32_t)R * (NUC_CC / 2); t += FH_WG) {
      const uint32_t a = t / (NUC_CC / 2), k = t % (NUC_CC / 2);
      const uint32_t row = row_of((int)a);
      d2 w = {0.0, 0.0};
      if (row < p.g.P && c0 + k < q2) w = *reinterpret_cast<const d2*>(p.W + (uint64_t)row * p.g.ld + 2 * (uint64_t)(c0 + k));
      *reinterpret_cast<d2*>(s_tile + a * NUC_LDT + 2 * k) = w;
    }
    __syncthreads();
#pragma unroll 4
    for (int k = grp; k < NUC_CC / 2; k += 2 * NG) {
      const d2 xa = *reinterpret_cast<const d2*>(s_tile + ea * NUC_LDT + 2 * k);
      const d2 xb = *reinterpret_cast<const d2*>(s_tile + eb * NUC_LDT + 2 * k);
      const d2 ya = *reinterpret_cast<const d2*>(s_tile + ea * NUC_LDT + 2 * (k + NG));
      const d2 yb = *reinterpret_cast<const d2*>(s_tile + eb * NUC_LDT + 2 * (k + NG));
      acc[0] = fma(xa.x, xb.x, acc[0]); acc[1] = fma(xa.y, xb.y, acc[1]);
      acc[2] = fma(ya.x, yb.x, acc[2]); acc[3] = fma(ya.y, yb.y, acc[3]);
    }
    __syncthreads();
  }
  s_part[tid] = (acc[0] + acc[1]) + (acc[2] + acc[3]);
  __syncthreads();
  if (tid < R * R) {
    double gsum = s_part[tid];
#pragma unroll
    for (int g = 1; g < NG; ++g) gsum += s_part[g * R * R + tid];                   // the lanes of an entry in order
    s_G[tid] = gsum;
  }
  __syncthreads();
  // 2. one wave diagonalises it
  if (tid < 64) {
    const double f2 = load_partial(p.fro2);
    const double dead_thr = (NUC_EPS * NUC_EPS) * f2;
    const double tol = NUC_EPS * sqrt((double)p.g.q);
    const unsigned rot = nuc_diagonalise<R>(s_G, s_V, dead_thr, tol, (int)tid);
    if (tid == 0) s_rot = rot;
  }
  __syncthreads();
  const unsigned rot = s_rot;
  if (rot == 0u) return;                                                            // rotated nothing: writes nothing
  // 3. rows <- V^T rows, a lane per 16-byte piece
  const uint32_t c2 = p.cols / 2;
  for (uint32_t k = tid; k < c2; k += FH_WG) {
    d2 w[R];
#pragma unroll
    for (int a = 0; a < R; ++a) {
      const uint32_t row = row_of(a);
      w[a] = (d2){0.0, 0.0};
      if (row < p.g.P) w[a] = *reinterpret_cast<const d2*>(p.W + (uint64_t)row * p.g.ld + 2 * (uint64_t)k);
    }
#pragma unroll
    for (int a = 0; a < R; ++a) {
      d2 o = {0.0, 0.0};
#pragma unroll
      for (int b = 0; b < R; ++b) {
        const double vba = s_V[b * R + a];
        o.x = fma(vba, w[b].x, o.x); o.y = fma(vba, w[b].y, o.y);
      }
      const uint32_t row = row_of(a);
      if (row < p.g.P) *reinterpret_cast<d2*>(p.W + (uint64_t)row * p.g.ld + 2 * (uint64_t)k) = o;
    }
  }
  if (tid == 0) atomicAdd(p.rotations, rot);
}

struct NucSigmaP {
  NucGeo g;
  const double* W;
  double thr;
  double* phi;          // [P] (nullptr: values only)
  double* red;          // [P][2]
  unsigned* counter;
  double* out_gsum;     // sum max(sigma_i - thr, 0) (nullptr: no sums at all -- the per-row records are what the caller wants, k_nuc_ball reads them)
  double* out_gmax;     // max max(sigma_i - thr, 0)
  double* out_rank;     // #{sigma_i > thr} (nullptr: not wanted)
  int to_host;          // out_* lie in the mapped scalar block: system-scope stores
};

// one workgroup per row of W
static __global__ __launch_bounds__(FH_WG) void k_nuc_sigma(const NucSigmaP p) {
  __shared__ __attribute__((aligned(16))) double s_scr[4 * 3];
  __shared__ __attribute__((aligned(16))) unsigned s_flag[4];
  const uint32_t tid = threadIdx.x, row = blockIdx.x;
  const d2* w = reinterpret_cast<const d2*>(p.W + (uint64_t)row * p.g.ld);
  double a0 = 0.0, a1 = 0.0;
  for (uint32_t k = tid; k < p.g.qpad / 2; k += FH_WG) { const d2 x = w[k]; a0 = fma(x.x, x.x, a0); a1 = fma(x.y, x.y, a1); }
  double v[1] = {a0 + a1};
  block_reduce<1>(v, s_scr, -1);
  if (tid == 0) {
    const double sigma = sqrt(v[0]);
    const double kept = fmax(sigma - p.thr, 0.0);
    const bool live = row < p.g.p;
    if (p.phi) p.phi[row] = live ? kept / (sigma + (sigma == 0.0 ? 1.0 : 0.0)) : 0.0;
    store_partial(p.red + 2 * (uint64_t)row, live ? kept : 0.0);
    store_partial(p.red + 2 * (uint64_t)row + 1, (live && sigma > p.thr) ? 1.0 : 0.0);
  }
  if (!arrive_last(p.counter, gridDim.x, s_flag)) return;
  if (!p.out_gsum) {                                                                 // (uniform: a kernel argument)
    if (tid == 0) __hip_atomic_store(p.counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return;
  }
  double s[3] = {0.0, 0.0, 0.0};
  for (uint32_t i = tid; i < gridDim.x; i += FH_WG) {
    const double kept = load_partial(p.red + 2 * (uint64_t)i);
    s[0] += kept; s[1] += load_partial(p.red + 2 * (uint64_t)i + 1); s[2] = fmax(s[2], kept);
  }
  block_reduce<3>(s, s_scr, 2);
  if (tid == 0) {
    if (p.to_host) { scal_store(p.out_gsum, s[0]); scal_store(p.out_gmax, s[2]); if (p.out_rank) scal_store(p.out_rank, s[1]); }
    else { store_partial(p.out_gsum, s[0]); store_partial(p.out_gmax, s[2]); if (p.out_rank) store_partial(p.out_rank, s[1]); }
    __hip_atomic_store(p.counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

struct NucBallP {
  uint32_t p, P;        // singular values; rows of the working buffer (phi has P entries, the padded rows' are 0)
  double radius;
  const double* red;    // [P][2] as k_nuc_sigma left it at thr = 0: [2 i] = sigma_i
  double* phi;          // [P]
  double* out_gsum;     // sum max(sigma_i - theta, 0)
  double* out_gmax;     // max max(sigma_i - theta, 0)
  double* out_rank;     // #{sigma_i > theta}
};

// ONE workgroup; p <= NUC_MAX_P.  Padded rows (row >= p) never enter the ordering.
static __global__ __launch_bounds__(FH_WG) void k_nuc_ball(const NucBallP p) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) double s_sig[NUC_MAX_P];
  __shared__ __attribute__((aligned(16))) double s_ord[NUC_MAX_P];      // the sigma in descending order, then their running sums
  __shared__ __attribute__((aligned(16))) double s_scr[4 * 3];
  __shared__ double s_theta;
  const uint32_t tid = threadIdx.x;
  const uint32_t n = p.p < NUC_MAX_P ? p.p : NUC_MAX_P;
  for (uint32_t i = tid; i < n; i += FH_WG) { s_sig[i] = load_partial(p.red + 2 * (uint64_t)i); s_ord[i] = 0.0; }
  __syncthreads();
  // 1. rank by counting, the index as tie-break (every lane reads the same word of s_sig: a broadcast, no bank conflict)
  for (uint32_t i = tid; i < n; i += FH_WG) {
    const double si = s_sig[i];
    uint32_t rank = 0;
    for (uint32_t j = 0; j < n; ++j) { const double sj = s_sig[j]; rank += (sj > si || (sj == si && j < i)) ? 1u : 0u; }
    s_ord[rank] = si;                                                    // (rank < n: a lane counts at most the n - 1 others)
  }
  __syncthreads();
  // 2. the running sums, serially, in index order
  if (tid == 0) { double c = 0.0; for (uint32_t k = 0; k < n; ++k) { c += s_ord[k]; s_ord[k] = c; } }
  __syncthreads();
  // 3. alpha = max_k (c_k - radius) / k, k = 1 .. n
  double a[1] = {-__builtin_inf()};
  for (uint32_t k = tid; k < n; k += FH_WG) a[0] = fmax(a[0], (s_ord[k] - p.radius) / (double)(k + 1u));
  block_reduce<1>(a, s_scr, 0);
  if (tid == 0) s_theta = fmax(a[0], 0.0);
  __syncthreads();
  const double theta = s_theta;
  // 4. phi and the three scalars, as k_nuc_sigma's last workgroup forms them
  double s[3] = {0.0, 0.0, 0.0};
  for (uint32_t i = tid; i < p.P; i += FH_WG) {
    const bool live = i < n;
    const double sigma = live ? s_sig[i] : 0.0;
    const double kept = live ? fmax(sigma - theta, 0.0) : 0.0;
    p.phi[i] = kept / (sigma + (sigma == 0.0 ? 1.0 : 0.0));
    s[0] += kept; s[1] += (live && sigma > theta) ? 1.0 : 0.0; s[2] = fmax(s[2], kept);
  }
  block_reduce<3>(s, s_scr, 2);
  if (tid == 0) { store_partial(p.out_gsum, s[0]); store_partial(p.out_gmax, s[2]); store_partial(p.out_rank, s[1]); }
}

struct NucReconP {
  NucGeo g;
  const double* W;
  const double* phi;
  double* xp;
};

#define NUC_TR 16       // rows of xprox (in W's orientation) per workgroup of k_nuc_recon
// workgroup (x, y): columns [256 x, 256 x + 256) of rows [16 y, 16 y + 16) of J diag(phi) W; a lane owns a column
static __global__ __launch_bounds__(FH_WG) void k_nuc_recon(const NucReconP p) {
  const uint32_t col = blockIdx.x * FH_WG + threadIdx.x;
  const uint32_t r0 = blockIdx.y * NUC_TR;
  const bool mine = col < p.g.q;
  const uint32_t cc = mine ? col : 0u;                                              // clamp: in-bounds redundant loads
  double acc[NUC_TR];
#pragma unroll
  for (int r = 0; r < NUC_TR; ++r) acc[r] = 0.0;
  for (uint32_t i = 0; i < p.g.p; ++i) {
    const double f = p.phi[i];
    if (f == 0.0) continue;                                                         // (uniform: phi is read through scalar loads)
    const double* wrow = p.W + (uint64_t)i * p.g.ld;
    const double w = wrow[cc];
#pragma unroll
    for (int r = 0; r < NUC_TR; ++r) {
      const double jt = (r0 + r < p.g.p) ? wrow[p.g.qpad + r0 + r] : 0.0;           // J[r0 + r][i] = (J^T)[i][r0 + r]
      acc[r] = fma(jt * f, w, acc[r]);
    }
  }
  if (!mine) return;
#pragma unroll
  for (int r = 0; r < NUC_TR; ++r) {
    const uint32_t row = r0 + r;
    if (row >= p.g.p) break;
    const uint64_t dst = p.g.transposed ? (uint64_t)col * p.g.N + row : (uint64_t)row * p.g.N + col;
    p.xp[dst] = acc[r];
  }
}

static __global__ void k_nuc_fill(double* x, uint64_t n, double value) {
  for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (uint64_t)gridDim.x * blockDim.x) x[j] = value;
}

#define NUC_KERNELS(DO)                                    \
  DO __global__ void k_nuc_step<1>(const NucStepP);        \
  DO __global__ void k_nuc_step<2>(const NucStepP);        \
  DO __global__ void k_nuc_step<4>(const NucStepP);        \
  DO __global__ void k_nuc_step<8>(const NucStepP);

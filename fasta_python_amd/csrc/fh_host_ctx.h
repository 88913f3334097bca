// fh_host_ctx.h -- host-side state of libfasta_hip.so: error reporting, RCCL through dlopen, the context (fh_ctx: one device,
// or a shell over one shard per device), buffer management, HIP-event timing, the scalar block's way back to the host and the
// sums over row blocks.  Included by fasta_hip.hip only (one translation unit); the C ABI itself is in fasta_hip.hip.
#pragma once
#include <atomic>
#include <chrono>
#include <thread>
#include <chrono>

// ------------------------------------------------------------------------------------------------
// errors
// ------------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";

static int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code ? code : FH_E_ARG;
}

#define HIP_TRY(expr)                                                                         \
  do {                                                                                        \
    hipError_t e_ = (expr);                                                                   \
    if (e_ != hipSuccess)                                                                     \
      return fail((int)e_, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)

#define FH_TRY(expr)          \
  do {                        \
    int r_ = (expr);          \
    if (r_ != 0) return r_;   \
  } while (0)

extern "C" const char* fh_last_error(void) { return g_err; }

// ------------------------------------------------------------------------------------------------
// RCCL through dlopen (no link-time dependency; the single-GPU path never touches it)
// ------------------------------------------------------------------------------------------------
typedef struct { char internal[128]; } fh_nccl_uid;
typedef void* fh_nccl_comm;
struct RcclApi {
  void* lib = nullptr;
  int (*GetUniqueId)(fh_nccl_uid*) = nullptr;
  int (*CommInitRank)(fh_nccl_comm*, int, fh_nccl_uid, int) = nullptr;
  int (*CommInitAll)(fh_nccl_comm*, int, const int*) = nullptr;
  int (*CommDestroy)(fh_nccl_comm) = nullptr;
  int (*CommCount)(const fh_nccl_comm, int*) = nullptr;
  int (*AllReduce)(const void*, void*, size_t, int, int, fh_nccl_comm, hipStream_t) = nullptr;
  int (*GroupStart)() = nullptr;
  int (*GroupEnd)() = nullptr;
  int (*GetVersion)(int*) = nullptr;          // optional (diagnostics only)
  const char* (*GetErrorString)(int) = nullptr;
};
static RcclApi g_rccl;
static const int kNcclFloat64 = 8;   // ncclDouble
static const int kNcclSum = 0;       // ncclSum

static char g_rccl_path[512] = "";     // what rccl_load() opened (fh_comm_library)
static int rccl_load() {
  if (g_rccl.lib) return 0;
  // FASTA_RCCL_LIB names another library with RCCL's entry points (a different RCCL build; the tests' multi-process stand-in).
  // A substitution is never silent: one line on stderr, and fh_comm_library() reports the path that was opened.
  const char* sub = getenv("FASTA_RCCL_LIB");
  const char* names[] = {sub, "/opt/rocm/lib/librccl.so.1", "librccl.so.1", "librccl.so"};
  for (const char* nm : names) {
    if (!nm || !*nm) continue;
    g_rccl.lib = dlopen(nm, RTLD_NOW | RTLD_LOCAL);
    if (g_rccl.lib) { snprintf(g_rccl_path, sizeof g_rccl_path, "%s", nm); break; }
    if (nm == sub) return fail(FH_E_RCCL, "FASTA_RCCL_LIB=%s cannot be opened: %s (unset it to use the system's RCCL)", nm, dlerror());
  }
  if (!g_rccl.lib) return fail(FH_E_RCCL, "cannot dlopen librccl: %s", dlerror());
  if (sub && *sub) fprintf(stderr, "libfasta_hip: collectives come from FASTA_RCCL_LIB=%s, not from the system's RCCL\n", sub);
#define SYM(field, name)                                                      \
  *(void**)(&g_rccl.field) = dlsym(g_rccl.lib, name);                         \
  if (!g_rccl.field) return fail(FH_E_RCCL, "librccl lacks symbol %s", name)
  SYM(GetUniqueId, "ncclGetUniqueId");
  SYM(CommInitRank, "ncclCommInitRank");
  SYM(CommInitAll, "ncclCommInitAll");
  SYM(CommDestroy, "ncclCommDestroy");
  SYM(CommCount, "ncclCommCount");
  SYM(AllReduce, "ncclAllReduce");
  SYM(GroupStart, "ncclGroupStart");
  SYM(GroupEnd, "ncclGroupEnd");
  SYM(GetErrorString, "ncclGetErrorString");
#undef SYM
  *(void**)(&g_rccl.GetVersion) = dlsym(g_rccl.lib, "ncclGetVersion");
  return 0;
}
#define NCCL_TRY(expr)                                                                        \
  do {                                                                                        \
    int r_ = (expr);                                                                          \
    if (r_ != 0) return fail(20000 + r_, "%s failed: %s", #expr, g_rccl.GetErrorString(r_));  \
  } while (0)

// geometry of the DCT operator's launches (csrc/fh_host_launch.h: dct_shape_for fills it)
struct DctShape { uint32_t levels, N1, N2, cap; DctRad r1, r2; uint32_t ldsn1, rpw1, grid1, ldsn2, rpw2, grid2, tiles, launches, lds_bytes; };
// geometry of the 2-D DCT operator's launches (csrc/fh_host_launch.h: dct2_shape_for fills it); suffix h: the W rows of length H, w: the H rows of length W
struct Dct2Shape { uint32_t served, H, W, cap; DctRad rh, rw; uint32_t ldsn_h, rpw_h, grid_h, ldsn_w, rpw_w, grid_w, tiles, launches, lds_bytes; };

// geometry of the nuclear-norm prox's launches (csrc/fh_host_launch.h: nuc_shape_for fills it)
struct NucShape { NucGeo g; uint32_t Bk, steps, wgs, chunks, lds_bytes; uint64_t bytes; };

// geometry of the convolution operator's launches (csrc/fh_host_launch.h: conv_shape_for fills it)
struct ConvShape { uint32_t th, tw, tw_log2, pitch, tiles_h, tiles_w, grid, lds_bytes; };

// ------------------------------------------------------------------------------------------------
// context
// ------------------------------------------------------------------------------------------------
enum { OP_NONE = 0, OP_DENSE = 1, OP_STENCIL = 2, OP_SPARSE = 3, OP_STENCIL3D = 4, OP_QUAD = 5, OP_BILINEAR = 6, OP_DCT = 7, OP_IDENTITY = 8, OP_CONV = 9 };

struct fh_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  int op = OP_NONE;
  uint64_t m = 0, n = 0;     // logical (local) rows / columns of A   (stencil: m = H*W, n = 2*H*W)
  uint64_t mp = 0, ld = 0;   // padded rows, device leading dimension in elements (dense)
  int f32 = 0;               // storage of A: 0 = float64, 1 = float32 (opt-in, fh_create_ex; vectors and arithmetic stay float64)
  uint64_t nv = 0, mv = 0;   // allocated n-side / m-side vector lengths (doubles; rows of LB doubles in multi-column form)
  uint32_t L = 0, LB = 0;    // multi-column form (fh_set_rhs, csrc/fh_multi.h; fh_set_matrix_csr_rhs, csrc/fh_spmulti.h; fh_set_quadratic, csrc/fh_quad.h): L columns per unknown, kept as LB in {2, 4, 8, 16} doubles per row; 0 = the vector form
  // bilinear smooth term (fh_set_factorization, csrc/fh_bilinear.h): S is (bl_m, bl_n), stored like a dense A in `A` (mp rows of ld doubles); the unknown
  // Z = [X; Y] has m = n = bl_m + bl_n rows.  bl_part: f of the latest pass (2 doubles), then the GX and the GY partials that pass wrote with the
  // geometry bl_nct / bl_nrp -- a buffer of its own, because they live from the forward launch to the adjoint one; bl_have_grad: they are there.
  // FH_PROX_ROWSPLIT (fh_set_prox_split): rows [0, rs_split) take rs_kind_top with mu / lo / hi, the other rows rs_kind_bot with rs_lo_bot / rs_hi_bot.
  uint64_t bl_m = 0, bl_n = 0;
  double* bl_part = nullptr;
  size_t bl_part_bytes = 0;
  uint32_t bl_nct = 0, bl_nrp = 0;
  bool bl_have_grad = false;
  uint64_t rs_split = 0;
  int rs_kind_top = 0, rs_kind_bot = 0;
  double rs_lo_bot = 0.0, rs_hi_bot = 0.0;
  uint64_t H = 0, W = 0;
  // subsampled DCT (fh_set_dct, csrc/fh_dct.h): m = n = N; tw[j] = e^{-2 pi i j / N}, pw[k] = e^{-i pi k / 2N}, the diagonal d (nullptr: all ones),
  // two work buffers of N double2 (two-level transforms only), and what is derived once when the operator is set
  d2* dct_tw = nullptr; d2* dct_pw = nullptr; double* dct_diag = nullptr;
  d2* dct_w0 = nullptr; d2* dct_w1 = nullptr;
  DctShape dct_sh = {};      // the geometry dct_shape_for gave when the operator was set (every launch reads it; fh_dct_shape reports it)
  double dct_sc0 = 0.0, dct_sck = 0.0;   // sqrt(1/N), sqrt(2/N)
  // the DCT operator in its 2-D geometry (fh_set_dct2, csrc/fh_dct2.h): op == OP_DCT and dct2; m = n = H * W; dct_tw / dct_pw / dct_sc0 / dct_sck serve
  // the H axis, the four below the W axis; dct_diag holds H * W values; two work buffers of H * W doubles
  bool dct2 = false;
  d2* dct2_tw = nullptr; d2* dct2_pw = nullptr;
  double* dct2_w0 = nullptr; double* dct2_w1 = nullptr;
  Dct2Shape dct2_sh = {};    // the geometry dct2_shape_for gave when the operator was set (every launch reads it; fh_dct2_shape reports it)
  double dct2_sc0 = 0.0, dct2_sck = 0.0;
  // periodic convolution (fh_set_conv2d, csrc/fh_conv.h): the image is (H, W), m = n = H * W; the taps (kh * kw, C order: they travel in the
  // kernels' argument block), the origin, the diagonal d (nullptr: all ones) and the geometry conv_shape_for gave when the operator was set
  uint32_t conv_kh = 0, conv_kw = 0, conv_oh = 0, conv_ow = 0;
  double conv_taps[256] = {};
  double* conv_diag = nullptr;
  ConvShape conv_sh = {};
  // identity operator (fh_set_identity, csrc/fh_nuclear.h): the unknown is an (id_M, id_N) matrix in the vector form's buffers.  FH_PROX_NUCLEAR
  // (fh_set_prox_nuclear): the geometry nuc_shape_for gave when the prox was set, the working buffer [ W | J^T ], phi, three device scalars
  // (||xhat||_F^2, the nuclear norm of xprox, the rank kept), one rotation counter per sweep with its pinned host copy, and the latest run's record
  uint64_t id_M = 0, id_N = 0;
  NucShape nuc_sh = {};
  int nuc_objective = 1;
  double* nuc_w = nullptr; double* nuc_phi = nullptr; double* nuc_scal = nullptr;
  unsigned* nuc_cnt = nullptr; unsigned* nuc_host = nullptr;
  uint64_t nuc_info[4] = {0, 0, 0, 0};      // sweeps, steps launched, rotations, rank kept
  // observation weights of the elementwise loss (fh_set_loss_weights): n doubles, or nullptr = unweighted.  They belong to the loss: fh_set_loss_* drops them.
  double* loss_w = nullptr;
  uint64_t D = 0;            // 3-D stencil (fh_set_stencil3d, csrc/fh_tv3d.h): the volume is (D, H, W), m = D*H*W, n = 3*m
  // sparse operator (fh_set_matrix_csr, csrc/fh_sparse.h): sp[0] = A by rows, sp[1] = A^T by rows, each with its non-zero-balanced row ranges,
  // its list of long rows and the lanes-per-row G chosen from its mean row length; sp_r = the adjoint's residual (m-side).  In multi-column form
  // (fh_set_matrix_csr_rhs, csrc/fh_spmulti.h) G, the long-row threshold and the row ranges are those of LB / 2 column lanes per entry: fixed when the operator is set
  SpMatP sp[2] = {};
  int sp_G[2] = {0, 0};
  uint64_t nnz = 0;
  double* sp_r = nullptr;
  double* A = nullptr;
  // squared column norms of A (fh_column_norms, csrc/fh_screen.h): nv doubles, kept until the operator goes; cn2_held: they are those of the operator held
  double* cn2 = nullptr;
  bool cn2_held = false;
  size_t a_block_bytes = 0;  // size of the block A lives in (>= the matrix: a kept block may be up to twice as large, see acquire_matrix_block)
  // n-side
  // iterate pool: X[xi] = x0, X[ti] = where the next x1 lands, X[bi] = best-quality iterate (may alias X[xi]):
  // the best iterate is tracked by index, never copied (a 1 GiB copy per improving iteration at 8192^2 TV)
  double* X[3] = {nullptr, nullptr, nullptr};
  int xi = 0, ti = 1, bi = 0;
  double* P[2] = {nullptr, nullptr};   // prox outputs: x_accel1 / x_accel0
  double* G[2] = {nullptr, nullptr};   // g0 / g1
  double* xhat = nullptr;
  double* xs = nullptr;      // multi-column form: K-fwd's operand in its streaming layout (csrc/fh_multi.h: mc_pack_row)
  double* T[4] = {nullptr, nullptr, nullptr, nullptr};
  int pc = 0, gc = 0, zc = 0;
  bool last_accel = false;
  bool at_state = false;     // x0, g0 and Z[zc] = A x0 belong together: set by fh_init / fh_setup, lost with the operator, the loss, the column count or a vector set from outside (fh_dual_gap asks)
  // m-side
  double* b = nullptr;
  double* Z[2] = {nullptr, nullptr};
  double* zt = nullptr;
  double* ZX[2] = {nullptr, nullptr};   // stencil + FISTA: extrapolated z' (the residual source of the next g0)
  int zxc = 0;
  const double* zcur = nullptr;         // stencil: z at the current x0 (Z[zc], or ZX[zxc] after an accelerated step)
  // stencil + FISTA in ONE pass (k_fused_tv_accel): the iterate and its image are kept LAZILY as (P1, P0, c) and (Z1, Z0, c):
  // x0 = P1 + c*(P1 - P0), z(x0) = Z1 + c*(Z1 - Z0) are formed inside the next sweep and never written.  Buffers are taken
  // from the n-side pool {X[0], X[1], X[2], P[0], P[1]} and the m-side pool {Z[0], Z[1], ZX[0]} by index.
  bool lazy = false;
  int lq1 = 0, lq0 = 0, lqn = 0;        // last prox output, the one before, target of the next launch
  int lz1 = 0, lz0 = 0, lzn = 0;        // their images
  int lb1 = 0, lb0 = 0;                 // best-quality iterate = nq(lb1) + lbc*(nq(lb1) - nq(lb0)), by reference
  double lbc = 0.0, lc = 0.0, lc_pending = 0.0;   // coefficient of the best iterate / of x0 / decided by the launch awaiting fh_commit
  uint64_t commits = 0;                 // fh_commit calls since fh_init
  // z-free one-pass stencil kernels (k_tv_onepass, the default): they neither read nor write z, so after such a step is
  // committed the stored image of x0 is stale; the two-launch kernels recompute it on demand (one plain div pass)
  int tv_zfree = 1;                     // FH_TUNE_TV_ZFREE
  bool tvz_pending = false;             // the latest launch was z-free (its z_new exists only inside the kernel)
  bool zcur_stale = false;
  bool has_b = false;
  int loss_kind = LOSS_LSQ;
  // prox
  int prox_kind = FH_PROX_IDENTITY;
  double mu = 0.0, lo = 0.0, hi = 0.0;
  // workspace
  double* ws = nullptr;
  size_t ws_bytes = 0;
  unsigned* counters = nullptr;      // kCounterWords (8192) words, zeroed at creation; kernels leave them zero
  double* dscal = nullptr;           // FH_NSCALARS + 16 doubles on device
  double* hscal = nullptr;           // pinned, device-mapped host block: single-GPU launches write their scalars here
  double* hscal_dev = nullptr;       // device-side address of hscal
  bool scal_mirrored = false;        // row-sharded runs: the last launch already copied the scalar block into hscal
  // tuning
  int fwd_rows = 0;          // 0 = auto
  long long fwd_cap = 0;     // 0 = auto (4 workgroups per CU, grid-stride over row groups)
  int adj_slab = 0;          // 0 = auto
  int adj_cpt = 0;           // 0 = auto
  int adj_cyclic = 0;        // 0 = auto = 2 = contiguous slabs, 1 = rows dealt cyclically to the slabs (A/B)
  int ld_pad = 0;
  int nt_loads = -1;         // K-fwd / K-adj stream A with non-temporal loads: 1 / 0, -1 = auto (nt_for below: plain loads for a matrix of at most 256 MiB)
  // stencil defaults measured on MI355X at 8192^2 (profiles/r01_tune_tv.txt): plain (not nt) accesses,
  // 8 rows in flight, 32 rows per workgroup for K-fwd and 128 for the read-only K-adj
  int tv_u = 0;              // 0 = auto: 8 for the kernels that stream z, 2 / 4 for the z-free one-pass sweeps (profiles/r02_tune_tv.txt)
  int tv_rows = 0;           // 0 = auto (32 fwd / 128 adj)
  int tv_nt = 0;
  int tv_lds_pad = 0;        // FH_TUNE_TV_LDS_PAD
  int tv_xcd = 0;            // FH_TUNE_TV_XCD: workgroup ids of the one-pass sweep dealt out XCD by XCD (0 / 1 = on, 2 = off)
  int tv_slots = 0;          // FH_TUNE_TV_SLOTS: persistent one-pass sweep, workgroups per CU (0 = one workgroup per chunk)
  int tv_ring = 0;           // FH_TUNE_TV_RING: LDS-DMA trip ring of the one-pass sweep (0 = auto, 1 = off, 2 / 3 = slots per wave)
  int tv3_planes = 0;        // FH_TUNE_TV3_PLANES: planes a workgroup of the 3-D stencil kernels marches over (0 = auto: tv3_shape_for)
  int nuc_block_rows = 0;    // FH_TUNE_NUC_BLOCK_ROWS: rows per block of the nuclear-norm prox's steps (0 = 8); read when the prox is set
  int dct_row_cap = 0;       // FH_TUNE_DCT_ROW_CAP: longest row transform of the DCT operator (0 = DCT_ROW_CAP); read when fh_set_dct sets the operator
  int tv_pipe = 0;           // FH_TUNE_TV_PIPE: rotating trip buffers of the one-pass sweep (0 = auto, 1 = burst, 2, 3)
  bool fused_variant_auto = true;   // cleared by FH_TUNE_FUSED_VARIANT: the caller's word is taken as it is (fused_variant_rule)
  int fused_variant = 2 | 32;   // 2: team members 32 blocks apart (one XCD), best in profiles/r01b_tune_fused.txt; 32 (round 6): rows dealt cyclically to the teams -- the
                             // whole grid streams ONE window of nteams x (rows in flight) consecutive rows instead of nteams windows spread over the matrix: 1-2 % faster on a
                             // well-placed matrix (65536^2: 4.76 vs 4.84-4.88 ms), 9 % at 20000 x 30000, and INSENSITIVE to where the allocator put the matrix (blocked: 5.2-5.45 ms
                             // for a 32 GiB matrix that got the far part of the device's memory, cyclic 4.79-4.81; profiles/r06_placement.txt)
  int test_hooks = 0;        // FH_TUNE_TEST_HOOKS (csrc/fh_experimental.h): fault injection, set by the test-suite only
  int fused_min_rows = 16;   // use fewer teams when m is small: at least this many rows per team (scripts/probes/fused_small_m.py)
  // one-pass kernel hand-off slots: two arrays alternate between launches, each launch re-arms the other one in passing;
  // the host fills both with the sentinel only when this signature (workspace, layout) changes or a launch timed out
  double* slotbuf = nullptr;     // dedicated allocation: the shared workspace `ws` is scribbled over by every other kernel
  size_t slotbuf_bytes = 0;
  uint64_t slots_sig = 0;
  int slots_parity = 0;
  // timing
  bool timing = false;
  // two event pairs per kernel id, used alternately: a pair is read (hipEventElapsedTime) when it is about to be re-recorded, i.e. two launches
  // after its own -- long complete, so the harvest never waits even when the host did not synchronise the stream in between (seq_wait below)
  hipEvent_t ev[FH_NKERNELS][2][2];
  bool ev_pending[FH_NKERNELS][2] = {};
  int ev_cur[FH_NKERNELS] = {};
  // "the scalars are there" by sequence number (fh_device.h:publish_seq): the launcher of a kernel whose finaliser publishes one sets seq_wait
  // to the number it passed; collect_scalars then spins on the word behind the mapped scalar block instead of synchronising the stream
  unsigned seq = 0, seq_wait = 0;
  int seq_poll = 1;          // FH_TUNE_SEQ_POLL: 0 = always hipStreamSynchronize (A/B)
  // FH_K_HOST_ISSUE: host time of a one-pass dense step from its entry to the start of its final synchronisation
  bool timing_skip_kernels = false;
  double host_issue_ms = 0.0; uint64_t host_issue_calls = 0;
  std::chrono::steady_clock::time_point issue_t0; bool issue_open = false;
  double tot_ms[FH_NKERNELS] = {};
  uint64_t launches[FH_NKERNELS] = {};
  // comm
  fh_nccl_comm comm = nullptr;
  int nranks = 1, rank = 0;
  int ncu = 0;               // compute units of the device (fused one-pass kernel: one workgroup per CU)
  int coresident = -1;       // -1 = not probed yet; 1 / 0 = fused_ncu() workgroups can / cannot run side by side (co_resident())
  int run_max_n = 0;         // FH_TUNE_RUN_MAX_N: widest row fh_run takes (0 = kRunDefaultMaxN)
  int fused_cus = 0;         // FH_TUNE_FUSED_CUS: the one-pass dense kernel uses at most this many CUs (0 = all the device reports)
  // ---- in-process row sharding (fh_create_ex with ndev > 1; SURVEY.md 8(b)/(e): one host thread, one context per device) ----
  // A context created over several devices is a SHELL: it owns one child context per entry of dev_ids (`shards`), each holding
  // a contiguous block of rows of A and the matching slice of b / z, while x, g, xhat are replicated.  Every entry point of the
  // C ABI runs on a shell as: local launches on every shard -> sum over the shards -> n-side epilogue on every shard -> ONE host
  // synchronisation, scalars from shard 0.  The sum is one grouped ncclAllReduce per shard (communicators from
  // ncclCommInitAll) when the device ids differ; when they REPEAT (several shards on one GPU: what a one-GPU box can run) all
  // shards share one stream and k_sum_shards adds their buffers in shard order.
  std::vector<fh_ctx*> shards;       // non-empty: this context is a shell
  std::vector<uint64_t> shard_row0;  // first row of every shard, plus the total (size shards + 1)
  fh_ctx* owner = nullptr;           // set in a shard
  // fh_run (csrc/fh_run.h): the host-mapped block the launch writes its final solver state to, and the host-mapped history block
  void* run_st_host = nullptr; void* run_st_host_dev = nullptr;
  double* run_hist = nullptr; double* run_hist_dev = nullptr; size_t run_hist_steps = 0;
  unsigned* gridbar = nullptr;       // 3 x GB_WORDS words: two-level grid barrier, two-level final arrival of the dense one-pass / set-up / persistent-loop kernels, final arrival of the stencil sweep (fh_device.h); zero between launches
  double* lvl_rec = nullptr;         // multi-workgroup level search: per-pass records and counters (allocated on first use, counters kept zero)
  unsigned* lvl_cnt = nullptr;
  double* selftest_buf = nullptr;    // fh_comm_selftest's scratch (freed before it returns)
  void* chain_state = nullptr;       // device block of the chained form of fh_run (csrc/fh_fused.h: ChainState)
  int run_chain_on = 0;              // FH_TUNE_RUN_CHAIN = 1: outside the persistent launch's window fh_run takes the chained form (opt-in: measured equal to the host-side loop)
  uint64_t run_timeouts = 0;         // persistent launches of fh_run that ended in a grid-barrier timeout (fh_recovered_count)
  bool pending_step = false;         // fh_step_begin has issued a step whose fh_step_end is still to come (every other entry point refuses)
  bool emulated = false;             // shell / shard: the device ids repeat (one device, one stream, k_sum_shards)
  bool owns_stream = true;           // false in shards 1.. of an emulated group (they run on shard 0's stream)
};

#define FH_MAX_SHARDS 64
static inline int nshards(fh_ctx* c) { return c->shards.empty() ? 1 : (int)c->shards.size(); }
static inline fh_ctx* shard_of(fh_ctx* c, int k) { return c->shards.empty() ? c : c->shards[k]; }
// a context whose launches leave the sums over rows to an exchange step: a rank of a multi-process run, or a shard of a shell
static inline bool row_sharded(const fh_ctx* c) { return c->comm != nullptr || c->owner != nullptr; }

// ------------------------------------------------------------------------------------------------
// operator forms: what each one serves, stated once
// ------------------------------------------------------------------------------------------------
// A form is c->op plus whether the unknown has columns (c->LB); the DCT operator is one form in both geometries.  Every entry point that accepts
// or refuses a prox kind, a loss or a column count asks a row of kForms, and so does every launch-time backstop; the sentences a caller reads
// stand here, whole, as they always were (the lists in parentheses included: they are behaviour).  A sentence may take the noun as %s.
// What a form can do beyond fwd / adj is a bit of `can`: a row that does not say so is refused by every entry point that asks (check_can), each
// in its own sentence with the row's noun; a new form is refused everywhere until its row says otherwise.  The launchers of a form: kLaunch,
// fh_host_launch.h.
enum { CAN_STEP = 1, CAN_RUN = 2, CAN_SHARD = 4, CAN_ROWS = 8 };      // the one-pass step; the device-side loop; row sharding; dense rows to read
enum { F_NONE, F_DENSE, F_DENSE_MC, F_STENCIL, F_SPARSE, F_SPARSE_MC, F_STENCIL3D, F_QUAD, F_BILINEAR, F_DCT, F_IDENTITY, F_CONV, F_COUNT };
struct OpForm {
  const char* noun;          // as the sentences name it, without its article
  const char* article;       // ... which fh_comm_init puts in front of it
  unsigned can;              // bits of CAN_*
  bool by_columns;           // an entry point that refuses answers with its sentence about the multi-column form, not with the noun's
  const char* no_rows;       // without CAN_ROWS: why fh_get_matrix_rows has nothing to read (nullptr: the entry points' sentences without a noun)
  const char* no_apply;      // fh_apply (noun; nullptr: the form is a linear map)
  unsigned prox;             // bits of FH_PROX_*: the kinds fh_set_prox accepts on this form and a setter of it keeps
  unsigned prox_run;         // ... the kinds its forward launch lets through, where that is another set (0 = the same)
  unsigned losses;           // bits of LOSS_*: what fh_set_loss_* may give it (0: it has no loss to set)
  bool weights;              // fh_set_loss_weights
  bool answers_first;        // fh_set_prox: this form's own sentence comes before the ROWBALL / GROUP ones
  const char* no_prox;       // an unserved kind (%d, noun): fh_set_prox, fh_set_rhs
  const char* no_prox_run;   // ... at launch (nullptr = the same)
  const char* no_loss;       // fh_set_loss_lsq / _logistic: the loss is refused (noun)
  const char* no_loss_run;   // ... at launch (nullptr = the same)
  const char* no_softmax;    // fh_set_loss_softmax
  const char* no_rhs;        // fh_set_rhs (nullptr: this form takes it)
  const char* no_f32;        // float32 storage, refused by the form's setter (entry point, noun; nullptr: the setter does not ask)
  bool gap;                  // fh_dual_gap (csrc/fh_gap.h): x0, g0, z = A x0 and b of this form are what the certificate reads
};
#define KIND(k) (1u << FH_PROX_##k)
#define LOSSBIT(k) (1u << (k))
static const unsigned KINDS_ELEM = KIND(IDENTITY) | KIND(SHRINK) | KIND(NONNEG) | KIND(BOX), KINDS_LEVEL = KIND(LINF) | KIND(L1BALL);
static const unsigned KINDS_ALL = (KIND(NUCBALL) << 1) - 1u;
static const unsigned LOSSES_ELEM = LOSSBIT(LOSS_LSQ) | LOSSBIT(LOSS_LOGISTIC), LOSSES_MC = LOSSBIT(LOSS_LSQ) | LOSSBIT(LOSS_SOFTMAX);
static const unsigned LOSSES_SET = LOSSES_ELEM | LOSSES_MC;      // what fh_set_loss_* can give at all (the quadratic and the bilinear form bring their own)
static const char kNoProxMc[] = "prox kind %d (LINF / L1BALL / TVBALL) has no multi-column form";
static const char kLsqOnly[] = "the %s serves the least-squares loss only (the logistic loss is implemented for the dense and sparse operators)";
static const char kNoLogisticMc[] = "the logistic loss has no multi-column form (fh_set_rhs / fh_set_matrix_csr_rhs)";
static const char kMcLsqOnly[] = "the multi-column form serves the least-squares loss only";
static const char kSoftmaxOps[] = "fh_set_loss_softmax: the softmax loss is implemented for the dense and the sparse operator in multi-column form only "
                                  "(fh_set_matrix + fh_set_rhs, or fh_set_matrix_csr_rhs), not for the stencil, DCT, convolution, identity, quadratic or bilinear operators";
static const char kSoftmaxMc[] = "fh_set_loss_softmax: the softmax loss needs the multi-column form, one column of the unknown per class: call fh_set_rhs (dense operator) "
                                 "or fh_set_matrix_csr_rhs (sparse operator) with L >= 2 first (two classes on a vector unknown: fh_set_loss_logistic)";
static const char kRhsSparse[] = "fh_set_rhs: the sparse operator has no multi-column form through fh_set_rhs: its column count is fixed when it is set (fh_set_matrix_csr_rhs)";
static const char kRhsNone[] = "fh_set_rhs: the %s has no multi-column form";
static const char kF32NoMatrix[] = "%s: float32 storage is a storage mode of a dense matrix; the %s stores no matrix and computes in float64";
static const char kF32HasNo[] = "%s: float32 storage has no %s";
static const char kNoApply[] = "fh_apply: the %s has no linear map to apply (A is the identity; S enters through the smooth term: fh_gradient_at)";
static const OpForm kForms[F_COUNT] = {
  // F_NONE: what an empty context may hold for the operator to come (free_operator drops every other kind); a communicator may come before the operator
  {"operator", "an", CAN_SHARD, false, nullptr, nullptr,
   KINDS_ELEM | KINDS_LEVEL | KIND(TVBALL) | KIND(GROUP), 0, 0, false, false, nullptr, nullptr, "set the operator before the loss", nullptr, nullptr,
   "fh_set_rhs: set the dense operator first (fh_set_matrix / fh_generate_matrix)", nullptr, false},
  // F_DENSE: accepts the TV-ball kind and refuses it at launch; its launch refuses nothing else
  {"dense operator", "a", CAN_STEP | CAN_RUN | CAN_SHARD | CAN_ROWS, false, nullptr, nullptr,
   KINDS_ELEM | KINDS_LEVEL | KIND(TVBALL), KINDS_ALL & ~KIND(TVBALL), LOSSES_ELEM, false, false, nullptr, "TV-ball prox needs the stencil operator", nullptr, nullptr,
   kSoftmaxMc, nullptr, nullptr, true},
  {"dense operator", "a", CAN_ROWS, true, nullptr, nullptr,
   KINDS_ELEM | KIND(GROUP), 0, LOSSES_MC, false, false, kNoProxMc, "prox kind %d has no multi-column form", kNoLogisticMc, kMcLsqOnly, nullptr, nullptr, nullptr, true},
  // F_STENCIL: accepts what the dense form accepts, runs the TV-ball prox or none; fh_run and fh_comm_init let it pass (the loop then finds no kernel for it
  // and says so in its own words; a row-sharded launch refuses)
  {"stencil operator", "a", CAN_STEP | CAN_RUN | CAN_SHARD, false, nullptr, nullptr,
   KINDS_ELEM | KINDS_LEVEL | KIND(TVBALL), KIND(IDENTITY) | KIND(TVBALL), LOSSBIT(LOSS_LSQ), false, false, nullptr,
   "the stencil operator supports the TV-ball prox or no prox (got kind %d)", "the logistic loss is implemented for the dense operator", nullptr, kSoftmaxOps, kRhsNone, nullptr, false},
  {"sparse operator", "a", 0, false, "keeps no dense rows", nullptr,
   KINDS_ELEM, 0, LOSSES_ELEM, false, false, "prox kind %d (LINF / L1BALL / TVBALL / GROUP) is not implemented for the %s", nullptr, nullptr, nullptr, kSoftmaxMc, kRhsSparse,
   "%s: float32 storage is not implemented for the %s", true},
  {"sparse operator", "a", 0, false, "keeps no dense rows", nullptr,
   KINDS_ELEM | KIND(GROUP), 0, LOSSES_MC, false, false, kNoProxMc, "prox kind %d has no multi-column form", kNoLogisticMc, kMcLsqOnly, nullptr, kRhsSparse,
   "%s: float32 storage is not implemented for the %s", true},
  {"3-D stencil operator", "a", 0, false, "keeps no dense rows", nullptr,
   KINDS_ELEM | KIND(TVBALL), 0, LOSSBIT(LOSS_LSQ), false, false, "prox kind %d (LINF / L1BALL / GROUP) is not implemented for the %s", nullptr, kLsqOnly, nullptr, kSoftmaxOps,
   kRhsNone, nullptr, false},
  {"quadratic operator", "a", 0, false, "is not read back (the caller holds Q)", nullptr,
   KINDS_ELEM | KIND(GROUP) | KIND(ROWBALL), 0, 0, false, false, "prox kind %d (LINF / L1BALL / TVBALL) has no quadratic form", nullptr,
   "the quadratic operator carries its own loss (Q and the linear term of fh_set_quadratic): fh_set_loss_lsq / fh_set_loss_logistic do not apply", nullptr, kSoftmaxOps,
   "fh_set_rhs: the column count of a quadratic operator is fixed when it is set (fh_set_quadratic)", kF32HasNo, false},
  {"bilinear operator", "a", 0, false, "is not read back (the caller holds S)", kNoApply,
   KINDS_ELEM | KIND(ROWSPLIT), 0, 0, false, true, "prox kind %d (LINF / L1BALL / TVBALL / GROUP / ROWBALL) has no bilinear form", nullptr,
   "the bilinear operator carries its own loss (S of fh_set_factorization): fh_set_loss_lsq / fh_set_loss_logistic do not apply", nullptr, kSoftmaxOps,
   "fh_set_rhs: the column count of a bilinear operator is fixed when it is set (fh_set_factorization)", kF32HasNo, false},
  {"DCT operator", "a", 0, false, "keeps no dense rows", nullptr,
   KINDS_ELEM | KINDS_LEVEL, 0, LOSSBIT(LOSS_LSQ), false, false, "prox kind %d (TVBALL / GROUP) is not implemented for the %s", nullptr, kLsqOnly, nullptr, kSoftmaxOps, kRhsNone, kF32NoMatrix, true},
  {"identity operator", "the", 0, false, "keeps no matrix", nullptr,
   KINDS_ELEM | KIND(NUCLEAR) | KIND(NUCBALL), 0, LOSSES_ELEM, true, true, "prox kind %d (LINF / L1BALL / TVBALL / GROUP / ROWBALL) is not implemented for the %s",
   "prox kind %d (LINF / L1BALL / TVBALL / GROUP / ROWBALL / ROWSPLIT) is not implemented for the %s", nullptr, nullptr, kSoftmaxOps,
   "fh_set_rhs: the %s has no multi-column form (its unknown is already an (M, N) matrix: fh_set_identity)", kF32NoMatrix, false},
  {"convolution operator", "a", 0, false, "keeps no dense rows", nullptr,
   KINDS_ELEM | KINDS_LEVEL, 0, LOSSBIT(LOSS_LSQ), false, false, "prox kind %d (TVBALL / GROUP) is not implemented for the %s", nullptr, kLsqOnly, nullptr, kSoftmaxOps, kRhsNone, kF32NoMatrix, true},
};
#undef KIND
#undef LOSSBIT
static inline int form_index(const fh_ctx* c) {
  static const int of_op[] = {F_NONE, F_DENSE, F_STENCIL, F_SPARSE, F_STENCIL3D, F_QUAD, F_BILINEAR, F_DCT, F_IDENTITY, F_CONV};      // by OP_*
  const int f = of_op[c->op];
  return c->LB && (f == F_DENSE || f == F_SPARSE) ? f + 1 : f;
}
static inline const OpForm& form_of(const fh_ctx* c) { return kForms[form_index(c)]; }
static inline bool serves_prox(const OpForm& f, int kind) { return kind >= 0 && kind < 32 && (f.prox >> kind & 1u); }
static inline bool runs_prox(const OpForm& f, int kind) { return kind >= 0 && kind < 32 && ((f.prox_run ? f.prox_run : f.prox) >> kind & 1u); }
static inline bool takes_loss(const OpForm& f, int loss) { return loss >= 0 && loss < 32 && (f.losses >> loss & 1u); }
static int refuse_prox(int code, const char* who, const OpForm& f, int kind) {      // f.no_prox behind the entry point's name
  char sentence[384];
  snprintf(sentence, sizeof sentence, "%s%s", who, f.no_prox);
  return fail(code, sentence, kind, f.noun);
}
// the launch-time backstops of launch_fwd_* / launch_adj_* (fh_host_launch.h): what set-up should never have let through
static int check_prox_run(const fh_ctx* c) {
  const OpForm& f = form_of(c);
  return runs_prox(f, c->prox_kind) ? 0 : fail(FH_E_STATE, f.no_prox_run ? f.no_prox_run : f.no_prox, c->prox_kind, f.noun);
}
static int check_loss_run(const fh_ctx* c) {
  const OpForm& f = form_of(c);
  return takes_loss(f, c->loss_kind) ? 0 : fail(FH_E_STATE, f.no_loss_run ? f.no_loss_run : f.no_loss, f.noun);
}
// an entry point beyond fwd / adj on a form whose row lacks `cap`: the entry point's own sentence with the noun (with_article: "a sparse operator"),
// or the one it has for the multi-column form
static int check_can(const fh_ctx* c, unsigned cap, const char* sentence, const char* sentence_columns, bool with_article = false) {
  const OpForm& f = form_of(c);
  if (f.can & cap) return 0;
  if (f.by_columns) return fail(FH_E_STATE, "%s", sentence_columns);
  char name[64];
  snprintf(name, sizeof name, "%s%s%s", with_article ? f.article : "", with_article ? " " : "", f.noun);
  return fail(FH_E_STATE, sentence, name);
}
// a context about to change its operator, or with none: the prox kinds and the loss its next operator cannot be assumed to serve go
static inline void reset_unserved(fh_ctx* c, const OpForm& next) {
  if (!serves_prox(next, c->prox_kind)) { c->prox_kind = FH_PROX_IDENTITY; c->mu = 0.0; }
  if (!(LOSSES_SET >> c->loss_kind & 1u)) c->loss_kind = LOSS_LSQ;
}

static const int kCounterWords = 8192;
enum { CNT_FWD = 0, CNT_ADJ_FIN = 1, CNT_AUX = 2, CNT_FUSED_BAR = 4, CNT_FUSED_ERR = 8, CNT_PROBE = 12, CNT_RUN_BAR = 14, CNT_ADJ_CC = 16,
       CNT_DIAG = kCounterWords - 8 };     // the last 8 words only ever grow: [0] level searches that fell back to one workgroup, [1] ... that found no level (fh_recovered_count)

static inline uint64_t round_up(uint64_t v, uint64_t q) { return (v + q - 1) / q * q; }
// multi-column form: doubles per device row of a vector buffer, columns per host row (both 1 in the vector form)
static inline uint64_t lb_of(const fh_ctx* c) { return c->LB ? c->LB : 1u; }
static inline uint64_t l_of(const fh_ctx* c) { return c->LB ? c->L : 1u; }
static inline uint32_t lb_for(uint32_t L) { return L <= 2 ? 2u : (L <= 4 ? 4u : (L <= 8 ? 8u : 16u)); }      // L columns are kept as LB in {2, 4, 8, 16}

// device scratch that is released on every exit path (the HIP_TRY macros return early)
struct DevBuf {
  double* p = nullptr;
  ~DevBuf() { if (p) (void)hipFree(p); }
};

static int use_device(fh_ctx* c) {
  HIP_TRY(hipSetDevice(c->device));
  return 0;
}

// ---- large frees and the allocations behind them -------------------------------------------------------------------------------------
// The driver clears freed device memory in the background, ~30 ms per GiB on MI355X.  Meanwhile a read-only stream over OTHER memory runs
// 0.7-3 % slow -- and a large allocation made while the clearing is still going on is mapped less favourably FOR ITS WHOLE LIFETIME.  What that costs
// depends on the kernel's access pattern (round 6, profiles/r06_placement.txt): with the rows dealt to the teams in contiguous blocks (rounds 1-5) the
// one-pass kernel ran 9-14 % slow on such a matrix (6 of 6 interleaved cycles: 5.49-5.54 against 4.85-4.89 ms per step, profiles/r06_alloc_settle.txt),
// and just as slow on a matrix that simply got the far part of the device's memory; with the rows dealt cyclically (the default now: the whole grid
// streams one window of the matrix) it does not care: 4.82-4.85 ms right behind a 128 GiB free, waited for or not (3 of 3).  What is left:
//   1. re-use (deterministic: no clearing, no new mapping, no sleep; worth ~1 % and the allocation's time): the matrix block (>= 1 GiB) a context gives up
//      is not returned to the driver but kept -- one block per device -- and handed to the next matrix on that device that fits it and fills at least
//      half of it; fh_release_cached() / fh_alloc_cache(0) return it to the driver.
//   2. settle (OFF by default since the cyclic dealing; fh_alloc_settle(1) for callers that run the blocked dealing or live on K-adj, which still
//      depend on the mapping): a matrix that cannot be served by 1. is allocated only after the device's earlier large frees have presumably been
//      cleared (35 ms per GiB behind the free); fh_alloc_settle_waited reports what it has cost so far.
#include <mutex>
#define FH_MAX_DEVICES 64
static std::atomic<long long> g_clear_until_ns[FH_MAX_DEVICES];       // steady clock, per device
static std::atomic<long long> g_settle_waited_ns{0};
static std::atomic<int> g_settle_on{0};
static std::atomic<int> g_cache_on{1};
static std::atomic<unsigned long long> g_cache_hits{0};
struct CachedBlock { double* p = nullptr; size_t bytes = 0; };
static std::mutex g_cache_mu;
static CachedBlock g_cache[FH_MAX_DEVICES];
static const size_t kSettleMinBytes = (size_t)1 << 30;
static const double kClearNsPerByte = 35.0e6 / (double)((size_t)1 << 30);     // 35 ms per GiB (measured: 2.9 s for 96 GiB)
static long long steady_ns() { return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
static inline int dev_slot(int device) { return device >= 0 && device < FH_MAX_DEVICES ? device : 0; }
static void note_large_free(int device, size_t bytes) {
  if (bytes < kSettleMinBytes) return;
  std::atomic<long long>& until = g_clear_until_ns[dev_slot(device)];
  const long long now = steady_ns(), add = (long long)(kClearNsPerByte * (double)bytes);
  long long cur = until.load();
  while (!until.compare_exchange_weak(cur, std::max(cur, now) + add)) { }
}
static void settle_before_large_alloc(int device, size_t bytes) {
  if (!g_settle_on.load() || bytes < kSettleMinBytes) return;
  const long long wait = g_clear_until_ns[dev_slot(device)].load() - steady_ns();
  if (wait <= 0) return;
  std::this_thread::sleep_for(std::chrono::nanoseconds(wait));
  g_settle_waited_ns.fetch_add(wait);
}
// a context gives up its matrix block: kept for the next matrix on this device (the block it displaces goes back to the driver), or freed
static void release_matrix_block(int device, double* p, size_t bytes) {
  if (!p) return;
  if (bytes >= kSettleMinBytes && g_cache_on.load()) {
    std::lock_guard<std::mutex> lk(g_cache_mu);
    CachedBlock& cb = g_cache[dev_slot(device)];
    if (cb.p) { (void)hipFree(cb.p); note_large_free(device, cb.bytes); }
    cb.p = p; cb.bytes = bytes;
    return;
  }
  (void)hipFree(p);
  note_large_free(device, bytes);
}
// a block for a matrix of `bytes` on `device` (the current device): the kept one if it fits and is at most twice as large, else a fresh one
// behind the settle wait.  *got = the size of the block handed out.
static hipError_t acquire_matrix_block(int device, size_t bytes, double** out, size_t* got) {
  {
    std::lock_guard<std::mutex> lk(g_cache_mu);
    CachedBlock& cb = g_cache[dev_slot(device)];
    if (cb.p && cb.bytes >= bytes && cb.bytes / 2 <= bytes) {
      *out = cb.p; *got = cb.bytes;
      cb = CachedBlock();
      g_cache_hits.fetch_add(1);
      return hipSuccess;
    }
    if (cb.p && bytes >= kSettleMinBytes) {            // it cannot serve this matrix and would only stand in its way: back to the driver
      (void)hipFree(cb.p); note_large_free(device, cb.bytes);
      cb = CachedBlock();
    }
  }
  settle_before_large_alloc(device, bytes);
  *got = bytes;
  return hipMalloc((void**)out, bytes);
}
static void release_cached_blocks(int device /* -1 = all */) {
  std::lock_guard<std::mutex> lk(g_cache_mu);
  for (int d = 0; d < FH_MAX_DEVICES; ++d) {
    if ((device >= 0 && d != device) || !g_cache[d].p) continue;
    (void)hipSetDevice(d);
    (void)hipFree(g_cache[d].p); note_large_free(d, g_cache[d].bytes);
    g_cache[d] = CachedBlock();
  }
}

static void free_vectors(fh_ctx* c) {
  auto fr = [](double*& p) { if (p) { (void)hipFree(p); p = nullptr; } };
  for (int i = 0; i < 2; ++i) { fr(c->P[i]); fr(c->G[i]); fr(c->Z[i]); }
  for (int i = 0; i < 3; ++i) fr(c->X[i]);
  fr(c->xhat); fr(c->xs); fr(c->b); fr(c->zt); fr(c->ZX[0]); fr(c->ZX[1]);
  for (int i = 0; i < 4; ++i) fr(c->T[i]);
}

// every operator setter but fh_set_identity calls this before it frees anything: a weighted problem never silently runs unweighted
static int refuse_weighted(const fh_ctx* c) {
  if (c->loss_w) return fail(FH_E_STATE, "the context holds observation weights (fh_set_loss_weights), which the identity operator alone serves: remove them "
                                         "(fh_set_loss_weights(ctx, NULL), or set the loss again) before another operator is set");
  return 0;
}

static int drop_loss_weights(fh_ctx* c) {
  if (!c->loss_w) return 0;
  HIP_TRY(hipStreamSynchronize(c->stream));
  HIP_TRY(hipFree(c->loss_w));
  c->loss_w = nullptr;
  return 0;
}

static void free_operator(fh_ctx* c) {
  for (fh_ctx* s : c->shards) { (void)hipSetDevice(s->device); free_operator(s); }
  auto fr = [](double*& p) { if (p) { (void)hipFree(p); p = nullptr; } };
  if (c->A && (c->op == OP_DENSE || c->op == OP_QUAD || c->op == OP_BILINEAR)) { release_matrix_block(c->device, c->A, c->a_block_bytes); c->A = nullptr; c->a_block_bytes = 0; }
  fr(c->A);
  for (SpMatP& a : c->sp) {
    if (a.ptr) (void)hipFree((void*)a.ptr);
    if (a.idx) (void)hipFree((void*)a.idx);
    if (a.val) (void)hipFree((void*)a.val);
    if (a.part) (void)hipFree((void*)a.part);
    if (a.longrows) (void)hipFree((void*)a.longrows);
    a = SpMatP();
  }
  fr(c->sp_r); c->nnz = 0;
  fr(c->cn2); c->cn2_held = false;
  for (d2** q : {&c->dct_tw, &c->dct_pw, &c->dct_w0, &c->dct_w1}) if (*q) { (void)hipFree(*q); *q = nullptr; }
  for (d2** q : {&c->dct2_tw, &c->dct2_pw}) if (*q) { (void)hipFree(*q); *q = nullptr; }
  fr(c->dct_diag); fr(c->dct2_w0); fr(c->dct2_w1); c->dct2 = false;
  fr(c->conv_diag);
  fr(c->nuc_w); fr(c->nuc_phi); fr(c->nuc_scal);
  if (c->nuc_cnt) { (void)hipFree(c->nuc_cnt); c->nuc_cnt = nullptr; }
  if (c->nuc_host) { (void)hipHostFree(c->nuc_host); c->nuc_host = nullptr; }
  c->id_M = c->id_N = 0;
  fr(c->loss_w);
  free_vectors(c);
  c->L = c->LB = 0;                  // a new operator starts in the vector form
  reset_unserved(c, kForms[F_NONE]);      // ... and leaves behind the loss a form brought with it and the prox kinds one form alone serves
  fr(c->bl_part); c->bl_part_bytes = 0; c->bl_have_grad = false; c->bl_m = c->bl_n = 0;
  fr(c->ws); c->ws_bytes = 0;
  fr(c->slotbuf); c->slotbuf_bytes = 0; c->slots_sig = 0;
  c->op = OP_NONE; c->has_b = false;
}

static int alloc_zero(fh_ctx* c, double** p, uint64_t elems) {
  HIP_TRY(hipMalloc((void**)p, elems * sizeof(double)));
  HIP_TRY(hipMemsetAsync(*p, 0, elems * sizeof(double), c->stream));
  return 0;
}

// stencil_pair: with the 2-D stencil operator's two extra m-side buffers (the extrapolated image of its accelerated step)
static int alloc_vectors(fh_ctx* c, bool stencil_pair = false) {
  const uint64_t nvl = c->nv * lb_of(c), mvl = c->mv * lb_of(c);
  // +16 slack doubles on the n-side so sharded runs can append scalars to the all-reduce buffer
  for (int i = 0; i < 2; ++i) {
    FH_TRY(alloc_zero(c, &c->P[i], nvl + 16));
    FH_TRY(alloc_zero(c, &c->G[i], nvl + 16));
    FH_TRY(alloc_zero(c, &c->Z[i], mvl + 16));
  }
  FH_TRY(alloc_zero(c, &c->xhat, nvl + 16));
  if (c->LB && !c->sp[0].ptr) FH_TRY(alloc_zero(c, &c->xs, nvl + 16));      // (the sparse gather reads the row-major xprox itself)
  for (int i = 0; i < 3; ++i) FH_TRY(alloc_zero(c, &c->X[i], nvl + 16));
  for (int i = 0; i < 4; ++i) FH_TRY(alloc_zero(c, &c->T[i], nvl + 16));
  FH_TRY(alloc_zero(c, &c->b, mvl + 16));
  FH_TRY(alloc_zero(c, &c->zt, mvl + 16));
  if (stencil_pair) { FH_TRY(alloc_zero(c, &c->ZX[0], mvl + 16)); FH_TRY(alloc_zero(c, &c->ZX[1], mvl + 16)); }
  c->pc = c->gc = c->zc = c->zxc = 0;
  c->xi = 0; c->ti = 1; c->bi = 0;
  c->zcur = nullptr;
  return 0;
}

static int ensure_ws(fh_ctx* c, size_t bytes) {
  if (bytes <= c->ws_bytes) return 0;
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (c->ws) { HIP_TRY(hipFree(c->ws)); c->ws = nullptr; c->ws_bytes = 0; }
  bytes = round_up(bytes, 1 << 20);
  HIP_TRY(hipMalloc((void**)&c->ws, bytes));
  c->ws_bytes = bytes;
  return 0;
}

// ---- timing helpers ------------------------------------------------------------------------------
// (timing_skip_kernels: a block of a same-device multi-block context that is not the sampled one -- fh_timing_enable)
static inline bool t_on(fh_ctx* c, int k) { return c->timing && !(c->timing_skip_kernels && k != FH_K_COMM); }
// read a recorded pair; wait = true: wait for its stop event first (only fh_timing_get and a pair reused before it completed need that)
static void t_harvest(fh_ctx* c, int k, int s, bool wait) {
  if (!c->ev_pending[k][s]) return;
  float ms = 0.f;
  hipError_t e = hipEventElapsedTime(&ms, c->ev[k][s][0], c->ev[k][s][1]);
  if (e == hipErrorNotReady) {
    (void)hipGetLastError();
    if (!wait) return;
    (void)hipEventSynchronize(c->ev[k][s][1]);
    e = hipEventElapsedTime(&ms, c->ev[k][s][0], c->ev[k][s][1]);
  }
  if (e == hipSuccess) { c->tot_ms[k] += ms; c->launches[k] += 1; }
  else (void)hipGetLastError();
  c->ev_pending[k][s] = false;
}
static inline void t_begin(fh_ctx* c, int k) {
  c->seq_wait = 0;                   // (every launcher passes here: only the LAST launch before collect_scalars may offer a sequence number)
  if (t_on(c, k)) {
    const int s = c->ev_cur[k] ^ 1;
    t_harvest(c, k, s, true);
    c->ev_cur[k] = s;
    (void)hipEventRecord(c->ev[k][s][0], c->stream);
  }
}
static inline void t_end(fh_ctx* c, int k) {
  if (t_on(c, k)) { (void)hipEventRecord(c->ev[k][c->ev_cur[k]][1], c->stream); c->ev_pending[k][c->ev_cur[k]] = true; }
}
// the sequence number the next launch's finaliser is to publish (0 = none: the caller will synchronise the stream)
static inline unsigned seq_offer(fh_ctx* c) {
  if (!c->seq_poll || !c->shards.empty() || c->comm != nullptr || c->owner != nullptr) return 0u;
  c->seq = c->seq + 1u ? c->seq + 1u : 1u;
  c->seq_wait = c->seq;
  return c->seq;
}
static int finish(fh_ctx* c) {   // synchronise the stream and harvest pending event pairs
  if (!c->shards.empty()) {        // shell: all shards (an emulated group shares one stream; its first shard's sync covers the rest)
    for (fh_ctx* s : c->shards) { HIP_TRY(hipSetDevice(s->device)); FH_TRY(finish(s)); }
    return 0;
  }
  c->seq_wait = 0;
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (c->timing) {
    for (int k = 0; k < FH_NKERNELS; ++k) { t_harvest(c, k, 0, true); t_harvest(c, k, 1, true); }
  }
  return 0;
}
// Wait until the scalar block of the latest launch is on the host: by its sequence number when the launch publishes one (the host
// returns ~5 us before the launch's completion signal would have let it; what follows on the stream is ordered behind the launch as
// always), else -- or if the stream goes idle without the number having arrived, which a healthy launch cannot do -- by synchronising.
static int wait_scalars(fh_ctx* c) {
  const unsigned want = c->seq_wait;
  if (!want) return finish(c);
  c->seq_wait = 0;
  volatile unsigned* word = reinterpret_cast<volatile unsigned*>(c->hscal + FH_SEQ_SLOT);
  for (unsigned spins = 1;; ++spins) {
    if (*word == want) return 0;
    if ((spins & 0xFFFu) == 0u) {                            // every few tens of microseconds: is the stream still busy at all?
      const hipError_t q = hipStreamQuery(c->stream);
      if (q == hipSuccess) { if (*word == want) return 0; return finish(c); }     // (idle: the block is as complete as it will get)
      if (q != hipErrorNotReady) return fail((int)q, "hipStreamQuery failed while waiting for a launch: %s", hipGetErrorString(q));
      (void)hipGetLastError();
    }
    __builtin_ia32_pause();
  }
}

// Where kernels write the FH_S_* block: straight into the mapped host block on one GPU (no D2H copy, the
// stream sync alone publishes it); device memory when row-sharded, because RCCL reduces scalars in place.
static inline double* scalar_out(fh_ctx* c) { return row_sharded(c) ? c->dscal : c->hscal_dev; }

// row-sharded runs: the block lives in device memory (RCCL reduces into it); a 16-lane kernel forwards it to the mapped
// host block -- a hipMemcpyAsync D2H of 128 bytes costs ~10 us more per iteration than this launch
__global__ void k_forward_scalars(const double* src, double* dst) {
  if (threadIdx.x < FH_NSCALARS) dst[threadIdx.x] = src[threadIdx.x];
}

// The scalar block's way back, in two halves so that a step can be issued now and waited for later (fh_step_begin / fh_step_end):
// issue_scalars enqueues what is still missing (row-sharded contexts forward the block from device memory to the mapped host block)
// and closes the host-issue stopwatch; collect_scalars is the call's ONE host synchronisation (per device of a shell) and the copy out.
static int issue_scalars(fh_ctx* c) {
  for (int k = 0; k < nshards(c); ++k) {
    fh_ctx* s = shard_of(c, k);
    const bool mirrored = s->scal_mirrored;
    s->scal_mirrored = false;
    if (row_sharded(s) && !mirrored) {
      HIP_TRY(hipSetDevice(s->device));
      k_forward_scalars<<<dim3(1), dim3(64), 0, s->stream>>>(s->dscal, s->hscal_dev);
      HIP_TRY(hipGetLastError());
    }
  }
  if (c->issue_open) {             // everything of this call has been issued: what follows is the wait
    c->host_issue_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - c->issue_t0).count();
    c->host_issue_calls += 1;
    c->issue_open = false;
  }
  return 0;
}
static int collect_scalars(fh_ctx* c, double* scalars) {
  FH_TRY(c->shards.empty() ? wait_scalars(c) : finish(c));               // ONE host wait per call (per device of a shell)
  // every shard holds the same block: each entry is either a sum over all shards or computed from replicated vectors
  fh_ctx* s0 = shard_of(c, 0);
  if (scalars) memcpy(scalars, s0->hscal, FH_NSCALARS * sizeof(double));
  // The clipping level of the l-infinity prox / l1-ball projection travels with every forward launch (FH_S_ALPHA).  NaN = the level
  // search could not finish (csrc/fh_prox.h: a hand-off timed out AND the single-workgroup fall-back was not available); prox_scalar
  // has propagated it into every output of the launch.  Typed, so that a caller can tell it from a device fault.
  if ((s0->prox_kind == FH_PROX_LINF || s0->prox_kind == FH_PROX_L1BALL) && s0->hscal[FH_S_ALPHA] != s0->hscal[FH_S_ALPHA])
    return fail(FH_E_TIMEOUT, "the clipping-level search of the l-infinity prox / l1-ball projection did not finish (hand-off between its workgroups "
                              "timed out and no fall-back was possible): the step's outputs are NaN");
  return 0;
}
static int fetch_scalars(fh_ctx* c, double* scalars) {
  FH_TRY(issue_scalars(c));
  return collect_scalars(c, scalars);
}

// ---- sums over the row blocks ------------------------------------------------------------------------------------------
// out[i] = ((v0[i] + v1[i]) + v2[i]) + ... written back to every shard's buffer: the in-library, fixed-order replacement for the
// all-reduce when several shards live on ONE device (device ids repeat; all shards share a stream, so plain ordering suffices)
struct SumShardsP { double* v[FH_MAX_SHARDS]; int n; };
__global__ __launch_bounds__(FH_WG) void k_sum_shards(const SumShardsP p, uint64_t count) {
  for (uint64_t i = (uint64_t)blockIdx.x * FH_WG + threadIdx.x; i < count; i += (uint64_t)gridDim.x * FH_WG) {
    double acc = p.v[0][i];
    for (int k = 1; k < p.n; ++k) acc += p.v[k][i];
    for (int k = 0; k < p.n; ++k) p.v[k][i] = acc;
  }
}

// Sum `count` doubles at sel(shard) -- and, in the same exchange, `count2` doubles at sel2(shard) -- over all row blocks, in place,
// on every shard:
//   plain context with a communicator (one process per GPU) -> ncclAllReduce on its stream;
//   shell over distinct devices -> one grouped ncclAllReduce per shard (ncclCommInitAll communicators, one host thread);
//   shell over a repeated device -> k_sum_shards;      plain context without a communicator -> nothing to do.
template <typename Sel, typename Sel2>
static int sum_over_shards(fh_ctx* c, Sel sel, size_t count, Sel2 sel2, size_t count2) {
  if (c->shards.empty()) {
    if (!c->comm) return 0;
    t_begin(c, FH_K_COMM);
    // (an error inside a group must still close it: the thread's group depth would otherwise stay open and every later collective,
    // the fallback path's included, would be queued and never run)
    if (count2) NCCL_TRY(g_rccl.GroupStart());
    int r1 = g_rccl.AllReduce(sel(c), sel(c), count, kNcclFloat64, kNcclSum, c->comm, c->stream);
    if (count2) {
      if (r1 == 0) r1 = g_rccl.AllReduce(sel2(c), sel2(c), count2, kNcclFloat64, kNcclSum, c->comm, c->stream);
      const int r2 = g_rccl.GroupEnd();
      if (r1 == 0) r1 = r2;
    }
    if (r1 != 0) return fail(20000 + r1, "ncclAllReduce over the row blocks failed: %s", g_rccl.GetErrorString(r1));
    t_end(c, FH_K_COMM);
    return 0;
  }
  if (c->emulated) {
    fh_ctx* s0 = c->shards[0];
    HIP_TRY(hipSetDevice(s0->device));
    t_begin(s0, FH_K_COMM);
    for (int pass = 0; pass < (count2 ? 2 : 1); ++pass) {
      SumShardsP sp;
      sp.n = (int)c->shards.size();
      for (int k = 0; k < sp.n; ++k) sp.v[k] = pass ? sel2(c->shards[k]) : sel(c->shards[k]);
      const uint64_t cnt = pass ? count2 : count;
      const unsigned grid = (unsigned)std::min<uint64_t>((cnt + FH_WG - 1) / FH_WG, 1024);
      k_sum_shards<<<dim3(grid), dim3(FH_WG), 0, s0->stream>>>(sp, cnt);
    }
    t_end(s0, FH_K_COMM);
    HIP_TRY(hipGetLastError());
    return 0;
  }
  for (fh_ctx* s : c->shards) { HIP_TRY(hipSetDevice(s->device)); t_begin(s, FH_K_COMM); }
  NCCL_TRY(g_rccl.GroupStart());
  int rg = 0;                                            // first error; the group is closed whatever happens
  for (fh_ctx* s : c->shards) {
    if (rg == 0) rg = g_rccl.AllReduce(sel(s), sel(s), count, kNcclFloat64, kNcclSum, s->comm, s->stream);
    if (rg == 0 && count2) rg = g_rccl.AllReduce(sel2(s), sel2(s), count2, kNcclFloat64, kNcclSum, s->comm, s->stream);
  }
  { const int re = g_rccl.GroupEnd(); if (rg == 0) rg = re; }
  if (rg != 0) return fail(20000 + rg, "grouped ncclAllReduce over the row blocks failed: %s", g_rccl.GetErrorString(rg));
  for (fh_ctx* s : c->shards) { HIP_TRY(hipSetDevice(s->device)); t_end(s, FH_K_COMM); }
  return 0;
}
template <typename Sel>
static int sum_over_shards(fh_ctx* c, Sel sel, size_t count) {
  return sum_over_shards(c, sel, count, [](fh_ctx*) { return (double*)nullptr; }, 0);
}

// ---- vector access --------------------------------------------------------------------------------
static double* vec_ptr(fh_ctx* c, int which, uint64_t* len) {
  const bool acc = c->last_accel;
  *len = c->n * l_of(c);             // host length: (n, L) row-major in multi-column form
  // the stencil path never materialises the gradient or xhat (fh_tv.h): those ids are not addressable there
  if (c->op == OP_STENCIL && (which == FH_VEC_G0 || which == FH_VEC_G1 || which == FH_VEC_XHAT)) return nullptr;
  switch (which) {
    case FH_VEC_X0: return c->X[c->xi];
    case FH_VEC_G0: return c->G[c->gc];
    case FH_VEC_XHAT: return c->xhat;
    case FH_VEC_XPROX: return c->P[c->pc ^ 1];
    case FH_VEC_X1: return acc ? c->X[c->ti] : c->P[c->pc ^ 1];
    case FH_VEC_G1: return c->G[c->gc ^ 1];
    case FH_VEC_BEST: return c->X[c->bi];
    case FH_VEC_B: *len = c->m * l_of(c); return c->b;
    case FH_VEC_Z: *len = c->m * l_of(c); return c->Z[c->zc ^ 1];
    case FH_VEC_T0: case FH_VEC_T1: case FH_VEC_T2: case FH_VEC_T3: return c->T[which - FH_VEC_T0];
    default: return nullptr;
  }
}

// `rows` logical rows between a contiguous row-major host array ((rows, L) in multi-column form) and a device buffer ((.., LB), whose padding
// columns are never touched and therefore stay zero).  The multi-column form moves the array as ONE contiguous copy to / from the workspace
// and re-strides it on the device (a strided copy of rows of 8..128 bytes would be one small transfer per row); everything is ordered on
// the context's stream, like every other user of the workspace.
static __global__ __launch_bounds__(FH_WG) void k_mc_restride(double* dst, uint32_t dst_ld, const double* src, uint32_t src_ld, uint32_t L, uint64_t count) {
  for (uint64_t t = (uint64_t)blockIdx.x * FH_WG + threadIdx.x; t < count; t += (uint64_t)gridDim.x * FH_WG)
    dst[t / L * dst_ld + t % L] = src[t / L * src_ld + t % L];
}
static int copy_in(fh_ctx* c, double* dev, const double* host, uint64_t rows) {
  if (!c->LB) { HIP_TRY(hipMemcpyAsync(dev, host, rows * sizeof(double), hipMemcpyHostToDevice, c->stream)); return 0; }
  const uint64_t count = rows * c->L;
  FH_TRY(ensure_ws(c, count * sizeof(double)));
  HIP_TRY(hipMemcpyAsync(c->ws, host, count * sizeof(double), hipMemcpyHostToDevice, c->stream));
  k_mc_restride<<<dim3((unsigned)std::min<uint64_t>((count + FH_WG - 1) / FH_WG, 4096)), dim3(FH_WG), 0, c->stream>>>(dev, c->LB, c->ws, c->L, c->L, count);
  HIP_TRY(hipGetLastError());
  return 0;
}
static int copy_out(fh_ctx* c, double* host, const double* dev, uint64_t rows) {
  if (!c->LB) { HIP_TRY(hipMemcpyAsync(host, dev, rows * sizeof(double), hipMemcpyDeviceToHost, c->stream)); return 0; }
  const uint64_t count = rows * c->L;
  FH_TRY(ensure_ws(c, count * sizeof(double)));
  k_mc_restride<<<dim3((unsigned)std::min<uint64_t>((count + FH_WG - 1) / FH_WG, 4096)), dim3(FH_WG), 0, c->stream>>>(c->ws, c->L, dev, c->LB, c->L, count);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(host, c->ws, count * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  return 0;
}

// the operands of a forward launch (launch_fwd_*, op_fwd: fh_host_launch.h), as AdjIO holds the adjoint's.  mode 0: z = A prox(x0 - tau g0),
// with xhat, xp and the n-side sums; mode 1: z = A x0.  sub_b: subtract b and sum the loss
struct FwdIO {
  int mode; double tau;
  const double* x0; const double* g0; const double* xacc0; double* xhat; double* xp; double* z; int sub_b;
};
// "apply to this vector": z = A x (the solver-state operands: solver_fwd_io, fh_host_launch.h)
static inline FwdIO apply_fwd_io(const double* x, double* z, int sub_b) { return FwdIO{1, 0.0, x, nullptr, nullptr, nullptr, nullptr, z, sub_b}; }
static int launch_fwd_tv(fh_ctx* c, const FwdIO& io);      // fh_host_launch.h
// z = div(x) into `z` (plain stencil pass; the scalar block is scratch afterwards)
static int tv_image(fh_ctx* c, const double* x, double* z) { return launch_fwd_tv(c, apply_fwd_io(x, z, 0)); }
// the two-launch stencil kernels read the stored image of x0: bring it up to date after z-free steps
static int tv_refresh_zcur(fh_ctx* c) {
  if (c->op != OP_STENCIL || !c->zcur_stale) return 0;
  FH_TRY(tv_image(c, c->X[c->xi], c->Z[c->zc]));
  c->zcur = c->Z[c->zc];
  c->zcur_stale = false;
  return 0;
}

// ---- lazily-kept stencil iterate (one-pass FISTA) ---------------------------------------------------
static inline double* nq(fh_ctx* c, int i) { return i < 3 ? c->X[i] : c->P[i - 3]; }
static inline double* mq(fh_ctx* c, int i) { return i < 2 ? c->Z[i] : c->ZX[0]; }
static void lazy_pick_targets(fh_ctx* c) {
  for (int k = 0; k < 5; ++k) if (k != c->lq1 && k != c->lq0 && k != c->lb1 && k != c->lb0) { c->lqn = k; break; }
  for (int k = 0; k < 3; ++k) if (k != c->lz1 && k != c->lz0) { c->lzn = k; break; }
}
static int not_lazy(fh_ctx* c, const char* what) {
  if (c->lazy) return fail(FH_E_STATE, "%s: this solve runs the one-pass accelerated stencil step (fh_step_accel), whose iterate is kept "
                           "in extrapolated-on-the-fly form; call fh_init before switching kernels", what);
  return 0;
}
// device pointer for fh_get_vector while the iterate is lazy: x0 / x1 / best are materialised into scratch T[2]
static int lazy_vec(fh_ctx* c, int which, double** out) {
  int a = -1, b = -1; double coef = 0.0;
  switch (which) {
    case FH_VEC_X0: case FH_VEC_X1: a = c->lq1; b = c->lq0; coef = c->lc; break;
    case FH_VEC_BEST: a = c->lb1; b = c->lb0; coef = c->lbc; break;
    case FH_VEC_XPROX: *out = nq(c, c->lqn); return 0;
    default: *out = nullptr; return 0;
  }
  const unsigned grid = (unsigned)std::min<uint64_t>((c->n + FH_WG - 1) / FH_WG, 4096);
  k_extrapolate_vec<<<dim3(grid), dim3(FH_WG), 0, c->stream>>>(c->T[2], nq(c, a), nq(c, b), coef, c->n);
  HIP_TRY(hipGetLastError());
  *out = c->T[2];
  return 0;
}


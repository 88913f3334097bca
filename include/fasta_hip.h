/* fasta_hip.h -- C ABI of libfasta_hip.so: the MI355X (gfx950) forward-backward-splitting hot path.
 *
 * The reference (phasepack/fasta-python) is pure Python and has no FFI; its plugin boundary for this
 * path is the Python call fasta.fasta(A[, At], f, gradf, g, proxg, x0, ...) (fasta/__init__.py:38-53).
 * This header is the boundary a binding for that call sits on: plain pointers and sizes, no torch
 * types.  Each entry point cites the reference arithmetic it replaces (paths relative to the
 * reference tree).  The ctypes binding that consumes it is fasta_python_amd/hip.py; INTEGRATION.md
 * shows the stub a reference maintainer would add.
 *
 * Conventions
 *   - every function returns 0 on success, otherwise a non-zero code (hipError_t / ncclResult_t
 *     value, or FH_E_*); fh_last_error() then describes it (thread-local string).
 *   - a context is NOT thread-safe; calls are synchronous from the caller's view (fh_fwd / fh_adj
 *     return once their scalars are on the host).  A context drives one device (fh_create), or --
 *     fh_create_ex with ndev > 1 -- several row blocks of A in ONE process from one host thread.
 *   - the library copies on every set_* and never keeps a host pointer past the call; it owns all
 *     device memory behind fh_ctx until fh_destroy.
 *   - all arithmetic is IEEE float64 (the reference is float64 throughout).
 */
#ifndef FASTA_HIP_H
#define FASTA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct fh_ctx fh_ctx;

#define FH_E_ARG      10001   /* bad argument / shape mismatch                      */
#define FH_E_STATE    10002   /* call out of order (e.g. fh_fwd before fh_set_*)     */
#define FH_E_RCCL     10003   /* librccl could not be loaded / symbol missing        */
#define FH_E_TIMEOUT  10004   /* a bounded in-launch hand-off ran out (workgroups not co-resident?) and no fall-back inside the library
                                 could finish the call: the clipping-level search of FH_PROX_LINF / FH_PROX_L1BALL (its outputs are NaN,
                                 never a finite wrong prox), or a grid barrier of fh_run's persistent launch (the state of the last
                                 completed iteration is adopted and the completed history returned: continue with fh_iterate / fh_step) */
#define FH_E_NOCONV   10005   /* the block-Jacobi decomposition behind FH_PROX_NUCLEAR / FH_PROX_NUCBALL still rotated after 30 sweeps: xprox is filled with NaN,
                                 never a finite wrong prox                                                                             */

/* prox operators g(x) <-> proxg(x, t)                                                   */
enum fh_prox_kind {
  FH_PROX_IDENTITY = 0,  /* g = None branch, fasta/__init__.py:88-90                     */
  FH_PROX_SHRINK   = 1,  /* proximal.shrink(x, t*mu), fasta/proximal.py:58-67            */
  FH_PROX_NONNEG   = 2,  /* np.maximum(x, 0), examples/nn_least_squares.py:42            */
  FH_PROX_LINF     = 3,  /* proximal.project_Linf_ball(x, t*mu), fasta/proximal.py:12-31 */
  FH_PROX_L1BALL   = 4,  /* proximal.project_L1_ball(x, mu), fasta/proximal.py:34-41     */
  FH_PROX_TVBALL   = 5,  /* per-pixel 2-vector / max(norm,1), examples/tv_denoising.py:89-96 */
  FH_PROX_BOX      = 6,  /* clip to [lo, hi], examples/svm.py:71                         */
  FH_PROX_GROUP    = 7,  /* row-wise l2 shrink of an (n, L) matrix, examples/mmv.py:51-59: with nu = ||xhat_j||_2 over the L entries of row j,
                            xprox_j = xhat_j * max(nu - t*mu, 0) / (nu + (nu == 0)).  Multi-column form only (fh_set_rhs, fh_set_matrix_csr_rhs).  FH_S_GSUM /
                            FH_S_GSUM_ADJ then carry sum_j ||xprox_j||_2 (of x1), so that g = mu * gsum; FH_S_GMAX is unchanged.            */
  FH_PROX_ROWBALL  = 8,  /* row-wise projection of an (n, L) matrix, examples/max_norm.py:53-59: with nu = ||xhat_j||_2 over the L entries of row j,
                            xprox_j = (mu * xhat_j) / (max(nu, mu) + (nu == 0)) -- independent of the step; g = 0, so the objective adds nothing for it.
                            Served by the quadratic operator only (fh_set_quadratic); every other operator refuses it with a sentence.        */
  FH_PROX_NUCLEAR  = 10, /* singular-value soft-threshold of an (M, N) matrix, examples/logistic_matrix_completion.py: xprox = U max(S - t*mu, 0) V^T of
                            xhat = U S V^T, by block one-sided Jacobi on the device (csrc/fh_nuclear.h).  FH_S_GSUM = sum max(sigma_i - t*mu, 0), the nuclear
                            norm of xprox; FH_S_GMAX = max max(sigma_i - t*mu, 0), its spectral norm -- which is what the example's g evaluates
                            (la.norm(np.diag(s), 1) is the induced 1-norm of a diagonal matrix: its largest entry); FH_S_ALPHA = the rank kept.  Served by the identity operator only (fh_set_identity); set by fh_set_prox (objective
                            = 1) or fh_set_prox_nuclear.                                                                                          */
  FH_PROX_NUCBALL  = 11, /* Euclidean projection of an (M, N) matrix onto the nuclear-norm ball { ||X||_* <= mu }: xprox = U max(S - theta, 0) V^T with
                            max(S - theta, 0) = proximal.project_L1_ball(S, mu) -- theta = max(0, max_k (c_k - mu) / k) over the running sums c_k of the
                            singular values in descending order.  Independent of the step; g = 0, so no values-only decomposition ever runs for it
                            (FH_S_GSUM of fh_init and FH_S_GSUM_ADJ of an accelerated fh_adj hold NaN: not evaluated).  After a forward launch FH_S_GSUM =
                            the nuclear norm of xprox (<= mu), FH_S_GMAX its spectral norm, FH_S_ALPHA the rank kept.  The decomposition, its bounds
                            (min(M, N) <= 1024), FH_E_NOCONV, fh_nuclear_info and fh_nuclear_shape* are FH_PROX_NUCLEAR's; one more one-workgroup launch
                            finds theta (csrc/fh_nuclear.h: k_nuc_ball).  Served by the identity operator only; set by fh_set_prox, mu = radius >= 0.     */
  FH_PROX_ROWSPLIT = 9  /* two elementwise kinds on one (n, L) matrix, examples/nn_factorization.py:60-61: rows [0, split) take one kind with its own
                            parameters (IDENTITY, SHRINK, NONNEG or BOX), rows [split, n) another (IDENTITY, NONNEG or BOX), each half bit for bit what
                            that kind gives alone.  Set by fh_set_prox_split, never by fh_set_prox.  FH_S_GSUM / FH_S_GSUM_ADJ sum |x| over the TOP rows
                            only, so that g = mu_top * gsum (fh_init takes FH_S_GMAX over the same rows; no kind served here uses it).  Served by the bilinear operator only (fh_set_factorization); every other operator
                            refuses it with a sentence.                                                                                          */
};

/* device vectors addressable through fh_set_vector / fh_get_vector                      */
enum fh_vec {
  FH_VEC_X0 = 0,    /* current iterate x0 (n)            fasta/__init__.py:176            */
  FH_VEC_G0 = 1,    /* gradient at x0: A^H grad f(A x0)  :177                             */
  FH_VEC_XHAT = 2,  /* forward point x0 - tau*g0         :181                             */
  FH_VEC_XPROX = 3, /* prox output (pre-acceleration x1) :184                             */
  FH_VEC_X1 = 4,    /* next iterate (post-acceleration)  :242                             */
  FH_VEC_G1 = 5,    /* next gradient                     :248                             */
  FH_VEC_BEST = 6,  /* best-quality iterate so far       :298-300                         */
  FH_VEC_B = 7,     /* least-squares target b (m)        examples/sparse_least_squares.py:41 */
  FH_VEC_Z = 8,     /* z1 = A xprox (m)                  :187                             */
  FH_VEC_T0 = 9, FH_VEC_T1 = 10, FH_VEC_T2 = 11, FH_VEC_T3 = 12   /* n-length scratch     */
};

/* layout of the scalar block written by fh_init / fh_fwd / fh_adj (FH_NSCALARS doubles)  */
enum fh_scalar {
  FH_S_FSQ = 0,     /* ||z1 - b||^2 ; f1 = .5*sqrt(.)**2      :188                        */
  FH_S_DXG0 = 1,    /* <Dx, g0>                                 :200                        */
  FH_S_DX2 = 2,     /* ||Dx||^2 , Dx = xprox - x0               :200, :258, :272            */
  FH_S_XH2 = 3,     /* ||xprox - xhat||^2 (normaliser, no accel):274                        */
  FH_S_G02 = 4,     /* ||g0||^2                                 :274                        */
  FH_S_GSUM = 5,    /* sum |xprox_i|   (g for shrink = mu*this) examples/sparse_least_squares.py:43 */
  FH_S_GMAX = 6,    /* max |xprox_i|   (g for linf  = mu*this)  examples/democratic_representation.py:41 */
  FH_S_RDOT = 7,    /* (x0 - xprox).(xprox - xacc0)  restart    :231                        */
  FH_S_DXDG = 8,    /* <Dx, Dg>, Dg = g1 + (xhat - x0)/tau      :254-255                    */
  FH_S_DG2 = 9,     /* ||Dg||^2                                 :260                        */
  FH_S_FSQ_ADJ = 10,/* ||z1' - b||^2 at the extrapolated z1'    :243-245                    */
  FH_S_XH2_ADJ = 11,/* ||x1 - xhat||^2 with extrapolated x1     :274                        */
  FH_S_GSUM_ADJ = 12, FH_S_GMAX_ADJ = 13,   /* g terms at the extrapolated x1 :285           */
  FH_S_ALPHA = 14,  /* threshold level used by LINF / L1BALL prox (diagnostic)              */
  FH_NSCALARS = 16
};

/* FH_K_HOST_ISSUE is not a kernel: fh_timing_get reports under it the HOST time a one-pass step of the dense operator (fh_step /
 * fh_step_accel) spends issuing its launches and exchanges -- from the call's entry to the start of its one final synchronisation --
 * and the number of such calls: what one host thread pays to drive all the row blocks of a multi-device context per iteration.   */
/* FH_K_LEVEL: the clipping-level search that precedes every forward launch of the LINF / L1BALL prox kinds (csrc/fh_prox.h). */
enum fh_kernel_id { FH_K_FWD = 0, FH_K_ADJ = 1, FH_K_AUX = 2, FH_K_COMM = 3, FH_K_FUSED = 4, FH_K_HOST_ISSUE = 5, FH_K_LEVEL = 6, FH_NKERNELS = 7 };

enum fh_tuning_key {
  FH_TUNE_FWD_ROWS = 0,      /* rows per workgroup pass in K-fwd: 4, 8, 16 (0 = auto)        */
  FH_TUNE_FWD_GRID_CAP = 1,  /* max workgroups of K-fwd (0 = auto: 1024, grid-stride over row groups) */
  FH_TUNE_ADJ_SLAB_ROWS = 2, /* rows per K-adj slab (multiple of 8; 0 = auto)               */
  FH_TUNE_ADJ_CPT = 3,       /* 16-byte column pairs per thread in K-adj: 1, 2, 4 (0 = auto) */
  FH_TUNE_LD_PAD = 4,        /* extra doubles appended to each device row of A (multiple of 16; set before the matrix) */
  FH_TUNE_NT_LOADS = 5,      /* K-fwd / K-adj / the device loop: 1 = stream A with non-temporal loads, 0 = default cache policy; unset = auto: plain
                                loads for a matrix of at most 256 MiB (it stays in the last-level cache between launches), non-temporal above  */
  FH_TUNE_TV_U = 6,          /* stencil kernels: rows of loads per trip and lane (2, 4, 8; 0 = auto)  */
  FH_TUNE_TV_ROWS = 7,       /* stencil kernels: image rows per workgroup (0 = auto)                 */
  FH_TUNE_TV_NT = 8,         /* stencil kernels: 0 = default, 1 = non-temporal loads and stores (two-launch kernels and the z-streaming
                                one-pass kernels; the z-free one-pass sweep never loads non-temporally: its halo columns and rows are
                                re-read through L2), 2 = non-temporal stores (the z-free sweep's default), 3 = plain accesses      */
  FH_TUNE_FUSED_VARIANT = 9, /* fused one-pass kernel: scheduling variant bits (see csrc/fh_fused.h: 2 = team members on one XCD, 4 = no
                                sleep between polls, 8 / 16 = A/B team shapes, 32 = rows dealt cyclically; default 2 | 32); other bits are FH_E_ARG */
  /* key 10 (the round-1 one-pass stencil kernels that stream z) is only present in -DFH_EXPERIMENTAL builds                    */
  FH_TUNE_TV_PIPE = 11,      /* z-free one-pass stencil sweep: 1 = load a trip of FH_TUNE_TV_U rows, consume it; 3 (2 is taken as 3) = three
                                rotating trip buffers (two trips of loads stay in flight behind the one being consumed); 0 = auto   */
  FH_TUNE_TV_XCD = 12,       /* z-free one-pass stencil sweep: deal the workgroup ids out XCD by XCD, so that strips that share halo
                                cache lines share an L2 (0 = auto = 1 = on, 2 = off: plain blockIdx order)                    */
  /* keys 13-15 (occupancy limiter, LDS-DMA trip ring, persistent chunk walk of the stencil sweep: measured flat twice,
     profiles/r04_tune_tv.txt) are only present in -DFH_EXPERIMENTAL builds (csrc/fh_experimental.h); FH_E_ARG otherwise        */
  FH_TUNE_RUN_MAX_N = 17,    /* fh_run: the widest row (columns) the device-side loop is offered for (fh_run_supported), whatever the number of
                                rows; 0 = the measured window (profiles/r06_device_loop.txt): n <= 4096 up to 32 Mi elements, n <= 6144 from 4096 rows
                                on up to 40 Mi elements -- elsewhere one launch per iteration issued by fh_iterate is as fast or faster; at most
                                7168 = the widest row it has a kernel for                                                          */
  FH_TUNE_RUN_CHAIN = 19,    /* 0 (default) / 1: outside the persistent launch's window fh_run takes the CHAINED form where it exists (float64, n <= 16384,
                                separable prox: max_steps one-pass launches enqueued back to back, step size and buffer roles from a device state
                                block, the loop's controller in each launch's finaliser).  Opt-in: measured equal to the host-side loop
                                (profiles/r06_chain.txt) -- the gap between launches disappears, the launches grow by as much             */
  FH_TUNE_ADJ_CYCLIC = 20,   /* K-adj: 1 = the rows are dealt cyclically to the slabs (slab s: rows s, s + nslab, ...), as bit 32 of FH_TUNE_FUSED_VARIANT does for
                                the one-pass kernel; 0 = auto = 2 = contiguous slabs.  Measured mixed (faster on small and mid shapes, 6 % slower at
                                65536^2; profiles/r06_placement.txt), so it stays an A/B switch                                                   */
  FH_TUNE_SEQ_POLL = 18,     /* 1 (default): a single-device step waits for its scalar block by the sequence number the launch writes behind
                                it into host-mapped memory (~5 us sooner than the launch's completion signal); 0: hipStreamSynchronize (A/B)  */
  FH_TUNE_TV3_PLANES = 21,   /* 3-D stencil kernels (fh_set_stencil3d): planes along d a workgroup marches over; 0 = auto (whole columns of planes unless
                                that leaves fewer than 8 workgroups per CU, then at least 8 planes per workgroup).  A small value gives a small
                                volume several workgroups along d (the tests); fh_tv3d_shape reports what a launch takes                        */
  FH_TUNE_DCT_ROW_CAP = 22,  /* DCT operator (fh_set_dct): longest row transform, 0 = default (2048) or 2..2048.  A small value gives a small N the
                                two-level form (the tests: N = 60 at a cap of 16).  Read when fh_set_dct sets the operator: set it before; fh_dct_shape
                                reports what the launches take                                                                                    */
  FH_TUNE_NUC_BLOCK_ROWS = 23, /* FH_PROX_NUCLEAR: rows per block of the block-Jacobi steps: 1, 2, 4, 8 (1: the classical pairwise rotation) or 0 = auto, which is 1 -- the fastest at every
                                shape measured with the present step kernel, profiles/nuclear_sizes.txt.
                                Read when the prox is set: set it before.  It exists so that small shapes reach several blocks, byes and Bk = 1   */
  FH_TUNE_FUSED_CUS = 16     /* dense one-pass kernel: launch it on at most this many CUs (one workgroup each; 0 = every CU the device
                                reports).  The co-residency probe then asks for that many.  Lets several one-pass grids run side by side
                                on one device: two solves at once, partitioned devices, ranks of a row-sharded run that share a GPU
                                (the tests: world x (CUs / world)).  The team shape needs a multiple of the team size (<= 32)        */
};

/* ---- library / context -------------------------------------------------------------- */
const char* fh_last_error(void);
int fh_device_count(int* count);
int fh_create(int device, fh_ctx** out);
/* SURVEY.md 8(b) form: device list + storage type of A.
 *   ndev == 1: a plain single-device context (what fh_create returns).
 *   ndev  > 1: IN-PROCESS ROW SHARDING (the op being sharded is `A @ x` / `A.T @ x`, fasta/linalg.py:41).  The
 *     context owns one shard per entry of dev_ids; fh_set_matrix / fh_set_matrix_f32 / fh_generate_matrix split A into contiguous
 *     row blocks (the first m mod ndev shards hold ceil(m/ndev) rows, the rest floor(m/ndev)), fh_set_loss_* and the m-side
 *     vectors (FH_VEC_B, FH_VEC_Z) are split the same way, n-side vectors are replicated.  Every solver step then runs as: local
 *     launch on each shard -> ONE sum over the shards -> n-side epilogue on each shard -> one host synchronisation; the scalar
 *     block is identical on all shards and is returned from shard 0.  The call sequence, arguments and results of every other
 *     entry point are those of a plain context (fh_set_stencil and fh_comm_* refuse: dense operator only, and the rows are
 *     already sharded).
 *       all dev_ids different: one GPU per shard; RCCL communicators from ncclCommInitAll, the sum is one grouped
 *                              ncclAllReduce(n + 3 doubles) per shard over xGMI;
 *       all dev_ids equal:     every shard on that one GPU, on one stream; the sum is an in-library kernel that adds the shards'
 *                              buffers in shard order -- same arithmetic structure, runnable (and tested) on a one-GPU box.
 *     (a mixture is FH_E_ARG.)  ndev <= 64.
 * dtype FH_DTYPE_F32_STORAGE keeps the device copy of A in float32 (rounded to nearest on
 * upload / generation): half the bytes per pass; every vector, accumulation and scalar stays float64.  OPT-IN: the iterates
 * are those of the reference run on the ROUNDED matrix, i.e. they differ from the float64-matrix run by the rounding of A
 * (relative 6e-8 per entry; SURVEY.md section 7: <= 3e-7 on the iterates away from the chaotic regime).                  */
enum fh_dtype { FH_DTYPE_F64 = 0, FH_DTYPE_F32_STORAGE = 1 };
/* or'ed into dtype: use the RCCL form of the multi-device context (ncclCommInitAll, grouped ncclAllReduce) where the default would
 * not: with ndev == 1 (one shard, a 1-rank communicator: same results as a plain context), or with a repeated device id (needs an
 * RCCL that accepts several ranks on one device -- real RCCL refuses, the tests' stand-in accepts).  Lets a one-GPU box run the
 * RCCL branch.                                                                                                               */
#define FH_CREATE_RCCL_SHELL 0x100
int fh_create_ex(int ndev, const int* dev_ids, int dtype, fh_ctx** out);
/* row blocks of a context (1 for a plain one); fh_shard lends shard k -- a complete single-device context that stays owned by
 * `ctx` -- with the rows of the whole operator it holds: [row0, row0 + rows).  For diagnostics and tests (e.g. reading a
 * replicated vector from every shard).                                                                                   */
int fh_shard_count(fh_ctx* ctx, int* count);
int fh_shard(fh_ctx* ctx, int k, fh_ctx** shard, uint64_t* row0, uint64_t* rows);
/* read-only: the FH_S_* block (FH_NSCALARS doubles) the latest call left on the host side of `ctx` -- of a shard lent by fh_shard,
 * that shard's own copy, which no other entry point returns (a multi-device context's calls return shard 0's).  No launch.      */
int fh_last_scalars(fh_ctx* ctx, double* scalars);
int fh_destroy(fh_ctx* ctx);
int fh_sync(fh_ctx* ctx);
int fh_set_tuning(fh_ctx* ctx, int key, long long value);

/* ---- operator A (replaces LinearMap.from_matrix closures `A @ x`, `A.T @ x`, fasta/linalg.py:37-41) */
/* dense row-major host matrix, m rows, n columns, leading dimension ld_host (doubles).          */
int fh_set_matrix(fh_ctx* ctx, const double* A, uint64_t m, uint64_t n, uint64_t ld_host);
/* float32 host matrix into a float32-storage context (fh_create_ex, FH_DTYPE_F32_STORAGE): copied as is, no rounding step  */
int fh_set_matrix_f32(fh_ctx* ctx, const float* A, uint64_t m, uint64_t n, uint64_t ld_host);
/* synthetic rows [row0, row0+m) of a (.., n) matrix: element (i,j) = ihall(seed, (row0+i)*n + j) * coef
 * (device twin of oracle/problems.py:synth_values).                                            */
int fh_generate_matrix(fh_ctx* ctx, uint64_t m, uint64_t n, uint64_t row0, uint64_t seed, double coef);
int fh_get_matrix_rows(fh_ctx* ctx, uint64_t row0, uint64_t nrows, double* out /* nrows*n */);
/* ---- sparse operator: A in canonical CSR (replaces the closures `S @ x`, `S.T @ y` of a scipy.sparse design matrix) ----------------------
 * indptr has m + 1 entries, starts at 0, is non-decreasing and ends at nnz; the column indices of a row are strictly increasing and < n
 * (sorted, duplicates summed); anything else is FH_E_ARG with a message naming the first offending row.  nnz == 0, empty rows and empty
 * columns are legal; explicit zeros are kept as entries.  The library keeps two device copies, A by rows and A^T by rows (built here by a
 * stable counting sort), and runs BOTH directions as gathers (csrc/fh_sparse.h): no atomics, fixed summation order, bitwise repeatable.
 * Vectors keep the vector form's layout, so fh_set_vector / fh_get_vector, fh_diff_norm, fh_commit, both losses and the prox kinds
 * IDENTITY / SHRINK / NONNEG / BOX work unchanged; served entry points: fh_init, fh_setup (its three-pass route), fh_gradient_at, fh_apply,
 * fh_fwd, fh_adj (accel / coef), fh_fwd_adj, fh_iterate, fh_timing_* (FH_K_FWD / FH_K_ADJ / FH_K_AUX).
 * Refused (FH_E_STATE / FH_E_ARG): fh_step*, fh_run, fh_set_rhs (a matrix unknown: fh_set_matrix_csr_rhs below), fh_comm_init (and a context that has a communicator), multi-device
 * contexts, float32 storage, fh_get_matrix_rows, fh_stream_read_ms, FH_PROX_LINF / L1BALL / TVBALL / GROUP (a context holding one of these
 * returns to IDENTITY when the sparse operator is set).  fh_fused_supported, fh_fused_agree and fh_run_supported report 0.               */
int fh_set_matrix_csr(fh_ctx* ctx, uint64_t m, uint64_t n, uint64_t nnz, const int64_t* indptr, const int32_t* indices, const double* values);
int fh_nnz(fh_ctx* ctx, uint64_t* nnz);     /* stored entries of the sparse operator; 0 for every other operator */
/* ---- sparse operator with a MATRIX unknown: the sparse operator and the multi-column form in ONE call (csrc/fh_spmulti.h) ------------------
 * L = 0 is fh_set_matrix_csr.  L in 1..16: the unknown is an (n, L) matrix, B and Z are (m, L); vectors, host formats (contiguous row-major
 * (n, L) / (m, L) arrays), scalars and the call sequence are those of the multi-column form below; fh_rhs reports L, fh_nnz nnz, fh_shape (m, n).
 * Every stored entry gathers one whole row of the operand and is read once for all L columns.  The lanes per row, the long-row threshold and
 * the balanced row ranges computed here depend on L, so the column count of a sparse operator is fixed when it is set: fh_set_rhs on a sparse
 * context stays FH_E_STATE.  CSR validation is that of fh_set_matrix_csr.  Served: fh_init, fh_setup (three-pass route), fh_gradient_at,
 * fh_apply, fh_diff_norm, fh_commit, fh_fwd, fh_adj (accel / coef), fh_fwd_adj, fh_iterate, fh_timing_*; least squares; prox kinds IDENTITY,
 * SHRINK, NONNEG, BOX, GROUP; FH_TUNE_NT_LOADS as for the vector form.  Refused: L > 16 (FH_E_ARG); fh_step* and fh_run (FH_E_STATE;
 * fh_fused_supported, fh_fused_agree, fh_run_supported report 0); the logistic loss; FH_PROX_LINF / L1BALL / TVBALL; float32 storage,
 * multi-device contexts and communicators.  Setting any new operator returns the context to the vector form.                              */
int fh_set_matrix_csr_rhs(fh_ctx* ctx, uint64_t m, uint64_t n, uint64_t nnz, const int64_t* indptr, const int32_t* indices, const double* values, uint32_t L);
/* read-only: what fh_set_matrix_csr[_rhs] chose for one copy of the sparse operator (side 0: A by rows, 1: A^T by rows) -- the lanes per row G
 * (which kernel instantiation a launch takes), the workgroups that share the ordinary rows and the long rows that get a workgroup each.  Any
 * output pointer may be NULL.  FH_E_STATE without a sparse operator, FH_E_ARG for another side.                                            */
int fh_sparse_lanes(fh_ctx* ctx, int side, int* G, uint32_t* nwg, uint32_t* nlong);
/* periodic difference stencil pair: A = div: (H,W,2)->(H,W), A^H = grad (examples/tv_denoising.py:26-63) */
int fh_set_stencil(fh_ctx* ctx, uint64_t H, uint64_t W);
/* ---- 3-D periodic difference stencil pair: A = div : (D,H,W,3) -> (D,H,W), A^H = grad (the N = 3 case of examples/tv_denoising.py:26-63) ------
 * m = P = D*H*W, n = 3*P (fh_shape reports them); every dimension >= 1 and 3*P < 2^31 (768^3 fits), anything else is FH_E_ARG with a sentence.
 * n-side vectors are the C order of (D,H,W,3), flat index 3*p + c; m-side vectors the C order of (D,H,W); both live in the vector form's padded
 * buffers, so fh_set_vector / fh_get_vector, fh_diff_norm, fh_commit, fh_set_loss_lsq and fh_set_prox work unchanged, and -- unlike the 2-D
 * stencil -- FH_VEC_G0 / G1 / XHAT are stored and addressable like any other operator's.  With p = (d,h,w) and indices modulo the dimension
 *   div(Y)[p]    = ((Y[d+1,h,w,0] - Y[p,0]) + (Y[d,h+1,w,1] - Y[p,1])) + (Y[d,h,w+1,2] - Y[p,2])       (NumPy's `out += ...` per axis, this order)
 *   grad(X)[p,c] = X[p - e_c] - X[p]
 * so a dimension of 1 contributes 0.0 and a dimension of 2 sees the same neighbour on both sides.  Two kernels (csrc/fh_tv3d.h), one launch per
 * direction, no atomics, fixed summation order, bitwise repeatable; measured at 512^3: 6.9 ms per pair, 4.85 TB/s (profiles/tv3d_sizes.txt).  Prox kinds served: FH_PROX_TVBALL -- here the projection of each voxel's
 * 3-vector, y / max(sqrt((y0*y0 + y1*y1) + y2*y2), 1) -- and IDENTITY, SHRINK, NONNEG, BOX (BOX(-1, 1): anisotropic TV); least squares only.
 * Served entry points, the FH_S_* scalars meaning what they mean for the sparse operator: fh_init, fh_setup (its three-pass route), fh_gradient_at,
 * fh_apply, fh_fwd, fh_adj (accel / coef), fh_fwd_adj, fh_iterate, fh_timing_* (FH_K_FWD / FH_K_ADJ).
 * Refused (FH_E_STATE / FH_E_ARG): fh_step*, fh_run, fh_set_rhs, fh_comm_init (and a context that has a communicator), multi-device contexts,
 * fh_get_matrix_rows, fh_stream_read_ms, the logistic loss, FH_PROX_LINF / L1BALL / GROUP (a context holding one of these returns to IDENTITY
 * when the operator is set).  fh_fused_supported, fh_fused_agree and fh_run_supported report 0.  Setting any other operator leaves this form. */
int fh_set_stencil3d(fh_ctx* ctx, uint64_t D, uint64_t H, uint64_t W);
/* read-only: the geometry both 3-D stencil launches take (csrc/fh_host_launch.h: tv3_shape_for, the ONE rule both launchers call), so that a test
 * can assert the path it meant to reach.  out[FH_TV3D_SHAPE_LEN] = { tile rows (h), tile columns (w), planes per workgroup, tiles along h, tiles
 * along w, chunks along d, grid = chunks * tiles, NT (1: non-temporal stores, FH_TUNE_NT_LOADS) }.  Workgroup (chunk, th, tw) owns the voxels
 * [chunk*planes, ...) x [th*tile rows, ...) x [tw*tile columns, ...), clipped to the volume: every voxel has exactly one owner.  fh_tv3d_shape
 * reads the context's volume, FH_TUNE_TV3_PLANES and CU count and is FH_E_STATE without a 3-D stencil operator; fh_tv3d_shape_for is the same
 * rule as a pure host function (no device needed; planes: 0 = auto; ncu: the device's compute units).                                        */
#define FH_TV3D_SHAPE_LEN 8
int fh_tv3d_shape(fh_ctx* ctx, uint32_t* out);
int fh_tv3d_shape_for(uint64_t D, uint64_t H, uint64_t W, int planes, int ncu, uint32_t* out);
/* ---- subsampled DCT: A = diag(d) * C, A^H = C^T * diag(d) (examples/democratic_representation.py:80-82 is the case of a 0/1 mask d) ------------
 * C is the orthonormal DCT-II of length N, scipy.fftpack.dct(x, norm='ortho'): C[k,n] = s_k cos(pi k (2n+1) / (2N)), s_0 = sqrt(1/N), s_k = sqrt(2/N).
 * m = n = N (fh_shape reports them).  d: N float64 values copied to the device, NULL = all ones; d[k] == 0.0 gives z[k] == 0.0 exactly.  No matrix is
 * stored: both directions are one complex FFT of length N done in LDS (Makhoul; Stockham autosort, radices 2, 3, 4, 5; csrc/fh_dct.h), from two
 * twiddle tables built on the host in long double when the operator is set (4 N cosl / sinl calls: of the order of a second at N = 2^22).  N <= the row cap (2048; FH_TUNE_DCT_ROW_CAP lowers it): one launch per direction; beyond:
 * N = N1 * N2, both at most the cap, five launches per direction (so N <= 2^22).  Vectors live in the vector form's padded buffers, so
 * fh_set_vector / fh_get_vector, fh_diff_norm, fh_commit, fh_set_loss_lsq, fh_set_prox and fh_shape work unchanged.  No atomics on floats, fixed
 * summation order, bitwise repeatable.  Prox kinds served: IDENTITY, SHRINK, NONNEG, BOX, LINF and L1BALL (the level search of the dense operator
 * reads x0, g0 and n only); least squares only.
 * Served entry points, the FH_S_* scalars meaning what they mean for the sparse operator: fh_init, fh_setup (its three-pass route), fh_gradient_at,
 * fh_apply, fh_fwd, fh_adj (accel / coef), fh_fwd_adj, fh_iterate, fh_commit, fh_timing_* (FH_K_FWD / FH_K_ADJ / FH_K_LEVEL).
 * Refused (FH_E_ARG with a sentence): N = 0, an N with a prime factor above 5, an N above the row cap that has no split N1 * N2 with both factors at
 * most the cap; FH_PROX_TVBALL / GROUP (a context holding one returns to IDENTITY when the operator is set) and fh_set_prox_split.  Refused
 * (FH_E_STATE): multi-device contexts, a context with a communicator and fh_comm_init, fh_set_rhs, float32 storage, the logistic loss, fh_step*,
 * fh_run, fh_get_matrix_rows, fh_stream_read_ms.  fh_fused_supported, fh_fused_agree and fh_run_supported report 0.  Setting any other operator
 * leaves this form.                                                                                                                            */
int fh_set_dct(fh_ctx* ctx, uint64_t N, const double* diag);
/* read-only: the geometry the DCT launches take (csrc/fh_host_launch.h: dct_shape_for, the ONE rule the launchers call), so that a test can assert
 * the path it meant to reach.  out[FH_DCT_SHAPE_LEN]: [0] levels (1: one row, one launch; 2: N1 x N2, five launches; 0: N is not served -- the call
 * then returns FH_E_ARG and the sentence), [1] N1, [2] N2 (1 for one level), [3] the row cap, [4] number of radix passes of a row of length N1,
 * [5..16] its radices in pass order, [17] and [18..29] the same for N2, [30] LDS class (double2 per ping-pong buffer: 128 / 512 / 2048), [31] rows
 * per workgroup and [32] grid of the row launch of length N1, [33..35] the same for N2, [36] threads per workgroup, [37] static LDS bytes of the
 * largest row kernel, [38] grid of each of the three tile launches (32 x 32 tiles of the N1 x N2 matrix), [39] launches per direction.
 * fh_dct_shape reads the context's N, the row cap it was set with and its CU count and is FH_E_STATE without a DCT operator; fh_dct_shape_for is
 * the same rule as a pure host function (no device needed; row_cap: 0 = 2048; ncu: the device's compute units).                              */
#define FH_DCT_SHAPE_LEN 40
int fh_dct_shape(fh_ctx* ctx, uint32_t* out);
int fh_dct_shape_for(uint64_t N, int row_cap, int ncu, uint32_t* out);
/* ---- subsampled 2-D DCT on an image: A x = d * (C_H X C_W^T), A^H w = C_H^T (d * w) C_W (csrc/fh_dct2.h) ------------------------------------------
 * X is the unknown as an (H, W) image in C order, C_L the orthonormal DCT-II of length L documented at fh_set_dct: the pair is
 * d * scipy.fftpack.dctn(x, norm='ortho') and scipy.fftpack.idctn(d * w, norm='ortho').  m = n = H * W (fh_shape reports them).  d: H * W float64
 * values in C order copied to the device, NULL = all ones; d[k] == 0.0 gives z[k] == 0.0 exactly.  No matrix is stored: each direction is the 1-D
 * operator's row transform (Makhoul, one complex Stockham FFT of the row's length in LDS, radices 2, 3, 4, 5) along W and along H with real H * W
 * images between them, four launches per direction, from one pair of twiddle tables per axis built on the host in long double when the operator
 * is set, and two work buffers of H * W doubles.  An axis of length 1 is the identity transform.  The context holds the DCT operator in its 2-D
 * geometry: vectors, prox kinds (IDENTITY, SHRINK, NONNEG, BOX, LINF, L1BALL), the least-squares loss, the served entry points and the FH_S_*
 * scalars are those of fh_set_dct, and so is everything fh_set_dct lists as refused (FH_E_STATE): multi-device contexts, a communicator,
 * fh_set_rhs, float32 storage, the logistic loss, fh_step*, fh_run, fh_get_matrix_rows, fh_stream_read_ms; fh_dct_shape is FH_E_STATE too (the
 * geometry is fh_dct2_shape's).  No atomics on floats, fixed summation order, bitwise repeatable.
 * Refused (FH_E_ARG with a sentence naming the axis): an axis of length 0, an axis with a prime factor above 5, an axis longer than the row cap
 * (2048; FH_TUNE_DCT_ROW_CAP lowers it) -- there is no two-level transform per axis.  Setting any other operator leaves this form.              */
int fh_set_dct2(fh_ctx* ctx, uint64_t H, uint64_t W, const double* diag);
/* read-only: the geometry the 2-D DCT launches take (csrc/fh_host_launch.h: dct2_shape_for, the ONE rule the launchers call).
 * out[FH_DCT_SHAPE_LEN]: [0] 1 (0: the shape is not served -- the call then returns FH_E_ARG and the sentence), [1] H, [2] W, [3] the row cap,
 * [4] number of radix passes of a row of length H, [5..16] its radices in pass order, [17] and [18..29] the same for W, [30] LDS class (double2 per
 * ping-pong buffer: 128 / 512 / 2048), [31] rows per workgroup and [32] grid of the row launches along H (W rows of length H), [33..35] the same
 * along W (H rows of length W), [36] threads per workgroup, [37] static LDS bytes of the largest row kernel, [38] grid of each tile launch (32 x 32
 * tiles of the H x W image), [39] launches per direction.  fh_dct2_shape reports what the context was set with and is FH_E_STATE without a 2-D DCT
 * operator; fh_dct2_shape_for is the same rule as a pure host function (no device needed; row_cap: 0 = 2048; ncu: the device's compute units). */
int fh_dct2_shape(fh_ctx* ctx, uint32_t* out);
int fh_dct2_shape_for(uint64_t H, uint64_t W, int row_cap, int ncu, uint32_t* out);
/* ---- periodic convolution with a small kernel: A x = d * (K conv x), A^T w = K corr (d * w) (csrc/fh_conv.h) --------------------------------------
 * Image x of shape (H, W) in C order (a signal: H = 1), taps K of shape (kh, kw) in C order with 1 <= kh, kw <= 16, origin (oh, ow) inside the
 * kernel, all indices modulo the dimension:
 *   (A x)[i,j]   = d[i,j] * sum_{a,b} K[a,b] * x[i-(a-oh), j-(b-ow)]        (A^T w)[i,j] = sum_{a,b} K[a,b] * (d*w)[i+(a-oh), j+(b-ow)]
 * m = n = H * W (fh_shape reports them).  d: H * W float64 values copied to the device, NULL = all ones (a 0/1 mask: inpainting, subsampled
 * convolution); d[i,j] == 0.0 gives z[i,j] == 0.0 exactly.  The arithmetic is fixed: the accumulator starts at +0.0, taps are visited a outer,
 * b inner, both ascending, each term is a rounded product followed by a rounded sum (no FMA), no tap is skipped, d is applied last in A and
 * first in A^T -- NumPy's `out += K[a,b] * np.roll(x, (a-oh, b-ow), axis=(0,1))`, bit for bit.  Any H, W >= 1 is served, images smaller than
 * the kernel included (taps then wrap more than once); H * W < 2^31.  No matrix is stored.  Vectors live in the vector form's padded buffers,
 * so fh_set_vector / fh_get_vector, fh_diff_norm, fh_commit, fh_set_loss_lsq, fh_set_prox and fh_shape work unchanged.  One launch per
 * direction, no atomics on floats, fixed summation order, bitwise repeatable.  Prox kinds served: IDENTITY, SHRINK, NONNEG, BOX, LINF and
 * L1BALL (the level search of the dense operator reads x0, g0 and n only); least squares only.
 * Served entry points, the FH_S_* scalars meaning what they mean for the sparse operator: fh_init, fh_setup (its three-pass route),
 * fh_gradient_at, fh_apply (both ways), fh_fwd, fh_adj (accel / coef), fh_fwd_adj, fh_iterate, fh_commit, fh_timing_* (FH_K_FWD / FH_K_ADJ /
 * FH_K_LEVEL).
 * Refused (FH_E_ARG with a sentence): a zero dimension, kh or kw outside 1..16, an origin outside the kernel, H * W >= 2^31; FH_PROX_TVBALL /
 * GROUP / ROWBALL / ROWSPLIT / NUCLEAR (a context holding one returns to IDENTITY when the operator is set).  Refused (FH_E_STATE):
 * fh_step*, fh_run, fh_set_rhs, multi-device contexts, a context with a communicator and fh_comm_init, float32 storage, the logistic and
 * softmax losses, fh_get_matrix_rows, fh_stream_read_ms.  fh_fused_supported, fh_fused_agree and fh_run_supported report 0.  Setting any
 * other operator leaves this form and frees its tables.                                                                                       */
int fh_set_conv2d(fh_ctx* ctx, uint64_t H, uint64_t W, uint32_t kh, uint32_t kw, uint32_t oh, uint32_t ow, const double* taps, const double* diag);
/* read-only: the geometry the convolution launches take (csrc/fh_host_launch.h: conv_shape_for, the ONE rule both launchers call), so that a
 * test can assert the path it meant to reach.  out[FH_CONV_SHAPE_LEN]: [0] tile rows, [1] tile columns (32 x 64; 1 x 2048 for a signal with
 * H == 1 and kh == 1), [2] tiles along h, [3] tiles along w, [4] grid (= [2] * [3]), [5] consecutive outputs along w per lane, [6] threads
 * per workgroup, [7] static LDS bytes of the tile.  fh_conv_shape is FH_E_STATE without this operator; fh_conv_shape_for is the same rule as
 * a pure host function (no device needed; ncu: the device's compute units) and answers FH_E_ARG, with out all zeros, for what fh_set_conv2d
 * refuses by shape.                                                                                                                          */
#define FH_CONV_SHAPE_LEN 8
int fh_conv_shape(fh_ctx* ctx, uint32_t* out);
int fh_conv_shape_for(uint64_t H, uint64_t W, uint32_t kh, uint32_t kw, int ncu, uint32_t* out);
int fh_shape(fh_ctx* ctx, uint64_t* m, uint64_t* n);

/* ---- the identity operator with an elementwise loss: the unknown is an (M, N) MATRIX, f(X) = sum of a loss over its entries (csrc/fh_nuclear.h) --
 * examples/logistic_matrix_completion.py: min mu ||X||_* + sum log(1 + e^X) - (B == 1) X, fasta(None, None, f, gradf, g, proxg, X0).  The matrix lives
 * in the vector form's buffers, M * N doubles in C order: m = n = M * N (fh_shape reports them), z = x, FH_VEC_B holds B.  The loss is set afterwards
 * by fh_set_loss_lsq / fh_set_loss_logistic (length M * N).  Both directions are elementwise launches with fixed-order reductions: no float atomics,
 * bitwise repeatable; with the prox kinds IDENTITY, SHRINK, NONNEG and BOX the prox is fused into K-fwd (one launch per direction).
 * FH_PROX_NUCLEAR (fh_set_prox_nuclear, or fh_set_prox with objective = 1) is the singular-value soft-threshold by block one-sided Jacobi: with
 * p = min(M, N), q = max(M, N), p rows of length q (xhat, transposed when M > N) in blocks of Bk rows (FH_TUNE_NUC_BLOCK_ROWS), a STEP = one launch
 * whose workgroups each own a disjoint pair of blocks of a round-robin schedule, a SWEEP = all steps; the host reads one integer rotation count per
 * sweep and stops after the first sweep without a rotation; more than 30 sweeps is FH_E_NOCONV and xprox is NaN.  The norms are not free at x0 (fh_init)
 * nor at the extrapolated x1 of an accelerated fh_adj: a values-only decomposition computes them there, unless objective = 0, when FH_S_GSUM (fh_init) and
 * FH_S_GSUM_ADJ (accelerated fh_adj) hold NaN and FH_S_GMAX / FH_S_GMAX_ADJ 0.  The thresholding's time is reported under FH_K_LEVEL.
 * Served entry points: fh_init, fh_setup (its three-pass route), fh_gradient_at, fh_apply (a copy), fh_diff_norm, fh_commit, fh_fwd, fh_adj
 * (accel / coef), fh_fwd_adj, fh_iterate, fh_timing_*.
 * Refused, each with a sentence: M or N = 0, M * N > 2^26 (FH_E_ARG); min(M, N) > 1024 for FH_PROX_NUCLEAR (FH_E_ARG); fh_step* and fh_run
 * (FH_E_STATE; fh_fused_supported, fh_fused_agree and fh_run_supported report 0); fh_set_rhs, float32 storage, multi-device contexts, communicators,
 * fh_get_matrix_rows, fh_stream_read_ms (FH_E_STATE); the prox kinds LINF, L1BALL, TVBALL, GROUP, ROWBALL and ROWSPLIT (FH_E_ARG).  Every other
 * operator refuses FH_PROX_NUCLEAR; a context holding it returns to IDENTITY when another operator is set.                                       */
int fh_set_identity(fh_ctx* ctx, uint64_t M, uint64_t N);
int fh_set_prox_nuclear(fh_ctx* ctx, double mu, int objective);
/* read-only: the geometry of the thresholding's launches (csrc/fh_host_launch.h: nuc_shape_for, the ONE rule the launchers call).
 * out[FH_NUCLEAR_SHAPE_LEN]: [0] transposed (M > N), [1] p, [2] q, [3] Bk, [4] P (p padded to a multiple of Bk), [5] nb = P / Bk, [6] steps per
 * sweep, [7] workgroups per step (the bye's included), [8] column chunk of the Gram pass, [9] chunks per row, [10] leading dimension of the working
 * buffer [ W | J^T ] in doubles, [11] its bytes, [12] static LDS bytes of the step kernel.  fh_nuclear_shape reads the context (FH_E_STATE unless it
 * holds the identity operator with FH_PROX_NUCLEAR or FH_PROX_NUCBALL); fh_nuclear_shape_for is the same rule as a pure host function (block_rows: 0 = auto = 1).           */
#define FH_NUCLEAR_SHAPE_LEN 13
int fh_nuclear_shape(fh_ctx* ctx, uint64_t* out);
int fh_nuclear_shape_for(uint64_t M, uint64_t N, int block_rows, int ncu, uint64_t* out);
/* the latest thresholding of this context: out[4] = { sweeps, steps launched, rotations, rank kept }                                             */
int fh_nuclear_info(fh_ctx* ctx, uint64_t* out);

/* ---- quadratic smooth term on an explicit symmetric matrix: f(X) = .5 <X, Q X> + <C, X>, A = identity (csrc/fh_quad.h) -----------------------
 * examples/max_norm.py:49-50 (Q = S + S^T, C = 0, X of shape (N, K)) and the dual of examples/svm.py:68-69 (Q = (l l^T) o (D D^T), C = -1, the box
 * prox of :71); box-constrained QP and kernel-SVM duals in general.  Q may be indefinite, and C need not lie in any range: this is not
 * .5 ||A x - b||^2 for any A.  ONE call sets the operator (m = n; fh_shape reports (n, n)) AND the loss: Q row-major float64 with leading dimension
 * ld_host, stored like a dense A (padded, zero padding, through the kept-block allocator); C a contiguous (n, L) array or NULL for zero; L in 1..16
 * columns of the unknown (L = 1: a vector unknown).  Q must be EXACTLY symmetric: checked on the host, FH_E_ARG names the first (i, j) with
 * Q[i,j] != Q[j,i].  The context takes the multi-column layout (LB in {2, 4, 8, 16}, the smallest >= L; fh_rhs reports L): fh_set_vector,
 * fh_get_vector and fh_apply take contiguous (n, L) arrays; fh_apply is out = Q in, whatever the adjoint flag; FH_VEC_Z holds W = Q xprox and
 * FH_VEC_B holds C.  One product W = Q X gives the value .5 <X, W> + <C, X> and the gradient W + C: an attempt of the step reads Q once, the
 * second direction is an elementwise launch.  FH_S_FSQ / FH_S_FSQ_ADJ carry f ITSELF (it may be negative), as for the logistic loss.
 * Served: fh_init, fh_setup (its three-pass route), fh_gradient_at (dst = Q src + C), fh_diff_norm, fh_commit, fh_fwd, fh_adj (accel / coef),
 * fh_fwd_adj, fh_iterate, fh_timing_*; prox kinds IDENTITY, SHRINK, NONNEG, BOX, GROUP and ROWBALL; FH_TUNE_FWD_GRID_CAP and FH_TUNE_NT_LOADS.
 * Refused, each with a sentence: L = 0 or L > 16 (FH_E_ARG); a multi-device context, a context with a communicator (and fh_comm_init on a
 * quadratic context), float32 storage (FH_E_STATE); fh_set_loss_lsq / fh_set_loss_logistic and fh_set_rhs on a quadratic context (FH_E_STATE: the
 * loss and the column count are part of the operator); FH_PROX_LINF / L1BALL / TVBALL (FH_E_ARG; a context holding one of these returns to
 * IDENTITY when the operator is set); fh_step* and fh_run (FH_E_STATE; fh_fused_supported, fh_fused_agree and fh_run_supported report 0);
 * fh_get_matrix_rows, fh_stream_read_ms.  Setting any other operator returns the context to the vector form, the least-squares loss and -- if it
 * held ROWBALL -- the IDENTITY prox.                                                                                                        */
int fh_set_quadratic(fh_ctx* ctx, const double* Q, uint64_t n, uint64_t ld_host, const double* c, uint32_t L);
/* read-only: the geometry the quadratic launches take (csrc/fh_host_launch.h: qd_shape_for, the ONE rule both launchers call).
 * out[FH_QUAD_SHAPE_LEN] = { LB, CH (columns a lane of K-fwd carries), R (rows of Q per K-fwd pass), NT (1: the non-temporal instantiations),
 * K-fwd grid, nrg (row groups the grid strides over), ntrip (trips of a lane group along a row), lanes of a lane group that hold a piece of
 * the row in the LAST trip (the others are clamped), most and fewest passes a workgroup of K-fwd makes (they differ when the grid does not
 * divide nrg), prologue workgroups, workgroups of the elementwise gradient launch }.  fh_quad_shape reads the context (FH_TUNE_FWD_GRID_CAP,
 * FH_TUNE_NT_LOADS) and is FH_E_STATE without a quadratic operator; fh_quad_shape_for is the same rule as a pure host function (no device
 * needed) of n, L and the two tuning values as fh_set_tuning takes them (0 = auto; nt_loads: -1 = auto, 0, 1).                          */
#define FH_QUAD_SHAPE_LEN 12
int fh_quad_shape(fh_ctx* ctx, uint32_t* out);
int fh_quad_shape_for(uint64_t n, uint32_t L, long long grid_cap, int nt_loads, uint32_t* out);

/* ---- bilinear smooth term: f(Z) = .5 ||S - X Y^T||_F^2, Z = [X; Y], A = identity (csrc/fh_bilinear.h) -------------------------------------
 * examples/nn_factorization.py:48-61: X is (m, K), Y is (n, K), the unknown Z = [X; Y] is (m + n, K), S is (m, n);
 * gradf(Z) = [d Y; d^T X] with d = X Y^T - S.  Sparse dictionary learning, topic models and sparse NMF have this form.  ONE call sets the operator
 * (fh_shape reports (m + n, m + n)) AND the loss: S row-major float64 with leading dimension ld_host, stored like a dense A (padded, zero padding,
 * through the kept-block allocator); K in 1..16.  The context takes the multi-column layout (LB in {2, 4, 8, 16}, the smallest >= K; fh_rhs
 * reports K): fh_set_vector and fh_get_vector take contiguous (m + n, K) arrays.  One pass over S at a point gives f and both halves of the
 * gradient: an attempt of the step reads S once (fh_fwd: the prox point; its gradient becomes g1 in fh_adj); with acceleration fh_adj makes a second
 * pass at the extrapolated point, because the form is not linear.  FH_S_FSQ / FH_S_FSQ_ADJ carry f ITSELF.  FH_VEC_B and FH_VEC_Z hold nothing.
 * SIZE LIMIT: m + n < 2^27 (row offsets (m + n) * LB fit 31 bits) and each of the two partial buffers -- column tiles * m * LB and
 * row panels * n * LB doubles, fh_bilinear_shape -- below 4 GiB; anything larger is FH_E_ARG.
 * Served: fh_init, fh_setup (its Lipschitz probes are two gradient passes), fh_gradient_at, fh_diff_norm, fh_commit, fh_fwd, fh_adj
 * (accel / coef), fh_fwd_adj, fh_iterate, fh_timing_*; fh_set_prox with IDENTITY, SHRINK, NONNEG or BOX (all rows) and fh_set_prox_split;
 * FH_TUNE_FWD_GRID_CAP and FH_TUNE_NT_LOADS.
 * Refused, each with a sentence naming what was asked: K = 0 or K > 16, an empty S, the size limit (FH_E_ARG); fh_apply (there is no linear operator
 * to apply); fh_set_loss_lsq / fh_set_loss_logistic and fh_set_rhs (the loss and the column count are part of the operator); FH_PROX_LINF / L1BALL /
 * TVBALL / GROUP / ROWBALL (a context holding one of these returns to IDENTITY when the operator is set); fh_step* and fh_run (fh_fused_supported,
 * fh_fused_agree and fh_run_supported report 0); multi-device contexts, communicators (and fh_comm_init on such a context), float32 storage;
 * fh_get_matrix_rows, fh_stream_read_ms.  Setting any other operator returns the context to the vector form, the least-squares loss and -- if it
 * held ROWSPLIT -- the IDENTITY prox.                                                                                                        */
int fh_set_factorization(fh_ctx* ctx, const double* S, uint64_t m, uint64_t n, uint64_t ld_host, uint32_t K);
/* FH_PROX_ROWSPLIT: rows [0, split) take kind_top (IDENTITY, SHRINK with mu_top, NONNEG, BOX with lo_top / hi_top), rows [split, ..) take
 * kind_bottom (IDENTITY, NONNEG, BOX with lo_bottom / hi_bottom).  On the bilinear operator split must equal m (the rows of X); every other
 * operator refuses the call (FH_E_STATE).                                                                                                    */
int fh_set_prox_split(fh_ctx* ctx, uint64_t split, int kind_top, double mu_top, double lo_top, double hi_top,
                      int kind_bottom, double lo_bottom, double hi_bottom);
/* read-only: the geometry the bilinear launches take (csrc/fh_host_launch.h: bl_shape_for, the ONE rule the launchers call).
 * out[FH_BILINEAR_SHAPE_LEN] = { LB, NT (1: the non-temporal instantiations), tile rows PR (rows of a row panel), tile columns (512), row panels,
 * column tiles, RB (rows of S per trip down a panel), trips down a full panel, rows of the LAST panel, live rows of its last trip, lanes that
 * hold a live column in the LAST column tile (of 256), workgroups of the pass, most and fewest tiles a workgroup takes (they differ when the
 * grid does not divide the tile count), workgroups of the elementwise launches, bytes of the GX partials, bytes of the GY partials }.
 * fh_bilinear_shape reads the context (FH_TUNE_FWD_GRID_CAP, FH_TUNE_NT_LOADS) and is FH_E_STATE without a bilinear operator;
 * fh_bilinear_shape_for is the same rule as a pure host function (no device needed) of m, n, K and the two tuning values as fh_set_tuning
 * takes them (0 = auto; nt_loads: -1 = auto, 0, 1).                                                                                          */
#define FH_BILINEAR_SHAPE_LEN 17
int fh_bilinear_shape(fh_ctx* ctx, uint32_t* out);
int fh_bilinear_shape_for(uint64_t m, uint64_t n, uint32_t K, long long grid_cap, int nt_loads, uint32_t* out);

/* ---- multi-column form: the unknown is an (n, L) MATRIX, one A for all L columns (examples/mmv.py; multi-column LASSO / NNLS) -----------
 * fh_set_rhs(ctx, L), L in 1..16, on a plain single-device context with a dense float64 operator (a sparse one: fh_set_matrix_csr_rhs above): every n-side vector (FH_VEC_X0 .. BEST,
 * T0 .. T3) becomes an (n, L) matrix, FH_VEC_B and FH_VEC_Z (m, L) matrices; fh_set_vector, fh_get_vector, fh_set_loss_lsq and fh_apply
 * take and return contiguous ROW-MAJOR host arrays of n*L or m*L doubles; fh_shape still reports (m, n) of A.  The call sequence and the
 * meaning of every FH_S_* scalar (now sums over all n*L or m*L entries), fh_commit, fh_init, fh_setup (its three-pass route),
 * fh_gradient_at, fh_diff_norm, fh_fwd, fh_adj (with accel / coef), fh_fwd_adj, fh_iterate and timing are those of the vector form; every
 * pass reads A once for all L columns (csrc/fh_multi.h).  Prox kinds served: IDENTITY, SHRINK, NONNEG, BOX (elementwise) and GROUP.
 * L = 0 returns the context to the vector form; a context that never calls fh_set_rhs behaves as before.  EVERY successful call -- also
 * one that repeats the current L -- resets every vector to zero and forgets the loss (set it again).  Setting a new operator returns the context to the vector form.
 * Refused (FH_E_ARG / FH_E_STATE): L > 16; a stencil operator; float32 storage; a multi-device context; a context with a communicator
 * (and fh_comm_init on a multi-column context); the logistic loss; FH_PROX_LINF / L1BALL / TVBALL.  In multi-column form
 * fh_fused_supported, fh_fused_agree and fh_run_supported report 0 and fh_step* / fh_run return FH_E_STATE.                               */
int fh_set_rhs(fh_ctx* ctx, uint32_t L);
int fh_rhs(fh_ctx* ctx, uint32_t* L);      /* L of the multi-column form, 0 in the vector form */
/* read-only: the geometry the multi-column dense launches take (csrc/fh_host_launch.h: mc_shape_for, the ONE rule both launchers call), so
 * that a test can assert the path it meant to reach.  out[FH_MULTI_SHAPE_LEN] = { LB (device columns per row), CH (columns a lane of K-fwd
 * carries), R (rows of A per K-fwd pass), NT (1: the non-temporal instantiations), K-fwd grid, nrg (row groups the grid strides over), ntrip
 * (trips of a lane group along a row), prologue workgroups, slab_rows, nslab, rows of the last slab, SB (rows of the residual K-adj stages at
 * a time), stages of a full slab, ncc (column chunks of K-adj) }.  fh_multi_shape reads the context's own device shape, column count and
 * tuning values (FH_TUNE_ADJ_SLAB_ROWS, FH_TUNE_FWD_GRID_CAP, FH_TUNE_NT_LOADS) and is FH_E_STATE unless the context is in multi-column dense
 * form; fh_multi_shape_for is the same rule as a pure host function (no device needed) of an (m, n) matrix, L columns and the three tuning
 * values as fh_set_tuning takes them (0 = auto; nt_loads: -1 = auto, 0, 1).                                                              */
#define FH_MULTI_SHAPE_LEN 14
int fh_multi_shape(fh_ctx* ctx, uint32_t* out);
int fh_multi_shape_for(uint64_t m, uint64_t n, uint32_t L, int slab_rows, long long grid_cap, int nt_loads, uint32_t* out);

/* ---- smooth term f(z) = .5||z - b||^2, grad f(z) = z - b (examples/sparse_least_squares.py:41-42) */
int fh_set_loss_lsq(fh_ctx* ctx, const double* b, uint64_t len);
/* ---- smooth term f(z) = sum log(1+exp(z)) - (b==1)*z, grad f(z) = -b/(1+exp(b*z)), labels b in {-1,+1}
 *      (examples/sparse_logistic.py:47-48); FH_S_FSQ / FH_S_FSQ_ADJ then carry f itself. Dense and sparse operators.   */
int fh_set_loss_logistic(fh_ctx* ctx, const double* labels, uint64_t len);
/* ---- observation weights on the identity operator: f(X) = sum_j w_j * loss(x_j, b_j) for either elementwise loss -- matrix completion from a subset
 *      of the entries (w a 0 / 1 mask), or weighted data.  w has B's length (M * N); every entry finite and >= 0 (FH_E_ARG names the first offender);
 *      NULL removes the weights.  A term is w == 0 ? 0 : w * term, a gradient entry w == 0 ? 0 : w * grad: an unobserved entry contributes exactly 0.0
 *      whatever x is, and w == 1 gives the unweighted bits.  FH_S_FSQ / FH_S_FSQ_ADJ carry sum w (x - b)^2 for least squares.  Weighted: fh_init, fh_setup,
 *      fh_gradient_at, fh_fwd, fh_adj, fh_fwd_adj, fh_iterate; fh_apply is the plain operator.  The weights belong to the loss: set them AFTER it, and
 *      fh_set_loss_lsq / fh_set_loss_logistic drop them.  FH_E_STATE: any operator but the identity; no loss set yet; and setting another operator
 *      on a context that holds weights (a weighted problem never silently runs unweighted) -- fh_set_identity itself drops them with the loss.      */
int fh_set_loss_weights(fh_ctx* ctx, const double* w);
/* ---- smooth term f(Z) = sum_i [ logsumexp(Z_i,:) - Z_i,y_i ] over the L columns of a MATRIX unknown (multinomial logistic regression, one column of
 *      X per class), grad f(Z)_i,l = exp(Z_i,l) / sum_k exp(Z_i,k) - [l == y_i]; labels y in {0 .. L-1}^m (csrc/fh_softmax.h).  The arithmetic of a row z:
 *      mx = max_l z_l, e_l = exp(z_l - mx), s = e_0 + e_1 + ... + e_{L-1} in index order, term = (mx + log(s)) - z_y, grad_l = e_l / s - Y_l: the maximum
 *      is always subtracted, so z = (800, -800) gives (1, 0) and a finite loss.  Needs the multi-column form with L >= 2: fh_set_rhs on a dense operator, or
 *      fh_set_matrix_csr_rhs.  FH_VEC_B then holds the one-hot matrix Y (m, L); FH_S_FSQ / FH_S_FSQ_ADJ carry f itself.  Each direction is the
 *      least-squares multi-column launch plus one short row pass over Z (the dense adjoint: plus a one-workgroup launch that writes FH_S_FSQ_ADJ).
 *      Served: fh_init, fh_setup (its three-pass route), fh_gradient_at, fh_apply (the plain operator), fh_fwd, fh_adj (accel / coef), fh_fwd_adj,
 *      fh_iterate, fh_commit; the prox kinds of the multi-column form (IDENTITY, SHRINK, NONNEG, BOX, GROUP).
 *      Refused: a label outside [0, L) (FH_E_ARG, naming the first offender), m != rows of the operator (FH_E_ARG); the vector form, L = 1, every operator
 *      other than dense and sparse in multi-column form, multi-device contexts and communicators (FH_E_STATE); fh_step* and fh_run as for every
 *      multi-column context.  fh_set_rhs and setting an operator return the context to the least-squares loss.                          */
int fh_set_loss_softmax(fh_ctx* ctx, const int32_t* labels, uint64_t m);
/* ---- prox term (kinds above); mu as in the closures, lo/hi for FH_PROX_BOX only              */
int fh_set_prox(fh_ctx* ctx, int kind, double mu, double lo, double hi);
/* read-only: which kernel the clipping-level search of FH_PROX_LINF / FH_PROX_L1BALL (csrc/fh_prox.h) takes for an unknown of n entries -- the ONE rule
 * the launcher calls (csrc/fh_host_launch.h: level_shape_for), as a pure host function (no device needed), so that a test can assert the kernel it
 * meant to reach.  out[FH_LEVEL_SHAPE_LEN]: [0] 1 = the search on several workgroups (k_level_search_multi), 0 = one workgroup (k_level_search),
 * [1] threads per workgroup, [2] entries a thread keeps in registers (0: none, re-read in every pass), [3] workgroups.  FH_E_ARG unless 1 <= n < 2^31. */
#define FH_LEVEL_SHAPE_LEN 4
int fh_level_shape_for(uint64_t n, uint32_t* out);

int fh_set_vector(fh_ctx* ctx, int which, const double* host, uint64_t len);
int fh_get_vector(fh_ctx* ctx, int which, double* host, uint64_t len);

/* ---- solver steps -------------------------------------------------------------------- */
/* fasta/__init__.py:132-137: z1 = A x0, f1 = f(z1), g0 = A^H grad f(z1); arms the acceleration
 * state (x_accel1 = x0, z_accel1 = z1, :154-157).  scalars: FH_S_FSQ, FH_S_GSUM, FH_S_GMAX.       */
int fh_init(fh_ctx* ctx, double* scalars);
/* The whole set-up of a solve in one call (fasta/__init__.py:100-113 Lipschitz probes + :135-137 initial pass): with the two probes
 * in FH_VEC_T0 / FH_VEC_T1 and x0 in FH_VEC_X0 it leaves the state fh_init leaves and returns fh_init's scalars plus
 * FH_S_DG2 = ||A^H grad f(A T0) - A^H grad f(A T1)||^2 and FH_S_DX2 = ||T0 - T1||^2 (L = sqrt of their quotient, :110).
 * FH_VEC_T2 / FH_VEC_T3 are scratch afterwards.  A dense least-squares operator with n <= 65536 (either storage) on a single-device context
 * is read ONCE for the whole set-up (csrc/fh_setup.h: two dot products and two rank-1 updates per row buffer -- x0, and the probes'
 * difference, since grad(T0) - grad(T1) = A^T A (T0 - T1) there); ROW BLOCKS (a multi-device context, a rank with a communicator) read
 * their block once each and sum the two gradients, the loss sums and the timeout words in one exchange -- a rank first settles the decision
 * with its peers: fh_setup is COLLECTIVE on a context with a communicator; every other operator takes the three passes fh_gradient_at x 2 +
 * fh_init inside the call.  z, f, g0 are bit-identical either way; the norm of the gradient difference agrees to ~1e-15 relative.  */
int fh_setup(fh_ctx* ctx, double* scalars);
/* dst = A^H grad f(A src) for n-length device vectors (Lipschitz probes, fasta/__init__.py:106-107) */
int fh_gradient_at(fh_ctx* ctx, int src_vec, int dst_vec);
/* ||a - b||_2 of two n-length device vectors (fasta/__init__.py:110)                             */
int fh_diff_norm(fh_ctx* ctx, int vec_a, int vec_b, double* out);
/* K-fwd, one launch: xhat = x0 - tau*g0; xprox = prox(xhat, tau); z1 = A xprox; reductions
 * FH_S_FSQ..FH_S_RDOT (fasta/__init__.py:181-188, 200, 231, 272-274).  May be called repeatedly
 * with a smaller tau (backtracking, :204-213).                                                   */
int fh_fwd(fh_ctx* ctx, double tau, double* scalars);
/* K-adj, one launch (+ one RCCL all-reduce when row-sharded): z1' = z1 + coef*(z1 - z_accel0),
 * x1 = xprox + coef*(xprox - x_accel0) (coef = 0 and accel = 0 without acceleration, :242-243);
 * g1 = A^H (z1' - b) (:248); reductions FH_S_DXDG..FH_S_GMAX_ADJ (:254-260, 274, 285).          */
int fh_adj(fh_ctx* ctx, double tau, int accel, double coef, double* scalars);
/* fh_fwd followed by fh_adj (no acceleration) under ONE synchronisation: the complete FH_S_* block comes back in one round
 * trip.  For short launches, where the host round trip dominates; the caller speculates on the step being accepted.      */
int fh_fwd_adj(fh_ctx* ctx, double tau, double* scalars);
/* ONE-PASS iteration (dense operator, no acceleration): K-fwd and K-adj of the same tau from a SINGLE read of A
 * (teams of 1 to 16 co-resident workgroups cover a row and exchange partial dot products; see csrc/fh_fused.h).  Writes the complete
 * FH_S_* block (both halves); scalars[15] != 0 reports a bounded-spin timeout (results invalid).  The caller uses it
 * speculatively: if the backtracking test on FH_S_FSQ fails it re-runs fh_fwd (smaller tau) + fh_adj.
 * fh_fused_supported: 0 = no (n > 262144, TV prox on a dense operator); 1 = dense, recommended (n >= 16384 or at least
 * 8 Mi elements); 3 = dense, available but no faster than two short launches; 2 = stencil operator (one sweep replaces both). */
int fh_fused_supported(fh_ctx* ctx, int* yes);
/* fh_fused_supported is a purely LOCAL query: safe to call from one rank alone.  The ranks of a row-sharded run (one process per GPU)
 * must all take the same kind of step, so they settle on ONE verdict with fh_fused_agree: a COLLECTIVE call -- every rank of the
 * communicator calls it at the same point (FBSolver.setup does) -- that sums the ranks' "0" and "3" verdicts; any 0 makes it 0
 * everywhere, else any 3 makes it 3.  A rank whose local query failed still enters the exchange (contributing "0") before it
 * returns its error, so its peers are never left waiting.  Without a communicator it equals fh_fused_supported.               */
int fh_fused_agree(fh_ctx* ctx, int* yes);
/* The dense one-pass kernel needs one workgroup on every compute unit at the same time.  The library checks that once per context
 * with a ~20 us probe launch (fh_fused_supported then reports 0 for the dense operator if CUs are hidden by a mask, a partition
 * mode or a co-tenant); this entry runs the same probe for `workgroups` whole-CU workgroups and reports whether they all ran side
 * by side (at most 2 ms when they cannot).                                                                                  */
int fh_coresident_probe(fh_ctx* ctx, int workgroups, int* ok);
/* Which variant of the one-pass kernel serves rows of n columns -- shape5 = {pieces per lane, posting distance, team members,
 * x slice in LDS, row buffers} (all 0: no one-pass kernel for this width) -- and whether that variant is compiled into the
 * library (csrc/fh_fused_instances.inc).  A pure host function: no device needed.  dtype: fh_dtype; variant: FH_TUNE_FUSED_VARIANT
 * bits; ncu: compute units (256 on MI355X).                                                                                */
int fh_fused_shape(uint64_t n, int dtype, int variant, int ncu, int* shape5, int* instantiated);
/* The whole geometry of a one-pass launch, from the one host function the launcher itself takes it from (csrc/fh_host_launch.h:
 * fused_launch_for), so that a test can assert the path it meant to reach.  out[FH_FUSED_LAUNCH_SHAPE_LEN] = { PPT, PIPE, TEAM, XLDS, NBO, F32
 * (the template key of k_fused_dense: fh_fused_shape's five numbers and the storage), workgroups per CU, teams, rows per team, workgroups
 * (teams x TEAM), the scheduling word the kernel receives (bit 32 -- rows dealt cyclically -- resolved: cleared by the host below 128 rows
 * per team unless FH_TUNE_FUSED_VARIANT set the word), ld2 (16-byte pieces of a row that hold data), nv2 (double pairs per n-side vector) }.
 * fh_fused_launch_shape reads the context (its matrix, prox kind, FH_TUNE_FUSED_CUS capped by the device's CUs, FH_TUNE_FUSED_VARIANT) and is
 * FH_E_STATE where the one-pass kernel has no shape; fh_fused_launch_shape_for is the same rule as a pure host function (no device needed) of
 * an (m, n) matrix of storage `dtype`: variant_word = the low half of FH_TUNE_FUSED_VARIANT (34 by default), variant_auto = 1 if nobody set
 * it, cus = the CUs the launch may take, min_rows = the rows-per-team floor (16 by default, 0 = none).
 * fh_setup_shape / fh_setup_shape_for: the same for fh_setup's one-read launch (csrc/fh_setup.h) of a least-squares problem --
 * out[FH_SETUP_SHAPE_LEN] = { MPP, PIPE, TEAM, threads per workgroup, NR, F32 (the template key of k_setup_dense), workgroups per CU (1), teams,
 * rows per team, workgroups, the scheduling word, ld2, nv2 }; FH_E_STATE where fh_setup takes the three passes instead.               */
#define FH_FUSED_LAUNCH_SHAPE_LEN 13
#define FH_SETUP_SHAPE_LEN 13
int fh_fused_launch_shape(fh_ctx* ctx, uint32_t* out);
int fh_fused_launch_shape_for(uint64_t m, uint64_t n, int dtype, int variant_word, int variant_auto, int cus, int min_rows, uint32_t* out);
int fh_setup_shape(fh_ctx* ctx, uint32_t* out);
int fh_setup_shape_for(uint64_t m, uint64_t n, int dtype, int variant_word, int variant_auto, int cus, int min_rows, uint32_t* out);
int fh_step(fh_ctx* ctx, double tau, double* scalars);
/* fh_step in two halves (the loop body of fasta/__init__.py:171-188 issued now, waited for later): fh_step_begin enqueues the launch
 * on the context's stream and returns at once; fh_step_end waits and delivers the scalar block.  In between the host may drive
 * OTHER contexts -- two solves side by side on one device (FH_TUNE_FUSED_CUS each) from one host thread.  Every other entry point
 * of `ctx` returns FH_E_STATE until fh_step_end has been called.                                                              */
int fh_step_begin(fh_ctx* ctx, double tau);
int fh_step_end(fh_ctx* ctx, double* scalars);
/* ONE-PASS iteration with acceleration (fasta/__init__.py:220-248; dense operator, also row-sharded): as fh_step, plus
 * x1 = xprox + c*(xprox - x_accel0) and the gradient taken at z1 + c*(z1 - z_accel0) with c = coef, or 0 when restart != 0
 * and this step's restart dot <x0 - xprox, xprox - x_accel0> (:231) exceeds 1e-30; the dot is returned in FH_S_RDOT and
 * f at the extrapolated point in FH_S_FSQ_ADJ, so the caller updates alpha exactly as after fh_fwd + fh_adj.
 * Stencil operator: one sweep as well (csrc/fh_tv.h, k_fused_tv_accel) -- it carries both candidates of the coefficient and
 * keeps the extrapolated iterate in (prox output, previous prox output, coefficient) form, formed on the fly by the next
 * sweep; a solve that uses it must use it from the first iteration after fh_init (FH_E_STATE otherwise, and fh_fwd /
 * fh_adj / fh_step refuse until the next fh_init).  fh_get_vector(X0 | X1 | BEST) materialises the iterate.              */
int fh_step_accel(fh_ctx* ctx, double tau, double coef, int restart, double* scalars);
/* ---- the loop itself on the device (opt-in: fasta(..., device_iters=K)) -----------------------------------------------------------
 * fh_run executes up to max_steps FBS iterations -- fasta/__init__.py:171-312: forward step, prox, both matvecs, the non-monotone
 * backtracking test with its retries (:195-217), FISTA restart and alpha recursion (:220-238), Barzilai-Borwein step (:253-270),
 * residuals, best iterate (:272-300) and ONE OF THE FOUR BUILT-IN stop rules (fasta/stopping.py:6-51) -- in ONE persistent launch
 * (csrc/fh_run.h), and returns the iterations' histories in one block.  For short launches, where the fixed cost of a launch and the
 * host round trip between two launches dominate (a workgroup owns whole rows: n <= 6144).  Arithmetic and decisions are those of the
 * per-iteration path (fh_step + fh_iterate), so iteration and backtrack counts are the same and histories agree to rounding.
 *   opts    the options of fasta() the loop reads; stop_rule: 0 residual, 1 norm_residual, 2 ratio_residual, 3 hybrid_residual
 *   state   in/out, carried from call to call: after fh_init / fh_setup set tau_next = tau0, alpha1 = 1, max_residual = -inf,
 *           best_quality = +inf, iteration = backtracks = 0, f_window[0] = f(x0) (f_window[j % 64] holds f_hist[j]; window <= 64)
 *   history max_steps records of FH_RUN_HIST doubles: residual, norm_residual, stepsize, f_hist[i+1], objective, backtracks of the
 *           iteration, alpha0, 1 if the iterate became the best one (+ 2 if the acceleration was restarted, :231-233)
 *   steps_done  iterations executed (fewer than max_steps when the stop rule fired: state->stopped = 1)
 * fh_run_supported: 1 if this context's operator, loss and prox have a kernel for it (dense float64 operator inside the measured window of FH_TUNE_RUN_MAX_N -- n <= 6144, at most 32-40 Mi elements -- on a
 * single-device context, a scalar-separable prox without level search, every CU free for one resident workgroup).                 */
#define FH_RUN_HIST 8
#define FH_RUN_WINDOW_MAX 64
/* how fh_iterate's forward launches reach the device (fh_run ignores it).  The caller settles it once per solve -- over the ranks of a
 * row-sharded run with fh_fused_agree -- from fh_fused_agree's verdict: 1 / 2 -> ALWAYS, 3 -> SPECULATIVE, else PAIR (small dense
 * operator, no acceleration) or SEPARATE.  A policy changes which launches produce the results, never the results.                    */
enum fh_launch_mode {
  FH_LAUNCH_SEPARATE = 0,            /* fh_fwd, decide, fh_adj                                                                      */
  FH_LAUNCH_ONEPASS_ALWAYS = 1,      /* fh_step / fh_step_accel for every launch of the loop, backtracking retries included          */
  FH_LAUNCH_ONEPASS_SPECULATIVE = 2, /* fh_step / fh_step_accel, except for 8 iterations after a backtrack and in the retries         */
  FH_LAUNCH_PAIR = 3                 /* fh_fwd_adj (one synchronisation), same exceptions; no acceleration                            */
};
typedef struct fh_run_opts {
  int adaptive, accelerate, backtrack, restart, evaluate_objective, stop_rule, window, max_backtracks;
  double stepsize_shrink, tolerance;
  int launch_mode;                   /* fh_iterate only: enum fh_launch_mode                                                        */
  int reserved;
} fh_run_opts;
typedef struct fh_run_state {
  double tau_next, alpha1, max_residual, best_quality;
  uint64_t iteration, backtracks;
  int stopped, reserved;             /* stopped: 0 = ran out of steps, 1 = the stop rule fired, 3 = fh_run's launch timed out (FH_E_TIMEOUT) */
  double f_window[FH_RUN_WINDOW_MAX];
  /* fh_iterate only -- the launch policy's memory, carried from call to call like the rest (set spec_cooldown = 0, onepass_off_until = -1,
   * onepass_backoff = 64 and the three counters to 0 before the first call):                                                       */
  int spec_cooldown;                 /* iterations left before the one-pass kernel / the pair is speculated on again after a backtrack */
  int onepass_backoff;               /* iterations to stay off the one-pass kernel after its NEXT hand-off timeout (doubles per failure) */
  int64_t onepass_off_until;         /* -1, or the iteration from which the one-pass kernel is tried again after a hand-off timeout    */
  uint64_t onepass_launches, pair_launches, onepass_timeouts;   /* totals: one-pass launches that delivered, pairs, hand-off timeouts  */
} fh_run_state;
/* sizeof(fh_run_opts), sizeof(fh_run_state), FH_RUN_HIST, FH_RUN_WINDOW_MAX as THIS build of the library sees them: a binding checks its own
 * struct layouts against them before the first call (fasta_python_amd/hip.py:load_library does).  No device needed.                           */
int fh_abi_sizes(uint64_t sizes[4]);
int fh_run_supported(fh_ctx* ctx, int* yes);
/* After a grid-barrier timeout of the persistent launch (workgroups not co-resident) fh_run returns FH_E_TIMEOUT with state->stopped = 3:
 * the context and `state` are those of the last COMPLETED iteration (state->tau_next = the step the interrupted iteration started with),
 * `history` / `steps_done` describe the completed ones -- the caller continues with fh_iterate or fh_step.  Any other failure: FH_E_STATE. */
int fh_run(fh_ctx* ctx, int max_steps, const fh_run_opts* opts, fh_run_state* state, double* history, int* steps_done);
/* The geometry of fh_run's persistent launch, from the one host function the launcher itself takes it from (csrc/fasta_hip.hip: run_shape_for),
 * so that a test can assert the path it meant to reach.  out[FH_RUN_SHAPE_LEN] = { PPT (16-byte pieces per lane: the instantiation
 * k_run_dense<PPT>), the pieces per lane the row needs (PPT is the next table entry: 1, 2, 4, 5, 6, 7, 8, 10, 12, 14), XLDS (1: the dot products
 * read the prox output from LDS), BIG (1: g0 and x_accel0 come from L2 in every attempt), NB (row buffers), G (workgroups), rows per workgroup,
 * workgroups with no rows, rows of the last workgroup that has any, phase B: columns pairs per workgroup (share), slices of the workgroup
 * range a workgroup sums side by side, workgroups per slice (tps), trips over its share; NT (1: A is streamed with non-temporal loads), ld2
 * (16-byte pieces per row) }.  fh_run_shape reads the context (its matrix, prox kind, FH_TUNE_FUSED_CUS capped by the device's CUs, the
 * rows-per-team floor of FH_TUNE_FUSED_VARIANT, FH_TUNE_RUN_MAX_N, FH_TUNE_NT_LOADS) and is FH_E_STATE where the persistent launch has no kernel;
 * fh_run_shape_for is the same rule as a pure host function (no device needed) of an (m, n) dense float64 matrix, `cus` = the CUs the launch
 * may take, `min_rows` = the rows-per-team floor (16 by default, 0 = none) and the two tuning values as fh_set_tuning takes them.       */
#define FH_RUN_SHAPE_LEN 15
int fh_run_shape(fh_ctx* ctx, uint32_t* out);
int fh_run_shape_for(uint64_t m, uint64_t n, int cus, int min_rows, int run_max_n, int nt_loads, uint32_t* out);
/* The same loop driven from the HOST side of the library (csrc/fh_host_iterate.h), for EVERY operator, loss, prox and sharding form the
 * step entry points serve -- a dense matrix of any width, the level-search prox kinds, the stencil, float32 storage, row blocks in this
 * process, a rank of a row-sharded run (every rank calls it with the same arguments).  Per iteration it issues what the Python driver of
 * round 1-5 issued (fh_step / fh_step_accel / fh_fwd / fh_adj / fh_fwd_adj by opts->launch_mode, then fh_commit), synchronises once and takes
 * the reference's decisions (fasta/__init__.py:195-217, :220-238, :253-270, :272-300; fasta/stopping.py:6-51) in float64 exactly as that
 * driver does -- results are bit-identical to it -- without the 17-19 us of interpreter time per iteration.  Arguments, state, history
 * records (record[7] = 1 if the iterate became the best one, + 2 if the acceleration was restarted) and steps_done as fh_run.  On an
 * error the completed iterations stay committed and are reported (state, history, steps_done); the failed one has changed nothing.   */
int fh_iterate(fh_ctx* ctx, int max_steps, const fh_run_opts* opts, fh_run_state* state, double* history, int* steps_done);
/* how often this context got over an in-launch timeout by itself: what = 0 clipping-level searches finished by the single-workgroup
 * fall-back, 1 = searches that found no level (reported as FH_E_TIMEOUT), 2 = fh_run launches that ended in a barrier timeout      */
int fh_recovered_count(fh_ctx* ctx, int what, uint64_t* count);
/* x0 <- x1, g0 <- g1, acceleration history rotates (:176-177, :222-226); save_best != 0 also
 * copies x1 into FH_VEC_BEST (:298-300).                                                         */
int fh_commit(fh_ctx* ctx, int save_best);
/* ---- duality-gap certificate of the committed iterate (csrc/fh_gap.h; the host statement is fasta_python_amd/certificates.py) --------------------
 * For min_x f(A x) + mu * Omega(x), from FH_VEC_X0, FH_VEC_G0 = A^H grad f(A x0), z = A x0 and FH_VEC_B as they lie in device memory, with the mu
 * and the prox kind the context holds: Omega = sum |x_ij| and Omega° = max |g_ij| for FH_PROX_SHRINK, Omega = sum_j ||x_j,:||_2 and
 * Omega° = max_j ||g_j,:||_2 (row norms summed in column order) for FH_PROX_GROUP; s = 1 if Omega° <= mu else mu / Omega°; u = s * grad f(z) is dual
 * feasible; P = f(z) + mu * Omega, D = -f*(u), gap = P - D >= 0 bounds the suboptimality of x0.  Least squares (r = z - b):
 * D = -.5 s^2 ||r||^2 - s <r, b>, f(0) = .5 ||b||^2.  Logistic: D = -sum h(y_i + s (sigma(z_i) - y_i)), h(p) = p log p + (1 - p) log(1 - p) evaluated
 * without cancellation, f(0) = m log 2.  out[FH_GAP_NOUT] = { P, D, gap, f(z), Omega(x0), Omega°(g0), s, f(0) }; at x0 = 0, out[5] is the critical mu
 * above which the solution is zero.  Two ordinary launches (three for the logistic loss), no float atomics, fixed summation order, bitwise
 * repeatable; no vector, scalar or state of the context changes (the shared workspace holds the partial sums); fh_timing_* reports the launches under FH_K_AUX.
 * z = A x0 is Z[zc], the image every committed state keeps of its latest prox output -- NOT what FH_VEC_Z addresses (the image of the prox output
 * of the latest forward launch, the next z1).  Valid after fh_init, fh_setup, and fh_commit / a returned fh_iterate / fh_run WITHOUT acceleration:
 * an accelerated step commits the extrapolated x1, whose image the adjoint launch forms on the fly and never stores.
 * Served: the dense and the sparse operator, vector and multi-column, either storage of A, the DCT in both geometries and the convolution;
 * least squares with FH_PROX_SHRINK (any L) or FH_PROX_GROUP; the logistic loss with FH_PROX_SHRINK on the vector forms.
 * Refused, FH_E_ARG with one sentence each: any other prox kind or loss; mu <= 0; a context that holds observation weights; the identity, stencil,
 * quadratic and bilinear forms; a multi-device context or one with a communicator; no committed state (no fh_init / fh_setup since the operator, the
 * loss, the column count, x0, g0 or b were set); a step in flight (fh_step_begin); a latest step that was accelerated.                          */
#define FH_GAP_NOUT 8
int fh_dual_gap(fh_ctx* ctx, double* out);
/* ---- gap-safe screening (csrc/fh_screen.h; the host statement is fasta_python_amd/certificates.py: screen) ----------------------------------------
 * Least squares with FH_PROX_SHRINK (any L) or FH_PROX_GROUP.  With the certificate above at the committed iterate and norms2_j = sum_i a_ij^2:
 *   gap_safe = gap + kappa * eps * (P + f + 2 sqrt(f * f(0))),  rho = sqrt(2 * gap_safe),
 *   feature j is zero at every solution when each of its L entries has (s * |g0_jl| + rho * sqrt(norms2_j)) * (1 + 2^-48) < mu
 * (FH_PROX_GROUP: s * ||g0_j,:||_2 in place of s * |g0_jl|).  kappa * eps * (...) bounds what rounding can take from the computed gap: kappa is the
 * longest addition chain of the certificate's sums at this shape (fh_screen_shape_for reports it); at x0 = 0 inside the dual ball (Omega = 0, s = 1) the
 * gap is zero as an identity and so is rho.  Ordinary launches, no float atomics, fixed summation order, bitwise repeatable; FH_K_AUX.
 * fh_column_norms: norms2 of the dense operator (vector and multi-column, either storage: one streaming read of A) or of the sparse operator (its
 * by-columns copy, entries in stored order), kept in the context until the operator goes -- any operator setter and fh_set_rhs drop them -- so a second
 * call launches nothing; out: n doubles, or NULL.  Refused, FH_E_STATE with one sentence each: every other form, an empty context, a multi-device
 * context, one with a communicator, a step in flight.
 * fh_screen: the certificate's launches, the norms if they are not held, the test.  report[FH_SCREEN_NOUT] = { rho, features kept, gap_safe, mu };
 * keep: one byte per feature (1 = kept), or NULL.  The preconditions and refusals of fh_dual_gap under its own name (FH_E_ARG), then the logistic loss
 * (FH_E_ARG) and the forms fh_column_norms refuses (FH_E_STATE: the DCT and the convolution store no columns).  Nothing of the context changes but the
 * workspace and the kept norms.
 * fh_gather_columns: dst <- the `count` columns idx[0] < idx[1] < ... of src's dense matrix, device to device, as fh_generate_matrix would have set an
 * (m, count) matrix: dst comes out in vector form and keeps its prox kind and loss as a dense setter keeps them; padding rows and columns are zero.
 * src: a plain context holding a dense matrix (vector or multi-column form), never written.  dst: another plain context on the same device with the same
 * storage.  Refused with one sentence each: dst == src, another device, another storage, an index out of [0, n), indices not strictly increasing,
 * count > n (FH_E_ARG); count == 0 (FH_E_ARG: "every feature is screened: the solution is zero"); a multi-device context, a communicator or a step in
 * flight on either side, a source without a dense matrix, observation weights on dst (FH_E_STATE).  If an allocation fails dst is left without an
 * operator; src is untouched.
 * fh_screen_shape_for: the pure rule, out[FH_SCREEN_SHAPE_LEN] = { rows per slab, slabs, columns per tile, tiles, workgroups of the norms kernel, kappa }
 * for an (m, n) matrix, L columns of the unknown (0 = a vector), on ncu CUs (<= 0: 256).                                                          */
#define FH_SCREEN_NOUT 4
#define FH_SCREEN_SHAPE_LEN 6
int fh_column_norms(fh_ctx* ctx, double* out);
int fh_screen(fh_ctx* ctx, double* report, uint8_t* keep);
int fh_gather_columns(fh_ctx* dst, fh_ctx* src, const int32_t* idx, uint64_t count);
int fh_screen_shape_for(uint64_t m, uint64_t n, uint32_t L, int dtype, int ncu, uint32_t* out);
/* ---- standardised features (csrc/fh_standardize.h; the host statement is fasta_python_amd/preprocess.py: standardize) -------------------------------
 * The matrix the context holds is rewritten in place, in float64 arithmetic, every line one rounded operation:
 *   mean_j = (sum_i a_ij) / m   (center != 0; else 0),      d_ij = a_ij - mean_j   (float32 storage promoted to double first),
 *   scale_j = sqrt((sum_i d_ij^2) / m), 1 where that is 0   (scale != 0; else 1),   a_ij <- d_ij / scale_j   (float32 storage: rounded on the store).
 * Dense operator, vector and multi-column, either storage: the launches of fh_column_norms' geometry (fh_screen_shape_for) -- the sums (skipped
 * when center == 0), the centred squares (skipped when scale == 0), the rewrite of rows i < m and columns j < n: the zero padding of the block
 * stays zero.  Sparse operator: scale alone (centring would fill the matrix), scale_j = sqrt(norms2_j / m) from its by-columns copy, both stored
 * copies divided, identical bits in both.  Ordinary launches, no float atomics, fixed summation order, bitwise repeatable; FH_K_AUX.
 * means, scales: n doubles each on the host, or NULL; the statistics are those of the float64 values before a float32 store rounds them.
 * Afterwards the context is as after an operator setter: no committed state (fh_dual_gap and the others answer as before fh_init), the kept column
 * norms dropped; the prox kind, the loss, b, x0 and the column count stay.  A second call standardises what is there.  If a launch fails the
 * context is left without committed state.  Refused with one sentence each: a null context, center == 0 && scale == 0, center != 0 on the sparse
 * operator (FH_E_ARG); no operator, a form that stores no columns, a multi-device context, a communicator, a step in flight, observation
 * weights (FH_E_STATE).                                                                                                                         */
int fh_standardize(fh_ctx* ctx, int center, int scale, double* means, double* scales);
/* plain operator application on host vectors (tests, synthetic b): adjoint=0: out(m) = A in(n);
 * adjoint=1: out(n) = A^H in(m).                                                                 */
int fh_apply(fh_ctx* ctx, int adjoint, const double* in, double* out);

/* ---- row sharding across PROCESSES: one process per GPU, RCCL communicator by rank (the in-process form is fh_create_ex
 *      with ndev > 1; the two are not combined: these refuse a multi-device context, except fh_comm_count, which reports
 *      its number of shards) ------------------------------------------------------------------------------------------ */
/* writes an ncclUniqueId (128 bytes) -- rank 0 calls it and ships the bytes to the other ranks     */
int fh_comm_unique_id(void* id128);
int fh_comm_init(fh_ctx* ctx, int nranks, int rank, const void* id128);
/* ranks of the attached communicator as RCCL reports them (ncclCommCount); 1 without a communicator */
int fh_comm_count(fh_ctx* ctx, int* nranks);
int fh_comm_destroy(fh_ctx* ctx);
/* Large frees and the allocations behind them.  The driver clears freed device memory in the background (~30 ms per GiB on MI355X); a large
 * allocation made meanwhile is mapped less favourably for its whole lifetime.  The one-pass kernel of rounds 1-5 (rows dealt to the teams in blocks) ran
 * 9-14 % slow on such a matrix (profiles/r06_alloc_settle.txt: 6 of 6 cycles); with the rows dealt cyclically (default since round 6) it does not care
 * (profiles/r06_placement.txt: 3 of 3).  Per device:
 *   - the matrix block (>= 1 GiB) a context gives up (fh_destroy, a new fh_set_matrix / fh_generate_matrix / fh_set_stencil) is KEPT, one block
 *     per device, and handed to the next matrix on that device that fits it and fills at least half of it: no clearing, no new mapping, no
 *     waiting.  The memory stays allocated until then: fh_release_cached(device | -1 = all) returns it to the driver, fh_alloc_cache(0)
 *     switches the keeping off (and releases), fh_alloc_cache_hits counts the re-uses;
 *   - fh_alloc_settle(1) (default 0 since the cyclic dealing): a matrix of >= 1 GiB that no kept block serves is allocated only after the device's
 *     earlier large frees have presumably been cleared (35 ms per GiB behind the free) -- for callers that select the blocked dealing or live on the
 *     two-launch path, whose K-adj still depends on the mapping; fh_alloc_settle_waited returns the seconds spent in it.                     */
int fh_alloc_settle(int enable);
int fh_alloc_settle_waited(double* seconds);
int fh_alloc_cache(int enable);
int fh_release_cached(int device);
int fh_alloc_cache_hits(uint64_t* hits);

/* RCCL's version code as ncclGetVersion reports it; -1 when no library is loaded yet or it does not export the symbol           */
int fh_comm_version(int* version);
/* The context's exchange (the rank's all-reduce, or a multi-device context's grouped all-reduce / in-library sum) on a known
 * pattern of `count` doubles, checked against its closed-form sum: max_abs_err must come back 0, nblocks = the ranks / row blocks
 * summed over.  COLLECTIVE on a context with a communicator.  The multi-GPU preflight's first contact with RCCL
 * (fasta_python_amd/preflight.py); the op being sharded is `A.T @ x`, fasta/linalg.py:41.                                      */
int fh_comm_selftest(fh_ctx* ctx, uint64_t count, double* max_abs_err, int* nblocks);
/* path of the library the collectives' entry points were taken from: the system's RCCL, or what $FASTA_RCCL_LIB names (a
 * substitution is also announced once on stderr); "" before the first communicator                                         */
const char* fh_comm_library(void);
/* CUs the device reports, and CUs the dense one-pass kernel is launched on (FH_TUNE_FUSED_CUS)                               */
int fh_cu_count(fh_ctx* ctx, int* device_cus, int* one_pass_cus);

/* ---- measurement: HIP-event timing of each launch on the context's stream ---------------------
 * A multi-device context reports sums over its row blocks.  When the blocks share ONE device (a repeated device id: one stream) only
 * ONE block's launches carry event records -- the MIDDLE block's (index nblocks / 2; the first one starts on an idle device and reads
 * high) -- and the figures are that block's scaled by the number of blocks: an ESTIMATE (row blocks may differ by one row), taken
 * because two records around each of the 8 x 2 launches cost more than the plumbing being measured (profiles/r04_inproc_issue.txt).
 * The sum over the blocks (FH_K_COMM) is one launch and is timed as such.                                                        */
int fh_timing_enable(fh_ctx* ctx, int on);
int fh_timing_get(fh_ctx* ctx, int kernel_id, double* total_ms, uint64_t* launches);
int fh_timing_reset(fh_ctx* ctx);
/* Did the latest timed launch of `kernel_id` on context a and on context b (plain contexts on one device, timing enabled, both
 * waited for) run at the same time?  a_ms / b_ms: the two launches' durations; overlap_ms: how long both were running
 * (<= 0: one had ended before the other began).  From the HIP events that bracket each launch on its own stream.              */
int fh_timing_overlap(fh_ctx* a, fh_ctx* b, int kernel_id, double* a_ms, double* b_ms, double* overlap_ms);
/* streaming-read ceiling: one read-only pass over the device copy of A by k_stream_probe<16,1> (csrc/fh_dense.h): one persistent
 * workgroup per CU (FH_TUNE_FWD_GRID_CAP overrides), three rotating register buffers of 16 non-temporal 16-byte loads per lane
 * (32 loads in flight behind the buffer being summed), loads + adds only; returns ms per pass.  A multi-device context
 * measures shard 0's row block.                                                                                           */
int fh_stream_read_ms(fh_ctx* ctx, int reps, double* ms_per_pass, uint64_t* bytes_per_pass);

#ifdef __cplusplus
}
#endif
#endif /* FASTA_HIP_H */

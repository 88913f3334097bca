// fh_host_launch.h -- kernel launchers of libfasta_hip.so: shapes, grids and workspace of every kernel in fh_dense.h / fh_quad.h / fh_bilinear.h / fh_tv.h / fh_tv3d.h / fh_dct.h / fh_dct2.h / fh_conv.h /
// fh_prox.h / fh_fused.h, the one-pass kernel's shape rule and dispatch table, the co-residency probe, and the three-stage form
// (local launch / sum over row blocks / n-side epilogue) the C ABI in fasta_hip.hip builds its entry points from.
#pragma once

// ------------------------------------------------------------------------------------------------
// kernel launchers
// ------------------------------------------------------------------------------------------------
static ProxP make_prox(fh_ctx* c, double tau) {
  ProxP px;
  px.kind = c->prox_kind;
  px.thr = tau * c->mu;               // `t*self.mu`, examples/sparse_least_squares.py:44
  px.lo = c->lo; px.hi = c->hi;
  px.level = c->dscal + FH_NSCALARS;  // device scalar written by the level search
  px.seq = 0;
  return px;
}

// K-fwd / K-adj: non-temporal loads of A (+10 % on matrices that only stream through) -- except for a matrix of at most 256 MiB, the size of the device's
// last-level cache, which the next launch finds there again if it was loaded with the default policy: 4096^2 K-adj 0.049 against 0.075 ms, 5120^2 0.063 / 0.088,
// K-fwd 0.030 / 0.033; from 8192^2 (512 MiB) on the non-temporal form is the faster one again (profiles/r06_placement.txt, section 11).  The one-pass kernels
// always load non-temporally (plain: +-3 % at these sizes, where their time is mostly fixed cost).
static inline int nt_rule(int nt_loads, uint64_t mp, uint64_t ld, int f32) {
  if (nt_loads >= 0) return nt_loads;
  return mp * ld * (f32 ? 4u : 8u) > ((uint64_t)256 << 20);
}
static inline int nt_for(const fh_ctx* c) { return nt_rule(c->nt_loads, c->mp, c->ld, c->f32); }

template <int R, int KIND>
static void launch_fwd_rk(fh_ctx* c, const FwdP& p, unsigned grid) {
  if (c->f32) {                                   // float32 storage: non-temporal loads only, R = 4 or 8
    if constexpr (R == 16) k_fwd_dense<8, 1, KIND, 1><<<dim3(grid), dim3(FH_WG), 0, c->stream>>>(p);
    else k_fwd_dense<R, 1, KIND, 1><<<dim3(grid), dim3(FH_WG), 0, c->stream>>>(p);
  }
  else if (nt_for(c)) k_fwd_dense<R, 1, KIND><<<dim3(grid), dim3(FH_WG), 0, c->stream>>>(p);
  else k_fwd_dense<R, 0, KIND><<<dim3(grid), dim3(FH_WG), 0, c->stream>>>(p);
}
template <int R>
static void launch_fwd_r(fh_ctx* c, const FwdP& p, unsigned grid, int kind) {
  switch (kind) {
    case PX_PLAIN:  launch_fwd_rk<R, PX_PLAIN>(c, p, grid); break;
    case PX_SHRINK: launch_fwd_rk<R, PX_SHRINK>(c, p, grid); break;
    case PX_NONNEG: launch_fwd_rk<R, PX_NONNEG>(c, p, grid); break;
    case PX_LINF:   launch_fwd_rk<R, PX_LINF>(c, p, grid); break;
    case PX_L1BALL: launch_fwd_rk<R, PX_L1BALL>(c, p, grid); break;
    case PX_BOX:    launch_fwd_rk<R, PX_BOX>(c, p, grid); break;
    default:        launch_fwd_rk<R, PX_IDENTITY>(c, p, grid); break;
  }
}

// z := A * (mode 0: prox(x0 - tau g0) ; mode 1: x0) on the dense operator
static int launch_fwd_dense(fh_ctx* c, const FwdIO& io) {
  // rows per pass (sweep, profiles/r01_tune_sizes.txt): 4 up to n = 32768, 8 beyond
  // float32 storage: the x0/g0 pieces of a trip are twice as many per byte of A, so it takes 8 rows per pass from n = 32768 on
  // to keep as many bytes of A in flight (4 rows: 4.7 TB/s at 65536^2, profiles/r02_f32_storage.txt)
  int R = c->fwd_rows ? c->fwd_rows : (c->ld <= (c->f32 ? 16384u : 32768u) ? 4 : 8);
  if (c->f32 && R == 16) R = 8;
  if (io.mode == 0) FH_TRY(check_prox_run(c));
  FwdP p;
  p.A = c->A; p.ld = c->ld; p.ld2 = (uint32_t)(c->ld / (c->f32 ? 4 : 2)); p.nv2 = (uint32_t)(c->nv / 2); p.n = (uint32_t)c->n; p.m = (uint32_t)c->m;
  p.nrg = (uint32_t)(c->mp / R);
  p.nchunks = (p.nv2 + FH_WG - 1) / FH_WG;
  p.x0 = io.x0; p.g0 = io.g0; p.xacc0 = io.xacc0; p.xhat = io.xhat; p.xp = io.xp;
  p.b = c->b; p.z = io.z; p.tau = io.tau; p.sub_b = io.sub_b; p.loss = c->loss_kind;
  p.px = make_prox(c, io.tau);
  const int kind = io.mode == 0 ? c->prox_kind : (int)PX_PLAIN;
  unsigned grid = std::max(p.nrg, io.mode == 0 ? p.nchunks : 1u);
  // measured on MI355X (profiles/r01_tune_dense.txt, r01_tune_sizes.txt): 2 persistent workgroups per CU
  // grid-striding over the row groups beat one workgroup per row group by 5-12 %
  grid = (unsigned)std::min<long long>(grid, c->fwd_cap > 0 ? c->fwd_cap : 512);
  const size_t need = ((size_t)p.nchunks * 8 + grid) * sizeof(double);
  FH_TRY(ensure_ws(c, need));
  p.red_n = c->ws; p.red_m = c->ws + (size_t)p.nchunks * 8;
  p.counter = c->counters + CNT_FWD;
  p.out = scalar_out(c);
  t_begin(c, FH_K_FWD);
  p.px.seq = seq_offer(c);
  switch (R) {
    case 4: launch_fwd_r<4>(c, p, grid, kind); break;
    case 16: launch_fwd_r<16>(c, p, grid, kind); break;
    default: launch_fwd_r<8>(c, p, grid, kind); break;
  }
  t_end(c, FH_K_FWD);
  HIP_TRY(hipGetLastError());
  return 0;
}

template <int CPT>
static void launch_adj_c(fh_ctx* c, const AdjP& p, unsigned grid) {
  if (c->f32) k_adj_dense<CPT, 1, 1><<<dim3(grid), dim3(FH_WG), 0, c->stream>>>(p);
  else if (nt_for(c)) k_adj_dense<CPT, 1><<<dim3(grid), dim3(FH_WG), 0, c->stream>>>(p);
  else k_adj_dense<CPT, 0><<<dim3(grid), dim3(FH_WG), 0, c->stream>>>(p);
}

struct AdjIO {
  const double* z; const double* zacc0; int sub_b; int accel; double coef; int mode; double tau;
  const double* x0; const double* xp; const double* xacc0; const double* xhat; double* x1; double* g1;
  const double* g0;   // stencil path only: K-adj recomputes xhat = x0 - tau*g0
};

static int launch_adj_dense(fh_ctx* c, const AdjIO& io) {
  AdjP p;
  p.A = c->A; p.ld = c->ld; p.ld2 = (uint32_t)(c->ld / (c->f32 ? 4 : 2)); p.nv2 = (uint32_t)(c->nv / 2);
  p.n = (uint32_t)c->n; p.mp = (uint32_t)c->mp; p.m = (uint32_t)c->m;
  // auto rules from the MI355X sweeps (profiles/r01_tune_dense.txt, r01_tune_sizes.txt): about 32 slabs
  // (more when there are few column chunks, so that >= 128 workgroups exist), slabs of 32..2048 rows, and
  // column chunks of 2 x 16 B per lane below n = 32768, 4 x 16 B from there on (1 x for n <= 1024).
  int CPT = c->adj_cpt;
  if (CPT == 0) CPT = p.ld2 <= 512 ? 1 : (p.ld2 < 16384 ? 2 : 4);
  p.ncc = (p.ld2 + FH_WG * CPT - 1) / (FH_WG * CPT);
  uint32_t slab = (uint32_t)c->adj_slab;
  if (slab == 0) {
    // (float32 storage has half the column chunks per row: aim for the same ~1024 workgroups the float64 matrix gets at C2)
    const uint64_t target_slabs = std::max<uint64_t>(32, ((c->f32 ? 1024 : 128) + p.ncc - 1) / p.ncc);
    const uint64_t slab_min = p.ncc >= 8 ? 128 : 32;
    uint64_t s = round_up((c->mp + target_slabs - 1) / target_slabs, 8);
    slab = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(s, slab_min), ADJ_MAX_SLAB);
  }
  p.slab_rows = slab;
  p.nslab = (uint32_t)((c->mp + slab - 1) / slab);
  // K-adj keeps its contiguous slabs: dealt cyclically (FH_TUNE_ADJ_CYCLIC = 1) it is 1-14 % faster on some small and mid shapes but 6 % SLOWER at 65536^2 and not
  // less dependent on where the matrix lies (its workgroups are not in lockstep as the one-pass kernel's teams are; profiles/r06_placement.txt)
  p.cyclic = c->adj_cyclic == 1;
  if (p.ncc + CNT_ADJ_CC > (uint32_t)CNT_DIAG) return fail(FH_E_ARG, "too many column chunks (%u)", p.ncc);
  p.z = io.z; p.zacc0 = io.zacc0; p.b = c->b; p.sub_b = io.sub_b; p.loss = c->loss_kind; p.accel = io.accel; p.coef = io.coef;
  p.mode = io.mode; p.tau = io.tau;
  p.x0 = io.x0; p.xp = io.xp; p.xacc0 = io.xacc0; p.xhat = io.xhat; p.x1 = io.x1; p.g1 = io.g1;
  const size_t gpart_elems = (size_t)p.nslab * c->ld;
  const size_t need = (gpart_elems + (size_t)p.ncc * 8 + p.nslab) * sizeof(double);
  FH_TRY(ensure_ws(c, need));
  p.gpart = c->ws; p.red_bb = c->ws + gpart_elems; p.red_f = p.red_bb + (size_t)p.ncc * 8;
  p.cc_counter = c->counters + CNT_ADJ_CC; p.fin_counter = c->counters + CNT_ADJ_FIN;
  p.out = scalar_out(c);
  const unsigned grid = p.ncc * p.nslab;
  t_begin(c, FH_K_ADJ);
  p.seq = io.mode == 0 ? seq_offer(c) : 0u;      // (the plain-gradient / sharded forms are followed by further launches)
  switch (CPT) {
    case 1: launch_adj_c<1>(c, p, grid); break;
    case 4: launch_adj_c<4>(c, p, grid); break;
    default: launch_adj_c<2>(c, p, grid); break;
  }
  t_end(c, FH_K_ADJ);
  HIP_TRY(hipGetLastError());
  return 0;
}

// ---- multi-column form (fh_set_rhs; kernels in csrc/fh_multi.h, instantiated by fh_multi_part.hip) ---------------------------------------
#ifndef FH_SINGLE_TU
#define MC_DECLARE(LB, CH, R) MC_KERNELS(extern template, LB, CH, R)
MC_FOR_EACH(MC_DECLARE)
#undef MC_DECLARE
#endif
struct McEntry {
  int lb, ch, rows; void (*pro)(const McProP); void (*pack)(const double*, double*, uint32_t, uint32_t);
  void (*fwd[2])(const McFwdP); void (*adj[2])(const McAdjP);
};
#define MC_ROW(LB, CH, R) {LB, CH, R, k_mc_prologue<LB>, k_mc_pack<LB>, {k_mc_fwd<LB, CH, R, 0>, k_mc_fwd<LB, CH, R, 1>}, {k_mc_adj<LB, MC_ADJ_CPT, 0>, k_mc_adj<LB, MC_ADJ_CPT, 1>}},
static const McEntry kMcTable[] = { MC_FOR_EACH(MC_ROW) };
#undef MC_ROW
static const McEntry* mc_entry_lb(uint32_t LB) {
  for (const McEntry& e : kMcTable) if ((uint32_t)e.lb == LB) return &e;
  return nullptr;
}
static const McEntry* mc_entry(const fh_ctx* c) { return mc_entry_lb(c->LB); }

// THE GEOMETRY of both multi-column launches, stated once: a pure function of the device shape (mp rows of ld doubles, nv rows of X), the
// columns per row LB and the three tuning values (FH_TUNE_ADJ_SLAB_ROWS, FH_TUNE_FWD_GRID_CAP, FH_TUNE_NT_LOADS as the context keeps them:
// 0 / 0 / -1 = auto).  The launchers below take every number from here; fh_multi_shape / fh_multi_shape_for export it so that a test can
// assert the path it meant to reach (and the pure form needs no device).  `e` = nullptr when no kernel serves LB.
struct McShape {
  const McEntry* e;
  int nt;                            // 1: the non-temporal instantiations
  uint32_t ld2;                      // 16-byte pieces per device row of A = row pairs of X
  uint32_t fwd_grid, nrg, ntrip;     // K-fwd: workgroups, row groups of R rows they stride over, trips of a lane group along a row
  uint32_t npro;                     // workgroups of the n-side prologue (mode 0) / of the pack launch (mode 1)
  uint32_t slab_rows, nslab, last_rows, sb, stages, ncc;   // K-adj: slabs, rows of the last one, rows per residual stage, stages of a full slab, column chunks
};
static McShape mc_shape_for(uint64_t mp, uint64_t ld, uint64_t nv, uint32_t LB, int adj_slab, long long fwd_cap, int nt_loads) {
  McShape s;
  memset(&s, 0, sizeof(s));
  s.e = mc_entry_lb(LB);
  if (!s.e) return s;
  s.nt = nt_rule(nt_loads, mp, ld, 0) ? 1 : 0;
  s.ld2 = (uint32_t)(ld / 2);
  s.nrg = (uint32_t)(mp / (uint64_t)s.e->rows);
  s.fwd_grid = (uint32_t)std::min<long long>(s.nrg, fwd_cap > 0 ? fwd_cap : 512);
  const uint32_t GL = FH_WG / (uint32_t)(s.e->lb / s.e->ch);          // lanes of a column group (k_mc_fwd)
  s.ntrip = (s.ld2 + GL - 1) / GL;
  s.npro = (uint32_t)((nv + FH_WG - 1) / FH_WG);
  s.ncc = (s.ld2 + FH_WG * MC_ADJ_CPT - 1) / (FH_WG * MC_ADJ_CPT);
  // the vector kernel's slab rule (about 32 slabs, more when there are few column chunks): a slab's rows are staged 2048 / LB at a time
  uint32_t slab = (uint32_t)adj_slab;
  if (slab == 0) {
    const uint64_t target_slabs = std::max<uint64_t>(32, (128 + s.ncc - 1) / s.ncc);
    const uint64_t slab_min = s.ncc >= 8 ? 128 : 32;
    const uint64_t r = round_up((mp + target_slabs - 1) / target_slabs, 8);
    slab = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(r, slab_min), ADJ_MAX_SLAB);
  }
  s.slab_rows = slab;
  s.nslab = (uint32_t)((mp + slab - 1) / slab);
  s.last_rows = (uint32_t)(mp - (uint64_t)(s.nslab - 1) * slab);
  s.sb = MC_LDS_DOUBLES / LB;
  s.stages = (slab + s.sb - 1) / s.sb;
  return s;
}
static McShape mc_shape(const fh_ctx* c) { return mc_shape_for(c->mp, c->ld, c->nv, c->LB, c->adj_slab, c->fwd_cap, c->nt_loads); }

static void mc_shape_report(const McShape& s, uint32_t* out) {
  const uint32_t v[FH_MULTI_SHAPE_LEN] = {(uint32_t)s.e->lb, (uint32_t)s.e->ch, (uint32_t)s.e->rows, (uint32_t)s.nt, s.fwd_grid, s.nrg, s.ntrip, s.npro,
                                          s.slab_rows, s.nslab, s.last_rows, s.sb, s.stages, s.ncc};
  memcpy(out, v, sizeof(v));
}
// read-only: the geometry the next fh_fwd / fh_adj of this context launches with
extern "C" int fh_multi_shape(fh_ctx* c, uint32_t* out) {
  if (!c || !out) return fail(FH_E_ARG, "fh_multi_shape: null argument");
  if (c->op != OP_DENSE || !c->LB) return fail(FH_E_STATE, "fh_multi_shape: the context is not in multi-column dense form (fh_set_matrix + fh_set_rhs)");
  const McShape s = mc_shape(c);
  if (!s.e) return fail(FH_E_STATE, "multi-column form: no kernel for %u columns per row", c->LB);
  mc_shape_report(s, out);
  return 0;
}
// ... and the same rule for an (m, n) matrix with L columns that no context holds: a pure host function, no device needed
extern "C" int fh_multi_shape_for(uint64_t m, uint64_t n, uint32_t L, int slab_rows, long long grid_cap, int nt_loads, uint32_t* out) {
  if (!out) return fail(FH_E_ARG, "fh_multi_shape_for: null argument");
  if (m == 0 || n == 0 || m >= (1ull << 31) || n >= (1ull << 31)) return fail(FH_E_ARG, "fh_multi_shape_for: matrix dimensions must be in [1, 2^31)");
  if (L < 1 || L > 16) return fail(FH_E_ARG, "fh_multi_shape_for: 1 to 16 columns (got %u)", L);
  if (slab_rows < 0 || slab_rows > ADJ_MAX_SLAB || slab_rows % 8) return fail(FH_E_ARG, "ADJ_SLAB_ROWS must be a multiple of 8 in [0,%d]", ADJ_MAX_SLAB);
  if (grid_cap < 0) return fail(FH_E_ARG, "FWD_GRID_CAP must be >= 0");
  if (nt_loads < -1 || nt_loads > 1) return fail(FH_E_ARG, "fh_multi_shape_for: nt_loads is -1 (auto), 0 or 1");
  const uint32_t LB = lb_for(L);
  const uint64_t ld = round_up(n, 16);
  const McShape s = mc_shape_for(round_up(m, 16), ld, ld, LB, slab_rows, grid_cap, nt_loads);
  if (!s.e) return fail(FH_E_STATE, "multi-column form: no kernel for %u columns per row", LB);
  mc_shape_report(s, out);
  return 0;
}

// ---- softmax loss on a matrix unknown (fh_set_loss_softmax; row kernel in csrc/fh_softmax.h, instantiated by fh_softmax_part.hip) -----------
#ifndef FH_SINGLE_TU
#define SM_DECLARE(LB) SM_KERNELS(extern template, LB)
SM_FOR_EACH_LB(SM_DECLARE)
#undef SM_DECLARE
#endif
struct SmEntry { int lb; void (*rows)(const SmRowsP); };
#define SM_ROW(LB) {LB, k_sm_rows<LB>},
static const SmEntry kSmTable[] = { SM_FOR_EACH_LB(SM_ROW) };
#undef SM_ROW
// does this launch evaluate the softmax loss?  (sub_b = 0 is the plain operator: fh_apply)
static inline bool sm_on(const fh_ctx* c, int sub_b) { return sub_b && c->loss_kind == LOSS_SOFTMAX; }
static inline uint32_t sm_records(const fh_ctx* c) { return (uint32_t)((c->m * (uint64_t)(c->LB / 2) + FH_WG - 1) / FH_WG); }
// the row pass over Z' (Z, or its extrapolation): residual into `r` (nullptr: value only), sm_records(c) loss records into `red_f`.
// finalise: its last workgroup adds the records into out[slot] and publishes `seq`; otherwise the caller's next launch consumes them.
static int launch_sm_rows(fh_ctx* c, const double* z, const double* zacc0, int accel, double coef, double* r, double* red_f,
                          bool finalise, int slot, unsigned seq) {
  const SmEntry* e = nullptr;
  for (const SmEntry& k : kSmTable) if ((uint32_t)k.lb == c->LB) e = &k;
  if (!e) return fail(FH_E_STATE, "softmax loss: no kernel for %u columns per row", c->LB);
  SmRowsP q;
  q.m = (uint32_t)c->m; q.L = c->L; q.z = z; q.zacc0 = zacc0; q.b = c->b; q.r = r;
  q.accel = accel; q.coef = coef; q.red_f = red_f;
  q.counter = finalise ? c->counters + CNT_AUX : nullptr;
  q.out = scalar_out(c); q.slot = slot; q.seq = seq;
  e->rows<<<dim3(sm_records(c)), dim3(FH_WG), 0, c->stream>>>(q);
  return 0;
}

// Z := A * (mode 0: prox(X0 - tau G0), by the prologue launch ; mode 1: X0) for LB columns from one read of A
static int launch_fwd_multi(fh_ctx* c, const FwdIO& io) {
  const McShape sh = mc_shape(c);
  const McEntry* e = sh.e;
  if (!e) return fail(FH_E_STATE, "multi-column form: no kernel for %u columns per row", c->LB);
  FH_TRY(check_loss_run(c));
  if (io.mode == 0) FH_TRY(check_prox_run(c));
  const bool sm = sm_on(c, io.sub_b);             // K-fwd's sum of squares means nothing then: the row pass behind it writes FH_S_FSQ and publishes
  McFwdP p;
  p.A = c->A; p.ld2 = sh.ld2; p.m = (uint32_t)c->m; p.L = c->L;
  p.nrg = sh.nrg;
  const uint32_t npro = io.mode == 0 ? sh.npro : 0u;
  p.nred_n = npro;
  const unsigned grid = sh.fwd_grid;
  FH_TRY(ensure_ws(c, ((size_t)npro * 8 + grid + (sm ? sm_records(c) : 0u)) * sizeof(double)));
  p.red_n = c->ws; p.red_m = c->ws + (size_t)npro * 8;
  p.x = c->xs;                      // the operand in K-fwd's streaming layout: written by the prologue, or packed from a plain operand below
  p.b = c->b; p.z = io.z; p.sub_b = io.sub_b;
  p.counter = c->counters + CNT_FWD;
  p.out = scalar_out(c);
  t_begin(c, FH_K_FWD);
  if (io.mode == 0) {
    McProP q;
    q.n = (uint32_t)c->n; q.L = c->L; q.nv = (uint32_t)c->nv;
    q.x0 = io.x0; q.g0 = io.g0; q.xacc0 = io.xacc0; q.xhat = io.xhat; q.xp = io.xp; q.tau = io.tau;
    q.xs = c->xs; q.ld2 = p.ld2;
    q.px = make_prox(c, io.tau);
    q.red_n = c->ws;
    e->pro<<<dim3(npro), dim3(FH_WG), 0, c->stream>>>(q);
  } else {
    e->pack<<<dim3(sh.npro), dim3(FH_WG), 0, c->stream>>>(io.x0, c->xs, (uint32_t)c->nv, p.ld2);
  }
  p.seq = sm ? 0u : seq_offer(c);
  e->fwd[sh.nt]<<<dim3(grid), dim3(FH_WG), 0, c->stream>>>(p);
  if (sm) FH_TRY(launch_sm_rows(c, io.z, nullptr, 0, 0.0, nullptr, p.red_m + grid, true, FH_S_FSQ, seq_offer(c)));
  t_end(c, FH_K_FWD);
  HIP_TRY(hipGetLastError());
  return 0;
}

// ---- sparse operator (fh_set_matrix_csr; kernels in csrc/fh_sparse.h, instantiated by fh_sparse_part.hip) -------------------------------
#ifndef FH_SINGLE_TU
#define SP_DECLARE(G) SP_KERNELS(extern template, G)
SP_FOR_EACH(SP_DECLARE)
#undef SP_DECLARE
#endif
struct SpEntry { int g; void (*fwd[2])(const SpFwdP); void (*adj[2])(const SpAdjP); };
#define SP_ROW(G) {G, {k_sp_fwd<G, 0>, k_sp_fwd<G, 1>}, {k_sp_adj<G, 0>, k_sp_adj<G, 1>}},
static const SpEntry kSpTable[] = { SP_FOR_EACH(SP_ROW) };
#undef SP_ROW
static const SpEntry* sp_entry(int g) {
  for (const SpEntry& e : kSpTable) if (e.g == g) return &e;
  return nullptr;
}
// values and indices stream once and were the non-temporal candidates; measured (profiles/sparse_rows.txt), plain loads are as fast or faster at every
// shape (65536^2: 0.1 % 0.129 against 0.147 ms per pair, 1 % 0.550 / 0.557, 5 % 2.063 / 2.162; 1048576^2, 16 per row: 0.522 / 0.523), so plain is the
// default and FH_TUNE_NT_LOADS = 1 the opt-in
static inline int sp_nt_for(const fh_ctx* c) { return c->nt_loads > 0 ? 1 : 0; }

// z := A * (mode 0: prox(x0 - tau g0), by the prologue launch ; mode 1: x0)
static int launch_fwd_sparse(fh_ctx* c, const FwdIO& io) {
  const SpEntry* e = sp_entry(c->sp_G[0]);
  if (!e) return fail(FH_E_STATE, "sparse operator: no kernel for %d lanes per row", c->sp_G[0]);
  if (io.mode == 0) FH_TRY(check_prox_run(c));
  SpFwdP p;
  p.a = c->sp[0]; p.m = (uint32_t)c->m;
  const uint32_t npro = io.mode == 0 ? (uint32_t)((c->n + FH_WG - 1) / FH_WG) : 0u;
  p.nred_n = npro;
  const unsigned grid = p.a.nwg + p.a.nlong;
  FH_TRY(ensure_ws(c, ((size_t)npro * 8 + grid) * sizeof(double)));
  p.red_n = c->ws; p.red_m = c->ws + (size_t)npro * 8;
  p.x = io.mode == 0 ? io.xp : io.x0;
  p.b = c->b; p.z = io.z; p.sub_b = io.sub_b; p.loss = c->loss_kind;
  p.counter = c->counters + CNT_FWD;
  p.out = scalar_out(c);
  t_begin(c, FH_K_FWD);
  if (io.mode == 0) {
    SpProP q;
    q.n = (uint32_t)c->n; q.x0 = io.x0; q.g0 = io.g0; q.xacc0 = io.xacc0; q.xhat = io.xhat; q.xp = io.xp; q.tau = io.tau;
    q.px = make_prox(c, io.tau);
    q.red_n = c->ws;
    k_sp_prologue<<<dim3(npro), dim3(FH_WG), 0, c->stream>>>(q);
  }
  p.seq = seq_offer(c);
  e->fwd[sp_nt_for(c) ? 1 : 0]<<<dim3(grid), dim3(FH_WG), 0, c->stream>>>(p);
  t_end(c, FH_K_FWD);
  HIP_TRY(hipGetLastError());
  return 0;
}

// n-side epilogue as its own launch (row-sharded runs, after the all-reduce of g1)
static int bb_epilogue_only(fh_ctx* c, const AdjIO& io, const double* fsq_src, const double* coef_src = nullptr, const double* pack = nullptr) {
  AdjP p;
  memset(&p, 0, sizeof(p));
  p.ld = c->nv; p.ld2 = (uint32_t)(c->nv / 2); p.nv2 = p.ld2; p.n = (uint32_t)c->n;
  p.accel = io.accel; p.coef = io.coef; p.mode = 0; p.tau = io.tau;
  p.x0 = io.x0; p.xp = io.xp; p.xacc0 = io.xacc0; p.xhat = io.xhat; p.x1 = io.x1; p.g1 = io.g1;
  const uint32_t nchunks = (p.ld2 + FH_WG - 1) / FH_WG;
  FH_TRY(ensure_ws(c, (size_t)nchunks * 8 * sizeof(double)));
  p.red_bb = c->ws; p.fin_counter = c->counters + CNT_AUX; p.out = c->dscal;
  t_begin(c, FH_K_AUX);
  k_bb_epilogue<<<dim3(nchunks), dim3(FH_WG), 0, c->stream>>>(p, nchunks, fsq_src, coef_src, pack, c->hscal_dev);
  c->scal_mirrored = true;         // (always the last launch before the caller's fetch_scalars)
  t_end(c, FH_K_AUX);
  HIP_TRY(hipGetLastError());
  return 0;
}

static int launch_adj_multi(fh_ctx* c, const AdjIO& io) {
  const McShape sh = mc_shape(c);
  const McEntry* e = sh.e;
  if (!e) return fail(FH_E_STATE, "multi-column form: no kernel for %u columns per row", c->LB);
  if (io.sub_b) FH_TRY(check_loss_run(c));
  if (io.mode != 0 && io.mode != 1) return fail(FH_E_STATE, "the multi-column form has no row-sharded adjoint");
  const bool sm = sm_on(c, io.sub_b);
  if (sm && !c->sp_r) return fail(FH_E_STATE, "softmax loss: the residual buffer is missing (call fh_set_loss_softmax after fh_set_rhs)");
  McAdjP p;
  p.A = c->A; p.ld2 = sh.ld2; p.n = (uint32_t)c->n; p.L = c->L; p.mp = (uint32_t)c->mp; p.m = (uint32_t)c->m;
  p.ncc = sh.ncc;
  p.slab_rows = sh.slab_rows;
  p.nslab = sh.nslab;
  if (p.ncc + CNT_ADJ_CC > (uint32_t)CNT_DIAG) return fail(FH_E_ARG, "too many column chunks (%u)", p.ncc);
  p.z = io.z; p.zacc0 = io.zacc0; p.b = c->b; p.sub_b = io.sub_b; p.accel = io.accel; p.coef = io.coef;
  p.mode = io.mode; p.tau = io.tau; p.group = c->prox_kind == FH_PROX_GROUP ? 1 : 0;
  p.x0 = io.x0; p.xp = io.xp; p.xacc0 = io.xacc0; p.xhat = io.xhat; p.x1 = io.x1; p.g1 = io.g1;
  const size_t gpart_elems = (size_t)p.nslab * c->ld * c->LB;
  if ((uint64_t)c->ld * c->LB / 2 >= ((uint64_t)1 << 27)) return fail(FH_E_ARG, "multi-column K-adj: n * LB too large for one slab partial");
  FH_TRY(ensure_ws(c, (gpart_elems + (size_t)p.ncc * 8 + p.nslab + (sm ? sm_records(c) : 0u)) * sizeof(double)));
  p.gpart = c->ws; p.red_bb = c->ws + gpart_elems; p.red_f = p.red_bb + (size_t)p.ncc * 8;
  double* sm_red = p.red_f + p.nslab;
  p.cc_counter = c->counters + CNT_ADJ_CC; p.fin_counter = c->counters + CNT_ADJ_FIN;
  p.out = scalar_out(c);
  const unsigned grid = p.ncc * p.nslab;
  t_begin(c, FH_K_ADJ);
  if (sm) {
    // The row pass forms the residual R = softmax(Z') - Y at the (extrapolated) Z' and the loss records; K-adj then takes R as a residual that is
    // already formed: no right-hand side (sub_b = 0), and R as its own extrapolation partner -- extrapolate(R, R, coef) = R + coef * (R - R) is R
    // exactly for finite R and coef -- so its code is the least-squares launch's, instruction for instruction.  Its sum of squares of R in
    // FH_S_FSQ_ADJ means nothing: it publishes no sequence number, and the one-workgroup launch behind it writes the loss there and publishes.
    FH_TRY(launch_sm_rows(c, io.z, io.zacc0, io.accel, io.coef, c->sp_r, sm_red, false, 0, 0u));
    p.z = c->sp_r; p.zacc0 = c->sp_r; p.sub_b = 0;
    p.seq = 0u;
    e->adj[sh.nt]<<<dim3(grid), dim3(FH_WG), 0, c->stream>>>(p);
    k_sm_finish<<<dim3(1), dim3(FH_WG), 0, c->stream>>>(sm_red, sm_records(c), p.out, FH_S_FSQ_ADJ, io.mode == 0 ? seq_offer(c) : 0u);
  } else {
    p.seq = io.mode == 0 ? seq_offer(c) : 0u;
    e->adj[sh.nt]<<<dim3(grid), dim3(FH_WG), 0, c->stream>>>(p);
  }
  t_end(c, FH_K_ADJ);
  HIP_TRY(hipGetLastError());
  return 0;
}

// ---- quadratic smooth term on a symmetric matrix (fh_set_quadratic; kernels in csrc/fh_quad.h, instantiated by fh_quad_part.hip) ---------------
#ifndef FH_SINGLE_TU
#define QD_DECLARE(LB, CH, R) QD_KERNELS(extern template, LB, CH, R)
MC_FOR_EACH(QD_DECLARE)
#undef QD_DECLARE
#endif
struct QdEntry { int lb, ch, rows; void (*pro)(const McProP); void (*fwd[2])(const QdFwdP); void (*grad)(const QdGradP); };
#define QD_ROW(LB, CH, R) {LB, CH, R, k_qd_prologue<LB>, {k_qd_fwd<LB, CH, R, 0>, k_qd_fwd<LB, CH, R, 1>}, k_qd_grad<LB>},
static const QdEntry kQdTable[] = { MC_FOR_EACH(QD_ROW) };
#undef QD_ROW
static const QdEntry* qd_entry_lb(uint32_t LB) {
  for (const QdEntry& e : kQdTable) if ((uint32_t)e.lb == LB) return &e;
  return nullptr;
}

// THE GEOMETRY of the quadratic launches, stated once: a pure function of the device shape (mp rows of ld doubles, nv rows of X), the columns per
// row LB and the tuning values FH_TUNE_FWD_GRID_CAP and FH_TUNE_NT_LOADS as the context keeps them (0 / -1 = auto).  Both launchers take every
// number from here; fh_quad_shape / fh_quad_shape_for export it.  `e` = nullptr when no kernel serves LB.
struct QdShape {
  const QdEntry* e;
  int nt;
  uint32_t ld2;                      // 16-byte pieces per device row of Q = row pairs of X
  uint32_t fwd_grid, nrg, ntrip;     // K-fwd: workgroups, row groups of R rows they stride over, trips of a lane group along a row
  uint32_t last_live;                // lanes of a lane group whose piece of the last trip lies inside the row
  uint32_t pass_max, pass_min;       // passes of the busiest and of the idlest workgroup of K-fwd
  uint32_t npro, ngrad;              // workgroups of the prologue (mode 0) / pack launch (mode 1), and of the elementwise gradient launch
};
static QdShape qd_shape_for(uint64_t mp, uint64_t ld, uint64_t nv, uint32_t LB, long long fwd_cap, int nt_loads) {
  QdShape s;
  memset(&s, 0, sizeof(s));
  s.e = qd_entry_lb(LB);
  if (!s.e) return s;
  s.nt = nt_rule(nt_loads, mp, ld, 0) ? 1 : 0;
  s.ld2 = (uint32_t)(ld / 2);
  s.nrg = (uint32_t)(mp / (uint64_t)s.e->rows);
  s.fwd_grid = (uint32_t)std::min<long long>(s.nrg, fwd_cap > 0 ? fwd_cap : 512);
  const uint32_t GL = FH_WG / (uint32_t)(s.e->lb / s.e->ch);          // lanes of a column group (k_qd_fwd)
  s.ntrip = (s.ld2 + GL - 1) / GL;
  s.last_live = s.ld2 - (s.ntrip - 1) * GL;
  s.pass_max = (s.nrg + s.fwd_grid - 1) / s.fwd_grid;
  s.pass_min = s.nrg / s.fwd_grid;
  s.npro = (uint32_t)((nv + FH_WG - 1) / FH_WG);
  s.ngrad = (uint32_t)((mp + FH_WG - 1) / FH_WG);
  return s;
}
static QdShape qd_shape(const fh_ctx* c) { return qd_shape_for(c->mp, c->ld, c->nv, c->LB, c->fwd_cap, c->nt_loads); }
static void qd_shape_report(const QdShape& s, uint32_t* out) {
  const uint32_t v[FH_QUAD_SHAPE_LEN] = {(uint32_t)s.e->lb, (uint32_t)s.e->ch, (uint32_t)s.e->rows, (uint32_t)s.nt, s.fwd_grid, s.nrg, s.ntrip, s.last_live,
                                         s.pass_max, s.pass_min, s.npro, s.ngrad};
  memcpy(out, v, sizeof(v));
}
// read-only: the geometry the next fh_fwd / fh_adj of this context launches with
extern "C" int fh_quad_shape(fh_ctx* c, uint32_t* out) {
  if (!c || !out) return fail(FH_E_ARG, "fh_quad_shape: null argument");
  if (c->op != OP_QUAD) return fail(FH_E_STATE, "fh_quad_shape: the context holds no quadratic operator (fh_set_quadratic)");
  const QdShape s = qd_shape(c);
  if (!s.e) return fail(FH_E_STATE, "quadratic operator: no kernel for %u columns per row", c->LB);
  qd_shape_report(s, out);
  return 0;
}
// ... and the same rule for an (n, n) matrix with L columns that no context holds: a pure host function, no device needed
extern "C" int fh_quad_shape_for(uint64_t n, uint32_t L, long long grid_cap, int nt_loads, uint32_t* out) {
  if (!out) return fail(FH_E_ARG, "fh_quad_shape_for: null argument");
  if (n == 0 || n >= (1ull << 31)) return fail(FH_E_ARG, "fh_quad_shape_for: the matrix dimension must be in [1, 2^31)");
  if (L < 1 || L > 16) return fail(FH_E_ARG, "fh_quad_shape_for: 1 to 16 columns (got %u)", L);
  if (grid_cap < 0) return fail(FH_E_ARG, "FWD_GRID_CAP must be >= 0");
  if (nt_loads < -1 || nt_loads > 1) return fail(FH_E_ARG, "fh_quad_shape_for: nt_loads is -1 (auto), 0 or 1");
  const uint32_t LB = lb_for(L);
  const uint64_t ld = round_up(n, 16);
  const QdShape s = qd_shape_for(ld, ld, ld, LB, grid_cap, nt_loads);
  if (!s.e) return fail(FH_E_STATE, "quadratic operator: no kernel for %u columns per row", LB);
  qd_shape_report(s, out);
  return 0;
}

// W := Q * (mode 0: prox(X0 - tau G0), by the prologue launch ; mode 1: X0) for LB columns from one read of Q; with_f: the loss sum over (n, L)
static int launch_fwd_quad(fh_ctx* c, const FwdIO& io) {
  const QdShape sh = qd_shape(c);
  const QdEntry* e = sh.e;
  const McEntry* me = mc_entry_lb(c->LB);               // (k_mc_pack lays a plain operand out for the streaming loop)
  if (!e || !me) return fail(FH_E_STATE, "quadratic operator: no kernel for %u columns per row", c->LB);
  if (io.mode == 0) FH_TRY(check_prox_run(c));
  QdFwdP p;
  p.Q = c->A; p.ld2 = sh.ld2; p.n = (uint32_t)c->n; p.L = c->L;
  p.nrg = sh.nrg;
  const uint32_t npro = io.mode == 0 ? sh.npro : 0u;
  p.nred_n = npro;
  const unsigned grid = sh.fwd_grid;
  FH_TRY(ensure_ws(c, ((size_t)npro * 8 + grid) * sizeof(double)));
  p.red_n = c->ws; p.red_m = c->ws + (size_t)npro * 8;
  p.x = c->xs;
  p.xrow = io.mode == 0 ? io.xp : io.x0;
  p.c = c->b; p.w = io.z; p.with_f = io.sub_b;
  p.counter = c->counters + CNT_FWD;
  p.out = scalar_out(c);
  t_begin(c, FH_K_FWD);
  if (io.mode == 0) {
    McProP q;
    q.n = (uint32_t)c->n; q.L = c->L; q.nv = (uint32_t)c->nv;
    q.x0 = io.x0; q.g0 = io.g0; q.xacc0 = io.xacc0; q.xhat = io.xhat; q.xp = io.xp; q.tau = io.tau;
    q.xs = c->xs; q.ld2 = p.ld2;
    q.px = make_prox(c, io.tau);
    if (c->prox_kind == FH_PROX_ROWBALL) q.px.thr = c->mu;         // the radius itself: this projection does not scale with the step
    q.red_n = c->ws;
    e->pro<<<dim3(npro), dim3(FH_WG), 0, c->stream>>>(q);
  } else {
    me->pack<<<dim3(sh.npro), dim3(FH_WG), 0, c->stream>>>(io.x0, c->xs, (uint32_t)c->nv, p.ld2);
  }
  p.seq = seq_offer(c);
  e->fwd[sh.nt]<<<dim3(grid), dim3(FH_WG), 0, c->stream>>>(p);
  t_end(c, FH_K_FWD);
  HIP_TRY(hipGetLastError());
  return 0;
}

// g1 := W' + C, elementwise (W' = W or its extrapolation), and the n-side epilogue; sub_b = 0 (fh_apply's adjoint flag) never gets here
static int launch_adj_quad(fh_ctx* c, const AdjIO& io) {
  const QdShape sh = qd_shape(c);
  const QdEntry* e = sh.e;
  if (!e) return fail(FH_E_STATE, "quadratic operator: no kernel for %u columns per row", c->LB);
  if (io.mode != 0 && io.mode != 1) return fail(FH_E_STATE, "the quadratic operator has no row-sharded adjoint");
  QdGradP p;
  p.n = (uint32_t)c->n; p.L = c->L; p.rows = (uint32_t)c->mp;
  p.w = io.z; p.wacc0 = io.zacc0; p.c = c->b;
  p.accel = io.accel; p.mode = io.mode; p.group = c->prox_kind == FH_PROX_GROUP ? 1 : 0;
  p.coef = io.coef; p.tau = io.tau;
  p.x0 = io.x0; p.xp = io.xp; p.xacc0 = io.xacc0; p.xhat = io.xhat; p.x1 = io.x1; p.g1 = io.g1;
  FH_TRY(ensure_ws(c, (size_t)sh.ngrad * 8 * sizeof(double)));
  p.red = c->ws;
  p.counter = c->counters + CNT_ADJ_FIN;
  p.out = scalar_out(c);
  t_begin(c, FH_K_ADJ);
  p.seq = io.mode == 0 ? seq_offer(c) : 0u;
  e->grad<<<dim3(sh.ngrad), dim3(FH_WG), 0, c->stream>>>(p);
  t_end(c, FH_K_ADJ);
  HIP_TRY(hipGetLastError());
  return 0;
}

// ---- bilinear smooth term .5 ||S - X Y^T||^2 (fh_set_factorization; kernels in csrc/fh_bilinear.h, instantiated by fh_bilinear_part.hip) -------
#ifndef FH_SINGLE_TU
#define BL_DECLARE(LB) BL_KERNELS(extern template, LB)
BL_FOR_EACH(BL_DECLARE)
#undef BL_DECLARE
#endif
struct BlEntry { int lb; void (*pro)(const BlProP); void (*pass[2][2])(const BlPassP); void (*grad)(const BlGradP); };      // pass[GRAD][NT]
#define BL_ROW(LB) {LB, k_bl_prologue<LB>, {{k_bl_pass<LB, 0, 0>, k_bl_pass<LB, 0, 1>}, {k_bl_pass<LB, 1, 0>, k_bl_pass<LB, 1, 1>}}, k_bl_grad<LB>},
static const BlEntry kBlTable[] = { BL_FOR_EACH(BL_ROW) };
#undef BL_ROW
static const BlEntry* bl_entry_lb(uint32_t LB) {
  for (const BlEntry& e : kBlTable) if ((uint32_t)e.lb == LB) return &e;
  return nullptr;
}

// THE GEOMETRY of the bilinear launches, stated once: a pure function of S's shape (m, n; device rows of ld doubles), the columns per row LB and
// the tuning values FH_TUNE_FWD_GRID_CAP and FH_TUNE_NT_LOADS (0 / -1 = auto).  A work item of the pass is a row panel of PR rows x a column tile of
// BL_TC = 512 columns.  PR is chosen so that the items reach the pass's grid of 512 workgroups where S is large enough -- panels = 512 / column
// tiles, PR = m / panels rounded up to 16 -- and clamped to [16, 1024]: above 1024 rows a panel's GY partial is already 1 / 1024 of a column of S
// per column of the factors, below 16 the chunks of RB rows would straddle S's padded rows.  Partial traffic, written once and read once each:
// GX  LB / 512 and GY  LB / PR  of S's bytes (LB = 16, PR = 1024: 3.1 % + 1.6 %).
struct BlShape {
  const BlEntry* e;
  int nt;
  uint32_t ld2, pr, nrp, nct, rb;
  uint32_t trips, last_rows, last_live_rows, last_live_lanes;
  uint32_t grid, items_max, items_min, nelem;
  uint64_t px_bytes, py_bytes;
};
static BlShape bl_shape_for(uint64_t m, uint64_t n, uint64_t ld, uint32_t LB, long long fwd_cap, int nt_loads) {
  BlShape s;
  memset(&s, 0, sizeof(s));
  s.e = bl_entry_lb(LB);
  if (!s.e) return s;
  s.nt = nt_rule(nt_loads, round_up(m, 16), ld, 0) ? 1 : 0;
  s.ld2 = (uint32_t)(ld / 2);
  s.rb = (uint32_t)bl_ns((int)LB) / LB;
  s.nct = (uint32_t)((n + BL_TC - 1) / BL_TC);
  const uint64_t panels = std::max<uint64_t>(1, (512 + s.nct - 1) / s.nct);
  s.pr = (uint32_t)std::min<uint64_t>(1024, std::max<uint64_t>(16, round_up((m + panels - 1) / panels, 16)));
  s.nrp = (uint32_t)((m + s.pr - 1) / s.pr);
  s.trips = s.pr / s.rb;
  s.last_rows = (uint32_t)(m - (uint64_t)(s.nrp - 1) * s.pr);
  s.last_live_rows = s.last_rows - (s.last_rows - 1) / s.rb * s.rb;
  s.last_live_lanes = (uint32_t)((n + 1) / 2 - (uint64_t)(s.nct - 1) * (BL_TC / 2));
  const uint64_t items = (uint64_t)s.nrp * s.nct;
  s.grid = (uint32_t)std::min<uint64_t>(items, fwd_cap > 0 ? (uint64_t)fwd_cap : 512);
  s.items_max = (uint32_t)((items + s.grid - 1) / s.grid);
  s.items_min = (uint32_t)(items / s.grid);
  s.nelem = (uint32_t)((round_up(m + n, 16) + FH_WG - 1) / FH_WG);
  s.px_bytes = (uint64_t)s.nct * m * LB * sizeof(double);
  s.py_bytes = (uint64_t)s.nrp * n * LB * sizeof(double);
  return s;
}
static BlShape bl_shape(const fh_ctx* c) { return bl_shape_for(c->bl_m, c->bl_n, c->ld, c->LB, c->fwd_cap, c->nt_loads); }
static void bl_shape_report(const BlShape& s, uint32_t* out) {
  const uint32_t v[FH_BILINEAR_SHAPE_LEN] = {(uint32_t)s.e->lb, (uint32_t)s.nt, s.pr, BL_TC, s.nrp, s.nct, s.rb, s.trips, s.last_rows, s.last_live_rows,
                                             s.last_live_lanes, s.grid, s.items_max, s.items_min, s.nelem, (uint32_t)s.px_bytes, (uint32_t)s.py_bytes};
  memcpy(out, v, sizeof(v));
}
// the size limit of fh_set_factorization (include/fasta_hip.h), checked where the shape is known: nullptr, or what is too large
static const char* bl_too_large(uint64_t m, uint64_t n, const BlShape& s) {
  if (m + n >= (1ull << 27)) return "m + n must be below 2^27 (the row offsets (m + n) * LB are kept in 31 bits)";
  if (s.px_bytes >= (1ull << 32) || s.py_bytes >= (1ull << 32)) return "a partial buffer (column tiles * m * LB or row panels * n * LB doubles) would reach 4 GiB";
  return nullptr;
}
// read-only: the geometry the next fh_fwd / fh_adj of this context launches with
extern "C" int fh_bilinear_shape(fh_ctx* c, uint32_t* out) {
  if (!c || !out) return fail(FH_E_ARG, "fh_bilinear_shape: null argument");
  if (c->op != OP_BILINEAR) return fail(FH_E_STATE, "fh_bilinear_shape: the context holds no bilinear operator (fh_set_factorization)");
  const BlShape s = bl_shape(c);
  if (!s.e) return fail(FH_E_STATE, "bilinear operator: no kernel for %u columns per row", c->LB);
  bl_shape_report(s, out);
  return 0;
}
// ... and the same rule for an (m, n) matrix with K columns that no context holds: a pure host function, no device needed
extern "C" int fh_bilinear_shape_for(uint64_t m, uint64_t n, uint32_t K, long long grid_cap, int nt_loads, uint32_t* out) {
  if (!out) return fail(FH_E_ARG, "fh_bilinear_shape_for: null argument");
  if (m == 0 || n == 0) return fail(FH_E_ARG, "fh_bilinear_shape_for: the matrix must be non-empty");
  if (K < 1 || K > 16) return fail(FH_E_ARG, "fh_bilinear_shape_for: 1 to 16 columns (got %u)", K);
  if (grid_cap < 0) return fail(FH_E_ARG, "FWD_GRID_CAP must be >= 0");
  if (nt_loads < -1 || nt_loads > 1) return fail(FH_E_ARG, "fh_bilinear_shape_for: nt_loads is -1 (auto), 0 or 1");
  if (m >= (1ull << 27) || n >= (1ull << 27)) return fail(FH_E_ARG, "fh_bilinear_shape_for: m + n must be below 2^27 (the row offsets (m + n) * LB are kept in 31 bits)");
  const BlShape s = bl_shape_for(m, n, round_up(n, 16), lb_for(K), grid_cap, nt_loads);
  if (!s.e) return fail(FH_E_STATE, "bilinear operator: no kernel for %u columns per row", lb_for(K));
  if (const char* why = bl_too_large(m, n, s)) return fail(FH_E_ARG, "fh_bilinear_shape_for: %s", why);
  bl_shape_report(s, out);
  return 0;
}

// the partial buffer: [0] f of the latest pass, from 2 doubles on the GX partials, behind them the GY partials (kept until the adjoint launch)
static int bl_ensure_part(fh_ctx* c, const BlShape& sh) {
  const size_t bytes = 16 + (size_t)sh.px_bytes + (size_t)sh.py_bytes;
  if (bytes <= c->bl_part_bytes) return 0;
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (c->bl_part) { HIP_TRY(hipFree(c->bl_part)); c->bl_part = nullptr; c->bl_part_bytes = 0; }
  HIP_TRY(hipMalloc((void**)&c->bl_part, bytes));
  c->bl_part_bytes = bytes;
  c->bl_have_grad = false;
  return 0;
}
// one pass over S at `point`: f (and, grad = 1, the partials of both halves of the gradient); publish = 1: the forward half of the scalar block
static int bl_launch_pass(fh_ctx* c, const BlShape& sh, const double* point, int grad, int publish, uint32_t npro) {
  FH_TRY(bl_ensure_part(c, sh));
  BlPassP p;
  p.S = c->A; p.ld2 = sh.ld2; p.m = (uint32_t)c->bl_m; p.n = (uint32_t)c->bl_n; p.L = c->L;
  p.pr = sh.pr; p.nrp = sh.nrp; p.nct = sh.nct;
  p.z = point;
  p.fout = c->bl_part; p.px = c->bl_part + 2; p.py = c->bl_part + 2 + sh.px_bytes / sizeof(double);
  p.publish = publish; p.nred_n = npro;
  p.red_n = c->ws; p.red_m = c->ws + (size_t)npro * 8;
  p.counter = c->counters + CNT_FWD;
  p.out = scalar_out(c);
  p.seq = publish ? seq_offer(c) : 0u;
  sh.e->pass[grad ? 1 : 0][sh.nt]<<<dim3(sh.grid), dim3(FH_WG), 0, c->stream>>>(p);
  if (grad) { c->bl_have_grad = true; c->bl_nct = sh.nct; c->bl_nrp = sh.nrp; }
  else c->bl_have_grad = false;
  return 0;
}
static void bl_make_prox(fh_ctx* c, double tau, BlProP* q) {
  q->a.px = make_prox(c, tau);
  q->bot = q->a.px;
  q->split = 0; q->rowsplit = 0;
  if (c->prox_kind == FH_PROX_ROWSPLIT) {
    q->rowsplit = 1; q->split = (uint32_t)c->rs_split;
    q->a.px.kind = c->rs_kind_top;
    q->bot.kind = c->rs_kind_bot; q->bot.thr = 0.0; q->bot.lo = c->rs_lo_bot; q->bot.hi = c->rs_hi_bot;
  }
}

// mode 0: xhat, xprox = prox(X0 - tau G0) and the n-side sums by the prologue launch, then the pass at xprox; mode 1: the pass at X0.  The pass
// of mode 0 leaves the gradient out when the context's latest adjoint launch was accelerated (the next one then wants the gradient at another
// point anyway); launch_adj_bilinear makes up for a wrong guess, and f has the same bits either way.
static int launch_fwd_bilinear(fh_ctx* c, const FwdIO& io) {
  const BlShape sh = bl_shape(c);
  if (!sh.e) return fail(FH_E_STATE, "bilinear operator: no kernel for %u columns per row", c->LB);
  if (io.mode == 0) FH_TRY(check_prox_run(c));
  if (!io.sub_b) return fail(FH_E_STATE, "the bilinear operator has no linear map to apply");
  const uint32_t npro = io.mode == 0 ? sh.nelem : 0u;
  FH_TRY(ensure_ws(c, ((size_t)npro * 8 + sh.grid) * sizeof(double)));
  FH_TRY(bl_ensure_part(c, sh));
  t_begin(c, FH_K_FWD);
  if (io.mode == 0) {
    BlProP q;
    q.a.n = (uint32_t)c->n; q.a.L = c->L; q.a.nv = (uint32_t)c->nv;
    q.a.x0 = io.x0; q.a.g0 = io.g0; q.a.xacc0 = io.xacc0; q.a.xhat = io.xhat; q.a.xp = io.xp; q.a.tau = io.tau;
    q.a.xs = nullptr; q.a.ld2 = 0;
    bl_make_prox(c, io.tau, &q);
    q.a.red_n = c->ws;
    sh.e->pro<<<dim3(npro), dim3(FH_WG), 0, c->stream>>>(q);
  }
  const int rc = bl_launch_pass(c, sh, io.mode == 0 ? io.xp : io.x0, (io.mode == 1 || !c->last_accel) ? 1 : 0, 1, npro);
  t_end(c, FH_K_FWD);
  FH_TRY(rc);
  HIP_TRY(hipGetLastError());
  return 0;
}

// g1 := the gradient, summed from the partials of the latest pass, and the n-side epilogue.  With acceleration the gradient is wanted at the
// extrapolated point: k_bl_extrap forms it, a second pass runs there, and FH_S_FSQ_ADJ is f at that point.
static int launch_adj_bilinear(fh_ctx* c, const AdjIO& io) {
  const BlShape sh = bl_shape(c);
  if (!sh.e) return fail(FH_E_STATE, "bilinear operator: no kernel for %u columns per row", c->LB);
  if (io.mode != 0 && io.mode != 1) return fail(FH_E_STATE, "the bilinear operator has no row-sharded adjoint");
  if (!io.sub_b) return fail(FH_E_STATE, "the bilinear operator has no linear map to apply");
  FH_TRY(ensure_ws(c, ((size_t)sh.nelem * 8 + sh.grid) * sizeof(double)));
  t_begin(c, FH_K_ADJ);
  int rc = 0;
  if (io.mode == 0 && io.accel) {
    const uint64_t count = c->nv * c->LB;
    k_bl_extrap<<<dim3((unsigned)((count + FH_WG - 1) / FH_WG)), dim3(FH_WG), 0, c->stream>>>(io.xp, io.xacc0, io.coef, io.x1, (uint32_t)c->n, c->L, c->LB, count);
    rc = bl_launch_pass(c, sh, io.x1, 1, 0, 0);
  } else if (io.mode == 0 && !c->bl_have_grad) {
    rc = bl_launch_pass(c, sh, io.xp, 1, 0, 0);
  }
  if (rc == 0 && !c->bl_have_grad) rc = fail(FH_E_STATE, "the bilinear operator: no pass has left its gradient partials (fh_fwd / fh_init first)");
  if (rc == 0) {
    BlGradP p;
    p.m = (uint32_t)c->bl_m; p.n = (uint32_t)c->bl_n; p.L = c->L; p.rows = (uint32_t)c->nv;
    p.nct = c->bl_nct; p.nrp = c->bl_nrp;
    p.gtop = c->prox_kind == FH_PROX_ROWSPLIT ? (uint32_t)c->rs_split : (uint32_t)c->n;
    p.fsrc = c->bl_part; p.px = c->bl_part + 2; p.py = c->bl_part + 2 + (uint64_t)c->bl_nct * c->bl_m * c->LB;
    p.accel = io.accel; p.mode = io.mode; p.coef = io.coef; p.tau = io.tau;
    p.x0 = io.x0; p.xp = io.xp; p.xacc0 = io.xacc0; p.xhat = io.xhat; p.g1 = io.g1;
    p.red = c->ws;
    p.counter = c->counters + CNT_ADJ_FIN;
    p.out = scalar_out(c);
    p.seq = io.mode == 0 ? seq_offer(c) : 0u;
    sh.e->grad<<<dim3(sh.nelem), dim3(FH_WG), 0, c->stream>>>(p);
    c->bl_have_grad = false;                 // (consumed: the next adjoint launch without a forward one makes its own pass)
  }
  t_end(c, FH_K_ADJ);
  FH_TRY(rc);
  HIP_TRY(hipGetLastError());
  return 0;
}

// g1 := A^T grad f(z') by the gather over the A^T copy; the residual and the loss sum at z' come from the m-side prologue launch
static int launch_adj_sparse(fh_ctx* c, const AdjIO& io) {
  const SpEntry* e = sp_entry(c->sp_G[1]);
  if (!e) return fail(FH_E_STATE, "sparse operator: no kernel for %d lanes per row", c->sp_G[1]);
  if (io.mode != 0 && io.mode != 1) return fail(FH_E_STATE, "the sparse operator has no row-sharded adjoint");
  SpAdjP p;
  p.a = c->sp[1]; p.n = (uint32_t)c->n;
  const uint32_t nres = (uint32_t)((c->m + FH_WG - 1) / FH_WG);
  p.nred_f = nres;
  const unsigned grid = p.a.nwg + p.a.nlong;
  FH_TRY(ensure_ws(c, ((size_t)nres + (size_t)grid * 8) * sizeof(double)));
  p.red_f = c->ws; p.red_bb = c->ws + nres;
  p.r = c->sp_r;
  p.accel = io.accel; p.mode = io.mode; p.coef = io.coef; p.tau = io.tau;
  p.x0 = io.x0; p.xp = io.xp; p.xacc0 = io.xacc0; p.xhat = io.xhat; p.x1 = io.x1; p.g1 = io.g1;
  p.counter = c->counters + CNT_ADJ_FIN;
  p.out = scalar_out(c);
  SpResP q;
  q.m = (uint32_t)c->m; q.z = io.z; q.zacc0 = io.zacc0; q.b = c->b; q.r = c->sp_r;
  q.sub_b = io.sub_b; q.loss = c->loss_kind; q.accel = io.accel; q.coef = io.coef;
  q.red_f = c->ws;
  t_begin(c, FH_K_ADJ);
  k_sp_resid<<<dim3(nres), dim3(FH_WG), 0, c->stream>>>(q);
  p.seq = io.mode == 0 ? seq_offer(c) : 0u;
  e->adj[sp_nt_for(c) ? 1 : 0]<<<dim3(grid), dim3(FH_WG), 0, c->stream>>>(p);
  t_end(c, FH_K_ADJ);
  HIP_TRY(hipGetLastError());
  return 0;
}

// ---- matrix unknown over the sparse operator (fh_set_matrix_csr_rhs; kernels in csrc/fh_spmulti.h, instantiated by fh_spmulti_part.hip) ------
#ifndef FH_SINGLE_TU
#define SPMC_DECLARE_LB(LB) SPMC_LB_KERNELS(extern template, LB)
SPMC_FOR_EACH_LB(SPMC_DECLARE_LB)
#undef SPMC_DECLARE_LB
#define SPMC_DECLARE(G, LB) SPMC_KERNELS(extern template, G, LB)
SPMC_FOR_EACH(SPMC_DECLARE)
#undef SPMC_DECLARE
#endif
struct SpmcLbEntry { int lb; void (*pro)(const SpmcProP); void (*resid)(const SpmcResP); };
#define SPMC_LB_ROW(LB) {LB, k_spmc_prologue<LB>, k_spmc_resid<LB>},
static const SpmcLbEntry kSpmcLbTable[] = { SPMC_FOR_EACH_LB(SPMC_LB_ROW) };
#undef SPMC_LB_ROW
struct SpmcEntry { int g, lb; void (*fwd[2])(const SpmcFwdP); void (*adj[2])(const SpmcAdjP); };
#define SPMC_ROW(G, LB) {G, LB, {k_spmc_fwd<G, LB, 0>, k_spmc_fwd<G, LB, 1>}, {k_spmc_adj<G, LB, 0>, k_spmc_adj<G, LB, 1>}},
static const SpmcEntry kSpmcTable[] = { SPMC_FOR_EACH(SPMC_ROW) };
#undef SPMC_ROW
static const SpmcLbEntry* spmc_lb_entry(const fh_ctx* c) {
  for (const SpmcLbEntry& e : kSpmcLbTable) if ((uint32_t)e.lb == c->LB) return &e;
  return nullptr;
}
static const SpmcEntry* spmc_entry(const fh_ctx* c, int side) {
  for (const SpmcEntry& e : kSpmcTable) if (e.g == c->sp_G[side] && (uint32_t)e.lb == c->LB) return &e;
  return nullptr;
}

// Z := A * (mode 0: prox(X0 - tau G0), by the prologue launch ; mode 1: X0), LB columns per gathered row
static int launch_fwd_spmulti(fh_ctx* c, const FwdIO& io) {
  const SpmcEntry* e = spmc_entry(c, 0);
  const SpmcLbEntry* lbe = spmc_lb_entry(c);
  if (!e || !lbe) return fail(FH_E_STATE, "sparse multi-column form: no kernel for %d lanes per row at %u columns per row", c->sp_G[0], c->LB);
  FH_TRY(check_loss_run(c));
  if (io.mode == 0) FH_TRY(check_prox_run(c));
  const bool sm = sm_on(c, io.sub_b);             // as launch_fwd_multi: the row pass behind K-fwd writes FH_S_FSQ and publishes
  SpmcFwdP p;
  p.a = c->sp[0]; p.m = (uint32_t)c->m; p.L = c->L;
  const uint32_t npro = io.mode == 0 ? (uint32_t)((c->nv + FH_WG - 1) / FH_WG) : 0u;
  p.nred_n = npro;
  const unsigned grid = p.a.nwg + p.a.nlong;
  FH_TRY(ensure_ws(c, ((size_t)npro * 8 + grid + (sm ? sm_records(c) : 0u)) * sizeof(double)));
  p.red_n = c->ws; p.red_m = c->ws + (size_t)npro * 8;
  p.x = io.mode == 0 ? io.xp : io.x0;
  p.b = c->b; p.z = io.z; p.sub_b = io.sub_b;
  p.counter = c->counters + CNT_FWD;
  p.out = scalar_out(c);
  t_begin(c, FH_K_FWD);
  if (io.mode == 0) {
    SpmcProP q;
    q.n = (uint32_t)c->n; q.L = c->L; q.nv = (uint32_t)c->nv;
    q.x0 = io.x0; q.g0 = io.g0; q.xacc0 = io.xacc0; q.xhat = io.xhat; q.xp = io.xp; q.tau = io.tau;
    q.px = make_prox(c, io.tau);
    q.red_n = c->ws;
    lbe->pro<<<dim3(npro), dim3(FH_WG), 0, c->stream>>>(q);
  }
  p.seq = sm ? 0u : seq_offer(c);
  e->fwd[sp_nt_for(c) ? 1 : 0]<<<dim3(grid), dim3(FH_WG), 0, c->stream>>>(p);
  if (sm) FH_TRY(launch_sm_rows(c, io.z, nullptr, 0, 0.0, nullptr, p.red_m + grid, true, FH_S_FSQ, seq_offer(c)));
  t_end(c, FH_K_FWD);
  HIP_TRY(hipGetLastError());
  return 0;
}

// G1 := A^T (Z' - B) by the gather over the A^T copy; the residual and the loss sum at Z' come from the m-side prologue launch
static int launch_adj_spmulti(fh_ctx* c, const AdjIO& io) {
  const SpmcEntry* e = spmc_entry(c, 1);
  const SpmcLbEntry* lbe = spmc_lb_entry(c);
  if (!e || !lbe) return fail(FH_E_STATE, "sparse multi-column form: no kernel for %d lanes per row at %u columns per row", c->sp_G[1], c->LB);
  if (io.sub_b) FH_TRY(check_loss_run(c));
  if (io.mode != 0 && io.mode != 1) return fail(FH_E_STATE, "the sparse operator has no row-sharded adjoint");
  SpmcAdjP p;
  p.a = c->sp[1]; p.n = (uint32_t)c->n; p.L = c->L;
  const uint64_t pairs = c->m * (uint64_t)(c->LB / 2);
  const uint32_t nres = (uint32_t)((pairs + FH_WG - 1) / FH_WG);
  p.nred_f = nres;
  const unsigned grid = p.a.nwg + p.a.nlong;
  FH_TRY(ensure_ws(c, ((size_t)nres + (size_t)grid * 8) * sizeof(double)));
  p.red_f = c->ws; p.red_bb = c->ws + nres;
  p.r = c->sp_r;
  p.accel = io.accel; p.mode = io.mode; p.coef = io.coef; p.tau = io.tau; p.group = c->prox_kind == FH_PROX_GROUP ? 1 : 0;
  p.x0 = io.x0; p.xp = io.xp; p.xacc0 = io.xacc0; p.xhat = io.xhat; p.x1 = io.x1; p.g1 = io.g1;
  p.counter = c->counters + CNT_ADJ_FIN;
  p.out = scalar_out(c);
  SpmcResP q;
  q.m = (uint32_t)c->m; q.L = c->L; q.z = io.z; q.zacc0 = io.zacc0; q.b = c->b; q.r = c->sp_r;
  q.sub_b = io.sub_b; q.accel = io.accel; q.coef = io.coef;
  q.red_f = c->ws;
  t_begin(c, FH_K_ADJ);
  if (sm_on(c, io.sub_b)) FH_TRY(launch_sm_rows(c, io.z, io.zacc0, io.accel, io.coef, c->sp_r, c->ws, false, 0, 0u));   // the same contract (sp_r, red_f; nres = sm_records)
  else lbe->resid<<<dim3(nres), dim3(FH_WG), 0, c->stream>>>(q);
  p.seq = io.mode == 0 ? seq_offer(c) : 0u;
  e->adj[sp_nt_for(c) ? 1 : 0]<<<dim3(grid), dim3(FH_WG), 0, c->stream>>>(p);
  t_end(c, FH_K_ADJ);
  HIP_TRY(hipGetLastError());
  return 0;
}

// ---- 3-D stencil operator (fh_set_stencil3d; kernels in csrc/fh_tv3d.h, instantiated by fh_tv3d_part.hip) -------------------------------
#ifndef FH_SINGLE_TU
TV3_KERNELS(extern template)
#endif
// THE launch geometry of both kernels, a pure function of the volume, FH_TUNE_TV3_PLANES (0 = auto) and the device's CU count: tiles of
// TV3_TH x TV3_TW (h, w) positions, `planes` planes per workgroup along d, grid = chunks x tiles_h x tiles_w.  Auto: whole columns of planes
// unless that leaves fewer than 8 workgroups per CU; then as many chunks as reach that, but at least 8 planes per chunk (a chunk computes
// planes + 1: the d+1 halo of K-fwd, the d-1 halo of K-adj).
struct Tv3Shape { uint32_t planes, tiles_h, tiles_w, chunks, grid; };
static int tv3_shape_for(uint64_t D, uint64_t H, uint64_t W, int planes_tune, int ncu, Tv3Shape* sh) {
  if (D < 1 || H < 1 || W < 1) return fail(FH_E_ARG, "the 3-D stencil needs D >= 1, H >= 1 and W >= 1 (got %llu x %llu x %llu)", (unsigned long long)D, (unsigned long long)H, (unsigned long long)W);
  if (D >= (1ull << 31) || H >= (1ull << 31) || W >= (1ull << 31) || D * H >= (1ull << 31) || D * H * W * 3 >= (1ull << 31))
    return fail(FH_E_ARG, "the 3-D stencil needs 3 * D * H * W < 2^31: the n-side sums and vector lengths count in 32 bits (got %llu x %llu x %llu)", (unsigned long long)D, (unsigned long long)H, (unsigned long long)W);
  if (planes_tune < 0) return fail(FH_E_ARG, "TV3_PLANES must be >= 0 (0 = auto)");
  const uint64_t tiles_h = (H + TV3_TH - 1) / TV3_TH, tiles_w = (W + TV3_TW - 1) / TV3_TW, tiles = tiles_h * tiles_w;
  uint64_t planes;
  if (planes_tune > 0) planes = std::min<uint64_t>((uint64_t)planes_tune, D);
  else {
    const uint64_t want = (uint64_t)std::max(1, ncu) * 8u;
    const uint64_t chunks = std::max<uint64_t>(1, std::min<uint64_t>(D, (want + tiles - 1) / tiles));
    planes = std::max<uint64_t>((D + chunks - 1) / chunks, std::min<uint64_t>(D, 8));
  }
  const uint64_t chunks = (D + planes - 1) / planes;
  if (tiles * chunks >= (1ull << 31)) return fail(FH_E_ARG, "the 3-D stencil launch would need %llu workgroups", (unsigned long long)(tiles * chunks));
  sh->planes = (uint32_t)planes; sh->tiles_h = (uint32_t)tiles_h; sh->tiles_w = (uint32_t)tiles_w; sh->chunks = (uint32_t)chunks;
  sh->grid = (uint32_t)(tiles * chunks);
  return 0;
}
// plain stores are the default: the non-temporal ones measure within 1.4 % of them from 256^3 on; FH_TUNE_NT_LOADS = 1 opts in
static inline int tv3_nt_for(const fh_ctx* c) { return c->nt_loads > 0 ? 1 : 0; }
static void tv3_shape_out(const Tv3Shape& sh, int nt, uint32_t* out) {
  out[0] = TV3_TH; out[1] = TV3_TW; out[2] = sh.planes; out[3] = sh.tiles_h; out[4] = sh.tiles_w; out[5] = sh.chunks; out[6] = sh.grid; out[7] = (uint32_t)nt;
}
extern "C" int fh_tv3d_shape(fh_ctx* c, uint32_t* out) {
  if (!c || !out) return fail(FH_E_ARG, "fh_tv3d_shape: null argument");
  if (c->op != OP_STENCIL3D) return fail(FH_E_STATE, "fh_tv3d_shape: the context holds no 3-D stencil operator (fh_set_stencil3d)");
  Tv3Shape sh;
  FH_TRY(tv3_shape_for(c->D, c->H, c->W, c->tv3_planes, c->ncu, &sh));
  tv3_shape_out(sh, tv3_nt_for(c), out);
  return 0;
}
extern "C" int fh_tv3d_shape_for(uint64_t D, uint64_t H, uint64_t W, int planes, int ncu, uint32_t* out) {
  if (!out) return fail(FH_E_ARG, "fh_tv3d_shape_for: null argument");
  Tv3Shape sh;
  FH_TRY(tv3_shape_for(D, H, W, planes, ncu, &sh));
  tv3_shape_out(sh, 0, out);
  return 0;
}

// z := div(mode 0: prox(x0 - tau g0) ; mode 1: x0), ONE launch
static int launch_fwd_tv3(fh_ctx* c, const FwdIO& io) {
  FH_TRY(check_loss_run(c));
  if (io.mode == 0) FH_TRY(check_prox_run(c));
  Tv3Shape sh;
  FH_TRY(tv3_shape_for(c->D, c->H, c->W, c->tv3_planes, c->ncu, &sh));
  Tv3FwdP p;
  p.D = (uint32_t)c->D; p.H = (uint32_t)c->H; p.W = (uint32_t)c->W; p.planes = sh.planes; p.tiles_h = sh.tiles_h; p.tiles_w = sh.tiles_w;
  p.mode = io.mode; p.sub_b = io.sub_b;
  p.x0 = io.x0; p.g0 = io.g0; p.xacc0 = io.xacc0; p.xhat = io.xhat; p.xp = io.xp; p.b = c->b; p.z = io.z; p.tau = io.tau;
  p.px = make_prox(c, io.tau);
  FH_TRY(ensure_ws(c, (size_t)sh.grid * 8 * sizeof(double)));
  p.red = c->ws; p.counter = c->counters + CNT_FWD; p.out = scalar_out(c);
  const bool ball = io.mode == 0 && c->prox_kind == FH_PROX_TVBALL;
  t_begin(c, FH_K_FWD);
  p.seq = seq_offer(c);
  if (tv3_nt_for(c)) { if (ball) k_tv3_fwd<0, 1><<<dim3(sh.grid), dim3(FH_WG), 0, c->stream>>>(p); else k_tv3_fwd<1, 1><<<dim3(sh.grid), dim3(FH_WG), 0, c->stream>>>(p); }
  else { if (ball) k_tv3_fwd<0, 0><<<dim3(sh.grid), dim3(FH_WG), 0, c->stream>>>(p); else k_tv3_fwd<1, 0><<<dim3(sh.grid), dim3(FH_WG), 0, c->stream>>>(p); }
  t_end(c, FH_K_FWD);
  HIP_TRY(hipGetLastError());
  return 0;
}

// g1 := grad(z' - b) with the residual, the loss at z' and the n-side epilogue in the same launch
static int launch_adj_tv3(fh_ctx* c, const AdjIO& io) {
  FH_TRY(check_loss_run(c));
  if (io.mode != 0 && io.mode != 1) return fail(FH_E_STATE, "the 3-D stencil operator has no row-sharded adjoint");
  Tv3Shape sh;
  FH_TRY(tv3_shape_for(c->D, c->H, c->W, c->tv3_planes, c->ncu, &sh));
  Tv3AdjP p;
  p.D = (uint32_t)c->D; p.H = (uint32_t)c->H; p.W = (uint32_t)c->W; p.planes = sh.planes; p.tiles_h = sh.tiles_h; p.tiles_w = sh.tiles_w;
  p.z = io.z; p.zacc0 = io.zacc0; p.b = c->b; p.sub_b = io.sub_b; p.accel = io.accel; p.mode = io.mode; p.coef = io.coef; p.tau = io.tau;
  p.x0 = io.x0; p.xp = io.xp; p.xacc0 = io.xacc0; p.xhat = io.xhat; p.x1 = io.x1; p.g1 = io.g1;
  FH_TRY(ensure_ws(c, (size_t)sh.grid * 8 * sizeof(double)));
  p.red = c->ws; p.counter = c->counters + CNT_ADJ_FIN; p.out = scalar_out(c);
  t_begin(c, FH_K_ADJ);
  p.seq = io.mode == 0 ? seq_offer(c) : 0u;
  if (tv3_nt_for(c)) k_tv3_adj<1><<<dim3(sh.grid), dim3(FH_WG), 0, c->stream>>>(p);
  else k_tv3_adj<0><<<dim3(sh.grid), dim3(FH_WG), 0, c->stream>>>(p);
  t_end(c, FH_K_ADJ);
  HIP_TRY(hipGetLastError());
  return 0;
}

// ---- periodic convolution operator (fh_set_conv2d; kernels in csrc/fh_conv.h, instantiated by fh_conv_part.hip) ---------------------------
#ifndef FH_SINGLE_TU
CONV_KERNELS(extern template)
#endif
// THE launch geometry of both kernels, a pure function of the image, the kernel and the device's CU count: a workgroup owns a tile of
// th x tw = 2048 output pixels, 8 consecutive ones along w per lane.  32 x 64 in general (LDS: 47 rows at a pitch of 104 doubles hold the
// tile and a halo of up to 15 rows and 15 skewed columns); a signal -- H == 1 with kh == 1 -- takes 1 x 2048 (one row at a pitch of 2344),
// where the square tile would leave 31 of 32 lanes idle.  grid = tiles_h x tiles_w.  The CU count does not enter the rule today: an image
// of fewer tiles than CUs runs on fewer CUs, a smaller tile would only add halo (it is a parameter so that the rule may use it later
// without a change of the interface).
static int conv_shape_for(uint64_t H, uint64_t W, uint32_t kh, uint32_t kw, int ncu, ConvShape* sh) {
  (void)ncu;
  memset(sh, 0, sizeof(*sh));
  if (H < 1 || W < 1) return fail(FH_E_ARG, "the convolution operator needs H >= 1 and W >= 1 (got %llu x %llu)", (unsigned long long)H, (unsigned long long)W);
  if (kh < 1 || kh > CONV_MAXK || kw < 1 || kw > CONV_MAXK)
    return fail(FH_E_ARG, "the convolution operator serves kernels of 1 to %d taps along each axis (got %u x %u): a larger point-spread function is a job for an FFT", CONV_MAXK, kh, kw);
  if (H >= (1ull << 31) || W >= (1ull << 31) || H * W >= (1ull << 31))
    return fail(FH_E_ARG, "the convolution operator needs H * W < 2^31: pixel offsets and vector lengths count in 32 bits (got %llu x %llu)", (unsigned long long)H, (unsigned long long)W);
  const bool flat = H == 1 && kh == 1;
  sh->th = flat ? 1u : 32u; sh->tw = flat ? 2048u : 64u; sh->tw_log2 = flat ? 11u : 6u;
  sh->pitch = flat ? 2344u : 104u;                        // >= CONV_SKEW(tw + 15 - 1) + 1 and 8 mod 32 (csrc/fh_conv.h)
  sh->tiles_h = (uint32_t)((H + sh->th - 1) / sh->th); sh->tiles_w = (uint32_t)((W + sh->tw - 1) / sh->tw);
  sh->grid = sh->tiles_h * sh->tiles_w;                   // (< 2^31 / 2048)
  sh->lds_bytes = CONV_LDS_DOUBLES * (uint32_t)sizeof(double);
  return 0;
}
static void conv_shape_out(const ConvShape& sh, uint32_t* out) {
  out[0] = sh.th; out[1] = sh.tw; out[2] = sh.tiles_h; out[3] = sh.tiles_w; out[4] = sh.grid; out[5] = CONV_RUN; out[6] = FH_WG; out[7] = sh.lds_bytes;
}
extern "C" int fh_conv_shape(fh_ctx* c, uint32_t* out) {
  if (!c || !out) return fail(FH_E_ARG, "fh_conv_shape: null argument");
  if (c->op != OP_CONV) return fail(FH_E_STATE, "fh_conv_shape: the context holds no convolution operator (fh_set_conv2d)");
  conv_shape_out(c->conv_sh, out);                        // (what conv_shape_for gave when fh_set_conv2d set the operator: the launchers read the same copy)
  return 0;
}
extern "C" int fh_conv_shape_for(uint64_t H, uint64_t W, uint32_t kh, uint32_t kw, int ncu, uint32_t* out) {
  if (!out) return fail(FH_E_ARG, "fh_conv_shape_for: null argument");
  ConvShape sh;
  const int rc = conv_shape_for(H, W, kh, kw, ncu, &sh);
  conv_shape_out(sh, out);                                // (a refusal: all zeros beside the error and its sentence)
  return rc;
}
static int conv_alloc_diag(fh_ctx* c, const double* diag) {
  HIP_TRY(hipMalloc((void**)&c->conv_diag, c->m * sizeof(double)));
  HIP_TRY(hipMemcpy(c->conv_diag, diag, c->m * sizeof(double), hipMemcpyHostToDevice));
  return 0;
}
static ConvGeo conv_geo(const fh_ctx* c) {
  const ConvShape& sh = c->conv_sh;
  ConvGeo g;
  g.H = (uint32_t)c->H; g.W = (uint32_t)c->W; g.kh = c->conv_kh; g.kw = c->conv_kw; g.oh = c->conv_oh; g.ow = c->conv_ow;
  g.th = sh.th; g.tw = sh.tw; g.tw_log2 = sh.tw_log2; g.pitch = sh.pitch; g.tiles_w = sh.tiles_w;
  return g;
}

// z := d * (K conv (mode 0: prox(x0 - tau g0) ; mode 1: x0)), ONE launch
static int launch_fwd_conv(fh_ctx* c, const FwdIO& io) {
  FH_TRY(check_loss_run(c));
  if (io.mode == 0) FH_TRY(check_prox_run(c));
  const ConvShape& sh = c->conv_sh;
  ConvFwdP p;
  p.g = conv_geo(c);
  p.sub_b = io.sub_b;
  p.x0 = io.x0; p.g0 = io.g0; p.xacc0 = io.xacc0; p.xhat = io.xhat; p.xp = io.xp; p.b = c->b; p.z = io.z; p.diag = c->conv_diag; p.tau = io.tau;
  p.px = make_prox(c, io.tau);
  memcpy(p.taps, c->conv_taps, sizeof(p.taps));
  FH_TRY(ensure_ws(c, (size_t)sh.grid * 8 * sizeof(double)));
  p.red = c->ws; p.counter = c->counters + CNT_FWD; p.out = scalar_out(c);
  t_begin(c, FH_K_FWD);
  p.seq = seq_offer(c);
  if (io.mode == 0) k_conv_fwd<0><<<dim3(sh.grid), dim3(FH_WG), 0, c->stream>>>(p);
  else k_conv_fwd<1><<<dim3(sh.grid), dim3(FH_WG), 0, c->stream>>>(p);
  t_end(c, FH_K_FWD);
  HIP_TRY(hipGetLastError());
  return 0;
}

// g1 := K corr (d * (z' - b)) with the residual, the loss at z' and the n-side epilogue in the same launch
static int launch_adj_conv(fh_ctx* c, const AdjIO& io) {
  FH_TRY(check_loss_run(c));
  if (io.mode != 0 && io.mode != 1) return fail(FH_E_STATE, "the convolution operator has no row-sharded adjoint");
  const ConvShape& sh = c->conv_sh;
  ConvAdjP p;
  p.g = conv_geo(c);
  p.z = io.z; p.zacc0 = io.zacc0; p.b = c->b; p.diag = c->conv_diag; p.sub_b = io.sub_b; p.accel = io.accel; p.coef = io.coef; p.tau = io.tau;
  p.x0 = io.x0; p.xp = io.xp; p.xacc0 = io.xacc0; p.xhat = io.xhat; p.x1 = io.x1; p.g1 = io.g1;
  memcpy(p.taps, c->conv_taps, sizeof(p.taps));
  FH_TRY(ensure_ws(c, (size_t)sh.grid * 8 * sizeof(double)));
  p.red = c->ws; p.counter = c->counters + CNT_ADJ_FIN; p.out = scalar_out(c);
  t_begin(c, FH_K_ADJ);
  p.seq = io.mode == 0 ? seq_offer(c) : 0u;
  if (io.mode == 0) k_conv_adj<0><<<dim3(sh.grid), dim3(FH_WG), 0, c->stream>>>(p);
  else k_conv_adj<1><<<dim3(sh.grid), dim3(FH_WG), 0, c->stream>>>(p);
  t_end(c, FH_K_ADJ);
  HIP_TRY(hipGetLastError());
  return 0;
}

// ---- subsampled DCT operator (fh_set_dct; kernels in csrc/fh_dct.h, instantiated by fh_dct_part.hip) -------------------------------------
#ifndef FH_SINGLE_TU
#define DCT_DECLARE(LDSN) DCT_KERNELS(extern template, LDSN)
DCT_FOR_EACH(DCT_DECLARE)
#undef DCT_DECLARE
DCT_TILE_KERNELS(extern template)
#endif
// THE geometry of every launch of both directions, a pure function of N, the row cap (FH_TUNE_DCT_ROW_CAP; 0 = DCT_ROW_CAP) and the device's CU
// count.  N <= cap: one row of length N1 = N, N2 = 1, one workgroup, one launch.  Otherwise N = N1 * N2 with N2 the largest divisor of N that is
// at most the cap and leaves N1 = N / N2 at most the cap too (4096 = 2 * 2048, 6000 = 3 * 2000, 2^22 = 2048 * 2048): five launches, the row
// transforms of length N1 (N2 rows) and N2 (N1 rows) between three tile launches of ceil(N1 / 32) * ceil(N2 / 32) workgroups.  A row length takes
// the radices 5, 3, 4, 2 in that order; its LDS class is the smallest of 128 / 512 / 2048 that holds it; a workgroup takes as many rows as the
// class holds, at most DCT_MAX_ROWS, and fewer where that would leave fewer workgroups than CUs.
static bool dct_radices(uint64_t L, DctRad* rd) {
  rd->n = 0; memset(rd->r, 0, sizeof(rd->r));
  for (uint32_t r : {5u, 3u, 4u, 2u})
    while (L % r == 0 && L > 1) { if (rd->n == DCT_MAXRAD) return false; rd->r[rd->n++] = (uint8_t)r; L /= r; }
  return L == 1;
}
static inline uint32_t dct_ldsn(uint64_t L) { return L <= 128 ? 128u : (L <= 512 ? 512u : 2048u); }
static void dct_rows_geometry(uint64_t L, uint64_t nrows, int ncu, uint32_t* ldsn, uint32_t* rpw, uint32_t* grid) {
  *ldsn = dct_ldsn(L);
  uint64_t r = std::min<uint64_t>(std::min<uint64_t>(*ldsn / L, DCT_MAX_ROWS), nrows);
  r = std::max<uint64_t>(1, std::min<uint64_t>(r, nrows / (uint64_t)std::max(1, ncu)));
  *rpw = (uint32_t)r; *grid = (uint32_t)((nrows + r - 1) / r);
}
static int dct_shape_for(uint64_t N, int row_cap, int ncu, DctShape* sh) {
  memset(sh, 0, sizeof(*sh));
  if (row_cap != 0 && (row_cap < 2 || row_cap > DCT_ROW_CAP)) return fail(FH_E_ARG, "DCT_ROW_CAP must be 0 (default: %d) or in [2, %d] elements per row transform", DCT_ROW_CAP, DCT_ROW_CAP);
  const uint64_t cap = row_cap ? (uint64_t)row_cap : DCT_ROW_CAP;
  sh->cap = (uint32_t)cap;                                // (set from here on: a refusal below is about N, not about the cap)
  if (N == 0) return fail(FH_E_ARG, "the DCT operator needs N >= 1");
  uint64_t rest = N;
  for (uint64_t r : {2u, 3u, 5u}) while (rest % r == 0) rest /= r;
  if (rest != 1) return fail(FH_E_ARG, "the DCT operator serves lengths whose prime factors are 2, 3 and 5 only: N = %llu has a prime factor above 5", (unsigned long long)N);
  uint64_t N1 = N, N2 = 1;
  if (N > cap) {
    N2 = 0;
    if (N <= cap * cap)
      for (uint64_t d = cap; d >= 2; --d) if (N % d == 0 && N / d <= cap) { N2 = d; break; }
    if (!N2) return fail(FH_E_ARG, "the DCT operator needs N <= the row cap or a split N = N1 * N2 with both factors at most the row cap (%llu): N = %llu has none", (unsigned long long)cap, (unsigned long long)N);
    N1 = N / N2;
  }
  sh->levels = N2 > 1 ? 2u : 1u; sh->N1 = (uint32_t)N1; sh->N2 = (uint32_t)N2; sh->cap = (uint32_t)cap;
  if (!dct_radices(N1, &sh->r1) || !dct_radices(N2, &sh->r2)) return fail(FH_E_ARG, "the DCT operator: N = %llu needs more than %d radix passes per row", (unsigned long long)N, DCT_MAXRAD);
  if (sh->levels == 1) {
    sh->ldsn1 = dct_ldsn(N1); sh->rpw1 = 1; sh->grid1 = 1; sh->launches = 1;
    sh->lds_bytes = sh->ldsn1 * 2u * (uint32_t)sizeof(d2);
    return 0;
  }
  dct_rows_geometry(N1, N2, ncu, &sh->ldsn1, &sh->rpw1, &sh->grid1);
  dct_rows_geometry(N2, N1, ncu, &sh->ldsn2, &sh->rpw2, &sh->grid2);
  sh->tiles = (uint32_t)(((N1 + DCT_TT - 1) / DCT_TT) * ((N2 + DCT_TT - 1) / DCT_TT));
  sh->launches = 5;
  sh->lds_bytes = std::max(sh->ldsn1, sh->ldsn2) * 2u * (uint32_t)sizeof(d2);
  return 0;
}
static void dct_shape_out(const DctShape& sh, uint32_t* out) {
  memset(out, 0, FH_DCT_SHAPE_LEN * sizeof(uint32_t));
  out[0] = sh.levels; out[1] = sh.N1; out[2] = sh.N2; out[3] = sh.cap;
  out[4] = sh.r1.n; for (uint32_t i = 0; i < sh.r1.n; ++i) out[5 + i] = sh.r1.r[i];
  out[17] = sh.r2.n; for (uint32_t i = 0; i < sh.r2.n; ++i) out[18 + i] = sh.r2.r[i];
  out[30] = sh.ldsn1; out[31] = sh.rpw1; out[32] = sh.grid1; out[33] = sh.ldsn2; out[34] = sh.rpw2; out[35] = sh.grid2;
  out[36] = FH_WG; out[37] = sh.lds_bytes; out[38] = sh.tiles; out[39] = sh.launches;
}
extern "C" int fh_dct_shape(fh_ctx* c, uint32_t* out) {
  if (!c || !out) return fail(FH_E_ARG, "fh_dct_shape: null argument");
  if (c->op != OP_DCT) return fail(FH_E_STATE, "fh_dct_shape: the context holds no DCT operator (fh_set_dct)");
  if (c->dct2) return fail(FH_E_STATE, "fh_dct_shape: the context holds the DCT operator in its 2-D geometry (fh_set_dct2): fh_dct2_shape reports it");
  dct_shape_out(c->dct_sh, out);                          // (what dct_shape_for gave when fh_set_dct set the operator: the launchers read the same copy)
  return 0;
}
extern "C" int fh_dct_shape_for(uint64_t N, int row_cap, int ncu, uint32_t* out) {
  if (!out) return fail(FH_E_ARG, "fh_dct_shape_for: null argument");
  DctShape sh;
  const int rc = dct_shape_for(N, row_cap, ncu, &sh);
  dct_shape_out(sh, out);                                 // (a refused N: levels = 0, "not served", beside the error and its sentence)
  return rc;
}

// one pair of twiddle tables for a row length L (long double on the host, rounded once): tw[j] = e^{-2 pi i j / L}, pw[k] = e^{-i pi k / 2L}
static int dct_axis_tables(uint64_t L, d2** tw, d2** pw) {
  const long double pi = 3.14159265358979323846264338327950288L;
  std::vector<double> t(2 * L);
  HIP_TRY(hipMalloc((void**)tw, L * sizeof(d2)));
  HIP_TRY(hipMalloc((void**)pw, L * sizeof(d2)));
  for (uint64_t j = 0; j < L; ++j) { const long double a = 2.0L * pi * (long double)j / (long double)L; t[2 * j] = (double)cosl(a); t[2 * j + 1] = (double)-sinl(a); }
  HIP_TRY(hipMemcpy(*tw, t.data(), L * sizeof(d2), hipMemcpyHostToDevice));
  for (uint64_t k = 0; k < L; ++k) { const long double a = pi * (long double)k / (2.0L * (long double)L); t[2 * k] = (double)cosl(a); t[2 * k + 1] = (double)-sinl(a); }
  HIP_TRY(hipMemcpy(*pw, t.data(), L * sizeof(d2), hipMemcpyHostToDevice));
  return 0;
}
// the two twiddle tables, the diagonal and, for two levels, the work buffers.  A set-up cost, paid once
// per fh_set_dct: 4 N cosl / sinl calls and a host vector of 16 N bytes (N = 2^22: about 17 M long-double calls, of the order of a second)
static int dct_alloc_tables(fh_ctx* c, const DctShape& sh, const double* diag) {
  const uint64_t N = c->n;
  FH_TRY(dct_axis_tables(N, &c->dct_tw, &c->dct_pw));
  if (diag) {
    HIP_TRY(hipMalloc((void**)&c->dct_diag, N * sizeof(double)));
    HIP_TRY(hipMemcpy(c->dct_diag, diag, N * sizeof(double), hipMemcpyHostToDevice));
  }
  if (sh.levels == 2) {
    HIP_TRY(hipMalloc((void**)&c->dct_w0, N * sizeof(d2)));
    HIP_TRY(hipMalloc((void**)&c->dct_w1, N * sizeof(d2)));
  }
  return 0;
}
static DctOpP dct_op_params(fh_ctx* c, const DctShape& sh) {
  DctOpP o;
  o.N = (uint32_t)c->n; o.N1 = sh.N1; o.N2 = sh.N2; o.r1 = sh.r1; o.r2 = sh.r2;
  o.tw = c->dct_tw; o.pw = c->dct_pw; o.diag = c->dct_diag;
  o.sc0 = c->dct_sc0; o.sck = c->dct_sck;
  o.w0 = c->dct_w0; o.w1 = c->dct_w1;
  return o;
}
template <int CONJ>
static void dct_launch_rows_c(fh_ctx* c, uint32_t ldsn, uint32_t grid, const DctRowsP& q) {
  if (ldsn == 128u) k_dct_rows<128, CONJ><<<dim3(grid), dim3(FH_WG), 0, c->stream>>>(q);
  else if (ldsn == 512u) k_dct_rows<512, CONJ><<<dim3(grid), dim3(FH_WG), 0, c->stream>>>(q);
  else k_dct_rows<2048, CONJ><<<dim3(grid), dim3(FH_WG), 0, c->stream>>>(q);
}
// the three middle launches of a two-level transform: rows of length N1 (with the six-step twiddle), transpose, rows of length N2.
// K-fwd: real rows in w0 -> w1 -> w0 (in place); K-adj: complex rows in w0 (in place) -> w1 (in place).  A workgroup owns whole rows, so a
// row launch may write where it read.
static void dct_launch_middle(fh_ctx* c, const DctShape& sh, int conj) {
  DctRowsP q;
  q.N = (uint32_t)c->n; q.tw = c->dct_tw;
  q.L = sh.N1; q.nrows = sh.N2; q.rpw = sh.rpw1; q.rd = sh.r1; q.in = c->dct_w0; q.out = conj ? c->dct_w0 : c->dct_w1; q.real_in = conj ? 0 : 1; q.tw6 = 1;
  if (conj) dct_launch_rows_c<1>(c, sh.ldsn1, sh.grid1, q); else dct_launch_rows_c<0>(c, sh.ldsn1, sh.grid1, q);
  d2* tin = conj ? c->dct_w0 : c->dct_w1; d2* tout = conj ? c->dct_w1 : c->dct_w0;
  k_dct_tr<DCT_TT><<<dim3(sh.tiles), dim3(FH_WG), 0, c->stream>>>(tin, tout, sh.N2, sh.N1);
  q.L = sh.N2; q.nrows = sh.N1; q.rpw = sh.rpw2; q.rd = sh.r2; q.in = tout; q.out = tout; q.real_in = 0; q.tw6 = 0;
  if (conj) dct_launch_rows_c<1>(c, sh.ldsn2, sh.grid2, q); else dct_launch_rows_c<0>(c, sh.ldsn2, sh.grid2, q);
}

// ---- the DCT operator on an H x W image (fh_set_dct2; kernels in csrc/fh_dct2.h, instantiated by fh_dct2_part.hip) ---------------------------
#ifndef FH_SINGLE_TU
#define DCT2_DECLARE(LDSN) DCT2_KERNELS(extern template, LDSN)
DCT_FOR_EACH(DCT2_DECLARE)
#undef DCT2_DECLARE
DCT2_TILE_KERNELS(extern template)
#endif
// THE geometry of every launch of both directions, a pure function of (H, W), the row cap (FH_TUNE_DCT_ROW_CAP; 0 = DCT_ROW_CAP) and the device's CU
// count.  Each axis is ONE row transform: its length is at least 1, at most the cap and has the prime factors 2, 3 and 5 only (there is no two-level
// form per axis).  An axis takes the 1-D rule's radices and LDS class (dct_radices, dct_ldsn): along H there are W rows of length H, along W there
// are H rows of length W.  A workgroup takes as many rows as the class holds, at most DCT_MAX_ROWS, and fewer where that would leave fewer workgroups
// than CUs -- but never fewer than fill its 256 threads with one element each (short rows of a small image: lanes that would idle in every load and
// store loop otherwise).  Four launches per direction: two row launches and two tile launches of ceil(H / 32) * ceil(W / 32) workgroups.
static void dct2_rows_geometry(uint64_t L, uint64_t nrows, int ncu, uint32_t* ldsn, uint32_t* rpw, uint32_t* grid) {
  *ldsn = dct_ldsn(L);
  const uint64_t fit = std::max<uint64_t>(1, std::min<uint64_t>(std::min<uint64_t>(*ldsn / L, DCT_MAX_ROWS), nrows));
  const uint64_t fill = std::min<uint64_t>(fit, (FH_WG + L - 1) / L);
  const uint64_t r = std::max<uint64_t>(fill, std::min<uint64_t>(fit, nrows / (uint64_t)std::max(1, ncu)));
  *rpw = (uint32_t)r; *grid = (uint32_t)((nrows + r - 1) / r);
}
static int dct2_shape_for(uint64_t H, uint64_t W, int row_cap, int ncu, Dct2Shape* sh) {
  memset(sh, 0, sizeof(*sh));
  if (row_cap != 0 && (row_cap < 2 || row_cap > DCT_ROW_CAP)) return fail(FH_E_ARG, "DCT_ROW_CAP must be 0 (default: %d) or in [2, %d] elements per row transform", DCT_ROW_CAP, DCT_ROW_CAP);
  const uint64_t cap = row_cap ? (uint64_t)row_cap : DCT_ROW_CAP;
  sh->cap = (uint32_t)cap;                                // (set from here on: a refusal below is about the shape, not about the cap)
  const uint64_t len[2] = {H, W};
  const char* name[2] = {"H", "W"};
  for (int a = 0; a < 2; ++a) {
    const uint64_t L = len[a];
    if (L == 0) return fail(FH_E_ARG, "the 2-D DCT operator needs H, W >= 1: axis %d (%s) of the shape (%llu, %llu) is empty", a, name[a], (unsigned long long)H, (unsigned long long)W);
    uint64_t rest = L;
    for (uint64_t r : {2u, 3u, 5u}) while (rest % r == 0) rest /= r;
    if (rest != 1) return fail(FH_E_ARG, "the 2-D DCT operator serves axis lengths whose prime factors are 2, 3 and 5 only: axis %d (%s = %llu) of the shape (%llu, %llu) has a prime factor above 5",
                               a, name[a], (unsigned long long)L, (unsigned long long)H, (unsigned long long)W);
    if (L > cap) return fail(FH_E_ARG, "the 2-D DCT operator takes each axis as one row transform of at most the row cap (%llu): axis %d (%s = %llu) of the shape (%llu, %llu) is longer, and there is no two-level form per axis",
                             (unsigned long long)cap, a, name[a], (unsigned long long)L, (unsigned long long)H, (unsigned long long)W);
  }
  if (!dct_radices(H, &sh->rh) || !dct_radices(W, &sh->rw)) return fail(FH_E_ARG, "the 2-D DCT operator: the shape (%llu, %llu) needs more than %d radix passes per row", (unsigned long long)H, (unsigned long long)W, DCT_MAXRAD);
  sh->H = (uint32_t)H; sh->W = (uint32_t)W;
  dct2_rows_geometry(H, W, ncu, &sh->ldsn_h, &sh->rpw_h, &sh->grid_h);
  dct2_rows_geometry(W, H, ncu, &sh->ldsn_w, &sh->rpw_w, &sh->grid_w);
  sh->tiles = (uint32_t)(((H + DCT_TT - 1) / DCT_TT) * ((W + DCT_TT - 1) / DCT_TT));
  sh->launches = 4;
  sh->lds_bytes = std::max(sh->ldsn_h, sh->ldsn_w) * 2u * (uint32_t)sizeof(d2);
  sh->served = 1;
  return 0;
}
static void dct2_shape_out(const Dct2Shape& sh, uint32_t* out) {
  memset(out, 0, FH_DCT_SHAPE_LEN * sizeof(uint32_t));
  out[0] = sh.served; out[1] = sh.H; out[2] = sh.W; out[3] = sh.cap;
  out[4] = sh.rh.n; for (uint32_t i = 0; i < sh.rh.n; ++i) out[5 + i] = sh.rh.r[i];
  out[17] = sh.rw.n; for (uint32_t i = 0; i < sh.rw.n; ++i) out[18 + i] = sh.rw.r[i];
  out[30] = sh.ldsn_h; out[31] = sh.rpw_h; out[32] = sh.grid_h; out[33] = sh.ldsn_w; out[34] = sh.rpw_w; out[35] = sh.grid_w;
  out[36] = FH_WG; out[37] = sh.lds_bytes; out[38] = sh.tiles; out[39] = sh.launches;
}
extern "C" int fh_dct2_shape(fh_ctx* c, uint32_t* out) {
  if (!c || !out) return fail(FH_E_ARG, "fh_dct2_shape: null argument");
  if (c->op != OP_DCT || !c->dct2) return fail(FH_E_STATE, "fh_dct2_shape: the context holds no 2-D DCT operator (fh_set_dct2)");
  dct2_shape_out(c->dct2_sh, out);                        // (what dct2_shape_for gave when fh_set_dct2 set the operator: the launchers read the same copy)
  return 0;
}
extern "C" int fh_dct2_shape_for(uint64_t H, uint64_t W, int row_cap, int ncu, uint32_t* out) {
  if (!out) return fail(FH_E_ARG, "fh_dct2_shape_for: null argument");
  Dct2Shape sh;
  const int rc = dct2_shape_for(H, W, row_cap, ncu, &sh);
  dct2_shape_out(sh, out);                                // (a refused shape: [0] = 0, "not served", beside the error and its sentence)
  return rc;
}

// the tables of both axes, the diagonal and the two work images
static int dct2_alloc_tables(fh_ctx* c, const Dct2Shape& sh, const double* diag) {
  const uint64_t N = c->n;
  FH_TRY(dct_axis_tables(sh.H, &c->dct_tw, &c->dct_pw));
  FH_TRY(dct_axis_tables(sh.W, &c->dct2_tw, &c->dct2_pw));
  if (diag) {
    HIP_TRY(hipMalloc((void**)&c->dct_diag, N * sizeof(double)));
    HIP_TRY(hipMemcpy(c->dct_diag, diag, N * sizeof(double), hipMemcpyHostToDevice));
  }
  HIP_TRY(hipMalloc((void**)&c->dct2_w0, N * sizeof(double)));
  HIP_TRY(hipMalloc((void**)&c->dct2_w1, N * sizeof(double)));
  return 0;
}
static Dct2OpP dct2_op_params(fh_ctx* c, const Dct2Shape& sh) {
  Dct2OpP o;
  o.H = sh.H; o.W = sh.W;
  o.ah.L = sh.H; o.ah.rd = sh.rh; o.ah.tw = c->dct_tw; o.ah.pw = c->dct_pw; o.ah.sc0 = c->dct_sc0; o.ah.sck = c->dct_sck;
  o.aw.L = sh.W; o.aw.rd = sh.rw; o.aw.tw = c->dct2_tw; o.aw.pw = c->dct2_pw; o.aw.sc0 = c->dct2_sc0; o.aw.sck = c->dct2_sck;
  o.rpw_h = sh.rpw_h; o.rpw_w = sh.rpw_w;
  o.diag = c->dct_diag; o.w0 = c->dct2_w0; o.w1 = c->dct2_w1;
  return o;
}
template <int WHICH>
static void dct2_launch_fwd_rows(fh_ctx* c, uint32_t ldsn, uint32_t grid, const Dct2FwdP& p) {
  if (ldsn == 128u) k_dct2_fwd_rows<128, WHICH><<<dim3(grid), dim3(FH_WG), 0, c->stream>>>(p);
  else if (ldsn == 512u) k_dct2_fwd_rows<512, WHICH><<<dim3(grid), dim3(FH_WG), 0, c->stream>>>(p);
  else k_dct2_fwd_rows<2048, WHICH><<<dim3(grid), dim3(FH_WG), 0, c->stream>>>(p);
}
template <int WHICH>
static void dct2_launch_adj_rows(fh_ctx* c, uint32_t ldsn, uint32_t grid, const Dct2AdjP& p) {
  if (ldsn == 128u) k_dct2_adj_rows<128, WHICH><<<dim3(grid), dim3(FH_WG), 0, c->stream>>>(p);
  else if (ldsn == 512u) k_dct2_adj_rows<512, WHICH><<<dim3(grid), dim3(FH_WG), 0, c->stream>>>(p);
  else k_dct2_adj_rows<2048, WHICH><<<dim3(grid), dim3(FH_WG), 0, c->stream>>>(p);
}

// z := d * (C_H X C_W^T), X = prox(x0 - tau g0) (mode 0) or x0 (mode 1): four launches; the checks are launch_fwd_dct's
static int launch_fwd_dct2(fh_ctx* c, const FwdIO& io) {
  const Dct2Shape& sh = c->dct2_sh;
  Dct2FwdP p;
  memset(&p.f.op, 0, sizeof(p.f.op));                     // (the 1-D operator's block: the 2-D kernels do not read it)
  p.o = dct2_op_params(c, sh);
  p.f.mode = io.mode; p.f.sub_b = io.sub_b;
  p.f.x0 = io.x0; p.f.g0 = io.g0; p.f.xacc0 = io.xacc0; p.f.xhat = io.xhat; p.f.xp = io.xp; p.f.b = c->b; p.f.z = io.z; p.f.tau = io.tau;
  p.f.px = make_prox(c, io.tau);
  p.f.seq = 0u; p.f.nred_n = 0u;
  FH_TRY(ensure_ws(c, ((size_t)sh.tiles + sh.grid_w) * 8 * sizeof(double)));
  p.f.red = c->ws; p.f.red_n = c->ws + (size_t)sh.tiles * 8; p.f.counter = c->counters + CNT_FWD; p.f.out = scalar_out(c);
  t_begin(c, FH_K_FWD);
  dct2_launch_fwd_rows<1>(c, sh.ldsn_w, sh.grid_w, p);
  k_dct2_tr<DCT_TT><<<dim3(sh.tiles), dim3(FH_WG), 0, c->stream>>>(c->dct2_w0, c->dct2_w1, sh.H, sh.W);
  dct2_launch_fwd_rows<0>(c, sh.ldsn_h, sh.grid_h, p);
  p.f.nred_n = io.mode == 0 ? sh.grid_w : 0u;
  p.f.seq = seq_offer(c);
  k_dct2_post_fwd<DCT_TT><<<dim3(sh.tiles), dim3(FH_WG), 0, c->stream>>>(p);
  t_end(c, FH_K_FWD);
  HIP_TRY(hipGetLastError());
  return 0;
}

// g1 := C_H^T (d * (z' - b)) C_W with the residual, the loss at z' and the n-side epilogue: four launches; the checks are launch_adj_dct's
static int launch_adj_dct2(fh_ctx* c, const AdjIO& io) {
  const Dct2Shape& sh = c->dct2_sh;
  Dct2AdjP p;
  memset(&p.a.op, 0, sizeof(p.a.op));
  p.o = dct2_op_params(c, sh);
  p.a.z = io.z; p.a.zacc0 = io.zacc0; p.a.b = c->b; p.a.sub_b = io.sub_b; p.a.accel = io.accel; p.a.mode = io.mode; p.a.coef = io.coef; p.a.tau = io.tau;
  p.a.x0 = io.x0; p.a.xp = io.xp; p.a.xacc0 = io.xacc0; p.a.xhat = io.xhat; p.a.x1 = io.x1; p.a.g1 = io.g1;
  p.a.seq = 0u; p.a.nred_f = 0u;
  FH_TRY(ensure_ws(c, ((size_t)sh.tiles + sh.grid_w) * 8 * sizeof(double)));
  p.a.red = c->ws; p.a.red_f = c->ws + (size_t)sh.grid_w * 8; p.a.counter = c->counters + CNT_ADJ_FIN; p.a.out = scalar_out(c);
  t_begin(c, FH_K_ADJ);
  k_dct2_pre_adj<DCT_TT><<<dim3(sh.tiles), dim3(FH_WG), 0, c->stream>>>(p);
  dct2_launch_adj_rows<0>(c, sh.ldsn_h, sh.grid_h, p);
  k_dct2_tr<DCT_TT><<<dim3(sh.tiles), dim3(FH_WG), 0, c->stream>>>(c->dct2_w0, c->dct2_w1, sh.W, sh.H);
  p.a.nred_f = sh.tiles;
  p.a.seq = io.mode == 0 ? seq_offer(c) : 0u;
  dct2_launch_adj_rows<1>(c, sh.ldsn_w, sh.grid_w, p);
  t_end(c, FH_K_ADJ);
  HIP_TRY(hipGetLastError());
  return 0;
}

// z := d * C (mode 0: prox(x0 - tau g0) ; mode 1: x0): one launch (N <= row cap) or five
static int launch_fwd_dct(fh_ctx* c, const FwdIO& io) {
  FH_TRY(check_loss_run(c));
  if (io.mode == 0) FH_TRY(check_prox_run(c));
  if (c->dct2) return launch_fwd_dct2(c, io);
  const DctShape& sh = c->dct_sh;
  DctFwdP p;
  p.op = dct_op_params(c, sh);
  p.mode = io.mode; p.sub_b = io.sub_b;
  p.x0 = io.x0; p.g0 = io.g0; p.xacc0 = io.xacc0; p.xhat = io.xhat; p.xp = io.xp; p.b = c->b; p.z = io.z; p.tau = io.tau;
  p.px = make_prox(c, io.tau);
  p.seq = 0u; p.nred_n = 0u; p.red_n = nullptr;
  const uint32_t grid = sh.levels == 1 ? 1u : sh.tiles;
  FH_TRY(ensure_ws(c, (size_t)grid * 16 * sizeof(double)));
  p.red = c->ws; p.counter = c->counters + CNT_FWD; p.out = scalar_out(c);
  t_begin(c, FH_K_FWD);
  if (sh.levels == 1) {
    p.seq = seq_offer(c);
    if (sh.ldsn1 == 128u) k_dct1_fwd<128><<<dim3(1), dim3(FH_WG), 0, c->stream>>>(p);
    else if (sh.ldsn1 == 512u) k_dct1_fwd<512><<<dim3(1), dim3(FH_WG), 0, c->stream>>>(p);
    else k_dct1_fwd<2048><<<dim3(1), dim3(FH_WG), 0, c->stream>>>(p);
  } else {
    p.red_n = c->ws + (size_t)grid * 8;
    k_dct_pre_fwd<DCT_TT><<<dim3(grid), dim3(FH_WG), 0, c->stream>>>(p);
    dct_launch_middle(c, sh, 0);
    p.nred_n = io.mode == 0 ? grid : 0u;
    p.seq = seq_offer(c);
    k_dct_post_fwd<DCT_TT><<<dim3(grid), dim3(FH_WG), 0, c->stream>>>(p);
  }
  t_end(c, FH_K_FWD);
  HIP_TRY(hipGetLastError());
  return 0;
}

// g1 := C^T (d * (z' - b)) with the residual, the loss at z' and the n-side epilogue: one launch (N <= row cap) or five
static int launch_adj_dct(fh_ctx* c, const AdjIO& io) {
  FH_TRY(check_loss_run(c));
  if (io.mode != 0 && io.mode != 1) return fail(FH_E_STATE, "the DCT operator has no row-sharded adjoint");
  if (c->dct2) return launch_adj_dct2(c, io);
  const DctShape& sh = c->dct_sh;
  DctAdjP p;
  p.op = dct_op_params(c, sh);
  p.z = io.z; p.zacc0 = io.zacc0; p.b = c->b; p.sub_b = io.sub_b; p.accel = io.accel; p.mode = io.mode; p.coef = io.coef; p.tau = io.tau;
  p.x0 = io.x0; p.xp = io.xp; p.xacc0 = io.xacc0; p.xhat = io.xhat; p.x1 = io.x1; p.g1 = io.g1;
  p.seq = 0u; p.nred_f = 0u; p.red_f = nullptr;
  const uint32_t grid = sh.levels == 1 ? 1u : sh.tiles;
  FH_TRY(ensure_ws(c, (size_t)grid * 16 * sizeof(double)));
  p.red = c->ws; p.counter = c->counters + CNT_ADJ_FIN; p.out = scalar_out(c);
  t_begin(c, FH_K_ADJ);
  if (sh.levels == 1) {
    p.seq = io.mode == 0 ? seq_offer(c) : 0u;
    if (sh.ldsn1 == 128u) k_dct1_adj<128><<<dim3(1), dim3(FH_WG), 0, c->stream>>>(p);
    else if (sh.ldsn1 == 512u) k_dct1_adj<512><<<dim3(1), dim3(FH_WG), 0, c->stream>>>(p);
    else k_dct1_adj<2048><<<dim3(1), dim3(FH_WG), 0, c->stream>>>(p);
  } else {
    p.red_f = c->ws + (size_t)grid * 8;
    k_dct_pre_adj<DCT_TT><<<dim3(grid), dim3(FH_WG), 0, c->stream>>>(p);
    dct_launch_middle(c, sh, 1);
    p.nred_f = grid;
    p.op.w0 = c->dct_w1;                                  // (where the second row launch left the transform)
    p.seq = io.mode == 0 ? seq_offer(c) : 0u;
    k_dct_post_adj<DCT_TT><<<dim3(grid), dim3(FH_WG), 0, c->stream>>>(p);
  }
  t_end(c, FH_K_ADJ);
  HIP_TRY(hipGetLastError());
  return 0;
}

// ---- identity operator with an elementwise loss, and the nuclear-norm prox (fh_set_identity / fh_set_prox_nuclear; kernels in csrc/fh_nuclear.h) ----
#ifndef FH_SINGLE_TU
NUC_KERNELS(extern template)
#endif
static inline bool nuc_kind(int kind) { return kind == FH_PROX_NUCLEAR || kind == FH_PROX_NUCBALL; }      // the two kinds behind the Jacobi decomposition
// THE geometry of the thresholding, a pure function of (M, N) and FH_TUNE_NUC_BLOCK_ROWS (0 = auto = NUC_AUTO_BLOCK_ROWS): p = min, q = max, P = p padded to a multiple of
// Bk, nb = P / Bk blocks, a sweep of nb - 1 steps (nb even; nb for an odd nb, whose steps each give one block a bye; 1 for nb = 1: the self-pair) of
// ceil(nb / 2) workgroups, rows of [ W | J^T ] of ld = (q padded to even) + (P padded to even) doubles.
static int nuc_shape_for(uint64_t M, uint64_t N, int block_rows, NucShape* sh) {
  memset(sh, 0, sizeof(*sh));
  if (block_rows != 0 && block_rows != 1 && block_rows != 2 && block_rows != 4 && block_rows != 8) return fail(FH_E_ARG, "NUC_BLOCK_ROWS must be 0 (auto), 1, 2, 4 or 8 rows per block");
  if (M == 0 || N == 0) return fail(FH_E_ARG, "the identity operator needs a non-empty matrix unknown (got %llu x %llu)", (unsigned long long)M, (unsigned long long)N);
  if (M > (1ull << 26) || N > (1ull << 26) || M * N > (1ull << 26)) return fail(FH_E_ARG, "the identity operator serves at most 2^26 entries (got %llu x %llu)", (unsigned long long)M, (unsigned long long)N);
  const uint64_t p = std::min(M, N), q = std::max(M, N);
  if (p > NUC_MAX_P) return fail(FH_E_ARG, "FH_PROX_NUCLEAR / FH_PROX_NUCBALL serve min(M, N) <= %d (got %llu x %llu): the Jacobi sweeps are quadratic in it", NUC_MAX_P, (unsigned long long)M, (unsigned long long)N);
  const uint32_t Bk = block_rows ? (uint32_t)block_rows : NUC_AUTO_BLOCK_ROWS;
  NucGeo& g = sh->g;
  g.M = (uint32_t)M; g.N = (uint32_t)N; g.p = (uint32_t)p; g.q = (uint32_t)q; g.transposed = M > N ? 1 : 0;
  g.P = (uint32_t)round_up(p, Bk); g.nb = g.P / Bk;
  g.qpad = (uint32_t)round_up(q, 2); g.ld = g.qpad + (uint32_t)round_up(g.P, 2);
  const uint32_t nbe = g.nb + (g.nb & 1u);
  sh->Bk = Bk;
  sh->steps = g.nb == 1 ? 1u : nbe - 1u;
  sh->wgs = g.nb == 1 ? 1u : nbe / 2u;
  sh->chunks = (g.qpad + NUC_CC - 1) / NUC_CC;
  sh->bytes = (uint64_t)g.P * g.ld * sizeof(double);
  sh->lds_bytes = (uint32_t)((2 * Bk * NUC_LDT + 2 * (2 * Bk) * (2 * Bk) + FH_WG) * sizeof(double));
  return 0;
}
static void nuc_shape_out(const NucShape& sh, uint64_t* out) {
  const uint64_t v[FH_NUCLEAR_SHAPE_LEN] = {(uint64_t)sh.g.transposed, sh.g.p, sh.g.q, sh.Bk, sh.g.P, sh.g.nb, sh.steps, sh.wgs, NUC_CC, sh.chunks, sh.g.ld, sh.bytes, sh.lds_bytes};
  memcpy(out, v, sizeof(v));
}
extern "C" int fh_nuclear_shape(fh_ctx* c, uint64_t* out) {
  if (!c || !out) return fail(FH_E_ARG, "fh_nuclear_shape: null argument");
  if (c->op != OP_IDENTITY || !nuc_kind(c->prox_kind)) return fail(FH_E_STATE, "fh_nuclear_shape: the context holds no identity operator with FH_PROX_NUCLEAR or FH_PROX_NUCBALL (fh_set_identity, then fh_set_prox_nuclear / fh_set_prox)");
  nuc_shape_out(c->nuc_sh, out);                          // (what nuc_shape_for gave when the prox was set: the launchers read the same copy)
  return 0;
}
extern "C" int fh_nuclear_shape_for(uint64_t M, uint64_t N, int block_rows, int ncu, uint64_t* out) {
  (void)ncu;                                              // (the schedule is the tournament's: it does not depend on the device's size)
  if (!out) return fail(FH_E_ARG, "fh_nuclear_shape_for: null argument");
  NucShape sh;
  const int rc = nuc_shape_for(M, N, block_rows, &sh);
  nuc_shape_out(sh, out);
  return rc;
}

static void nuc_launch_step(fh_ctx* c, const NucStepP& q, uint32_t Bk, uint32_t wgs) {
  switch (Bk) {
    case 1: k_nuc_step<1><<<dim3(wgs), dim3(FH_WG), 0, c->stream>>>(q); break;
    case 2: k_nuc_step<2><<<dim3(wgs), dim3(FH_WG), 0, c->stream>>>(q); break;
    case 4: k_nuc_step<4><<<dim3(wgs), dim3(FH_WG), 0, c->stream>>>(q); break;
    default: k_nuc_step<8><<<dim3(wgs), dim3(FH_WG), 0, c->stream>>>(q); break;
  }
}
// W := the operand (x0 - tau*g0, kept in `xhat`, or x0 itself when g0 is null), then sweeps of steps until one rotates nothing.  ONE host
// synchronisation per sweep (the sweep's integer counter), none per step.  FH_E_NOCONV after NUC_MAX_SWEEPS sweeps that all rotated.
static int nuc_decompose(fh_ctx* c, const double* x0, const double* g0, double tau, double* xhat, int with_j, uint64_t* info) {
  const NucShape& sh = c->nuc_sh;
  const uint64_t total = (uint64_t)sh.g.P * sh.g.ld;
  const unsigned lgrid = (unsigned)std::min<uint64_t>((total + FH_WG - 1) / FH_WG, 2048);
  FH_TRY(ensure_ws(c, (size_t)lgrid * sizeof(double)));
  NucLoadP lp;
  lp.g = sh.g; lp.x0 = x0; lp.g0 = g0; lp.tau = tau; lp.xhat = xhat; lp.W = c->nuc_w; lp.with_j = with_j;
  lp.red = c->ws; lp.counter = c->counters + CNT_AUX; lp.fro2 = c->nuc_scal;
  HIP_TRY(hipMemsetAsync(c->nuc_cnt, 0, 32 * sizeof(unsigned), c->stream));
  k_nuc_load<<<dim3(lgrid), dim3(FH_WG), 0, c->stream>>>(lp);
  HIP_TRY(hipGetLastError());
  NucStepP q;
  q.g = sh.g; q.W = c->nuc_w; q.cols = with_j ? sh.g.ld : sh.g.qpad; q.fro2 = c->nuc_scal;
  info[0] = info[1] = info[2] = 0;
  for (int sweep = 0; sweep < NUC_MAX_SWEEPS; ++sweep) {
    q.rotations = c->nuc_cnt + sweep;
    for (uint32_t st = 0; st < sh.steps; ++st) { q.step = st; nuc_launch_step(c, q, sh.Bk, sh.wgs); }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(c->nuc_host + sweep, c->nuc_cnt + sweep, sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    info[0] += 1; info[1] += sh.steps; info[2] += c->nuc_host[sweep];
    if (c->nuc_host[sweep] == 0u) return 0;
  }
  return fail(FH_E_NOCONV, "FH_PROX_NUCLEAR / FH_PROX_NUCBALL: the block-Jacobi sweeps still rotated after %d sweeps (%llu rotations in the last one)", NUC_MAX_SWEEPS,
              (unsigned long long)c->nuc_host[NUC_MAX_SWEEPS - 1]);
}
static int nuc_sigma(fh_ctx* c, double thr, double* phi, double* out_gsum, double* out_gmax, double* out_rank, int to_host) {
  const NucShape& sh = c->nuc_sh;
  FH_TRY(ensure_ws(c, (size_t)sh.g.P * 2 * sizeof(double)));
  NucSigmaP sp;
  sp.g = sh.g; sp.W = c->nuc_w; sp.thr = thr; sp.phi = phi; sp.red = c->ws; sp.counter = c->counters + CNT_AUX;
  sp.out_gsum = out_gsum; sp.out_gmax = out_gmax; sp.out_rank = out_rank; sp.to_host = to_host;
  k_nuc_sigma<<<dim3(sh.g.P), dim3(FH_WG), 0, c->stream>>>(sp);
  HIP_TRY(hipGetLastError());
  return 0;
}
// xhat = x0 - tau*g0 and xp = its singular-value soft-threshold at tau*mu (FH_PROX_NUCBALL: its projection onto the nuclear-norm ball of radius mu, whose level
// k_nuc_ball finds from the sigma that k_nuc_sigma left in its per-row records at thr = 0, a launch that forms no sums); nuc_scal[1] = the nuclear norm of xp, [2] = the rank kept, [3] = its largest singular value
static int nuc_prox(fh_ctx* c, double tau, const double* x0, const double* g0, double* xhat, double* xp) {
  const NucShape& sh = c->nuc_sh;
  t_begin(c, FH_K_LEVEL);
  const int rc = nuc_decompose(c, x0, g0, tau, xhat, 1, c->nuc_info);
  if (rc != 0) {                                          // never a finite wrong prox
    char keep[sizeof(g_err)];
    memcpy(keep, g_err, sizeof(keep));
    k_nuc_fill<<<dim3(256), dim3(FH_WG), 0, c->stream>>>(xp, c->n, __builtin_nan(""));
    (void)hipStreamSynchronize(c->stream);
    t_end(c, FH_K_LEVEL);
    memcpy(g_err, keep, sizeof(keep));
    return rc;
  }
  if (c->prox_kind == FH_PROX_NUCBALL) {
    FH_TRY(nuc_sigma(c, 0.0, nullptr, nullptr, nullptr, nullptr, 0));
    NucBallP bp;
    bp.p = sh.g.p; bp.P = sh.g.P; bp.radius = c->mu; bp.red = c->ws; bp.phi = c->nuc_phi;
    bp.out_gsum = c->nuc_scal + 1; bp.out_gmax = c->nuc_scal + 3; bp.out_rank = c->nuc_scal + 2;
    k_nuc_ball<<<dim3(1), dim3(FH_WG), 0, c->stream>>>(bp);
    HIP_TRY(hipGetLastError());
  }
  else FH_TRY(nuc_sigma(c, tau * c->mu, c->nuc_phi, c->nuc_scal + 1, c->nuc_scal + 3, c->nuc_scal + 2, 0));
  NucReconP rp;
  rp.g = sh.g; rp.W = c->nuc_w; rp.phi = c->nuc_phi; rp.xp = xp;
  k_nuc_recon<<<dim3((sh.g.q + FH_WG - 1) / FH_WG, (sh.g.p + NUC_TR - 1) / NUC_TR), dim3(FH_WG), 0, c->stream>>>(rp);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(c->nuc_host + 32, c->nuc_scal + 2, sizeof(double), hipMemcpyDeviceToHost, c->stream));      // the rank kept, for fh_nuclear_info
  t_end(c, FH_K_LEVEL);
  return 0;
}
// the nuclear and the spectral norm of x (a values-only decomposition: the same steps, no J block, no reconstruction) -> *out_gsum, *out_gmax;
// objective = 0: NaN in *out_gsum instead, *out_gmax is left as it is
static __global__ void k_nuc_set(double* p, double v) { scal_store(p, v); }
static int nuc_norm(fh_ctx* c, const double* x, double* out_gsum, double* out_gmax) {
  if (!c->nuc_objective) {
    k_nuc_set<<<dim3(1), dim3(1), 0, c->stream>>>(out_gsum, __builtin_nan(""));
    HIP_TRY(hipGetLastError());
    return 0;
  }
  t_begin(c, FH_K_LEVEL);
  uint64_t info[3];                                       // (fh_nuclear_info reports on the latest PROX, not on this run)
  const int rc = nuc_decompose(c, x, nullptr, 0.0, nullptr, 0, info);
  if (rc == 0) FH_TRY(nuc_sigma(c, 0.0, nullptr, out_gsum, out_gmax, nullptr, 1));
  t_end(c, FH_K_LEVEL);
  return rc;
}

// z := prox(x0 - tau g0) (mode 0) or x0 (mode 1), the loss sum and the n-side sums: one elementwise launch (behind the thresholding for FH_PROX_NUCLEAR)
static int launch_fwd_identity(fh_ctx* c, const FwdIO& io) {
  if (io.mode == 0) FH_TRY(check_prox_run(c));
  const bool nuc = io.mode == 0 && nuc_kind(c->prox_kind);
  if (nuc) FH_TRY(nuc_prox(c, io.tau, io.x0, io.g0, io.xhat, io.xp));
  IdFwdP p;
  p.n = c->n; p.mode = io.mode; p.given = nuc ? 1 : 0; p.sub_b = io.sub_b; p.loss = c->loss_kind;
  p.x0 = io.x0; p.g0 = io.g0; p.xacc0 = io.xacc0; p.xhat = io.xhat; p.xp = io.xp; p.z = io.z; p.b = c->b; p.tau = io.tau;
  p.px = make_prox(c, io.tau);
  p.nuc = c->nuc_scal ? c->nuc_scal + 1 : nullptr;
  const unsigned grid = (unsigned)std::min<uint64_t>((c->n + FH_WG - 1) / FH_WG, 2048);
  FH_TRY(ensure_ws(c, (size_t)grid * 8 * sizeof(double)));
  p.red = c->ws; p.counter = c->counters + CNT_FWD; p.out = scalar_out(c);
  t_begin(c, FH_K_FWD);
  p.seq = seq_offer(c);
  if (c->loss_w) { IdFwdWP q; q.p = p; q.w = c->loss_w; k_id_fwd<true><<<dim3(grid), dim3(FH_WG), 0, c->stream>>>(q); }
  else k_id_fwd<false><<<dim3(grid), dim3(FH_WG), 0, c->stream>>>(p);
  t_end(c, FH_K_FWD);
  HIP_TRY(hipGetLastError());
  return 0;
}

// g1 := grad f(x1), x1 = xprox or its extrapolation, and the n-side epilogue; FH_PROX_NUCLEAR: the norms of x1 are the thresholding's when x1 is xprox,
// a values-only decomposition of the extrapolated x1 otherwise
static int launch_adj_identity(fh_ctx* c, const AdjIO& io) {
  if (io.mode != 0 && io.mode != 1) return fail(FH_E_STATE, "the identity operator has no row-sharded adjoint");
  const bool nuc = io.mode == 0 && nuc_kind(c->prox_kind);
  IdAdjP p;
  p.n = c->n; p.mode = io.mode; p.accel = io.accel; p.sub_b = io.sub_b; p.loss = c->loss_kind;
  p.gsum_mode = !nuc ? 0 : (!io.accel ? 1 : (c->nuc_objective ? 3 : 2));
  p.coef = io.coef; p.tau = io.tau; p.z = io.z; p.b = c->b;
  p.x0 = io.x0; p.xp = io.xp; p.xacc0 = io.xacc0; p.xhat = io.xhat; p.x1 = io.x1; p.g1 = io.g1;
  p.gsum_src = c->nuc_scal ? c->nuc_scal + 1 : nullptr;
  const unsigned grid = (unsigned)std::min<uint64_t>((c->n + FH_WG - 1) / FH_WG, 2048);
  FH_TRY(ensure_ws(c, (size_t)grid * 8 * sizeof(double)));
  p.red = c->ws; p.counter = c->counters + CNT_ADJ_FIN; p.out = scalar_out(c);
  t_begin(c, FH_K_ADJ);
  p.seq = (io.mode == 0 && p.gsum_mode != 3) ? seq_offer(c) : 0u;
  if (c->loss_w) { IdAdjWP q; q.p = p; q.w = c->loss_w; k_id_adj<true><<<dim3(grid), dim3(FH_WG), 0, c->stream>>>(q); }
  else k_id_adj<false><<<dim3(grid), dim3(FH_WG), 0, c->stream>>>(p);
  t_end(c, FH_K_ADJ);
  HIP_TRY(hipGetLastError());
  if (p.gsum_mode == 3) FH_TRY(nuc_norm(c, io.x1, scalar_out(c) + FH_S_GSUM_ADJ, scalar_out(c) + FH_S_GMAX_ADJ));
  return 0;
}

// sum|x_i| and max|x_i| of an n-length device vector -> dscal[GSUM], dscal[GMAX]  (g(x0) for objective_hist[0], :143)
static int launch_gterms(fh_ctx* c, const double* x) {
  if (c->op == OP_IDENTITY && nuc_kind(c->prox_kind))      // the norms of x0 are not free here (the forward pass that precedes wrote FH_S_GMAX = 0)
    return nuc_norm(c, x, scalar_out(c) + FH_S_GSUM, scalar_out(c) + FH_S_GMAX);
  if (c->LB) {              // (n, L) matrix: the same two terms, or the sum of row norms for FH_PROX_GROUP
    const unsigned mgrid = (unsigned)std::min<uint64_t>((c->n + FH_WG - 1) / FH_WG, 1024);
    FH_TRY(ensure_ws(c, (size_t)mgrid * 2 * sizeof(double)));
    const uint64_t grows = c->prox_kind == FH_PROX_ROWSPLIT ? c->rs_split : c->n;      // (FH_PROX_ROWSPLIT: the l1 term lives on the top rows)
    t_begin(c, FH_K_AUX);
    k_mc_gterms<<<dim3(mgrid), dim3(FH_WG), 0, c->stream>>>(x, (uint32_t)grows, c->L, c->LB, c->prox_kind == FH_PROX_GROUP ? 1 : 0, c->ws, c->counters + CNT_AUX, scalar_out(c));
    t_end(c, FH_K_AUX);
    HIP_TRY(hipGetLastError());
    return 0;
  }
  const unsigned grid = (unsigned)std::min<uint64_t>((c->n + FH_WG - 1) / FH_WG, 1024);
  FH_TRY(ensure_ws(c, (size_t)grid * 2 * sizeof(double)));
  t_begin(c, FH_K_AUX);
  k_gterms<<<dim3(grid), dim3(FH_WG), 0, c->stream>>>(x, (uint32_t)c->n, c->ws, c->counters + CNT_AUX, scalar_out(c));
  t_end(c, FH_K_AUX);
  HIP_TRY(hipGetLastError());
  return 0;
}

// Which search kernel a vector of n entries takes (csrc/fh_prox.h): the ONE rule, which launch_level_search calls and fh_level_shape_for exports.
//   n <= 1024: k_level_search<4, 256>;  <= 4096: <16, 256>;  <= 8192: <32, 256>;  <= 16384: <16> on 1024 threads;
//   <= 262144: k_level_search_multi on ceil(n / 8192) workgroups of 1024 threads, 8 entries per thread;  beyond: k_level_search<0> (re-read every pass)
struct LevelShape { uint32_t multi, threads, ept, workgroups; };
static LevelShape level_shape_for(uint32_t n) {
  if (n <= 4u * 256u) return {0u, 256u, 4u, 1u};
  if (n <= 16u * 256u) return {0u, 256u, 16u, 1u};
  if (n <= 32u * 256u) return {0u, 256u, 32u, 1u};
  if (n <= 16u * LVL_WG) return {0u, LVL_WG, 16u, 1u};
  if (n <= (uint32_t)LVL_MAXG * LVL_MEPT * LVL_WG) return {1u, LVL_WG, LVL_MEPT, (n + LVL_MEPT * LVL_WG - 1) / (LVL_MEPT * LVL_WG)};
  return {0u, LVL_WG, 0u, 1u};
}
extern "C" int fh_level_shape_for(uint64_t n, uint32_t* out) {
  if (!out) return fail(FH_E_ARG, "fh_level_shape_for: null argument");
  if (n == 0 || n >= (1ull << 31)) return fail(FH_E_ARG, "fh_level_shape_for: the vector length must be in [1, 2^31)");
  const LevelShape sh = level_shape_for((uint32_t)n);
  out[0] = sh.multi; out[1] = sh.threads; out[2] = sh.ept; out[3] = sh.workgroups;
  return 0;
}

// clipping level alpha for FH_PROX_LINF (radius tau*mu) / FH_PROX_L1BALL (radius mu) -> dscal[FH_NSCALARS]
static int launch_level_search(fh_ctx* c, double tau) {
  if (c->op != OP_DENSE && c->op != OP_DCT && c->op != OP_CONV) return fail(FH_E_STATE, "LINF / L1BALL prox need the dense operator");      // (the search reads x0, g0 and n only)
  const double radius = c->prox_kind == FH_PROX_L1BALL ? c->mu : tau * c->mu;
  const double* x0 = c->X[c->xi];
  const double* g0 = c->G[c->gc];
  double* out = c->dscal + FH_NSCALARS;
  const uint32_t n = (uint32_t)c->n;
  const LevelShape sh = level_shape_for(n);
  if (sh.multi) {      // several workgroups, LVL_MEPT values per thread (csrc/fh_prox.h)
    if (!c->lvl_rec) {
      HIP_TRY(hipMalloc((void**)&c->lvl_rec, (size_t)LVL_MAXPASS * LVL_MAXG * 2 * sizeof(double)));
      HIP_TRY(hipMalloc((void**)&c->lvl_cnt, (LVL_MAXPASS + 1) * sizeof(unsigned)));
      HIP_TRY(hipMemsetAsync(c->lvl_cnt, 0, (LVL_MAXPASS + 1) * sizeof(unsigned), c->stream));
    }
    LevelWs ws = {c->lvl_rec, c->lvl_cnt, c->counters + CNT_DIAG};
    const unsigned G = sh.workgroups;
    const int hooks = ((c->test_hooks & FH_HOOK_LEVEL_WITHHOLD) ? LVL_HOOK_WITHHOLD : 0) | ((c->test_hooks & FH_HOOK_LEVEL_NO_FALLBACK) ? LVL_HOOK_NO_FALLBACK : 0);
    t_begin(c, FH_K_LEVEL);
    k_level_search_multi<<<dim3(G), dim3(LVL_WG), 0, c->stream>>>(x0, g0, n, tau, radius, out, ws, hooks);
    t_end(c, FH_K_LEVEL);
    HIP_TRY(hipGetLastError());
    return 0;
  }
  t_begin(c, FH_K_LEVEL);
  if (sh.threads == 256u) {
    if (sh.ept == 4u) k_level_search<4, 256><<<dim3(1), dim3(256), 0, c->stream>>>(x0, g0, n, tau, radius, out);
    else if (sh.ept == 16u) k_level_search<16, 256><<<dim3(1), dim3(256), 0, c->stream>>>(x0, g0, n, tau, radius, out);
    else k_level_search<32, 256><<<dim3(1), dim3(256), 0, c->stream>>>(x0, g0, n, tau, radius, out);
  }
  else if (sh.ept == 16u) k_level_search<16><<<dim3(1), dim3(LVL_WG), 0, c->stream>>>(x0, g0, n, tau, radius, out);
  else k_level_search<0><<<dim3(1), dim3(LVL_WG), 0, c->stream>>>(x0, g0, n, tau, radius, out);
  t_end(c, FH_K_LEVEL);
  HIP_TRY(hipGetLastError());
  return 0;
}

static int launch_fwd_tv(fh_ctx* c, const FwdIO& io) {
  // (the stencil path materialises neither xhat nor the gradient, fh_tv.h: io.xhat and io.g0 are not read)
  if (io.mode == 0) FH_TRY(check_prox_run(c));
  const uint32_t H = (uint32_t)c->H, W = (uint32_t)c->W;
  const uint32_t rows_wg = (uint32_t)(c->tv_rows > 0 ? c->tv_rows : 32);
  const uint32_t row_chunks = (H + rows_wg - 1) / rows_wg;
  if (io.mode == 0) {
    if (!c->zcur) return fail(FH_E_STATE, "fh_fwd on the stencil operator before fh_init");
    TvStepFwdP p;
    p.H = H; p.W = W; p.rows_wg = rows_wg;
    p.strip_groups = ((W + TVS_FWD_OWN - 1) / TVS_FWD_OWN + 3) / 4;
    p.x0 = io.x0; p.xacc0 = io.xacc0; p.xp = io.xp; p.zc = c->zcur; p.b = c->b; p.zn = io.z; p.tau = io.tau;
    const unsigned grid = p.strip_groups * row_chunks;
    FH_TRY(ensure_ws(c, (size_t)grid * 8 * sizeof(double)));
    p.red = c->ws; p.counter = c->counters + CNT_FWD; p.out = scalar_out(c);
    t_begin(c, FH_K_FWD);
#define TV_STEP(U, NT)                                                                                           \
  do {                                                                                                           \
    if (c->prox_kind == FH_PROX_TVBALL) k_fwd_tv_step<0, U, NT><<<dim3(grid), dim3(FH_WG), 0, c->stream>>>(p);   \
    else k_fwd_tv_step<1, U, NT><<<dim3(grid), dim3(FH_WG), 0, c->stream>>>(p);                                  \
  } while (0)
    if (c->tv_nt == 1) { if (c->tv_u == 2) TV_STEP(2, 1); else if (c->tv_u == 4) TV_STEP(4, 1); else TV_STEP(8, 1); }
    else { if (c->tv_u == 2) TV_STEP(2, 0); else if (c->tv_u == 4) TV_STEP(4, 0); else TV_STEP(8, 0); }
#undef TV_STEP
    t_end(c, FH_K_FWD);
    HIP_TRY(hipGetLastError());
    return 0;
  }
  TvFwdP p;
  p.H = H; p.W = W; p.rows_wg = rows_wg;
  p.strip_groups = ((W + TV_SW - 1) / TV_SW + 3) / 4;
  p.x0 = io.x0; p.b = c->b; p.z = io.z; p.sub_b = io.sub_b;
  const unsigned grid = p.strip_groups * row_chunks;
  FH_TRY(ensure_ws(c, (size_t)grid * 8 * sizeof(double)));
  p.red = c->ws; p.counter = c->counters + CNT_FWD; p.out = scalar_out(c);
  t_begin(c, FH_K_FWD);
  if (c->tv_nt == 1) k_fwd_tv<4, 1><<<dim3(grid), dim3(FH_WG), 0, c->stream>>>(p);
  else k_fwd_tv<4, 0><<<dim3(grid), dim3(FH_WG), 0, c->stream>>>(p);
  t_end(c, FH_K_FWD);
  HIP_TRY(hipGetLastError());
  return 0;
}

static int launch_adj_tv(fh_ctx* c, const AdjIO& io) {
  const uint32_t H = (uint32_t)c->H, W = (uint32_t)c->W;
  const uint32_t rows_wg = (uint32_t)(c->tv_rows > 0 ? c->tv_rows : 128);
  const uint32_t row_chunks = (H + rows_wg - 1) / rows_wg;
  if (io.mode == 0) {          // FBS step: reductions only, the gradient is recomputed from z and b
    if (!c->zcur) return fail(FH_E_STATE, "fh_adj on the stencil operator before fh_init");
    TvStepAdjP p;
    p.H = H; p.W = W; p.rows_wg = rows_wg;
    p.strip_groups = ((W + TVS_ADJ_OWN - 1) / TVS_ADJ_OWN + 3) / 4;
    p.zn = io.z; p.zacc0 = io.zacc0; p.zc = c->zcur; p.b = c->b;
    p.accel = io.accel; p.coef = io.coef; p.tau = io.tau;
    p.x0 = io.x0; p.xp = io.xp; p.xacc0 = io.xacc0; p.x1 = io.x1; p.zx = c->ZX[c->zxc ^ 1];
    const unsigned grid = p.strip_groups * row_chunks;
    FH_TRY(ensure_ws(c, (size_t)grid * 8 * sizeof(double)));
    p.red = c->ws; p.counter = c->counters + CNT_ADJ_FIN; p.out = scalar_out(c);
    t_begin(c, FH_K_ADJ);
#define TV_STEP(U, NT) k_adj_tv_step<U, NT><<<dim3(grid), dim3(FH_WG), 0, c->stream>>>(p)
    if (c->tv_nt == 1) { if (c->tv_u == 2) TV_STEP(2, 1); else if (c->tv_u == 4) TV_STEP(4, 1); else TV_STEP(8, 1); }
    else { if (c->tv_u == 2) TV_STEP(2, 0); else if (c->tv_u == 4) TV_STEP(4, 0); else TV_STEP(8, 0); }
#undef TV_STEP
    t_end(c, FH_K_ADJ);
    HIP_TRY(hipGetLastError());
    return 0;
  }
  TvAdjP p;                    // plain gradient (Lipschitz probes, fh_apply): materialises g1 = grad(z - b)
  p.H = H; p.W = W; p.rows_wg = rows_wg;
  p.strip_groups = ((W + TV_SW - 1) / TV_SW + 3) / 4;
  p.z = io.z; p.b = c->b; p.sub_b = io.sub_b; p.g1 = io.g1;
  const unsigned grid = p.strip_groups * row_chunks;
  FH_TRY(ensure_ws(c, (size_t)grid * 8 * sizeof(double)));
  p.red = c->ws; p.counter = c->counters + CNT_ADJ_FIN; p.out = scalar_out(c);
  t_begin(c, FH_K_ADJ);
  if (c->tv_nt == 1) k_adj_tv<4, 1><<<dim3(grid), dim3(FH_WG), 0, c->stream>>>(p);
  else k_adj_tv<4, 0><<<dim3(grid), dim3(FH_WG), 0, c->stream>>>(p);
  t_end(c, FH_K_ADJ);
  HIP_TRY(hipGetLastError());
  return 0;
}

// ---- fused one-pass iteration (fh_fused.h) ---------------------------------------------------------------
// Shape of the one-pass launch: TEAM members x 256 lanes x PPT 16-byte pieces cover one row; lanes past the row's last
// piece are masked (clamped loads, zero x), so any n up to 262144 fits the next shape up.  A member's piece of a row is
// kept at 5..8 pieces per lane (20-32 KiB per workgroup per row) by choosing the team size -- fewer members means more
// teams, i.e. fewer rows (trips of ~0.7-1.2 us) per team:
//   n <= 4096  : 1 member  (a workgroup owns whole rows: no exchange), PPT = ceil(n/512) rounded up to 1, 2, 4, 5..8
//   n <= 8192  : 2 members x PPT = ceil(n/1024) in 5..8, posts one row ahead
//   n <= 16384 : 4 members x PPT = ceil(n/2048) in 5..8, posts one row ahead
//   n <= 32768 : 8 members x PPT = ceil(n/4096) in 5..8, posts one row ahead
//   n <= 65536 : 16 members x PPT = ceil(n/8192) in 5..8, posts two rows ahead
//   n <= 131072: 16 members x PPT = ceil(n/8192) in 9..16, x slice in LDS, posts one row ahead (3-4 row buffers)
//   n <= 262144: 32 members x PPT = ceil(n/16384) in 9..16, same schedule (6.1 TB/s at n = 262144: a trip with 32 members is
//                slower, but still 1.8x the two-launch path)
// FH_TUNE_FUSED_VARIANT bit 8 (A/B, tests): 8 members for every n <= 32768 and 8 members x 16 pieces in line at n = 65536;
// bit 16: n in (65536, 131072] as in round 1 (16 members x 16 pieces in registers, exchange in line).
// FusedShape = the template key of k_fused_dense (PPT, PIPE, TEAM, XLDS, NBO) for a row of n columns: a pure function of
// (n, row stride, storage, FH_TUNE_FUSED_VARIANT, #CUs), exported as fh_fused_shape so that it can be checked without a GPU.
struct FusedShape { int ppt, team, pipe, xlds, nbo; };
// The scheduling word a launch gets.  Rows are dealt cyclically (bit 32) where a team has at least 128 rows: below that the blocked dealing is as fast or
// 1-4 % faster (8192^2, teams of 2 with 64 rows each: 0.112 against 0.114 ms; 4096 x 8192: 0.0705 / 0.0735), from 256 rows per team on the cyclic one
// is 3-4 % faster on a well-placed matrix and up to 14 % on a badly placed one (profiles/r06_placement.txt) -- matrices of that size are small enough for
// their placement not to matter.  A word set through FH_TUNE_FUSED_VARIANT is passed on unchanged.
static int fused_variant_rule(int word, bool variant_auto, uint32_t rows_per_team) {
  int v = word;
  if (variant_auto && rows_per_team < 128u) v &= ~32;
  return v;
}

static FusedShape fused_shape_for(uint64_t n, uint64_t ld, int f32, int variant, int ncu) {
  const FusedShape none = {0, 0, 0, 0, 0};
  if (ld % 2 || n == 0) return none;
  // 16-byte pieces per row that hold data (the row stride ld may be padded): 2 columns each, 4 in float32 storage
  const uint64_t pieces = f32 ? round_up(n, 32) / 4 : round_up(n, 16) / 2;
  if (pieces > ld / (f32 ? 4 : 2)) return none;
  FusedShape sh = none;
  if (f32) {
    // float32 storage: the same byte rule (a member's piece of a row is 5..8 pieces per lane = 20-32 KiB per workgroup per
    // row), i.e. twice the columns per team size: n <= 8192 one member, then 2 / 4 / 8 / 16 members up to n = 131072.  A piece
    // carries four columns, so the x and g1 slices cost twice the registers per piece: from 5 pieces on the x slice lives in
    // LDS and 4 (5-6 pieces) or 3 (7-8 pieces) row buffers rotate, posting one row ahead -- the spill-free combinations
    // (-Rpass-analysis=kernel-resource-usage)
    for (int team = 1; team <= 16; team *= 2) {
      if (pieces > (uint64_t)team * FH_WG * 8) continue;
      int ppt = (int)((pieces + (uint64_t)team * FH_WG - 1) / ((uint64_t)team * FH_WG));
      if (ppt == 3) ppt = 4;
      if (team > 1 && ppt < 5) ppt = 5;          // (cannot happen: pieces > (team/2)*256*8 already means ppt >= 5)
      const int xl = ppt >= 5 ? 1 : 0;
      sh = {ppt, team, 1, xl, xl ? (ppt <= 6 ? 4 : 3) : 0};
      // A full 8-piece shape of 4 or 8 members (n in (28672, 32768] and (57344, 65536] = BASELINE config 2's
      // width) runs as TWICE the members x 4 pieces with TWO workgroups per CU (fh_fused.h:fused_wpc) and the x slice back in registers.
      // A float32 piece costs four conversions and eight float64 multiply-adds, twice the issue slots per byte of the float64 kernel, and
      // ONE wave per SIMD has nobody to hide its LDS, conversion and hand-off stalls behind; two have each other (x + g1 slices 64
      // registers, four 16-register row buffers: 219 of the 256 registers, no scratch in the loops).  profiles/r05_f32_shapes.txt:
      // 65536^2 2.577 -> 2.49-2.53 ms, 65536 x 32768 1.31-1.34 -> 1.26 ms.  (variant bit 8: the one-per-CU shapes, for A/B)
      // Teams of 1 and 2 (n <= 16384) stay one per CU: there the launch is short and the doubled grid barrier and hand-off cost more than
      // the second wave hides (8192^2: 91 -> 111 us, 16384^2: 212 -> 230 us; 32768^2 equal, 65536 x 32768 and 65536^2 3-5 % faster).
      if (ppt == 8 && team >= 4 && team <= 8 && !(variant & 8) && ncu % (2 * team) == 0) sh = {4, 2 * team, 1, 0, 4};
      break;
    }
  } else if (pieces <= (uint64_t)1 * FH_WG * 8 && !(variant & 8)) {
    int ppt = (int)((pieces + FH_WG - 1) / FH_WG);                       // n <= 4096: a workgroup owns whole rows, 256 "teams" of one
    if (ppt == 3) ppt = 4;
    sh = {ppt, 1, 1, 0, 0};
  } else if (pieces > (uint64_t)1 * FH_WG * 8 && pieces <= (uint64_t)2 * FH_WG * 8 && !(variant & 8)) {
    sh = {(int)((pieces + 2 * FH_WG - 1) / (2 * FH_WG)), 2, 1, 0, 0};  // n in (4096, 8192]: 2 members x 5..8 pieces, 128 teams
  } else if (pieces > (uint64_t)2 * FH_WG * 8 && pieces <= (uint64_t)4 * FH_WG * 8 && !(variant & 8)) {
    sh = {(int)((pieces + 4 * FH_WG - 1) / (4 * FH_WG)), 4, 1, 0, 0};  // n in (8192, 16384]: 4 members x 5..8 pieces, 64 teams
  } else if (pieces <= (uint64_t)8 * FH_WG * 8) {
    int ppt = (int)((pieces + 8 * FH_WG - 1) / (8 * FH_WG));
    if (ppt == 3) ppt = 4;
    sh = {ppt, 8, 1, 0, 0};
  } else if (pieces == (uint64_t)8 * FH_WG * 16 && (variant & 8)) {
    sh = {16, 8, 0, 0, 0};
  } else if (pieces <= (uint64_t)16 * FH_WG * 8) {
    sh = {(int)((pieces + 16 * FH_WG - 1) / (16 * FH_WG)), 16, 2, 0, 0};       // 16 members: posts run two rows ahead of the polls
  } else if (pieces <= (uint64_t)16 * FH_WG * 16) {
    // n in (65536, 131072]: 16 members x 9..16 pieces POSTING ONE ROW AHEAD, made possible by keeping the x slice in LDS (the
    // registers hold 3-4 row buffers -- the largest count hipcc allocates without spilling -- and the g1 slice); measured against
    // the round-1 in-line shape in profiles/r02_fused_wide.txt: 131072 columns 6.41 -> 4.80 ms (7.16 TB/s), 70000: 5.80 -> 2.87 ms
    // (variant bit 16: that round-1 shape -- 16 pieces, x slice in registers, 3 row buffers, exchange in line)
    const int ppt = (int)((pieces + 16 * FH_WG - 1) / (16 * FH_WG));
    sh = (variant & 16) ? FusedShape{16, 16, 0, 0, 0} : FusedShape{ppt, 16, 1, 1, ppt <= 10 ? 4 : 3};
  } else if (pieces <= (uint64_t)32 * FH_WG * 16) {
    // n in (131072, 262144]: 32 members (a whole XCD per team, 8 teams) x 9..16 pieces, same schedule
    const int ppt = (int)((pieces + 32 * FH_WG - 1) / (32 * FH_WG));
    sh = {ppt, 32, 1, 1, ppt <= 10 ? 4 : 3};
  }
  if (!sh.ppt || ncu < sh.team || ncu % sh.team) return none;     // one workgroup per CU, whole teams only
  return sh;
}
// workgroups per CU of a shape (fh_fused.h:fused_wpc): two for the float32-storage shape of 16 members x <= 4 pieces, else one
static int fused_wpc_of(const FusedShape& sh, int f32) { return (f32 && sh.team >= 8 && sh.ppt == 4 && !sh.xlds) ? 2 : 1; }
static const FusedEntry* fused_lookup(const FusedShape& sh, int f32) {
  for (const FusedEntry& e : kFusedTable)
    if (e.ppt == sh.ppt && e.pipe == sh.pipe && e.team == sh.team && e.xlds == sh.xlds && e.nbo == sh.nbo && e.f32 == f32) return &e;
  return nullptr;
}
// CUs (= workgroups) of the one-pass dense launch.  FH_TUNE_FUSED_CUS caps them, so that several one-pass grids can be co-resident
// on ONE device: two solves side by side, or -- in the tests -- the ranks of a row-sharded run that share a GPU (K ranks x ncu / K CUs).
static int fused_ncu(fh_ctx* c) { return c->fused_cus > 0 ? std::min(c->fused_cus, std::max(1, c->ncu)) : c->ncu; }
static FusedShape fused_shape(fh_ctx* c) {
  if (c->op != OP_DENSE || c->prox_kind == FH_PROX_TVBALL || c->LB) return FusedShape{0, 0, 0, 0, 0};      // (no one-pass kernel for the multi-column form)
  return fused_shape_for(c->n, c->ld, c->f32, c->fused_variant, fused_ncu(c));
}
static int fused_ppt(fh_ctx* c) { return fused_shape(c).ppt; }
// diagnostic / test entry: the shape chosen for n columns and whether its kernel is instantiated (no device needed)
extern "C" int fh_fused_shape(uint64_t n, int dtype, int variant, int ncu, int* shape5, int* instantiated) {
  if (!shape5 || !instantiated) return fail(FH_E_ARG, "null argument");
  const int f32 = dtype == FH_DTYPE_F32_STORAGE ? 1 : 0;
  const FusedShape sh = fused_shape_for(n, round_up(n, f32 ? 32 : 16), f32, variant, ncu);
  shape5[0] = sh.ppt; shape5[1] = sh.pipe; shape5[2] = sh.team; shape5[3] = sh.xlds; shape5[4] = sh.nbo;
  *instantiated = sh.ppt && fused_lookup(sh, f32) ? 1 : 0;
  return 0;
}
// the one-pass launch beats K-fwd + K-adj once its fixed cost is amortised: wide rows, or at least 8 Mi elements
// (profiles/r02_fused_crossover.txt; 32 Mi in round 1, when every launch still refilled its hand-off slots from the host)
static bool fused_pays_for(uint64_t m, uint64_t n) { return n >= 16384 || m * n >= ((uint64_t)1 << 23); }
static bool fused_pays(fh_ctx* c) { return fused_pays_for(c->m, c->n); }

// THE GEOMETRY of a one-pass launch, stated once: a pure function of the matrix (mp = round_up(m, 16) rows on the device, n columns, rows of ld
// elements, storage), the scheduling word (FH_TUNE_FUSED_VARIANT's low half; variant_auto: nobody set it, the host resolves the cyclic bit), the
// CUs the launch may take (fused_ncu) and the rows-per-team floor (0 = none).  launch_fused_dense takes every number from here;
// fh_fused_launch_shape / fh_fused_launch_shape_for export it so that a test can assert the path it meant to reach.  sh.ppt == 0: no kernel.
struct FusedLaunch {
  FusedShape sh;
  int f32, wpc;                      // storage; workgroups per CU
  uint32_t nteams, rows_per_team, grid;
  int variant;                       // the word the kernel receives (bit 32 resolved; without the fault-injection bit)
  uint32_t ld2, nv2;                 // 16-byte pieces of a row that hold data; double pairs per n-side vector
};
// few rows: fewer teams (at least `min_rows` rows each when possible, and a multiple of 8 teams so that the members of
// a team stay on one XCD): a smaller grid barrier and fewer g1 partials to sum in the epilogue
static uint32_t fused_teams_for(uint64_t mp, uint32_t nteams, int min_rows) {
  if (min_rows > 0) {
    const uint64_t want = std::max<uint64_t>(8, round_up((mp + min_rows - 1) / min_rows, 8));
    nteams = (uint32_t)std::min<uint64_t>(nteams, want);
  }
  return nteams;
}
static FusedLaunch fused_launch_for(uint64_t mp, uint64_t n, uint64_t ld, int f32, int word, bool variant_auto, int ncu, int min_rows) {
  FusedLaunch L;
  memset(&L, 0, sizeof(L));
  L.sh = fused_shape_for(n, ld, f32, word, ncu);
  if (!L.sh.ppt) return L;
  L.f32 = f32 ? 1 : 0;
  L.wpc = fused_wpc_of(L.sh, f32);
  L.ld2 = (uint32_t)(f32 ? round_up(n, 32) / 4 : round_up(n, 16) / 2);
  L.nv2 = L.ld2 * (f32 ? 2u : 1u);
  L.nteams = fused_teams_for(mp, (uint32_t)(ncu * L.wpc / L.sh.team), min_rows);
  L.rows_per_team = (uint32_t)((mp + L.nteams - 1) / L.nteams);
  L.grid = L.nteams * (uint32_t)L.sh.team;
  L.variant = fused_variant_rule(word, variant_auto, L.rows_per_team);
  return L;
}
static FusedLaunch fused_launch(fh_ctx* c) {
  if (!fused_shape(c).ppt) { FusedLaunch L; memset(&L, 0, sizeof(L)); return L; }
  return fused_launch_for(c->mp, c->n, c->ld, c->f32, c->fused_variant, c->fused_variant_auto, fused_ncu(c), c->fused_min_rows);
}
static void fused_launch_report(const FusedLaunch& L, uint32_t* out) {
  const uint32_t v[FH_FUSED_LAUNCH_SHAPE_LEN] = {(uint32_t)L.sh.ppt, (uint32_t)L.sh.pipe, (uint32_t)L.sh.team, (uint32_t)L.sh.xlds, (uint32_t)L.sh.nbo, (uint32_t)L.f32,
                                                 (uint32_t)L.wpc, L.nteams, L.rows_per_team, L.grid, (uint32_t)L.variant, L.ld2, L.nv2};
  memcpy(out, v, sizeof(v));
}
// read-only: the geometry the next fh_step / fh_step_accel of this context launches with (FH_E_STATE where the one-pass kernel has no shape)
extern "C" int fh_fused_launch_shape(fh_ctx* c, uint32_t* out) {
  if (!c || !out) return fail(FH_E_ARG, "fh_fused_launch_shape: null argument");
  if (!c->shards.empty()) return fail(FH_E_STATE, "fh_fused_launch_shape: a multi-device context launches per shard (ask fh_shard's contexts)");
  const FusedLaunch L = fused_launch(c);
  if (!L.sh.ppt || !fused_lookup(L.sh, L.f32)) return fail(FH_E_STATE, "fh_fused_launch_shape: no one-pass kernel for this operator / prox / shape (see fh_fused_supported)");
  fused_launch_report(L, out);
  return 0;
}
// ... and the same rule for an (m, n) dense matrix that no context holds: a pure host function, no device needed
extern "C" int fh_fused_launch_shape_for(uint64_t m, uint64_t n, int dtype, int variant_word, int variant_auto, int cus, int min_rows, uint32_t* out) {
  if (!out) return fail(FH_E_ARG, "fh_fused_launch_shape_for: null argument");
  if (m == 0 || n == 0 || m >= (1ull << 31) || n >= (1ull << 31)) return fail(FH_E_ARG, "fh_fused_launch_shape_for: matrix dimensions must be in [1, 2^31)");
  if (dtype != FH_DTYPE_F64 && dtype != FH_DTYPE_F32_STORAGE) return fail(FH_E_ARG, "fh_fused_launch_shape_for: dtype is FH_DTYPE_F64 or FH_DTYPE_F32_STORAGE");
  if (variant_word < 0 || variant_word > 0xFFFF) return fail(FH_E_ARG, "fh_fused_launch_shape_for: the scheduling word is the low half of FH_TUNE_FUSED_VARIANT");
  if (cus < 1 || cus > 65536) return fail(FH_E_ARG, "fh_fused_launch_shape_for: cus (the CUs the launch may take) must be in [1, 65536]");
  if (min_rows < 0 || min_rows >= 0xFFFF) return fail(FH_E_ARG, "fh_fused_launch_shape_for: min_rows must be in [0, 65535) (0 = no floor)");
  const int f32 = dtype == FH_DTYPE_F32_STORAGE ? 1 : 0;
  const FusedLaunch L = fused_launch_for(round_up(m, 16), n, round_up(n, f32 ? 32 : 16), f32, variant_word, variant_auto != 0, cus, min_rows);
  if (!L.sh.ppt || !fused_lookup(L.sh, L.f32))
    return fail(FH_E_STATE, "fh_fused_launch_shape_for: no one-pass kernel for rows of %llu columns on %d CUs (see fh_fused_shape)", (unsigned long long)n, cus);
  fused_launch_report(L, out);
  return 0;
}

// (the prox kind travels in p.px.kind: a run-time switch in the kernel's n-side prologue; FH_PROX_* == PX_* numerically.  The
// one-pass kernels always stream A with non-temporal loads, +10 % in the dense sweeps: only NT = 1 is built.)
// operands of one fused launch; fh_step takes them from the solver state, fh_init / fh_gradient_at pass their own
struct FusedIO {
  const double* x0; const double* g0; double* xhat; double* xp; double* z; double* g1;
  int kind;     // prox kind (FH_PROX_IDENTITY with tau = 0 gives the plain pair z = A x0, g1 = A^T grad f(z))
  int mode;     // 0 = with the n-side epilogue, 2 = g1 (+ loss) only
  // FISTA (zero-initialised = off): x1 = xp + c*(xp - xacc0), gradient at z + c*(z - zacc0), c = coef or 0 after a restart
  int accel = 0, restart = 0; double coef = 0.0;
  const double* xacc0 = nullptr; const double* zacc0 = nullptr; double* x1 = nullptr; double* coef_out = nullptr;
  double* pack = nullptr;      // row-sharded: where the launch appends its loss sums and timeout word (behind g1)
};

// after the synchronisation that follows a one-pass launch: a launch that timed out has left slots un-posted / un-armed
static inline void fused_after(fh_ctx* c) { if (c->hscal[15] != 0.0) c->slots_sig = 0; }

static const ChainEntry* chain_lookup(const FusedShape& sh, int f32) {
  for (const ChainEntry& e : kChainTable)
    if (e.ppt == sh.ppt && e.pipe == sh.pipe && e.team == sh.team && e.xlds == sh.xlds && e.nbo == sh.nbo && e.f32 == f32) return &e;
  return nullptr;
}
// chain != nullptr: the CHAINED form (k_fused_chain): tau and the solver-state pointers of `io` are placeholders, the launch takes them
// from chain->st; no per-launch event records (the caller brackets the whole chain) and no sequence number (nobody waits for a single launch)
static int launch_fused_dense(fh_ctx* c, double tau, const FusedIO& io, const ChainP* chain = nullptr) {
  const FusedLaunch L = fused_launch(c);            // (the geometry: fused_launch_for above, what fh_fused_launch_shape reports)
  const FusedShape sh = L.sh;
  if (!sh.ppt) return fail(FH_E_STATE, "fused one-pass step: unsupported operator shape (needs a dense A with n <= 262144 and a scalar-separable prox)");
  const FusedEntry* k_fused_dense_entry = fused_lookup(sh, c->f32);
  if (!k_fused_dense_entry)
    return fail(FH_E_STATE, "fused one-pass step: no instantiation for PPT %d, PIPE %d, TEAM %d, XLDS %d, NBO %d, F32 %d (fh_fused_instances.inc)",
                sh.ppt, sh.pipe, sh.team, sh.xlds, sh.nbo, c->f32);
  FusedP p;
  p.A = c->A; p.ld = c->ld; p.n = (uint32_t)c->n; p.m = (uint32_t)c->m; p.mp = (uint32_t)c->mp;
  p.ld2 = L.ld2;
  p.ldp = (uint32_t)(c->ld / (c->f32 ? 4 : 2));
  p.nv2 = L.nv2;
  p.nteams = L.nteams;
  p.rows_per_team = L.rows_per_team;
  p.x0 = io.x0; p.g0 = io.g0; p.xhat = io.xhat; p.xp = io.xp;
  p.b = c->b; p.z = io.z; p.tau = tau; p.loss = c->loss_kind; p.mode = io.mode;
  p.px = make_prox(c, tau);
  p.px.kind = io.kind;
  p.accel = io.accel; p.restart = io.restart; p.coef = io.coef; p.xacc0 = io.xacc0; p.zacc0 = io.zacc0; p.x1 = io.x1; p.coef_out = io.coef_out;
  p.pack = io.pack;
  const unsigned grid = L.grid;
  const size_t slots_elems = ((size_t)c->mp + p.nteams) * (sh.team < 8 ? 8 : sh.team);     // (32 members: four 64-byte lines per row)   // whole 64-byte lines; + one line per team for the restart dot
  const size_t gpart_elems = (size_t)p.nteams * p.nv2 * 2;
  FH_TRY(ensure_ws(c, (gpart_elems + (size_t)grid * 16) * sizeof(double)));
  p.gpart = c->ws; p.red = p.gpart + gpart_elems;
  if (2 * slots_elems * sizeof(double) > c->slotbuf_bytes) {
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->slotbuf) { HIP_TRY(hipFree(c->slotbuf)); c->slotbuf = nullptr; c->slotbuf_bytes = 0; }
    const size_t bytes = round_up(2 * slots_elems * sizeof(double), 1 << 20);
    HIP_TRY(hipMalloc((void**)&c->slotbuf, bytes));
    c->slotbuf_bytes = bytes;
    c->slots_sig = 0;
  }
  p.g1 = io.g1;
  p.bar = c->counters + CNT_FUSED_BAR; p.gbar = c->gridbar; p.err = c->counters + CNT_FUSED_ERR;
  p.variant = L.variant | ((c->test_hooks & FH_HOOK_WITHHOLD_PARTIAL) ? 64 : 0);      // (bit 64 of FusedP.variant: the kernel's fault-injection switch)
  p.out = scalar_out(c);
  const ChainEntry* chain_entry = chain ? chain_lookup(sh, c->f32) : nullptr;
  if (chain && !chain_entry) return fail(FH_E_STATE, "chained one-pass launch: no instantiation for this shape (teams of 1 / 2 / 4 members, float64)");
  if (!chain) t_begin(c, FH_K_FUSED);
  {
    // signature of everything the slot layout depends on; 0 = "refill" (set after a timed-out launch, see fused_after)
    uint64_t sig = fh_mix((uint64_t)(uintptr_t)c->slotbuf ^ fh_mix(slots_elems * 131 + (uint64_t)sh.team * 7 + p.nteams)) | 1ull;
    if (sig != c->slots_sig) {
      // (a team of one exchanges nothing through the slots, but its grid barrier and error word are the same counters: a launch
      // that timed out in another shape must not leave them armed for it)
      if (sh.team > 1) HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)c->slotbuf, (int)FT_SENTINEL_HI, 2 * slots_elems * 2, c->stream));
      HIP_TRY(hipMemsetAsync(c->counters + CNT_FUSED_BAR, 0, 8 * sizeof(unsigned), c->stream));
      HIP_TRY(hipMemsetAsync(c->gridbar, 0, 2 * GB_WORDS * sizeof(unsigned), c->stream));
      c->slots_sig = sig;
      c->slots_parity = 0;
    }
    p.slots = c->slotbuf + (size_t)c->slots_parity * slots_elems;
    p.slots_next = c->slotbuf + (size_t)(c->slots_parity ^ 1) * slots_elems;
    c->slots_parity ^= 1;
  }
  if (chain) {
    p.px.seq = 0u;
    chain_entry->kernel<<<dim3(grid), dim3(FH_WG), 0, c->stream>>>(p, *chain);
    HIP_TRY(hipGetLastError());
    return 0;
  }
  p.px.seq = io.mode == 0 ? seq_offer(c) : 0u;
  k_fused_dense_entry->kernel<<<dim3(grid), dim3(FH_WG), 0, c->stream>>>(p);
  t_end(c, FH_K_FUSED);
  HIP_TRY(hipGetLastError());
  return 0;
}

// z = A x, g = A^T grad f(z) from ONE read of A when the one-pass kernel pays off (single GPU, fused_pays()):
// identity prox and tau = 0 make xprox = x.  `xhat` and the prox target serve as the launch's scratch outputs.
// ---- co-residency probe ----------------------------------------------------------------------------------------------------
// The one-pass dense kernel needs ONE WORKGROUP ON EVERY compute unit it is launched on -- all the device reports, or the
// FH_TUNE_FUSED_CUS of them -- all at the same time (teams exchange partial sums while they run).  A CU mask, a partition mode or a co-tenant that hides CUs does not change the reported count, and
// the kernel would run into its bounded spins (0.4-0.5 s) before the solver drops it.  k_coresident finds out in ~20 us instead:
// it launches that many workgroups, each claiming more than half of a CU's LDS (so no two can share a CU), which count themselves
// in and wait -- at most 2 ms -- for the count to reach the grid size.  If some of them cannot start until others have ended, the
// count stalls: not co-resident, and fh_fused_supported reports 0 for the dense operator.  Run once per context, on first use.
#define FH_PROBE_LDS (96 * 1024)
__global__ __launch_bounds__(FH_WG, 1) void k_coresident(unsigned* counter, unsigned* failed) {
  __shared__ volatile unsigned claim[FH_PROBE_LDS / 4];
  if (threadIdx.x == 0) {
    claim[blockIdx.x % (FH_PROBE_LDS / 4)] = 1u;                               // volatile round trip: the allocation cannot be optimised away
    const unsigned one = claim[blockIdx.x % (FH_PROBE_LDS / 4)];
    __hip_atomic_fetch_add(counter, one, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();            // 100 MHz
    bool all = false;
    while (__builtin_amdgcn_s_memrealtime() - t0 < 200000ull) {                // 2 ms
      if (__hip_atomic_load(counter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= gridDim.x) { all = true; break; }
      __builtin_amdgcn_s_sleep(8);
    }
    if (!all) __hip_atomic_store(failed, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}
static bool run_coresident_probe(fh_ctx* c, unsigned grid) {                    // false on any failure
  unsigned* w = c->counters + CNT_PROBE;
  if (hipSetDevice(c->device) != hipSuccess) return false;
  if (hipMemsetAsync(w, 0, 2 * sizeof(unsigned), c->stream) != hipSuccess) return false;
  k_coresident<<<dim3(grid), dim3(FH_WG), 0, c->stream>>>(w, w + 1);
  unsigned host[2] = {0, 1};
  if (hipGetLastError() != hipSuccess) return false;
  if (hipMemcpyAsync(host, w, sizeof(host), hipMemcpyDeviceToHost, c->stream) != hipSuccess) return false;
  if (hipStreamSynchronize(c->stream) != hipSuccess) return false;
  (void)hipMemsetAsync(w, 0, 2 * sizeof(unsigned), c->stream);
  return host[1] == 0 && host[0] == grid;
}
static bool co_resident(fh_ctx* c) {
  if (c->test_hooks & FH_HOOK_PROBE_SAYS_NO) return false;      // test hook (FH_TUNE_TEST_HOOKS, csrc/fh_experimental.h): "this rank's probe said no"
  if (c->coresident >= 0) return c->coresident != 0;
  // (the probe decides, nothing else: no environment variable is consulted.  A second try: a transient co-tenant must not cost this
  // context the one-pass kernel.)
  const unsigned grid = (unsigned)std::max(1, fused_ncu(c));
  c->coresident = (run_coresident_probe(c, grid) || run_coresident_probe(c, grid)) ? 1 : 0;
  return c->coresident != 0;
}
// diagnostic: can `workgroups` whole-CU workgroups run side by side on this context's device?  (ncu: yes on a healthy device;
// ncu + 1: never -- which is how the tests see the probe say "no")
extern "C" int fh_coresident_probe(fh_ctx* c, int workgroups, int* ok) {
  if (!c || !ok || workgroups < 1 || workgroups > 65536) return fail(FH_E_ARG, "fh_coresident_probe: bad argument");
  if (!c->shards.empty()) c = c->shards[0];
  *ok = run_coresident_probe(c, (unsigned)workgroups) ? 1 : 0;
  return 0;
}
static bool plain_pair_fused_ok(fh_ctx* c) { return c->op == OP_DENSE && !row_sharded(c) && c->shards.empty() && fused_ppt(c) && fused_pays(c) && co_resident(c); }
// returns 0 and sets *ok = false when the launch reported a spin timeout (caller falls back to two launches)
static int plain_pair_fused(fh_ctx* c, const double* x, double* z, double* g, bool* ok) {
  const FusedIO fio = {x, x, c->xhat, c->P[c->pc ^ 1], z, g, FH_PROX_IDENTITY, 2};
  FH_TRY(launch_fused_dense(c, 0.0, fio));
  FH_TRY(finish(c));                          // single GPU: the scalar block (incl. the timeout word) is in mapped host memory
  *ok = c->hscal[15] == 0.0;
  fused_after(c);
  return 0;
}

// ---- operator-generic wrappers ---------------------------------------------------------------------
// the launchers of each operator form, by F_* (csrc/fh_host_ctx.h: kForms holds what the form serves)
struct FormLaunch { int (*fwd)(fh_ctx*, const FwdIO&); int (*adj)(fh_ctx*, const AdjIO&); };
static int no_operator_fwd(fh_ctx*, const FwdIO&) { return fail(FH_E_STATE, "no operator set"); }
static int no_operator_adj(fh_ctx*, const AdjIO&) { return fail(FH_E_STATE, "no operator set"); }
static const FormLaunch kLaunch[] = {
  {no_operator_fwd, no_operator_adj}, {launch_fwd_dense, launch_adj_dense}, {launch_fwd_multi, launch_adj_multi}, {launch_fwd_tv, launch_adj_tv},
  {launch_fwd_sparse, launch_adj_sparse}, {launch_fwd_spmulti, launch_adj_spmulti}, {launch_fwd_tv3, launch_adj_tv3}, {launch_fwd_quad, launch_adj_quad},
  {launch_fwd_bilinear, launch_adj_bilinear}, {launch_fwd_dct, launch_adj_dct}, {launch_fwd_identity, launch_adj_identity}, {launch_fwd_conv, launch_adj_conv},
};
static_assert(sizeof(kLaunch) / sizeof(kLaunch[0]) == F_COUNT, "one pair of launchers per operator form, in the order of F_*");
static int op_fwd(fh_ctx* c, const FwdIO& io) { return kLaunch[form_index(c)].fwd(c, io); }

// ---- the adjoint launch in three stages, so that a shell can run stage 1 on every shard, ONE exchange, stage 3 on every shard ----
// stage 1, local: row-sharded contexts leave the n-side epilogue (mode 0) to adj_tail, which needs the summed g1
static int adj_local(fh_ctx* c, const AdjIO& io_in) {
  AdjIO io = io_in;
  if (row_sharded(c) && c->op != OP_DENSE) return fail(FH_E_STATE, "row sharding is implemented for the dense operator only");
  if (row_sharded(c) && io.mode == 0) io.mode = 2;
  return kLaunch[form_index(c)].adj(c, io);
}
// stage 2, exchange: A_k^T r_k partials (nv doubles at g1(shard)) and the local loss sums (FH_S_FSQ_ADJ) summed over the row blocks
template <typename Sel>
static int adj_sum(fh_ctx* c, Sel g1) {
  return sum_over_shards(c, g1, (size_t)c->nv, [](fh_ctx* s) { return s->dscal + FH_S_FSQ_ADJ; }, 1);
}
// stage 3: the n-side epilogue on the summed g1
static int adj_tail(fh_ctx* c, const AdjIO& io) {
  if (!row_sharded(c) || io.mode != 0) return 0;
  return bb_epilogue_only(c, io, c->dscal + FH_S_FSQ_ADJ);
}
// all three on a plain context (fh_init, fh_gradient_at, fh_apply of a single context)
static int op_adj(fh_ctx* c, const AdjIO& io) {
  FH_TRY(adj_local(c, io));
  double* g1 = io.g1;
  FH_TRY(adj_sum(c, [g1](fh_ctx*) { return g1; }));
  return adj_tail(c, io);
}

// local ||r_k||^2 (or logistic loss sum) of the forward launch summed over the row blocks, before the host's line-search test
static int reduce_fsq_over_ranks(fh_ctx* c) {
  return sum_over_shards(c, [](fh_ctx* s) { return s->dscal + FH_S_FSQ; }, 1);
}

static int check_ready(fh_ctx* c, bool need_b) {
  if (!c) return fail(FH_E_ARG, "null context");
  if (c->pending_step) return fail(FH_E_STATE, "a step issued by fh_step_begin is still in flight on this context: call fh_step_end first");
  if (c->op == OP_NONE) return fail(FH_E_STATE, "no operator set (call fh_set_matrix / fh_set_matrix_csr / fh_generate_matrix / fh_set_stencil / fh_set_stencil3d / fh_set_dct / fh_set_dct2 / fh_set_conv2d / fh_set_identity / fh_set_quadratic / fh_set_factorization)");
  if (need_b && !c->has_b) return fail(FH_E_STATE, "no loss set (call fh_set_loss_lsq)");
  return c->shards.empty() ? use_device(c) : 0;      // (a shell selects the device shard by shard)
}

// the solver-state operands of K-adj / the n-side epilogue (fh_adj, fh_fwd_adj, fh_step on a row-sharded context)
static AdjIO solver_adj_io(fh_ctx* c, double tau, int accel, double coef) {
  AdjIO io;
  io.z = c->Z[c->zc ^ 1]; io.zacc0 = c->Z[c->zc]; io.sub_b = 1; io.accel = accel ? 1 : 0; io.coef = coef;
  io.mode = 0; io.tau = tau;
  io.x0 = c->X[c->xi]; io.xp = c->P[c->pc ^ 1]; io.xacc0 = c->P[c->pc]; io.xhat = c->xhat;
  io.x1 = c->X[c->ti]; io.g1 = c->G[c->gc ^ 1]; io.g0 = c->G[c->gc];
  return io;
}
static FwdIO solver_fwd_io(fh_ctx* c, double tau) {
  return FwdIO{0, tau, c->X[c->xi], c->G[c->gc], c->P[c->pc], c->xhat, c->P[c->pc ^ 1], c->Z[c->zc ^ 1], 1};
}
// K-fwd of the solver state (level search for the two sort-free prox kinds first)
static int solver_fwd_local(fh_ctx* c, double tau, const char* who) {
  FH_TRY(use_device(c));
  FH_TRY(not_lazy(c, who));
  FH_TRY(tv_refresh_zcur(c));
  c->tvz_pending = false;
  if (c->prox_kind == FH_PROX_LINF || c->prox_kind == FH_PROX_L1BALL) FH_TRY(launch_level_search(c, tau));
  return op_fwd(c, solver_fwd_io(c, tau));
}

// ---- stencil one-pass launchers ---------------------------------------------------------------------------------------------
#ifdef FH_EXPERIMENTAL      // the round-1 one-pass stencil kernels that stream z (FH_TUNE_TV_ZFREE = 0, csrc/fh_experimental.h)
static int launch_fused_tv(fh_ctx* c, double tau) {
  FH_TRY(check_prox_run(c));
  if (!c->zcur) return fail(FH_E_STATE, "fh_step on the stencil operator before fh_init");
  TvStepFwdP p;
  p.H = (uint32_t)c->H; p.W = (uint32_t)c->W;
  p.rows_wg = (uint32_t)(c->tv_rows > 0 ? c->tv_rows : 32);
  p.strip_groups = ((p.W + TVF_OWN - 1) / TVF_OWN + 3) / 4;
  p.x0 = c->X[c->xi]; p.xacc0 = nullptr; p.xp = c->P[c->pc ^ 1]; p.zc = c->zcur; p.b = c->b; p.zn = c->Z[c->zc ^ 1];
  p.tau = tau;
  const unsigned grid = p.strip_groups * ((p.H + p.rows_wg - 1) / p.rows_wg);
  FH_TRY(ensure_ws(c, (size_t)grid * 16 * sizeof(double)));
  p.red = c->ws; p.counter = c->counters + CNT_FWD; p.out = scalar_out(c);
  t_begin(c, FH_K_FUSED);
#define TV_FUSED(U, NT)                                                                                            \
  do {                                                                                                             \
    if (c->prox_kind == FH_PROX_TVBALL) k_fused_tv_step<0, U, NT><<<dim3(grid), dim3(FH_WG), 0, c->stream>>>(p);   \
    else k_fused_tv_step<1, U, NT><<<dim3(grid), dim3(FH_WG), 0, c->stream>>>(p);                                  \
  } while (0)
  if (c->tv_nt == 1) { if (c->tv_u == 2) TV_FUSED(2, 1); else if (c->tv_u == 4) TV_FUSED(4, 1); else TV_FUSED(8, 1); }
  else { if (c->tv_u == 2) TV_FUSED(2, 0); else if (c->tv_u == 4) TV_FUSED(4, 0); else TV_FUSED(8, 0); }
#undef TV_FUSED
  t_end(c, FH_K_FUSED);
  HIP_TRY(hipGetLastError());
  return 0;
}

static int launch_fused_tv_accel(fh_ctx* c, double tau, double coef, int restart) {
  FH_TRY(check_prox_run(c));
  TvAccelP p;
  p.H = (uint32_t)c->H; p.W = (uint32_t)c->W;
  p.rows_wg = (uint32_t)(c->tv_rows > 0 ? c->tv_rows : 32);
  p.strip_groups = ((p.W + TVF_OWN - 1) / TVF_OWN + 3) / 4;
  p.p1 = nq(c, c->lq1); p.p0 = nq(c, c->lq0); p.pn = nq(c, c->lqn);
  p.z1 = mq(c, c->lz1); p.z0 = mq(c, c->lz0); p.zn = mq(c, c->lzn);
  p.b = c->b; p.tau = tau; p.cprev = c->lc; p.coef = coef; p.restart = restart;
  const unsigned grid = p.strip_groups * ((p.H + p.rows_wg - 1) / p.rows_wg);
  FH_TRY(ensure_ws(c, (size_t)grid * 16 * sizeof(double)));
  p.red = c->ws; p.counter = c->counters + CNT_FWD; p.out = scalar_out(c);
  t_begin(c, FH_K_FUSED);
#define TV_ACCEL(U, NT)                                                                                             \
  do {                                                                                                              \
    if (c->prox_kind == FH_PROX_TVBALL) k_fused_tv_accel<0, U, NT><<<dim3(grid), dim3(FH_WG), 0, c->stream>>>(p);   \
    else k_fused_tv_accel<1, U, NT><<<dim3(grid), dim3(FH_WG), 0, c->stream>>>(p);                                  \
  } while (0)
  if (c->tv_nt == 1) { if (c->tv_u == 2) TV_ACCEL(2, 1); else if (c->tv_u == 4) TV_ACCEL(4, 1); else TV_ACCEL(8, 1); }
  else { if (c->tv_u == 2) TV_ACCEL(2, 0); else if (c->tv_u == 4) TV_ACCEL(4, 0); else TV_ACCEL(8, 0); }
#undef TV_ACCEL
  t_end(c, FH_K_FUSED);
  HIP_TRY(hipGetLastError());
  return 0;
}

#endif

// z-free one-pass stencil step (k_tv_onepass): accel = 0 -> x0 = X[xi]; accel = 1 -> the lazily-kept (P1, P0, c) state
static int launch_tv_onepass(fh_ctx* c, double tau, int accel, double coef, int restart) {
  FH_TRY(check_prox_run(c));
  TvZP p;
  p.H = (uint32_t)c->H; p.W = (uint32_t)c->W;
  p.strip_groups = ((p.W + TVZ_OWN - 1) / TVZ_OWN + 3) / 4;
  if (c->tv_rows > 0) p.rows_wg = (uint32_t)c->tv_rows;
  else {
    // auto: as many row chunks as make the grid just FILL the resident capacity (5 workgroups per CU at 88 registers), so that all
    // workgroups run side by side and finish together -- 2240 workgroups of 128 rows on 1280 slots ran 1.75 rounds, the last one
    // three-quarters empty (8192^2: 128 rows 0.607 ms, 228-235 rows 0.588; profiles/r02_tune_tv.txt, r03_tune_tv.txt).  At least
    // 32 rows per chunk (rows + 4 are read and computed), at most the image.
    // SMALL images (round 6; the reference's own example is 512 x 512, tv_denoising.py:113-125): a chunk's rows are walked two (four) at a
    // time, each trip a dependent ~1-us round trip to L2 -- with 32-row chunks a 512^2 sweep is 48 workgroups x 18 trips = 23 us for 10 MB.
    // 8-row chunks (192 workgroups x 6 trips) take 16.5 us, 4 and 16 rows 18.5; at 1024^2 the plain sweep gains the same way (36.0 -> 27.9 us),
    // the FISTA sweep (two streams, 4-row trips) does not (31.0 -> 35.2); from 2048^2 on 32 rows are best again (profiles/r06_tv_rows_small.txt).
    const uint64_t pixels = (uint64_t)p.H * p.W;
    const uint32_t min_rows = pixels <= (1u << 18) ? 8u : ((pixels <= (1u << 20) && !accel) ? 8u : 32u);
    const uint32_t slots = (uint32_t)std::max(1, c->ncu) * 5u;
    const uint32_t chunks = std::max(1u, slots / p.strip_groups);
    p.rows_wg = std::min(p.H, std::max(min_rows, (p.H + chunks - 1) / chunks));
  }
  // rows per trip / rotating trip buffers: 2 rows, load-then-consume for the plain sweep; 4 rows x 3 rotating buffers with FISTA
  // (two streams to read): profiles/r03_tune_tv.txt.  Every combination produces the same bits (tests/test_gpu_tv_paths.py).
  const int tvu = c->tv_u ? c->tv_u : (accel ? 4 : 2);
  if (accel) { p.p1 = nq(c, c->lq1); p.p0 = nq(c, c->lq0); p.pn = nq(c, c->lqn); p.cprev = c->lc; }
  else { p.p1 = c->X[c->xi]; p.p0 = c->X[c->xi]; p.pn = c->P[c->pc ^ 1]; p.cprev = 0.0; }
  p.b = c->b; p.tau = tau; p.coef = coef; p.restart = restart;
  p.xcd_order = c->tv_xcd != 2;                  // FH_TUNE_TV_XCD: 0 / 1 = on, 2 = off
  p.nchunks = p.strip_groups * ((p.H + p.rows_wg - 1) / p.rows_wg);
  // FH_TUNE_TV_SLOTS: persistent form -- at most that many workgroups per CU, each walking the chunk ids with the grid as its stride
  // (0 = one workgroup per chunk, the round-3 form)
  unsigned grid = p.nchunks;
#ifdef FH_EXPERIMENTAL
  if (c->tv_slots > 0) grid = std::min(grid, (unsigned)std::max(1, c->ncu) * (unsigned)c->tv_slots);
#endif
  FH_TRY(ensure_ws(c, (size_t)grid * 16 * sizeof(double)));
  p.red = c->ws; p.counter = c->counters + CNT_FWD; p.out = scalar_out(c);
  p.arrive = c->gridbar + 2 * GB_WORDS;
  t_begin(c, FH_K_FUSED);
  p.seq = seq_offer(c);
  // tunables -> template parameters.  Non-temporal LOADS lose 12 % here (the halo columns and rows are re-read by the neighbouring
  // waves and workgroups through L2), so this sweep only distinguishes non-temporal (default) and plain STORES (FH_TUNE_TV_NT = 3).
  const int nb = c->tv_pipe ? c->tv_pipe : (accel ? 3 : 1);
  const bool nts = c->tv_nt != 3;       // stores are non-temporal unless FH_TUNE_TV_NT = 3 asks for plain ones (+2-3 %: xprox is not re-read by this launch)
  const bool ident = c->prox_kind != FH_PROX_TVBALL;
  // FH_TUNE_TV_LDS_PAD: bytes of (unused) dynamic LDS per workgroup -- an occupancy limiter for experiments (fewer, fatter streams)
#define TVZ(ID, AC, U, NT, NB) k_tv_onepass<ID, AC, U, NT, NB><<<dim3(grid), dim3(FH_WG), (size_t)c->tv_lds_pad, c->stream>>>(p)
#define TVZ_NB(AC, U, NT) do { if (nb >= 2) TVZ(0, AC, U, NT, 3); else TVZ(0, AC, U, NT, 1); } while (0)
#define TVZ_U(AC, NT) do { if (tvu <= 2) TVZ_NB(AC, 2, NT); else if (tvu == 8) TVZ_NB(AC, 8, NT); else TVZ_NB(AC, 4, NT); } while (0)
#define TVZ_NT(AC) do { if (nts) TVZ_U(AC, 2); else TVZ_U(AC, 0); } while (0)
#ifdef FH_EXPERIMENTAL
  // FH_TUNE_TV_RING: LDS-DMA trip ring (2-row trips; the b pieces need 16-byte aligned rows, i.e. an even width)
  const int ring = (c->tv_ring >= 2 && p.W % 2 == 0 && !ident) ? c->tv_ring : 0;
#define TVZ_RING(AC, R) do { if (nts) k_tv_onepass<0, AC, 2, 2, 1, R><<<dim3(grid), dim3(FH_WG), (size_t)c->tv_lds_pad, c->stream>>>(p); \
                             else k_tv_onepass<0, AC, 2, 0, 1, R><<<dim3(grid), dim3(FH_WG), (size_t)c->tv_lds_pad, c->stream>>>(p); } while (0)
  if (ring) {
    if (accel) { if (ring == 2) TVZ_RING(1, 2); else TVZ_RING(1, 3); }
    else { if (ring == 2) TVZ_RING(0, 2); else TVZ_RING(0, 3); }
  } else
#undef TVZ_RING
#endif
  if (ident) {        // no prox (g = None): the round-2 burst form
    if (accel) { if (tvu == 2) TVZ(1, 1, 2, 0, 1); else if (tvu == 8) TVZ(1, 1, 8, 0, 1); else TVZ(1, 1, 4, 0, 1); }
    else { if (tvu == 2) TVZ(1, 0, 2, 0, 1); else if (tvu == 8) TVZ(1, 0, 8, 0, 1); else TVZ(1, 0, 4, 0, 1); }
  } else if (accel) TVZ_NT(1);
  else TVZ_NT(0);
#undef TVZ_NB
#undef TVZ_NT
#undef TVZ_U
#undef TVZ
  t_end(c, FH_K_FUSED);
  HIP_TRY(hipGetLastError());
  c->tvz_pending = true;
  return 0;
}


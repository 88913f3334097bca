"""Cases, claimed geometry and models for the tests of the ROW-BLOCK machinery: the three stages a multi-GPU run and
`ShardedDenseMatrixMap(A, devices=[0] * p)` on one GPU share -- the local launch in mode 2 (k_adj_dense, the one-pass kernel's finaliser with its
pack, the one-read set-up), the sum over the blocks (csrc/fh_host_ctx.h: k_sum_shards, in its three counts) and the n-side epilogue as a launch of
its own (csrc/fh_dense.h: k_bb_epilogue).  A plain helper module in the mould of tests/mc_paths.py: the CPU tier (tests/test_blocks_cpu.py) proves
every claim made here, the GPU tier (tests/test_gpu_blocks.py) runs the kernels.

No new arithmetic: the operands and models are those of tests/sparse_lanes.py (the two-launch step on tests/mc_paths.py's matrices), of
tests/fused_paths.py (the one-pass step in its four modes, the set-up) and of tests/level_cases.py (the two level kinds).  On these data every
partial sum is exact in any order, so the result of a shell of p blocks must EQUAL the model of the whole matrix however the rows are cut.

What is restated here, once each: the row split of csrc/fasta_hip.hip:shell_partition (split), the slab / chunk rule of
csrc/fh_host_launch.h:launch_adj_dense (adj_launch), the chunks of bb_epilogue_only (epilogue_chunks) and -- as a MODEL of the three stages, held
to the whole-matrix model by the CPU tier -- block_model, with the defects a shell could have (DEFECTS)."""
import collections
import functools

import numpy as np

from fasta_python_amd import hip
from tests import fused_paths as FP
from tests import level_cases as LC
from tests import mc_paths as MC
from tests import run_paths as RP
from tests import sparse_lanes as SL

FH_WG = 256                                   # csrc/fh_device.h
FH_MAX_SHARDS = 64                            # csrc/fh_host_ctx.h
ADJ_MAX_SLAB = MC.ADJ_MAX_SLAB                # csrc/fh_dense.h
round_up, cdiv = MC.round_up, FP.cdiv


# ---- the row split ------------------------------------------------------------------------------------------------------------------------------
def split(m, p):
    """[(row0, rows)] of the p blocks of m rows: contiguous, the first m mod p blocks hold ceil(m / p) rows, the others floor(m / p)."""
    out, r0 = [], 0
    for k in range(p):
        rows = m // p + (1 if k < m % p else 0)
        out.append((r0, rows))
        r0 += rows
    return out


def split_remainder_last(m, p):
    """the DEFECT: the remainder rows given to the last blocks instead of the first"""
    out, r0 = [], 0
    for k in range(p):
        rows = m // p + (1 if k >= p - m % p else 0)
        out.append((r0, rows))
        r0 += rows
    return out


def padding_rows(m, p):
    """rows every block carries behind its live ones: each block is padded to 16 rows on its own"""
    return [round_up(rows, 16) - rows for _, rows in split(m, p)]


# ---- the launch rules of the two-launch adjoint and of the separate epilogue, restated ---------------------------------------------------------------
AdjLaunch = collections.namedtuple("AdjLaunch", "CPT ncc slab_rows nslab last_slab_rows")


def row_length(n, storage, ld_pad=0):
    """ld: doubles (float32 storage: floats) per device row, = nv, the length of every n-side buffer"""
    return round_up(n, 32 if storage == "f32" else 16) + ld_pad


def adj_launch(rows, n, storage, cpt=0, slab=0, ld_pad=0):
    """launch_adj_dense on a block of `rows` rows: 16-byte pieces per row (four columns in float32 storage), the automatic CPT keyed on them, column
    chunks of 256 * CPT pieces, about 32 slabs (more where the chunks are few) of 32 .. 2048 rows unless FH_TUNE_ADJ_SLAB_ROWS says otherwise."""
    f32 = storage == "f32"
    mp = round_up(rows, 16)
    ld2 = row_length(n, storage, ld_pad) // (4 if f32 else 2)
    CPT = cpt or (1 if ld2 <= 512 else (2 if ld2 < 16384 else 4))
    ncc = cdiv(ld2, FH_WG * CPT)
    if not slab:
        target = max(32, cdiv(1024 if f32 else 128, ncc))
        slab = min(max(round_up(cdiv(mp, target), 8), 128 if ncc >= 8 else 32), ADJ_MAX_SLAB)
    nslab = cdiv(mp, slab)
    return AdjLaunch(CPT, ncc, slab, nslab, mp - (nslab - 1) * slab)


def epilogue_chunks(n, storage, ld_pad=0):
    """(workgroups of k_bb_epilogue, live lanes of the last): one lane per PAIR of an n-side vector, 256 pairs per workgroup"""
    nv2 = row_length(n, storage, ld_pad) // 2
    nchunks = cdiv(nv2, FH_WG)
    return nchunks, nv2 - (nchunks - 1) * FH_WG


# ---- B: the two-launch entry points on a shell ---------------------------------------------------------------------------------------------------
# name: grid | level | one_row_each | one_more | max_shards;  tuning: sorted (key, value) pairs (hashable);  kind: an exact prox kind or a level kind
Shell = collections.namedtuple("Shell", "name m n p storage tuning kind")
SHELL_M, SHELL_WIDTHS, SHELL_BLOCKS = MC.VECTOR_M, (MC.N_WIDE, MC.N_RAGGED_F32), (2, 3, 4, 7)
N_SMALL = 40


def shell_slab(m, p):
    """FH_TUNE_ADJ_SLAB_ROWS of a shell of p blocks of m rows: two full slabs and a last one of 16 rows in EVERY block (the CPU tier checks it)"""
    return (round_up(cdiv(m, p), 16) - 16) // 2


def adj_tunings():
    """the FH_TUNE_ADJ_CPT x FH_TUNE_NT_LOADS x FH_TUNE_ADJ_CYCLIC tunings of tests/mc_paths.py:vector_cases, without its slab"""
    return [{k: v for k, v in t.items() if k != hip.TUNE_ADJ_SLAB_ROWS} for t, _ in MC.vector_cases() if hip.TUNE_ADJ_CPT in t]


@functools.lru_cache(maxsize=None)
def shell_cases():
    out = []
    for s, storage in enumerate(("f64", "f32")):
        for i, t in enumerate(adj_tunings()):
            p = SHELL_BLOCKS[(i + s) % 4]
            n = SHELL_WIDTHS[(i // 4 + i + s) % 2]
            tuning = {**t, hip.TUNE_ADJ_SLAB_ROWS: shell_slab(SHELL_M, p)}
            out.append(Shell("grid", SHELL_M, n, p, storage, tuple(sorted(tuning.items())), SL.PROX_KINDS[(i + i // 4 + 2 * s) % 4]))
    base = {hip.TUNE_FWD_GRID_CAP: MC.VECTOR_CAP}
    for p, storage, kind in ((3, "f64", "linf"), (4, "f32", "l1ball")):
        out.append(Shell("level", SHELL_M, MC.N_WIDE, p, storage, tuple(sorted({**base, hip.TUNE_ADJ_SLAB_ROWS: shell_slab(SHELL_M, p)}.items())), kind))
    out += [Shell("one_row_each", 3, N_SMALL, 3, "f64", (), "shrink"), Shell("one_row_each", 7, N_SMALL, 7, "f32", (), "box"),
            Shell("one_more", 4, N_SMALL, 3, "f64", (), "nonneg"), Shell("one_more", 8, N_SMALL, 7, "f32", (), "none"),
            Shell("max_shards", FH_MAX_SHARDS + 3, N_SMALL, FH_MAX_SHARDS, "f64", (), "shrink")]
    return tuple(out)


def exact_shell_cases():
    return tuple(c for c in shell_cases() if c.kind in SL.PROX_KINDS)


def level_shell_cases():
    return tuple(c for c in shell_cases() if c.kind in LC.PROX_KINDS)


def shell_id(c):
    t = dict(c.tuning)
    tune = "-".join(f"{MC.TUNE_NAMES[k]}{t[k]}" for k in sorted(t) if k in MC.TUNE_NAMES)
    return f"{c.name}-{c.m}x{c.n}-p{c.p}-{c.storage}-{c.kind}" + (f"-{tune}" if tune else "")


@functools.lru_cache(maxsize=None)
def sequence_extras(m, n):
    """what the B sequence runs beside the step, on the step's (A, B): fh_apply both ways on integer operands and fh_gradient_at at V --
    A V, A^T W and A^T (A V - B), all exact (the CPU tier proves it)"""
    A, X0, B = MC.step_inputs(m, n, None)
    V, W = SL.apply_operands(A, None)
    out = dict(V=V, W=W, AV=A @ V, ATW=A.T @ W, GRAD=A.T @ (A @ V - B))
    for v in out.values():
        v.setflags(write=False)
    return out


# ---- C: the one-pass step on a shell --------------------------------------------------------------------------------------------------------------
# The split is the library's, so the cuts are chosen through the row count: 7 rows as 4 + 3 and 3 + 2 + 2, 4 rows as 2 + 2 and 2 + 1 + 1 (the only way
# to a single-row block, and to fewer rows than teams where 64 CUs hold two teams of 32 members).  A case is a case of tests/fused_paths.py --
# its width, storage, scheduling word, prox kind and density -- with that row count, 64 CUs and the mode this table assigns; operands, model and
# proof are fused_paths' own, applied to it.
STEP_BLOCKS = (2, 3)
STEP_CUS = 64


def _with_rows(base, form, mode, m):
    return base._replace(name=f"blocks-{form.replace(' ', '_')}", m=m, cus=STEP_CUS, mode=mode)


@functools.lru_cache(maxsize=None)
def step_shell_cases():
    """one case per loop form (fused_paths.FORMS), then the single-row case; the modes in rotation, so that each occurs twice"""
    out = []
    forms = list(FP.FORMS) + ["TEAM 1"]
    for i, form in enumerate(forms):
        mode = FP.MODES[i % 4]
        # every other form at a width whose last epilogue chunk is ragged (an odd n, or n % 4 != 0: the widths that meet the box), the others at a full width
        ragged_first = sorted(FP.exact_step_cases(), key=lambda b: (epilogue_chunks(b.n, b.storage)[1] == FH_WG) == (i % 2 == 1))
        for base in ragged_first:
            if not base.cus or base.cus > 64 or base.variant is None or FP.form_of(FP.expected_shape(base)) != form:
                continue
            if base.kind == "box" and base.n > 65536:         # (the box's 2^-6 costs 12 bits: its widest rows keep their headroom only with their own 40 rows)
                continue
            probe = _with_rows(base, form, mode, 7)
            sh = FP.expected_shape(probe)
            if FP.form_of(sh) != form:
                continue
            m = 4 if (sh.nteams <= 3 or i == len(forms) - 1) else 7
            out.append(_with_rows(base, form + (" single row" if i == len(forms) - 1 else ""), mode, m))
            break
    return tuple(out)


def block_case(case, rows):
    """the case a block of `rows` rows of `case` is to its own launch"""
    return case._replace(m=rows)


def block_shapes(case, p):
    """the hip.FusedLaunchShape / hip.SetupShape every block of a shell of p must be launched with (None: no kernel for that block), from the
    library's own rule in its pure form at the block's row count"""
    fn = hip.fused_launch_shape_for if case.what == "step" else hip.setup_shape_for
    out = []
    for _, rows in split(case.m, p):
        try:
            out.append(fn(rows, case.n, case.storage, FP.word_of(case), case.variant is None, FP.cus_of(case), FP.floor_of(case)))
        except hip.HipError:
            out.append(None)
    return out


# ---- D: fh_setup on a shell -----------------------------------------------------------------------------------------------------------------------
MIXED = FP.Case("mixed-blocks", "setup", 4095, 4096, "f64", 64, 0, 34, "plain", "shrink", "lsq", 4)     # 2048 rows pay for the one-read kernel (2^23 entries), 2047 do not


@functools.lru_cache(maxsize=None)
def setup_shell_cases():
    """(case, p, one_read): a 512-thread float64 case and a float32 case of fused_paths.setup_cases(), each as 2 and 3 blocks that all keep a
    one-read kernel; then MIXED, whose second block has none, so that all blocks take the three passes"""
    wide = [c for c in FP.setup_cases() if c.n >= 16384 and c.cus <= 64]
    f64 = next(c for c in wide if c.storage == "f64" and FP.expected_shape(c).threads == 512)
    f32 = next(c for c in wide if c.storage == "f32")
    return tuple((c, p, True) for c in (f64, f32) for p in (2, 3)) + ((MIXED, 2, False),)


# ---- F: the logistic loss on blocks ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def logistic_shell_cases():
    """(case, p, route): 11 rows as 6 + 5 through the two launches, 27 rows as 9 + 9 + 9 through the one-pass step: padding rows in every block"""
    plain = next(c for c in FP.logistic_cases() if c.mode == "plain" and c.storage == "f64" and c.cus <= 64)
    accel = next(c for c in FP.logistic_cases() if c.mode != "plain" and c.storage == "f64" and c.cus <= 64)
    return ((plain._replace(name="blocks-logistic-6-5", m=11), 2, "two-launch"), (accel._replace(name="blocks-logistic-9-9-9", m=27), 3, "one-pass"))


# ---- H: fh_iterate on a shell ---------------------------------------------------------------------------------------------------------------------
ITERATE_MODES = {"plain": dict(adaptive=0, accelerate=0), "adaptive": dict(adaptive=1, accelerate=0), "accelerated": dict(adaptive=0, accelerate=1)}
ITERATE_BLOCKS = 3


# ---- the three stages as a model ---------------------------------------------------------------------------------------------------------------------
DEFECTS = ("last block's g1 left out", "padding row of a middle block in f", "FSQ_ADJ from pack[0] under acceleration", "last ragged chunk skipped",
           "restart coefficient kept", "remainder rows to the last blocks")
Blocks = collections.namedtuple("Blocks", "sums vectors cuts pack")


def block_model(case, p, defect=None):
    """One one-pass step of a step case as a shell of p blocks runs it, in float64.  Stage 1, per block (the launch in mode 2): xhat, xprox, the
    restart dot and the coefficient from replicated data, z_k = A_k xprox, the PARTIAL g1_k = A_k^T r_k and pack = (f_k, timeout word, f_k at the
    extrapolated point) -- run_paths.attempt on the block's rows.  Stage 2: g1 and pack added in shard order (k_sum_shards: ((v0 + v1) + v2) ...).
    Stage 3 (k_bb_epilogue, in chunks of 256 pairs): x1 and the five n-side sums from the summed g1 under the coefficient stage 1 chose,
    FH_S_FSQ := pack[0], FH_S_FSQ_ADJ := pack[2] under acceleration and pack[0] without.  defect: one of DEFECTS."""
    assert defect is None or defect in DEFECTS
    st = FP.operands(case)
    accel = case.mode != "plain"
    b = st.labels if case.loss == "logistic" else st.b
    rule = (lambda rdot: FP.COEF) if defect == "restart coefficient kept" else FP.coef_rule(case)
    cuts = (split_remainder_last if defect == "remainder rows to the last blocks" else split)(case.m, p)
    parts = []
    for k, (r0, rows) in enumerate(cuts):
        rs = slice(r0, r0 + rows)
        sums, v = RP.attempt(st.A[rs], b[rs], st.x0, st.g0, st.xacc0, st.zacc0[rs], FP.TAU, rule, accel, case.kind, case.loss)
        pack = [sums[0], 0.0, sums[10] if accel else sums[0]]
        if defect == "padding row of a middle block in f" and k == p // 2:
            term = RP.loss_sum(np.zeros(1), np.zeros(1), case.loss)            # a padding row: z = 0, b = 0
            pack = [pack[0] + term, 0.0, pack[2] + term]
        parts.append((sums, v, pack))
    summed = parts[:-1] if defect == "last block's g1 left out" else parts
    g1 = summed[0][1]["g1"].copy()
    for _, v, _ in summed[1:]:
        g1 = g1 + v["g1"]
    pack = list(parts[0][2])
    for _, _, q in parts[1:]:
        pack = [a + c for a, c in zip(pack, q)]
    sums0, v0, _ = parts[0]
    xhat, xp, coef = v0["xhat"], v0["xprox"], (v0["coef"] if accel else 0.0)
    x1 = xp + coef * (xp - st.xacc0) if accel else xp.copy()
    dx, dg, dh1 = xp - st.x0, g1 + (xhat - st.x0) / FP.TAU, x1 - xhat
    live = case.n
    if defect == "last ragged chunk skipped":
        nchunks, last = epilogue_chunks(case.n, case.storage)
        if last < FH_WG:
            live = min(case.n, 2 * FH_WG * (nchunks - 1))
            x1 = np.concatenate([x1[:live], np.zeros(case.n - live)])       # never written
    e = slice(0, live)
    fsq_adj = pack[0] if (not accel or defect == "FSQ_ADJ from pack[0] under acceleration") else pack[2]
    sums = [pack[0]] + [float(s) for s in sums0[1:7]] + [float(sums0[7]) if accel else 0.0, np.sum(dx[e] * dg[e]), np.sum(dg[e] * dg[e]), fsq_adj,
                                                          np.sum(dh1[e] * dh1[e]), np.sum(np.abs(x1[e])), np.max(np.abs(x1[e]), initial=0.0)]
    z = np.concatenate([v["z"] for _, v, _ in parts])
    return Blocks([float(s) for s in sums], dict(xhat=xhat, xprox=xp, z=z, g1=g1, x1=x1, coef=coef), tuple(cuts), pack)


def compared(blocks):
    """the fields the GPU tier compares: the 14 scalars, the five vectors, and the cuts it holds fh_shard to"""
    return FP.compared(FP.Result(blocks.sums, blocks.vectors)) + [np.array(blocks.cuts)]


def sensitivity_cases():
    """(case, p) a defect may show on: every one-pass shell case, and the logistic one (a padding row's least-squares term is (0 - 0)^2)"""
    return [(c, p) for c in step_shell_cases() for p in STEP_BLOCKS] + [(c, p) for c, p, route in logistic_shell_cases() if route == "one-pass"]

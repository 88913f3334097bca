"""GPU tests of the ROW-BLOCK machinery, each against exact arithmetic: the three stages a multi-GPU run shares with
`ShardedDenseMatrixMap(A, devices=[0] * p)` on one GPU -- the local launch in mode 2 (k_adj_dense's partial g1 and local loss sum; the one-pass
kernel's finaliser with pack[0..2]; the one-read set-up per block), the sum over the blocks (csrc/fh_host_ctx.h: k_sum_shards with its three
counts, the single-scalar sum of the forward launch) and the n-side epilogue as its own launch (csrc/fh_dense.h: k_bb_epilogue: several chunks and
a ragged last one, x1 under acceleration, the coefficient the one-pass kernel chose on the device, FH_S_FSQ and the timeout word from behind g1).

tests/block_cases.py holds the cases; tests/test_blocks_cpu.py proves, without a device, that every block has the geometry its case claims and
that on these operands every partial sum is exact in any order.  A shell of p blocks must therefore EQUAL the model of the WHOLE matrix -- every
vector and every scalar, == / np.array_equal -- however the rows are cut.  After every call each shard's n-side vectors and 16-scalar block are
bit-identical to shard 0's, the shards' z and b blocks tile the shell's, and fh_shard reports the restated split (check_shards).

Only the logistic loss is not exact: np.longdouble at the tolerances of tests/test_gpu_fused_paths.py::test_a_logistic_launch_against_longdouble."""
import numpy as np
import pytest

import fasta_python_amd as fa
from fasta_python_amd import hip, proximal
from tests import block_cases as BC
from tests import fused_paths as FP
from tests import level_cases as LC
from tests import mc_paths as MC
from tests import run_paths as RP
from tests import sparse_lanes as SL
from tests.test_gpu_mc_paths import first_bad

pytestmark = pytest.mark.gpu
LEVEL_PROX = {"linf": hip.PROX_LINF, "l1ball": hip.PROX_L1BALL}
N_SIDE = (hip.VEC_X0, hip.VEC_G0, hip.VEC_XHAT, hip.VEC_XPROX, hip.VEC_X1, hip.VEC_G1)
STEP_VECTORS = {"xhat": hip.VEC_XHAT, "xprox": hip.VEC_XPROX, "x1": hip.VEC_X1, "g1": hip.VEC_G1, "z": hip.VEC_Z}


@pytest.fixture(autouse=True)
def no_scratch_contexts_left_behind():
    yield
    proximal.release_scratch()


# ---- E: what every call must leave --------------------------------------------------------------------------------------------------------------
def check_shards(c, m, n, where=""):
    """every shard's n-side vectors and scalar block bit-identical to shard 0's; the z and b blocks tile the shell's; fh_shard == the split rule"""
    p = c.shard_count()
    views = [c.shard(k) for k in range(p)]
    if c.devices is not None:
        assert [(r0, rows) for _, r0, rows in views] == BC.split(m, p), where
    first = views[0][0]
    scal = first.last_scalars().tobytes()
    mine = [first.get_vector(vec, n).tobytes() for vec in N_SIDE]
    for k, (view, _, _) in enumerate(views[1:], 1):
        assert view.last_scalars().tobytes() == scal, (where, "scalar block of shard", k, view.last_scalars(), first.last_scalars())
        for vec, want in zip(N_SIDE, mine):
            assert view.get_vector(vec, n).tobytes() == want, (where, "vector", vec, "of shard", k)
    if c.devices is not None:
        for which in (hip.VEC_Z, hip.VEC_B):
            whole = c.get_vector(which, m)
            for view, r0, rows in views:
                assert np.array_equal(view.get_vector(which, rows), whole[r0:r0 + rows]), (where, which, r0)


def assert_matrix_rows_cross_the_boundaries(c, A):
    cuts = BC.split(A.shape[0], c.shard_count())
    for r0, rows in cuts[1:]:
        lo, hi = max(r0 - 1, 0), min(r0 + 2, A.shape[0])
        assert np.array_equal(c.get_matrix_rows(lo, hi - lo), A[lo:hi]), r0
    assert np.array_equal(c.get_matrix_rows(0, A.shape[0]), A)


# ---- the two-launch sequence ----------------------------------------------------------------------------------------------------------------------
def two_launch_sequence(c, A, X0, B, tag, extras, after):
    """fh_init -> fh_fwd -> fh_adj -> fh_fwd_adj -> fh_adj(accel) -> fh_commit, then fh_gradient_at and fh_apply both ways; `after(name)` runs behind
    every call.  Keyed as tests/sparse_lanes.py:exact_step keys its model."""
    m, n = A.shape
    vec = lambda which: c.get_vector(which, m if which == hip.VEC_Z else n)
    got = {}
    c.set_loss_lsq(B)
    c.set_prox(tag.kind, tag.mu, tag.lo, tag.hi)
    c.set_vector(hip.VEC_X0, X0)
    got["init"] = c.init(); after("fh_init")
    got["G0"] = vec(hip.VEC_G0)
    got["fwd"] = c.fwd(SL.TAU); after("fh_fwd")
    got["XHAT"], got["XPROX"], got["Z"] = vec(hip.VEC_XHAT), vec(hip.VEC_XPROX), vec(hip.VEC_Z)
    got["adj"] = c.adj(SL.TAU); after("fh_adj")
    got["G1"] = vec(hip.VEC_G1)
    got["pair"] = c.fwd_adj(SL.TAU); after("fh_fwd_adj")
    got["G1_pair"], got["Z_pair"] = vec(hip.VEC_G1), vec(hip.VEC_Z)
    got["adja"] = c.adj(SL.TAU, accel=True, coef=SL.COEF); after("fh_adj(accel)")
    got["G1A"], got["X1"] = vec(hip.VEC_G1), vec(hip.VEC_X1)
    c.commit(); after("fh_commit")
    got["X0_committed"], got["G0_committed"] = vec(hip.VEC_X0), vec(hip.VEC_G0)
    c.set_vector(hip.VEC_T0, extras["V"])
    c.gradient_at(hip.VEC_T0, hip.VEC_T1); after("fh_gradient_at")
    got["GRAD"] = vec(hip.VEC_T1)
    got["AV"] = c.apply(extras["V"]); after("fh_apply")
    got["ATW"] = c.apply(extras["W"], adjoint=True); after("fh_apply(adjoint)")
    return got


def assert_two_launch_model(got, want, extras):
    for name in SL.MATRICES:
        msg = first_bad(name, got[name], want[name])
        assert msg is None, msg
    for block in SL.BLOCKS:
        for slot, v in want[block].items():
            assert got[block][slot] == v, f"{block} scalar {slot}: {got[block][slot]!r} != {v!r}"
    assert np.array_equal(got["adj"][:hip.S_DXDG], got["fwd"][:hip.S_DXDG])                      # the adjoint leaves the forward half alone
    assert np.array_equal(got["pair"][:hip.S_ALPHA], np.concatenate([got["fwd"][:hip.S_DXDG], got["adj"][hip.S_DXDG:hip.S_ALPHA]]))
    assert np.array_equal(got["G1_pair"], want["G1"]) and np.array_equal(got["Z_pair"], want["Z"])
    assert np.array_equal(got["X0_committed"], want["X1"]) and np.array_equal(got["G0_committed"], want["G1A"])
    for name in ("GRAD", "AV", "ATW"):
        msg = first_bad(name, got[name], extras[name])
        assert msg is None, msg
    for block in ("init", "fwd", "adj", "pair", "adja"):
        assert got[block][15] == 0.0, block


def run_two_launch(op, m, n, kind, shards=True):
    A, X0, B = MC.step_inputs(m, n, None)
    c = op.ctx
    after = (lambda where: check_shards(c, m, n, where)) if shards else (lambda where: None)
    got = two_launch_sequence(c, A, X0, B, SL.prox_tag(kind), BC.sequence_extras(m, n), after)
    assert_two_launch_model(got, MC.step_model(m, n, None, kind), BC.sequence_extras(m, n))


# ---- A: the two-launch kernels in float32 storage, plain context -------------------------------------------------------------------------------------
@pytest.mark.parametrize("tuning,kind,n", MC.vector_cases("f32"), ids=MC.vector_id)
def test_one_vector_step_in_float32_storage_is_exact_over_the_tuning_grid(tuning, kind, n):
    """k_fwd_dense<4|8, 1, KIND, 1> (FH_TUNE_FWD_ROWS = 16 must launch the 8-row form: only then is every row of Z written) and k_adj_dense<1|2|4, 1, 1>,
    contiguous and cyclic slabs: four columns per 16-byte piece, two xprox pairs per piece, rows padded to 32 columns; the plain kind through fh_apply."""
    op = fa.DenseMatrixMap(MC.matrix(MC.VECTOR_M, n), tuning=tuning, storage="f32")
    try:
        assert op.ctx.rhs == 0 and op.ctx.storage == "f32"
        run_two_launch(op, MC.VECTOR_M, n, kind, shards=False)
        assert np.array_equal(op.ctx.get_matrix_rows(MC.VECTOR_M - 3, 3), MC.matrix(MC.VECTOR_M, n)[-3:])
    finally:
        op.close()


def level_step(c, p, prox, after):
    """fh_init -> fh_fwd -> fh_adj on tests/level_cases.py's step problem: the level, the vectors and every sum of the step against its model"""
    m, n = p.A.shape
    mdl = LC.step_model(p, prox)
    c.set_loss_lsq(p.b)
    c.set_prox(LEVEL_PROX[prox], p.radius / p.tau if prox == "linf" else p.radius)
    c.set_vector(hip.VEC_X0, p.x0)
    c.init(); after("fh_init")
    assert np.array_equal(c.get_vector(hip.VEC_G0, n), p.g0)
    s = c.fwd(p.tau); after("fh_fwd")
    a = c.adj(p.tau); after("fh_adj")
    assert s[hip.S_ALPHA] == a[hip.S_ALPHA] == mdl["level"] == 2.0
    for name, which in (("xhat", hip.VEC_XHAT), ("xprox", hip.VEC_XPROX), ("z", hip.VEC_Z), ("g1", hip.VEC_G1)):
        msg = first_bad(name, c.get_vector(which, m if name == "z" else n), mdl[name])
        assert msg is None, msg
    t = mdl["terms"]
    for block, k, name in ((s, hip.S_FSQ, "fsq"), (s, hip.S_DXG0, "dxg0"), (s, hip.S_DX2, "dx2"), (s, hip.S_XH2, "xh2"), (s, hip.S_G02, "g02"),
                           (s, hip.S_GSUM, "gsum"), (a, hip.S_DXDG, "dxdg"), (a, hip.S_DG2, "dg2"), (a, hip.S_FSQ_ADJ, "fsq"), (a, hip.S_FSQ, "fsq")):
        assert block[k] == np.sum(t[name]), (name, block[k], np.sum(t[name]))


@pytest.mark.parametrize("tuning,prox", MC.vector_level_cases(), ids=MC.vector_id)
def test_the_level_kinds_in_float32_storage_against_the_level_model(tuning, prox):
    """k_fwd_dense<4|8, 1, PX_LINF | PX_L1BALL, 1>"""
    p = LC.step_problem(MC.VECTOR_M, MC.N_WIDE)
    op = fa.DenseMatrixMap(p.A, tuning=tuning, storage="f32")
    try:
        level_step(op.ctx, p, prox, lambda where: None)
    finally:
        op.close()


# ---- B: the two-launch entry points on a shell ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", BC.exact_shell_cases(), ids=BC.shell_id)
def test_the_two_launch_sequence_on_a_shell_equals_the_model_of_the_whole_matrix(case):
    """k_adj_dense<CPT, NT, F32> in mode 2 on every block (at least two slabs and a ragged last one each), k_sum_shards over nv doubles plus one
    scalar, the single-scalar sum of the forward launch, k_bb_epilogue in three chunks with 8 live lanes in the last (float32 storage: 16), x1
    written under acceleration; the degenerate splits: one row per block behind fifteen padding rows, m = p + 1, 64 blocks."""
    A = MC.matrix(case.m, case.n)
    op = fa.ShardedDenseMatrixMap(A, devices=[0] * case.p, tuning=dict(case.tuning), storage=case.storage)
    try:
        assert op.ctx.shard_count() == case.p and op.row_blocks() == BC.split(case.m, case.p)
        run_two_launch(op, case.m, case.n, case.kind)
        assert_matrix_rows_cross_the_boundaries(op.ctx, A)
    finally:
        op.close()


@pytest.mark.parametrize("case", BC.level_shell_cases(), ids=BC.shell_id)
def test_the_level_kinds_on_a_shell(case):
    """every shard searches the level on its replicated xhat: equal on all of them (check_shards compares FH_S_ALPHA too) and the model's"""
    p = LC.step_problem(case.m, case.n)
    op = fa.ShardedDenseMatrixMap(p.A, devices=[0] * case.p, tuning=dict(case.tuning), storage=case.storage)
    try:
        level_step(op.ctx, p, case.kind, lambda where: check_shards(op.ctx, case.m, case.n, where))
    finally:
        op.close()


def test_fewer_rows_than_blocks_are_refused_by_code_and_sentence():
    with hip.HipContext(devices=[0, 0, 0]) as c:
        for setter in (lambda: c.set_matrix(np.ones((2, 8))), lambda: c.generate_matrix(2, 8, 0, 1, 1.0)):
            with pytest.raises(hip.HipError, match=rf"^\[{hip.E_ARG}\] a matrix of 2 rows cannot be split over 3 shards$"):
                setter()
        c.set_matrix(np.ones((3, 8)))                                       # ... and m = p is served
        assert [c.shard(k)[1:] for k in range(3)] == BC.split(3, 3)
    with hip.HipContext(devices=[0, 0, 0], storage="f32") as c:
        with pytest.raises(hip.HipError, match=rf"^\[{hip.E_ARG}\] a matrix of 2 rows cannot be split over 3 shards$"):
            c.set_matrix(np.ones((2, 8), dtype=np.float32))


# ---- C: the one-pass step on a shell ----------------------------------------------------------------------------------------------------------------
def shell_context(case, p, A, b_or_labels, devices=None, rccl_shell=False):
    c = hip.HipContext(0, storage=case.storage, devices=[0] * p if devices is None else devices, rccl_shell=rccl_shell)
    try:
        for key, value in FP.tuning_of(case).items():
            c.set_tuning(key, value)
        c.set_matrix(A)
        (c.set_loss_lsq if case.loss == "lsq" else c.set_loss_logistic)(b_or_labels)
        kind, mu, lo, hi = RP.PROX[case.kind]
        c.set_prox(kind, mu, lo, hi)
    except Exception:
        c.close()
        raise
    return c


def assert_block_geometry(c, case, p):
    """every shard view is about to launch what the library's pure rule gives at that block's row count: the path the case meant to reach"""
    device_cus, used = c.cu_count()
    assert device_cus >= 64 and used == case.cus, (device_cus, used)
    want = BC.block_shapes(case, p)
    query = (lambda v: v.fused_launch_shape()) if case.what == "step" else (lambda v: v.setup_shape())
    for k in range(p):
        view, r0, rows = c.shard(k)
        assert (r0, rows) == BC.split(case.m, p)[k] and view.shape() == (rows, case.n)
        if want[k] is None:
            with pytest.raises(hip.HipError, match=rf"^\[{hip.E_STATE}\]"):
                query(view)
        else:
            assert query(view) == want[k], (k, query(view), want[k])


def enter(c, case, st, after):
    """tests/test_gpu_fused_paths.py:enter on a shell: fh_init, and for an accelerated (or logistic) case one accelerated launch whose outputs are
    overwritten with the state the case enters with, then committed"""
    c.set_vector(hip.VEC_X0, st.x0)
    c.init(); after("fh_init")
    if case.mode == "plain" and case.loss == "lsq":
        assert np.array_equal(c.get_vector(hip.VEC_G0, case.n), st.g0)
        return
    c.step_accel(FP.TAU, 0.0, False); after("fh_step_accel(0)")
    for which, v in ((hip.VEC_XPROX, st.xacc0), (hip.VEC_Z, st.zacc0), (hip.VEC_X1, st.x0), (hip.VEC_G1, st.g0)):
        c.set_vector(which, v)
    c.commit(); after("fh_commit")
    assert np.array_equal(c.get_vector(hip.VEC_X0, case.n), st.x0) and np.array_equal(c.get_vector(hip.VEC_G0, case.n), st.g0)


def launch(c, case, after):
    if case.mode == "plain":
        scal = c.step(FP.TAU)
    else:
        scal = c.step_accel(FP.TAU, FP.COEF, case.mode in ("restart_hi", "restart_lo"))
    after(f"fh_step ({case.mode})")
    out = {"sums": scal[:14].copy(), "tail": scal[14:].copy()}
    for name, which in STEP_VECTORS.items():
        out[name] = c.get_vector(which, case.m if name == "z" else case.n)
    return out


def assert_step_model(got, case):
    mdl = FP.model(case)
    bad = [f"{name}: {g!r} != {w!r}" for name, g, w in zip(RP.SUMS, got["sums"], mdl.sums) if g != w]
    assert not bad, bad
    assert got["tail"][0] == 0.0 and got["tail"][1] == 0.0                      # no clipping level; scalars[15] == 0: no hand-off timeout on any block
    for name in STEP_VECTORS:
        msg = first_bad(name, got[name], mdl.vectors[name])
        assert msg is None, msg


STEP_SHELLS = [(c, p) for c in BC.step_shell_cases() for p in BC.STEP_BLOCKS]


@pytest.mark.parametrize("case,p", STEP_SHELLS, ids=[f"{FP.case_id(c)}-p{p}" for c, p in STEP_SHELLS])
def test_the_one_pass_step_on_a_shell_equals_the_model_of_the_whole_matrix(case, p):
    """fh_step / fh_step_accel: the finaliser in mode 2 writes the partial g1 and pack[0..2] on every block -- blocks with fewer rows than teams,
    a block of a single row --, k_sum_shards adds nv + 3 doubles, k_bb_epilogue takes the coefficient the kernel chose under the restart rule,
    FH_S_FSQ and the timeout word from behind g1 and FH_S_FSQ_ADJ from pack + 2 under acceleration; twice (the other slot parity)."""
    st = FP.operands(case)
    c = shell_context(case, p, st.A, st.b)
    try:
        assert_block_geometry(c, case, p)
        after = lambda where: check_shards(c, case.m, case.n, where)
        enter(c, case, st, after)
        assert_step_model(launch(c, case, after), case)
        assert_step_model(launch(c, case, after), case)
        assert_matrix_rows_cross_the_boundaries(c, st.A)
    finally:
        c.close()


# ---- D: fh_setup on a shell ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,p,one_read", BC.setup_shell_cases(), ids=[f"{FP.case_id(c)}-p{p}" for c, p, one_read in BC.setup_shell_cases()])
def test_the_set_up_on_a_shell_equals_the_model_of_the_whole_matrix(case, p, one_read):
    """setup_row_blocks: one one-read launch per block, nv + 2 and nv doubles in one exchange; where one block has no one-read kernel ALL blocks
    take the three passes (K-fwd + K-adj three times per block).  Either way g0, z, the difference of the probes' gradients and the scalars equal
    the model of the whole matrix."""
    o, mdl = FP.setup_operands(case), FP.setup_model(case)
    c = shell_context(case, p, o.A, o.b)
    try:
        assert_block_geometry(c, case, p)
        after = lambda where: check_shards(c, case.m, case.n, where)
        for rep in range(2):
            for which, v in ((hip.VEC_T0, o.t0), (hip.VEC_T1, o.t1), (hip.VEC_X0, o.x0), (hip.VEC_T2, np.ones(case.n)), (hip.VEC_G0, np.ones(case.n))):
                c.set_vector(which, v)
            c.timing_reset()
            c.timing_enable(True)
            s = c.setup(); after("fh_setup")
            c.timing_enable(False)
            launches = (c.timing_get(hip.K_FUSED)[1], c.timing_get(hip.K_FWD)[1], c.timing_get(hip.K_ADJ)[1])
            assert launches == ((p, 0, 0) if one_read else (0, 3 * p, 3 * p)), launches                # the route: as tests/test_gpu_setup.py tells them apart
            assert s[15] == 0.0
            for name, slot in (("FSQ", hip.S_FSQ), ("DX2", hip.S_DX2), ("DG2", hip.S_DG2), ("GSUM", hip.S_GSUM)):
                assert s[slot] == mdl[name], (rep, name, s[slot], mdl[name])
            assert s[hip.S_GMAX] == np.max(np.abs(o.x0))
            t2 = c.get_vector(hip.VEC_T2, case.n)
            if not one_read:                                                  # the three passes leave the two gradients: their difference is A^T A (T0 - T1)
                t2 = t2 - c.get_vector(hip.VEC_T3, case.n)
            for name, got in (("g0", c.get_vector(hip.VEC_G0, case.n)), ("t2", t2)):
                msg = first_bad(name, got, mdl[name])
                assert msg is None, (rep, msg)
            for k in range(p):
                view = c.shard(k)[0]
                assert np.array_equal(view.get_vector(hip.VEC_T2, case.n), c.get_vector(hip.VEC_T2, case.n)), k
        c.commit(); after("fh_commit")                                        # z1 := the z the set-up left (the next step's z_accel0)
        msg = first_bad("z", c.get_vector(hip.VEC_Z, case.m), mdl["z"])
        assert msg is None, msg
    finally:
        c.close()


# ---- F: the logistic loss on blocks (not exact) -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,p,route", BC.logistic_shell_cases(), ids=[f"{FP.case_id(c)}-p{p}-{route}" for c, p, route in BC.logistic_shell_cases()])
def test_the_logistic_loss_on_blocks_against_longdouble(case, p, route):
    """Blocks of 5, 6 and 9 rows: padding rows in every block, none of which may carry a loss term (log 2 each).  Z, XHAT, XPROX and X1 stay exact;
    the tolerances are those of tests/test_gpu_fused_paths.py::test_a_logistic_launch_against_longdouble."""
    st = FP.operands(case)
    mag = {}
    sums, want = FP._attempt(case, st, dtype=np.longdouble, magnitudes=mag)
    c = shell_context(case, p, st.A, st.labels)
    try:
        assert_block_geometry(c, case, p)
        after = lambda where: check_shards(c, case.m, case.n, where)
        enter(c, case, st, after)
        if route == "one-pass":
            got = launch(c, case, after)
            compared = range(len(RP.SUMS))
        else:
            assert case.mode == "plain"
            s = c.fwd(FP.TAU); after("fh_fwd")
            a = c.adj(FP.TAU); after("fh_adj")
            assert np.array_equal(a[:hip.S_DXDG], s[:hip.S_DXDG])
            got = {"sums": a[:14].copy(), "tail": a[14:].copy()}
            for name, which in STEP_VECTORS.items():
                got[name] = c.get_vector(which, case.m if name == "z" else case.n)
            compared = [k for k, name in enumerate(RP.SUMS) if name != "RDOT"]       # (the two launches form the restart dot, the plain one-pass launch leaves it zero)
    finally:
        c.close()
    for name in ("xhat", "xprox", "z", "x1"):
        msg = first_bad(name, got[name], np.asarray(want[name], dtype=np.float64))
        assert msg is None, msg
    assert got["tail"][1] == 0.0
    eps = 64 * 2.0 ** -52
    g1 = np.asarray(want["g1"], dtype=np.float64)
    dev = np.max(np.abs(got["g1"] - g1) / (1e-11 * np.abs(g1) + eps * np.asarray(mag["G1"], dtype=np.float64) + 1e-13))
    assert dev <= 1.0, ("g1", dev)
    slack = {"DXG0": eps * float(mag["DXG0"]), "DXDG": eps * float(mag["DXDG"])}
    f_wrong = FP.padding_rows_in_f(case)[1]
    for k in compared:
        name, w = RP.SUMS[k], float(sums[k])
        rtol = 1e-10 if name in ("DXDG", "DG2") else 1e-11
        print(f"\n{name}: got {got['sums'][k]!r} model {w!r}", end="")
        assert abs(got["sums"][k] - w) <= rtol * abs(w) + slack.get(name, 0.0), (name, got["sums"][k], w)
    assert abs(got["sums"][0] - f_wrong) > 1e-11 * abs(f_wrong)                  # (a single padding row's log 2 is far outside the tolerance)


# ---- G: the other two exchange forms ------------------------------------------------------------------------------------------------------------------
G_SHELL = next(c for c in BC.exact_shell_cases() if c.name == "grid" and c.storage == "f64" and dict(c.tuning)[hip.TUNE_ADJ_CPT] == 2)
G_STEP = next(c for c in BC.step_shell_cases() if c.mode == "restart_hi")


def exchange_form(form, storage, tunings, A):
    """a plain context with a one-rank communicator (the ncclAllReduce of a multi-process run), or the RCCL branch of the in-process form over one
    device: reached as tests/test_gpu_dense.py and tests/test_gpu_inproc_sharding.py reach them"""
    if form == "one-rank communicator":
        c = hip.HipContext(0, storage=storage)
    else:
        c = hip.HipContext(0, storage=storage, devices=[0], rccl_shell=True)
    try:
        for key, value in tunings.items():
            c.set_tuning(key, value)
        c.set_matrix(A)
        if form == "one-rank communicator":
            c.comm_init(1, 0, hip.comm_unique_id())
        assert c.comm_count() == 1 and c.shard_count() == 1
    except Exception:
        c.close()
        raise
    return c


@pytest.fixture(scope="module")
def rccl_started():
    """The first communicator of a process loads RCCL and starts it up (seconds, whichever test comes first): paid here once, not by a case."""
    with hip.HipContext(0) as c:
        c.set_matrix(np.eye(16))
        c.comm_init(1, 0, hip.comm_unique_id())
        assert c.comm_count() == 1


@pytest.mark.parametrize("form", ["one-rank communicator", "rccl shell"])
def test_the_two_launch_sequence_through_the_other_exchange_forms(form, rccl_started):
    case = G_SHELL
    A, X0, B = MC.step_inputs(case.m, case.n, None)
    c = exchange_form(form, case.storage, dict(case.tuning), A)
    try:
        after = lambda where: check_shards(c, case.m, case.n, where)
        got = two_launch_sequence(c, A, X0, B, SL.prox_tag(case.kind), BC.sequence_extras(case.m, case.n), after)
        assert_two_launch_model(got, MC.step_model(case.m, case.n, None, case.kind), BC.sequence_extras(case.m, case.n))
    finally:
        c.close()


@pytest.mark.parametrize("form", ["one-rank communicator", "rccl shell"])
def test_the_one_pass_step_through_the_other_exchange_forms(form, rccl_started):
    case = G_STEP
    st = FP.operands(case)
    c = exchange_form(form, case.storage, FP.tuning_of(case), st.A)
    try:
        c.set_loss_lsq(st.b)
        kind, mu, lo, hi = RP.PROX[case.kind]
        c.set_prox(kind, mu, lo, hi)
        assert c.shard(0)[0].fused_launch_shape() == FP.expected_shape(case, c.cu_count()[0])
        after = lambda where: check_shards(c, case.m, case.n, where)
        enter(c, case, st, after)
        assert_step_model(launch(c, case, after), case)
        assert_step_model(launch(c, case, after), case)
    finally:
        c.close()


# ---- H: fh_iterate with max_steps = 1 on a shell -------------------------------------------------------------------------------------------------------
def one_iteration(c, m, n, mode, launch_mode):
    A, X0, B = MC.step_inputs(m, n, None)
    c.set_loss_lsq(B)
    c.set_prox(hip.PROX_SHRINK, 1.0)
    c.set_vector(hip.VEC_X0, X0)
    s = c.init()
    o = hip.RunOpts()
    o.backtrack, o.stop_rule, o.window, o.max_backtracks, o.stepsize_shrink, o.tolerance = 1, 3, 10, 20, 0.5, 0.0
    o.evaluate_objective, o.restart = 1, 1
    o.adaptive, o.accelerate = BC.ITERATE_MODES[mode]["adaptive"], BC.ITERATE_MODES[mode]["accelerate"]
    o.launch_mode = launch_mode
    st = hip.RunState()
    st.tau_next, st.alpha1, st.max_residual, st.best_quality = SL.TAU, 1.0, -np.inf, np.inf
    st.f_window[0] = .5 * s[hip.S_FSQ]
    st.onepass_off_until, st.onepass_backoff = -1, 64
    hist = c.iterate(1, o, st)
    state = (st.tau_next, st.alpha1, st.max_residual, st.best_quality, st.iteration, st.backtracks, st.stopped, st.f_window[0], st.f_window[1])
    vectors = {which: c.get_vector(which, m if which == hip.VEC_Z else n) for which in N_SIDE + (hip.VEC_Z, hip.VEC_BEST)}
    return hist, state, vectors


@pytest.mark.parametrize("launch_mode", [hip.LAUNCH_SEPARATE, hip.LAUNCH_ONEPASS_ALWAYS], ids=["two-launch", "one-pass"])
@pytest.mark.parametrize("mode", sorted(BC.ITERATE_MODES))
def test_one_iteration_of_the_library_loop_on_a_shell_is_the_plain_contexts(mode, launch_mode):
    """fh_iterate(max_steps = 1) on three blocks against the same call on a plain context: the one record, the state and every vector bit for bit
    (the data are exact and the step shrink a power of two, so a backtracked attempt is exact too)."""
    m, n = BC.SHELL_M, MC.N_WIDE
    A = MC.matrix(m, n)
    runs = []
    for devices in (None, [0] * BC.ITERATE_BLOCKS):
        op = fa.DenseMatrixMap(A) if devices is None else fa.ShardedDenseMatrixMap(A, devices=devices)
        try:
            runs.append(one_iteration(op.ctx, m, n, mode, launch_mode))
            if devices is not None:
                check_shards(op.ctx, m, n, "fh_iterate")
        finally:
            op.close()
    (h0, s0, v0), (h1, s1, v1) = runs
    assert len(h0) == len(h1) == 1 and h0.tobytes() == h1.tobytes(), (h0, h1)
    assert s0 == s1, (s0, s1)
    for which in v0:
        assert np.array_equal(v0[which], v1[which]), which

"""GPU tests of EVERY loop of the multi-column dense kernels (csrc/fh_multi.h: k_mc_fwd / k_mc_adj<LB, .., NT>), each against exact arithmetic,
and of the tuning grid of the vector kernels (csrc/fh_dense.h) through the same harness.

Under the automatic launch rules the residual stage loop of k_mc_adj, a ragged last slab next to it and the grid-stride loop of k_mc_fwd need
m > 4096 .. 32768, and the non-temporal instantiations 256 MiB of matrix.  tests/mc_paths.py reaches each of them at about 2000 x 1000 with
FH_TUNE_ADJ_SLAB_ROWS, FH_TUNE_FWD_GRID_CAP and FH_TUNE_NT_LOADS, and every test here first asks the library what it is about to launch
(fh_multi_shape), so a change of the host's rule fails the test instead of emptying it.  The operands are such that every product and every
sum of a step is exactly representable in float64 whatever the order of summation (tests/test_mc_paths_cpu.py proves it on the inputs,
without a device), so the comparisons are np.array_equal: a stage that is not accumulated, a clamped lane that keeps its X or an epilogue
mask one column too wide cannot hide inside a tolerance.

Only the GroupShrink prox (a square root and a division per row) is not exact; it is compared against an np.longdouble model at the
tolerances this project already holds those quantities to (tests/sparse_lanes.py: GROUP_TOL, scalar_tol)."""
import numpy as np
import pytest

import fasta_python_amd as fa
from fasta_python_amd import hip, proximal
from tests import mc_paths as MC
from tests import sparse_lanes as SL
from tests.test_gpu_mmv import padding_is_zero
from tests.test_gpu_sparse_lanes import run_step

pytestmark = pytest.mark.gpu
CASES = MC.cases()


@pytest.fixture(autouse=True)
def no_scratch_contexts_left_behind():
    yield
    proximal.release_scratch()


def assert_shape(c, case, nt):
    """The library's own report of what it is about to launch == the geometry the case claims."""
    sh = c.multi_shape()
    print(f"\n{MC.case_id(case)} nt={nt}: {sh}", end="")
    assert sh == MC.expected_shape(case, nt), (sh, MC.expected_shape(case, nt))
    return sh


def first_bad(name, got, want):
    bad = np.argwhere(got != want)
    if bad.size:
        i = tuple(bad[0])
        return f"{name}: {len(bad)} wrong entries, first at {bad[0]}: {got[i]!r} != {want[i]!r}"
    return None


def test_the_window_is_refused_outside_the_multi_column_dense_form():
    S = SL.exact_matrix(8, 4)
    with hip.HipContext(0) as c:
        for prepare in (lambda: None, lambda: c.set_matrix(np.eye(4)), lambda: c.set_stencil(8, 8),
                        lambda: c.set_matrix_csr(S.indptr, S.indices, S.data, S.shape),
                        lambda: c.set_matrix_csr_rhs(S.indptr, S.indices, S.data, S.shape, 4)):
            prepare()
            with pytest.raises(hip.HipError, match=rf"^\[{hip.E_STATE}\]"):
                c.multi_shape()
        c.set_matrix(np.eye(40))
        c.set_rhs(3)
        assert c.multi_shape() == hip.multi_shape(40, 40, 3)               # the context form and the pure form: one rule
        c.set_rhs(0)
        with pytest.raises(hip.HipError, match=rf"^\[{hip.E_STATE}\]"):
            c.multi_shape()


# ---- apply ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=MC.case_id)
def test_apply_is_exact_on_every_path(case):
    """Both directions under both load policies on integer operands: k_mc_pack + k_mc_fwd (mode 1) and k_mc_adj's plain-gradient mode."""
    A = MC.matrix(case.m, case.n)
    V, W = SL.apply_operands(A, case.L)
    want_fwd, want_adj = A @ V, A.T @ W
    op = fa.DenseMatrixMap(A, rhs=case.L, tuning=MC.tuning_of(case, 0))
    try:
        c = op.ctx
        for nt in (0, 1):
            c.set_tuning(hip.TUNE_NT_LOADS, nt)
            assert_shape(c, case, nt)
            Z, Gt = op.device_apply(V), op.device_apply(W, adjoint=True)
            assert Z.shape == want_fwd.shape and Gt.shape == want_adj.shape
            for name, got, want in ((f"A V, nt={nt}", Z, want_fwd), (f"A^T W, nt={nt}", Gt, want_adj)):
                msg = first_bad(name, got, want)
                assert msg is None, msg
            assert padding_is_zero(c, hip.VEC_T3, case.n, case.L)
    finally:
        op.close()


# ---- one step ------------------------------------------------------------------------------------------------------------------------------
def assert_zero_padding(c, m, n, L):
    for which in (hip.VEC_G0, hip.VEC_XHAT, hip.VEC_XPROX, hip.VEC_X1, hip.VEC_G1):
        assert padding_is_zero(c, which, n, L), which
    assert padding_is_zero(c, hip.VEC_Z, m, L, m_side=True)


def assert_exact_step(c, A, L, X0, B, kind, want):
    """init -> fwd -> adj -> fwd_adj -> adj(accel, coef = 1/4): every matrix and every scalar the model keys, bit for bit."""
    got = run_step(c, A, L, X0, B, SL.prox_tag(kind), MC.TAU, MC.COEF)
    for name in SL.MATRICES:
        msg = first_bad(name, got[name], want[name])
        assert msg is None, msg
    for block in SL.BLOCKS:
        for slot, v in want[block].items():
            assert got[block][slot] == v, f"{block} scalar {slot}: {got[block][slot]!r} != {v!r}"
    # K-adj leaves the forward half of the block alone; fh_fwd_adj is both launches under one synchronisation
    assert np.array_equal(got["adj"][:hip.S_DXDG], got["fwd"][:hip.S_DXDG])
    assert np.array_equal(got["pair"][:hip.S_ALPHA], np.concatenate([got["fwd"][:hip.S_DXDG], got["adj"][hip.S_DXDG:hip.S_ALPHA]]))
    assert np.array_equal(got["G1_pair"], want["G1"]) and np.array_equal(got["Z_pair"], want["Z"])
    return got


@pytest.mark.parametrize("nt", [0, 1])
@pytest.mark.parametrize("case", CASES, ids=MC.case_id)
def test_one_step_is_exact_on_every_path(case, nt):
    A, X0, B = MC.step_inputs(case.m, case.n, case.L)
    want = MC.step_model(case.m, case.n, case.L, case.kind)
    op = fa.DenseMatrixMap(A, rhs=case.L, tuning=MC.tuning_of(case, nt))
    try:
        c = op.ctx
        assert_shape(c, case, nt)
        assert_exact_step(c, A, case.L, X0, B, case.kind, want)
        assert_zero_padding(c, case.m, case.n, case.L)
    finally:
        op.close()


# ---- GroupShrink ---------------------------------------------------------------------------------------------------------------------------
def group_step(case, nt):
    A, X0, B, tau, mu = SL.group_problem(MC.matrix(case.m, case.n), case.L)
    op = fa.DenseMatrixMap(A, rhs=case.L, tuning=MC.tuning_of(case, nt))
    try:
        c = op.ctx
        assert_shape(c, case, nt)
        got = run_step(c, A, case.L, X0, B, fa.GroupShrink(mu), tau, 0.37)
        assert_zero_padding(c, case.m, case.n, case.L)
        return got, (A, X0, B, tau, mu)
    finally:
        op.close()


@pytest.mark.parametrize("case,nt", MC.group_cases(), ids=lambda v: MC.case_id(v) if isinstance(v, MC.Case) else f"nt{v}")
def test_group_step_on_every_path(case, nt):
    got, (A, X0, B, tau, mu) = group_step(case, nt)
    want = SL.exact_step(A, X0, B, fa.GroupShrink(mu), tau=tau, coef=0.37, dtype=np.longdouble)
    for name, (rtol, atol) in SL.GROUP_TOL.items():
        np.testing.assert_allclose(got[name], want[name].astype(np.float64), rtol=rtol, atol=atol, err_msg=name)
    for block in SL.BLOCKS:
        for slot, v in want[block].items():
            rtol, atol = SL.scalar_tol(block, slot)
            np.testing.assert_allclose(got[block][slot], float(v), rtol=rtol, atol=atol, err_msg=f"{block} scalar {slot}")
    assert np.array_equal(got["pair"][:hip.S_ALPHA], np.concatenate([got["fwd"][:hip.S_DXDG], got["adj"][hip.S_DXDG:hip.S_ALPHA]]))


# ---- repeatability -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,nt", [(c, nt) for c, nt in MC.group_cases() if c.name in ("staged", "many stages")],
                         ids=lambda v: MC.case_id(v) if isinstance(v, MC.Case) else f"nt{v}")
def test_a_group_step_on_a_fresh_context_is_bit_identical(case, nt):
    """The staged geometry of every LB (and the sixteen stages), run twice, each on a context of its own: every matrix and the whole scalar
    block agree bit for bit (GroupShrink, so that roundings are there to differ)."""
    runs = [group_step(case, nt)[0] for _ in range(2)]
    assert set(runs[0]) == set(runs[1])
    for key in runs[0]:
        assert np.array_equal(runs[0][key], runs[1][key]), key


# ---- the vector kernels through the same harness ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tuning,kind", MC.vector_cases(), ids=MC.vector_id)
def test_one_vector_step_is_exact_over_the_tuning_grid(tuning, kind):
    """k_fwd_dense<R, NT, PROX> for R in {4, 8, 16} and k_adj_dense<CPT, NT> for CPT in {1, 2, 4}, contiguous and cyclic slabs, both load
    policies, under a forced slab with a ragged last slab and three K-fwd workgroups that make unequal numbers of passes."""
    m, n = MC.VECTOR_M, MC.VECTOR_N
    A, X0, B = MC.step_inputs(m, n, None)
    want = MC.step_model(m, n, None, kind)
    op = fa.DenseMatrixMap(A, tuning=tuning)
    try:
        assert op.ctx.rhs == 0
        assert_exact_step(op.ctx, A, None, X0, B, kind, want)
    finally:
        op.close()

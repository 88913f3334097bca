"""GPU tests of EVERY instantiation of the sparse gather kernels (csrc/fh_sparse.h: k_sp_fwd / k_sp_adj<G>; csrc/fh_spmulti.h: k_spmc_fwd /
k_spmc_adj<G, LB>), each against exact arithmetic.

The host picks the instantiation from the mean row length of each copy of the operator; tests/sparse_lanes.py builds a matrix for each one,
and every test here first asks the library what it chose (fh_sparse_lanes), so a change of the host's rule fails the test instead of
emptying it.  The operands are such that every product and every sum of a step is exactly representable in float64 whatever the order of
summation (tests/test_sparse_lanes_cpu.py proves it on the inputs, without a device), so the comparisons are np.array_equal: a wrong lane
permutation, a dropped column pair or a lane walk that stops one entry early cannot hide inside a tolerance.

Only the GroupShrink prox (a square root and a division per row) is not exact; it is compared against an np.longdouble model at the
tolerances of tests/test_gpu_sparse_mmv.py, and the sum of row norms that goes through the column-lane tree is pinned separately."""
import numpy as np
import pytest

import fasta_python_amd as fa
from fasta_python_amd import hip, proximal
from tests import sparse_lanes as SL
from tests.test_gpu_sparse_mmv import padding_is_zero

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def no_scratch_contexts_left_behind():
    yield
    proximal.release_scratch()


def open_map(S, L, nt=None):
    return fa.SparseMatrixMap(S, rhs=L, tuning=None if nt is None else {hip.TUNE_NT_LOADS: nt})


def assert_lanes(c, S, LB, G=None, nlong=(0, 0)):
    """The library's own report of what it chose == the intended instantiation (and the restated rule) on both copies."""
    for side, la in enumerate(SL.both_lanes(S, LB)):
        got_G, nwg, got_long = c.sparse_lanes(side)
        assert got_G == la.G and got_long == la.long_rows.size == nlong[side], (side, got_G, la, got_long)
        assert G is None or got_G == G, (side, got_G, G)
        M = S.tocsr() if side == 0 else S.T.tocsr()
        assert nwg == len(SL.row_ranges(M, SL.column_lanes(LB), ncu=c.cu_count()[0])) - 1


def test_the_window_is_refused_without_a_sparse_operator_and_for_a_third_side():
    S = SL.exact_matrix(8, 4)
    with hip.HipContext(0) as c:
        with pytest.raises(hip.HipError, match=rf"^\[{hip.E_STATE}\]"):
            c.sparse_lanes(0)
        c.set_matrix(np.eye(4))
        with pytest.raises(hip.HipError, match=rf"^\[{hip.E_STATE}\]"):
            c.sparse_lanes(1)
        c.set_matrix_csr_rhs(S.indptr, S.indices, S.data, S.shape, 4)
        with pytest.raises(hip.HipError, match=rf"^\[{hip.E_ARG}\]"):
            c.sparse_lanes(2)
        assert c.sparse_lanes(0)[0] == c.sparse_lanes(1)[0] == 8
        c.set_matrix_csr(S.indptr, S.indices, S.data, S.shape)          # the same matrix as a vector operator: 3 entries per row, G = 4
        assert c.sparse_lanes(0) == (4, 4, 0)


# ---- apply ---------------------------------------------------------------------------------------------------------------------------------
def check_apply(S, L, G=None, nlong=(0, 0)):
    V, W = SL.apply_operands(S, L)
    want_fwd, want_adj = S @ V, S.T @ W
    op = open_map(S, L)
    try:
        c = op.ctx
        assert_lanes(c, S, SL.lb_of(L), G, nlong)
        for nt in (0, 1):
            c.set_tuning(hip.TUNE_NT_LOADS, nt)
            Z, Gt = op.device_apply(V), op.device_apply(W, adjoint=True)
            assert Z.shape == want_fwd.shape and Gt.shape == want_adj.shape
            bad = np.argwhere(Z != want_fwd)
            assert bad.size == 0, f"A V, nt={nt}: {len(bad)} wrong entries, first at {bad[0]}: {Z[tuple(bad[0])]} != {want_fwd[tuple(bad[0])]}"
            bad = np.argwhere(Gt != want_adj)
            assert bad.size == 0, f"A^T W, nt={nt}: {len(bad)} wrong entries, first at {bad[0]}: {Gt[tuple(bad[0])]} != {want_adj[tuple(bad[0])]}"
    finally:
        op.close()


@pytest.mark.parametrize("G,LB,L", SL.apply_cases(), ids=lambda v: str(v))
def test_apply_is_exact_on_every_instantiation(G, LB, L):
    """Both directions, both load policies; L = LB and LB - 1 (a padding column absent or present); LB = 0 is the vector form."""
    check_apply(SL.exact_matrix(G, LB), L, G)


@pytest.mark.parametrize("LB", (0,) + SL.ALL_LB)
def test_apply_is_exact_on_a_whole_workgroup_row(LB):
    check_apply(SL.long_matrix(LB), LB or None, nlong=(1, 1))


@pytest.mark.parametrize("LB", [0, 2, 16])
def test_apply_is_exact_across_uneven_row_ranges(LB):
    check_apply(SL.staircase(), LB or None)


# ---- one step ------------------------------------------------------------------------------------------------------------------------------
VECS = {"G0": hip.VEC_G0, "XHAT": hip.VEC_XHAT, "XPROX": hip.VEC_XPROX, "Z": hip.VEC_Z, "G1": hip.VEC_G1, "X1": hip.VEC_X1}


def run_step(c, S, L, X0, B, tag, tau, coef):
    """init -> fwd -> adj -> fwd_adj -> adj(accel): what the device returned, keyed as tests/sparse_lanes.py:exact_step keys its model."""
    m, n = S.shape
    cols = L or 1
    mat = lambda name: c.get_vector(VECS[name], (m if name == "Z" else n) * cols).reshape(np.shape(B) if name == "Z" else np.shape(X0))
    got = {}
    c.set_loss_lsq(B)
    c.set_prox(tag.kind, tag.mu, tag.lo, tag.hi)
    c.set_vector(hip.VEC_X0, X0)
    got["init"] = c.init()
    got["G0"] = mat("G0")
    got["fwd"] = c.fwd(tau)
    got["XHAT"], got["XPROX"], got["Z"] = mat("XHAT"), mat("XPROX"), mat("Z")
    got["adj"] = c.adj(tau)
    got["G1"] = mat("G1")
    got["pair"] = c.fwd_adj(tau)
    got["G1_pair"], got["Z_pair"] = mat("G1"), mat("Z")
    got["adja"] = c.adj(tau, accel=True, coef=coef)
    got["G1A"], got["X1"] = mat("G1"), mat("X1")
    return got


def assert_zero_padding(c, S, L):
    if not L:
        return                      # (the vector form's padding is never written: csrc/fh_sparse.h)
    m, n = S.shape
    for which in (hip.VEC_G0, hip.VEC_XHAT, hip.VEC_XPROX, hip.VEC_X1, hip.VEC_G1):
        assert padding_is_zero(c, which, n, L), which
    assert padding_is_zero(c, hip.VEC_Z, m, L, m_side=True)


def check_exact_step(S, L, kind, G=None, nlong=(0, 0), nt=0):
    tag = SL.prox_tag(kind)
    X0, B = SL.step_operands(S, L)
    want = SL.exact_step(S, X0, B, tag)
    op = open_map(S, L, nt)
    try:
        c = op.ctx
        assert_lanes(c, S, SL.lb_of(L), G, nlong)
        got = run_step(c, S, L, X0, B, tag, SL.TAU, SL.COEF)
        for name in SL.MATRICES:
            bad = np.argwhere(got[name] != want[name])
            assert bad.size == 0, f"{name}: {len(bad)} wrong entries, first at {bad[0]}: {got[name][tuple(bad[0])]} != {want[name][tuple(bad[0])]}"
        for block in SL.BLOCKS:
            for slot, v in want[block].items():
                assert got[block][slot] == v, f"{block} scalar {slot}: {got[block][slot]!r} != {v!r}"
        # K-adj leaves the forward half of the block alone; fh_fwd_adj is both launches under one synchronisation
        assert np.array_equal(got["adj"][:hip.S_DXDG], got["fwd"][:hip.S_DXDG])
        assert np.array_equal(got["pair"][:hip.S_ALPHA], np.concatenate([got["fwd"][:hip.S_DXDG], got["adj"][hip.S_DXDG:hip.S_ALPHA]]))
        assert np.array_equal(got["G1_pair"], want["G1"]) and np.array_equal(got["Z_pair"], want["Z"])
        assert_zero_padding(c, S, L)
        return got, want, X0
    finally:
        op.close()


@pytest.mark.parametrize("G,LB,L,kind", SL.step_cases(), ids=lambda v: str(v))
def test_one_step_is_exact_on_every_instantiation(G, LB, L, kind):
    """Every matrix and every scalar of init, fwd, adj, fwd_adj and the accelerated adj == the model; the rows of the three empty columns of
    A (empty rows of the A^T copy) get g = 0 and exactly the epilogue's values for it."""
    got, want, X0 = check_exact_step(SL.exact_matrix(G, LB), L, kind, G, nt=(G // 4) % 2)
    tag = SL.prox_tag(kind)
    xp = np.asarray(tag.prox(X0[-3:], SL.TAU)) if kind != "none" else X0[-3:]            # g0 = 0 there: xhat = x0
    assert not got["G0"][-3:].any() and not got["G1"][-3:].any() and not got["G1A"][-3:].any()
    assert np.array_equal(got["XHAT"][-3:], X0[-3:]) and np.array_equal(got["XPROX"][-3:], xp)
    assert np.array_equal(got["X1"][-3:], xp + SL.COEF * (xp - X0[-3:])) and got["X1"][-3:].any()


@pytest.mark.parametrize("LB", (0,) + SL.ALL_LB)
def test_one_step_is_exact_on_a_whole_workgroup_row(LB):
    check_exact_step(SL.long_matrix(LB), LB or None, "shrink", nlong=(1, 1))


@pytest.mark.parametrize("LB", [0, 2, 16])
def test_one_step_is_exact_across_uneven_row_ranges(LB):
    check_exact_step(SL.staircase(), LB or None, "box")


# ---- GroupShrink ---------------------------------------------------------------------------------------------------------------------------
def check_group_step(S, L, G=None, nlong=(0, 0)):
    S, X0, B, tau, mu = SL.group_problem(S, L)
    tag, coef = fa.GroupShrink(mu), 0.37
    want = SL.exact_step(S, X0, B, tag, tau=tau, coef=coef, dtype=np.longdouble)
    n = S.shape[1]
    op = open_map(S, L)
    try:
        c = op.ctx
        assert_lanes(c, S, SL.lb_of(L), G, nlong)
        got = run_step(c, S, L, X0, B, tag, tau, coef)
        for name, (rtol, atol) in SL.GROUP_TOL.items():
            np.testing.assert_allclose(got[name], want[name].astype(np.float64), rtol=rtol, atol=atol, err_msg=name)
        for block in SL.BLOCKS:
            for slot, v in want[block].items():
                rtol, atol = SL.scalar_tol(block, slot)
                np.testing.assert_allclose(got[block][slot], float(v), rtol=rtol, atol=atol, err_msg=f"{block} scalar {slot}")
        # The two sums that go through the tree over a row's column lanes, against the row norms of what the DEVICE returned.  n non-negative
        # terms; each is the square root of a sum of at most 16 squares -- 16 products, 15 additions (pair, then tree), one root: each
        # rounding at most 2^-53 relative on a sum of non-negative terms, halved by the root, so a term is good to 16 roundings -- and the
        # n terms are then added in some order, at most n - 1 more roundings on a non-negative sum: (n + 16) * 2^-53 relative.
        bound = (n + 16) * 2.0 ** -53
        for block, name in (("adj", "XPROX"), ("adja", "X1")):
            ref = SL.row_norm_sum(got[name])
            err = abs(np.longdouble(got[block][hip.S_GSUM_ADJ]) - ref) / ref
            print(f" {block}: |S_GSUM_ADJ - sum of row norms| = {float(err):.2e} relative (bound {bound:.2e})", end="")
            assert ref > 0 and err <= bound, (block, float(err), bound)
        assert np.array_equal(got["pair"][:hip.S_ALPHA], np.concatenate([got["fwd"][:hip.S_DXDG], got["adj"][hip.S_DXDG:hip.S_ALPHA]]))
        assert_zero_padding(c, S, L)
    finally:
        op.close()


@pytest.mark.parametrize("G,LB,L", SL.group_cases(), ids=lambda v: str(v))
def test_group_step_on_every_instantiation(G, LB, L):
    check_group_step(SL.exact_matrix(G, LB), L, G)


@pytest.mark.parametrize("LB", SL.ALL_LB)
def test_group_step_on_a_whole_workgroup_row(LB):
    check_group_step(SL.long_matrix(LB), LB, nlong=(1, 1))


# ---- repeatability -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G,LB,L", [(16, 0, None), (32, 2, 2), (8, 4, 3), (16, 8, 7), (64, 16, 16)], ids=lambda v: str(v))
def test_a_group_step_on_a_fresh_context_is_bit_identical(G, LB, L):
    """One case per LB, run twice, each on a context of its own: every matrix and the whole scalar block agree bit for bit (GroupShrink where
    the form has it, so that roundings are there to differ)."""
    S = SL.exact_matrix(G, LB)
    if L:
        S, X0, B, tau, mu = SL.group_problem(S, L)
        tag = fa.GroupShrink(mu)
    else:
        (X0, B), tau, tag = SL.step_operands(S, L), 0.3, fa.Shrink(0.7)
    runs = []
    for _ in range(2):
        op = open_map(S, L)
        try:
            runs.append(run_step(op.ctx, S, L, X0, B, tag, tau, 0.37))
        finally:
            op.close()
    assert set(runs[0]) == set(runs[1])
    for key in runs[0]:
        assert np.array_equal(runs[0][key], runs[1][key]), key

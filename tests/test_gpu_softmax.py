"""GPU tests of the softmax loss over a matrix unknown (fh_set_loss_softmax, csrc/fh_softmax.h) -- through the C ABI and through fasta().

The row kernel is observed through an IDENTITY matrix as the operator (dense and sparse): Z = X0 exactly and G0 = A^T R = R exactly (products
with 1 and sums with zeros are exact), so fh_init hands back the kernel's residual and, in FH_S_FSQ, the loss its value-only pass computed.
Bounds (tests/softmax_cases.py, derived in the issue): a residual entry within 2 (L + 3) 2^-53 of a longdouble evaluation from the
float64-rounded d = z - mx (exp at 1 ulp, at most L - 1 additions, a division, a subtraction, probabilities <= 1, a factor 2 of margin); the loss
within 2^-52 [(m + 4) sum_i (|mx_i| + log s_i + |z_i,y|) + m (L + 2)] of the longdouble sum.
test_random_rows_against_longdouble prints the measured maxima (`-s`); DESIGN.md section 17 records them.
One whole step is held to the tolerances of tests/test_gpu_mmv.py / tests/test_gpu_sparse_mmv.py:test_single_step_scalars_match_numpy, against
NumPy on the device's own vectors; whole solves to equal iteration and backtrack counts, histories rtol 1e-6 / atol 1e-14 over the whole run
(no fixture's row-permuted twin ever parts), solution rtol 1e-5 with a floor of 1e-6 of its largest entry."""
import warnings

import numpy as np
import pytest
from scipy import sparse as sp

import fasta_python_amd as fa
from fasta_python_amd import hip, proximal
from fasta_python_amd import stopping as fstop
from tests import gpu_util as G
from tests import softmax_cases as SC

pytestmark = pytest.mark.gpu

FIELDS = ("residuals", "norm_residuals", "stepsizes", "objectives")
ROWS = [1, 33, 97]


@pytest.fixture(autouse=True)
def no_scratch_contexts_left_behind():
    yield
    proximal.release_scratch()


def identity_operator(form, m, L):
    return fa.DenseMatrixMap(np.eye(m), rhs=L) if form == "dense" else fa.SparseMatrixMap(sp.identity(m, format="csr"), rhs=L)


def rows_through_identity(form, Z, y):
    """(R, loss, padding is zero) of the row kernel at Z: fh_init on the identity operator."""
    m, L = Z.shape
    op = identity_operator(form, m, L)
    c = op.ctx
    try:
        c.set_loss_softmax(y)
        assert np.array_equal(c.get_vector(hip.VEC_B, m * L).reshape(m, L), np.eye(L)[y])          # the one-hot matrix
        c.set_vector(hip.VEC_X0, Z)
        s = c.init()
        R = c.get_vector(hip.VEC_G0, m * L).reshape(m, L)
        c.set_vector(hip.VEC_T0, R)                                     # (fh_diff_norm adds up the WHOLE device buffers: zero only if G0's padding is zero)
        clean = c.diff_norm(hip.VEC_G0, hip.VEC_T0) == 0.0
        c.set_vector(hip.VEC_T1, Z)                                     # ... and fh_gradient_at runs the same two passes
        c.gradient_at(hip.VEC_T1, hip.VEC_T2)
        assert np.array_equal(c.get_vector(hip.VEC_T2, m * L).reshape(m, L), R)
        return R, s[hip.S_FSQ], clean
    finally:
        op.close()


# ---- the row kernel alone ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["dense", "sparse"])
@pytest.mark.parametrize("L", SC.ALL_L)
@pytest.mark.parametrize("m", ROWS)
def test_constant_rows_are_bit_exact_and_padding_stays_zero(m, L, form):
    y = np.arange(m) % L
    Z = np.repeat(np.linspace(-3.5, 700.0, m)[:, None], L, axis=1)       # every row constant, the rows differ
    R, loss, clean = rows_through_identity(form, Z, y)
    assert np.array_equal(R, np.float64(1.0) / np.float64(L) - np.eye(L)[y]) and clean
    R2, _, _, want = SC.kernel_model(Z, y, L)
    assert np.array_equal(R, R2[:, :L])
    _, _, mags = SC.longdouble_rows(Z, y)
    assert abs(loss - want) <= SC.loss_bound(m, L, mags)                 # (log(L) is the device library's: its last ulp may differ from NumPy's)


@pytest.mark.parametrize("form", ["dense", "sparse"])
def test_the_800_rows_are_exact_and_finite(form):
    Z = np.array([[800.0, -800.0], [-800.0, 800.0], [800.0, -800.0]])
    for y, want in ((np.array([0, 1, 0]), 0.0), (np.array([1, 0, 0]), 3200.0), (np.array([0, 0, 1]), 3200.0)):
        R, loss, clean = rows_through_identity(form, Z, y)
        assert np.array_equal(R + np.eye(2)[y], np.array([[1.0, 0.0], [0.0, 1.0], [1.0, 0.0]])) and clean
        assert loss == want
    Z3 = np.array([[800.0, -800.0, 0.0]])
    R, loss, _ = rows_through_identity(form, Z3, np.array([2]))
    assert np.array_equal(R, np.array([[1.0, 0.0, -1.0]])) and loss == 800.0


@pytest.mark.parametrize("form", ["dense", "sparse"])
@pytest.mark.parametrize("L", SC.ALL_L)
def test_random_rows_against_longdouble(L, form):
    m = 97
    rng = np.random.RandomState(500 + L)
    Z, y = rng.uniform(-30.0, 30.0, (m, L)), rng.randint(0, L, m)
    R, loss, clean = rows_through_identity(form, Z, y)
    want, terms, mags = SC.longdouble_rows(Z, y)
    err = float(np.abs(R.astype(np.longdouble) - want).max())
    lerr, lbound = float(abs(np.longdouble(loss) - terms.sum())), SC.loss_bound(m, L, mags)
    print(f"\n{form} L={L}: residual error {err:.3e} = {err / SC.residual_bound(L):.3f} of the bound; loss error {lerr:.3e} = {lerr / lbound:.2e} of the bound", end="")
    assert clean and err <= SC.residual_bound(L)
    assert lerr <= lbound
    model_R, _, _, model_loss = SC.kernel_model(Z, y, L)                 # the same order with NumPy's exp / log: the device libm's last ulp apart
    assert np.abs(R - model_R[:, :L]).max() <= SC.residual_bound(L) and abs(loss - model_loss) <= lbound


@pytest.mark.parametrize("form", ["dense", "sparse"])
def test_the_row_pass_is_bitwise_repeatable(form):
    rng = np.random.RandomState(9)
    Z, y = rng.uniform(-30.0, 30.0, (97, 16)), rng.randint(0, 16, 97)
    a, b = rows_through_identity(form, Z, y), rows_through_identity(form, Z, y)
    assert np.array_equal(a[0], b[0]) and a[1] == b[1]


# ---- one whole step ---------------------------------------------------------------------------------------------------------------------------
# how the step test holds the device against NumPy (rtol, atol): shared with the stations of tests/carry_cases.py
STEP_TOL = {"G0": dict(rtol=1e-12, atol=1e-13), "F0": dict(rtol=1e-12), "Z": dict(rtol=1e-12, atol=1e-13), "G1": dict(rtol=1e-11, atol=1e-13),
            "fwd scalars": dict(rtol=1e-11, atol=1e-13)}


def empty_row_matrix():
    S = sp.random(120, 90, density=0.1, format="lil", random_state=np.random.RandomState(15), data_rvs=np.random.RandomState(16).standard_normal)
    S[7, :] = 0
    S = S.tocsr()
    S.eliminate_zeros()
    assert np.diff(S.indptr)[7] == 0
    return S


STEP_OPERATORS = {
    "dense97": lambda: np.random.RandomState(14).randn(97, 33) * 0.3,
    "dense33": lambda: np.random.RandomState(14).randn(33, 33) * 0.3,
    "dense1": lambda: np.random.RandomState(14).randn(1, 33) * 0.3,
    "sparse": lambda: sp.random(120, 90, density=0.1, format="csr", random_state=np.random.RandomState(14), data_rvs=np.random.RandomState(17).standard_normal),
    "sparse_empty_row": empty_row_matrix,
}


@pytest.mark.parametrize("L,kind,operator", [(3, "group", "dense97"), (16, "group", "dense97"), (2, "shrink", "dense97"), (5, "nonneg", "dense33"),
                                            (9, "box", "dense97"), (4, "none", "dense1"), (8, "shrink", "dense33"),
                                            (7, "group", "sparse"), (16, "shrink", "sparse"), (2, "nonneg", "sparse"), (9, "box", "sparse_empty_row"),
                                            (4, "none", "sparse"), (3, "group", "sparse_empty_row")])
def test_single_step_scalars_match_numpy(L, kind, operator):
    """init -> fwd -> adj -> fwd_adj -> adj(accel) -> commit: matrices and all scalars against NumPy on the device's own vectors."""
    rng = np.random.RandomState(13 + L)
    A = STEP_OPERATORS[operator]()
    At = A.T.tocsr() if sp.issparse(A) else A.T
    (m, n), mu, tau = A.shape, 0.05, 0.3
    X0, y = rng.randn(n, L) * 0.5, rng.randint(0, L, m)
    sm = fa.SoftmaxLoss(y, classes=L)
    tag = {"group": fa.GroupShrink(mu), "shrink": fa.Shrink(mu), "nonneg": fa.NonNeg(), "box": fa.Box(-0.05, 0.08), "none": fa.NoProx()}[kind]
    gsum = (lambda V: np.sum(np.sqrt(np.sum(V * V, axis=1)))) if kind == "group" else (lambda V: np.abs(V).sum())
    mat = lambda which, rows: c.get_vector(which, rows * L).reshape(rows, L)
    op = fa.SparseMatrixMap(A, rhs=L) if sp.issparse(A) else fa.DenseMatrixMap(A, rhs=L)
    c = op.ctx
    try:
        sm.bind(c)
        c.set_prox(tag.kind, tag.mu, tag.lo, tag.hi)
        c.set_vector(hip.VEC_X0, X0)
        s0 = c.init()
        Z0 = A @ X0
        G0 = mat(hip.VEC_G0, n)
        np.testing.assert_allclose(G0, At @ sm.gradf(Z0), **STEP_TOL["G0"])
        np.testing.assert_allclose(s0[hip.S_FSQ], sm.f(Z0), **STEP_TOL["F0"])
        np.testing.assert_allclose(s0[hip.S_GSUM], gsum(X0), rtol=1e-12)
        s = c.fwd(tau)
        Xh = X0 - tau * G0
        Xp = np.asarray(tag.prox(Xh, tau)) * np.ones((n, L))
        np.testing.assert_allclose(mat(hip.VEC_XHAT, n), Xh, rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(mat(hip.VEC_XPROX, n), Xp, rtol=1e-12, atol=1e-14)
        Xp, Z = mat(hip.VEC_XPROX, n), mat(hip.VEC_Z, m)                 # the device's own vectors from here on
        dX = Xp - X0
        np.testing.assert_allclose(Z, A @ Xp, **STEP_TOL["Z"])
        want = {hip.S_FSQ: sm.f(Z), hip.S_DXG0: np.sum(dX * G0), hip.S_DX2: np.sum(dX * dX), hip.S_XH2: np.sum((Xp - Xh) ** 2),
                hip.S_G02: np.sum(G0 * G0), hip.S_GSUM: gsum(Xp), hip.S_GMAX: np.abs(Xp).max(), hip.S_RDOT: np.sum((X0 - Xp) * (Xp - X0))}
        for k, v in want.items():
            np.testing.assert_allclose(s[k], v, err_msg=str(k), **STEP_TOL["fwd scalars"])
        a = c.adj(tau)
        G1 = At @ sm.gradf(Z)
        dG = G1 + (Xh - X0) / tau
        np.testing.assert_allclose(mat(hip.VEC_G1, n), G1, **STEP_TOL["G1"])
        np.testing.assert_allclose(a[hip.S_DXDG], np.sum(dX * dG), rtol=1e-10, atol=1e-13)
        np.testing.assert_allclose(a[hip.S_DG2], np.sum(dG * dG), rtol=1e-10, atol=1e-13)
        np.testing.assert_allclose(a[hip.S_FSQ_ADJ], sm.f(Z), rtol=1e-11)
        assert a[hip.S_FSQ_ADJ] == s[hip.S_FSQ]                          # the same rows in the same order, value-only or not
        np.testing.assert_allclose(a[hip.S_GSUM_ADJ], gsum(Xp), rtol=1e-11)
        np.testing.assert_allclose(a[hip.S_XH2_ADJ], np.sum((Xp - Xh) ** 2), rtol=1e-11, atol=1e-13)
        np.testing.assert_allclose(a[hip.S_GMAX_ADJ], np.abs(Xp).max(), rtol=1e-12)
        assert np.array_equal(a[:hip.S_DXDG], s[:hip.S_DXDG])            # K-adj leaves the forward half of the block alone
        g1_plain = mat(hip.VEC_G1, n)
        pair = c.fwd_adj(tau)                                            # both launches under one synchronisation: the same block
        assert np.array_equal(pair[:hip.S_ALPHA], np.concatenate([s[:hip.S_DXDG], a[hip.S_DXDG:hip.S_ALPHA]]))
        assert np.array_equal(mat(hip.VEC_G1, n), g1_plain)
        coef = 0.37                                                      # accelerated variant (fasta/__init__.py:242-245)
        a2 = c.adj(tau, accel=True, coef=coef)
        X1, Z1 = Xp + coef * (Xp - X0), Z + coef * (Z - Z0)
        np.testing.assert_allclose(mat(hip.VEC_X1, n), X1, rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(a2[hip.S_FSQ_ADJ], sm.f(Z1), rtol=1e-11)
        np.testing.assert_allclose(mat(hip.VEC_G1, n), At @ sm.gradf(Z1), rtol=1e-11, atol=1e-13)
        np.testing.assert_allclose(a2[hip.S_XH2_ADJ], np.sum((X1 - Xh) ** 2), rtol=1e-11)
        np.testing.assert_allclose(a2[hip.S_GSUM_ADJ], gsum(X1), rtol=1e-11)
        np.testing.assert_allclose(a2[hip.S_GMAX_ADJ], np.abs(X1).max(), rtol=1e-12)
        for which in (hip.VEC_G0, hip.VEC_XHAT, hip.VEC_XPROX, hip.VEC_X1, hip.VEC_G1):      # padding columns and rows: exact zeros
            v = c.get_vector(which, n * L)
            c.set_vector(hip.VEC_T0, v)
            assert c.diff_norm(which, hip.VEC_T0) == 0.0, which
        g1_accel = mat(hip.VEC_G1, n)
        c.commit(True)
        assert np.array_equal(mat(hip.VEC_X0, n), mat(hip.VEC_BEST, n)) and np.array_equal(mat(hip.VEC_G0, n), g1_accel)
        np.testing.assert_allclose(mat(hip.VEC_X0, n), X1, rtol=1e-12, atol=1e-14)
        # the plain operator (fh_apply) is untouched by the loss
        V = rng.randn(n, L)
        np.testing.assert_allclose(op.device_apply(V), A @ V, rtol=1e-12, atol=1e-12)
        c.timing_enable(True)
        c.fwd(tau), c.adj(tau), c.init()
        assert c.timing_get(hip.K_FWD)[1] >= 2 and c.timing_get(hip.K_ADJ)[1] >= 2 and c.timing_get(hip.K_FUSED)[1] == 0
    finally:
        op.close()


# ---- whole solves -----------------------------------------------------------------------------------------------------------------------------
def solve(name, **extra):
    meta, z, d = SC.load(name)
    ms = SC.capture_script()
    A = ms.matrix_of(d)
    L = int(d["classes"])
    loss, reg = ms.tags(meta["prox"], d)
    g, proxg = (None, None) if reg is None else (reg.g, reg.prox)
    op = fa.SparseMatrixMap(A, rhs=L) if sp.issparse(A) else fa.DenseMatrixMap(A, rhs=L)
    try:
        o = ms.resolve(dict(meta["options"], **extra), fstop)
        np.random.seed(meta["solver_seed"])
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return fa.fasta(op, op.H, loss.f, loss.gradf, g, proxg, np.zeros((A.shape[1], L)), verbose=False, backend="hip", **o)
    finally:
        op.close()


_runs = {}


def library_run(name):
    """The library-driven device solve of a fixture, computed once and shared by the tests below; never modified."""
    if name not in _runs:
        _runs[name] = solve(name, driver="library")
    return _runs[name]


def assert_same_bits(a, b):
    assert a.iteration_count == b.iteration_count and a.backtracks == b.backtracks
    for f in FIELDS:
        if getattr(b, f) is not None:
            assert np.array_equal(getattr(a, f), getattr(b, f), equal_nan=True), f
    assert np.array_equal(a.solution, b.solution)


@pytest.mark.parametrize("name", SC.CASES)
def test_fixture_solves_on_the_device(name):
    meta, z, d = SC.load(name)
    lib = library_run(name)
    k = int(z["iteration_count"])
    assert meta["twin_divergence"] == k                                  # the twin never parts: the whole run is compared
    assert lib.library_steps == lib.iteration_count and lib.device_steps == 0
    print(f"\n{name}: device {lib.iteration_count} iterations / {lib.backtracks} backtracks, reference {k} / {int(z['backtracks'])}", end="")
    assert lib.iteration_count == k and lib.backtracks == int(z["backtracks"])
    worst = G.compare_histories(lib, lambda f: z[f] if f in z.files else None, k, rtol=1e-6, atol=1e-14)
    print(f"; worst relative deviation of a history entry {worst:.2e}")
    np.testing.assert_allclose(lib.solution, z["solution"], rtol=1e-5, atol=1e-6 * float(np.max(np.abs(z["solution"]))))


@pytest.mark.parametrize("name", SC.CASES)
def test_the_python_driver_and_a_second_run_give_the_same_bits(name):
    lib = library_run(name)
    py = solve(name, driver="python")
    assert py.library_steps == 0
    assert_same_bits(py, lib)
    if name in ("group_60x40x3_adaptive", "sparse_120x90x7_accelerated", "l1_97x33x16_adaptive"):
        assert_same_bits(solve(name, driver="library"), lib)


# ---- the example ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [[], ["--sparse", "0.2"], ["--group"]], ids=["dense", "sparse", "group"])
def test_the_example_matches_its_host_twin(extra, capsys):
    from fasta.examples import multiclass_logistic as ex
    argv = ["--rows", "40", "--features", "24", "--classes", "3"] + extra
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        dev = ex.main(["--backend", "hip"] + argv)
        host = ex.main(["--backend", "numpy"] + argv)
    assert "Iterations (adaptive, accelerated, plain)" in capsys.readouterr().out
    for (sol, c), (wsol, w) in zip(dev, host):
        assert c.iteration_count == w.iteration_count >= 1 and c.backtracks == w.backtracks
        k = c.iteration_count
        np.testing.assert_allclose(c.residuals[:k], w.residuals[:k], rtol=1e-6, atol=1e-13)
        np.testing.assert_allclose(c.stepsizes[:k], w.stepsizes[:k], rtol=1e-6)
        np.testing.assert_allclose(c.objectives[:k + 1], w.objectives[:k + 1], rtol=1e-8)
        np.testing.assert_allclose(sol, wsol, rtol=1e-5, atol=1e-6 * float(np.max(np.abs(wsol))))


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------
def refusal(fn, *args):
    with pytest.raises(hip.HipError) as e:
        fn(*args)
    text = str(e.value)
    return int(text[1:text.index("]")]), text


def test_refusals_by_code_and_sentence():
    rng = np.random.RandomState(0)
    A = rng.randn(40, 24)
    y = np.arange(40) % 4
    with hip.HipContext(0) as c:
        code, text = refusal(c.set_loss_softmax, y)
        assert code == hip.E_STATE and "set the operator before the loss" in text
        c.set_matrix(A)
        code, text = refusal(c.set_loss_softmax, y)                      # before fh_set_rhs
        assert code == hip.E_STATE and "needs the multi-column form" in text and "fh_set_rhs" in text
        c.set_rhs(1)
        code, text = refusal(c.set_loss_softmax, np.zeros(40, dtype=int))
        assert code == hip.E_STATE and "at least two columns" in text and "L = 1" in text
        c.set_rhs(4)
        code, text = refusal(c.set_loss_softmax, np.where(np.arange(40) == 17, 4, y))
        assert code == hip.E_ARG and "[0, 4)" in text and "entry 17 is 4" in text
        code, text = refusal(c.set_loss_softmax, np.where(np.arange(40) >= 5, -1, y))
        assert code == hip.E_ARG and "entry 5 is -1" in text
        code, text = refusal(c.set_loss_softmax, y[:39])
        assert code == hip.E_ARG and "39 entries" in text and "40 rows" in text
        code, text = refusal(c.set_loss_logistic, np.ones(40 * 4))       # unchanged: the elementwise logistic loss has no multi-column form
        assert code == hip.E_STATE and text.endswith("the logistic loss has no multi-column form (fh_set_rhs / fh_set_matrix_csr_rhs)")
        c.set_loss_softmax(y)
        c.set_prox(hip.PROX_GROUP, 0.1)
        c.set_vector(hip.VEC_X0, np.zeros((24, 4)))
        s = c.init()
        assert s[hip.S_FSQ] == 40 * np.log(4.0) or abs(s[hip.S_FSQ] - 40 * np.log(4.0)) < 1e-12
        assert c.fused_supported() == 0 and not c.run_supported()
        for fn, args in ((c.step, (0.1,)), (c.step_begin, (0.1,)), (c.step_accel, (0.1, 0.0, True))):
            code, text = refusal(fn, *args)
            assert code == hip.E_STATE and "multi-column form" in text
        o, st = hip.RunOpts(), hip.RunState()
        o.window, o.stop_rule = 10, 3
        code, text = refusal(c.run, 4, o, st)
        assert code == hip.E_STATE and "fh_run" in text
        assert np.isfinite(c.fwd(0.1)[hip.S_FSQ])                        # still usable
        c.set_rhs(4)                                                     # the column count again: back to least squares, the loss to be set again
        code, text = refusal(c.init)
        assert code == hip.E_STATE and "no loss set" in text
        c.set_loss_lsq(np.zeros((40, 4)))
        assert c.init()[hip.S_FSQ] == 0.0
    for what, setter in (("stencil", lambda c: c.set_stencil(8, 8)), ("DCT", lambda c: c.set_dct(64)), ("identity", lambda c: c.set_identity(8, 5)),
                         ("quadratic", lambda c: c.set_quadratic(np.eye(40), None, 4))):
        with hip.HipContext(0) as c:
            setter(c)
            code, text = refusal(c.set_loss_softmax, y)
            assert code == hip.E_STATE and "dense and the sparse operator in multi-column form only" in text and what in text, what
    S = sp.random(40, 24, density=0.2, format="csr", random_state=rng)
    with hip.HipContext(0) as c:
        c.set_matrix_csr(S.indptr, S.indices, S.data, S.shape)
        code, text = refusal(c.set_loss_softmax, y)
        assert code == hip.E_STATE and "fh_set_matrix_csr_rhs" in text
        c.set_matrix_csr_rhs(S.indptr, S.indices, S.data, S.shape, 4)
        code, text = refusal(c.set_loss_softmax, y + 1)
        assert code == hip.E_ARG and "entry 3 is 4" in text
        c.set_loss_softmax(y)
        c.set_vector(hip.VEC_X0, np.zeros((24, 4)))
        assert abs(c.init()[hip.S_FSQ] - 40 * np.log(4.0)) < 1e-12
    with hip.HipContext(devices=[0, 0]) as c:
        c.set_matrix(A)
        code, text = refusal(c.set_loss_softmax, y)
        assert code == hip.E_STATE and "multi-device" in text

"""GPU tests of standardised features on the device (fh_standardize: csrc/fh_standardize.h) against the host statement
(fasta_python_amd/preprocess.py) and of path(standardize=..., intercept=...).  Shapes, data and the path problems: tests/standardize_cases.py.

Bounds.  Balanced dyadic data: sums, means and sums of squares are exact in any order, the rest is a chain of single correctly rounded operations
spelled alike on both sides -- means, scales and the rewritten matrix are compared with `==` (float32 storage: `.astype(np.float32)` of the float64
statement).  Any data, split in two: (a) a returned mean and ss = m * scale^2 lie within (slab + nslab + 1) eps sum_i |term_i| of the exact sum of the
column -- the chain the shape rule gives has at most slab - 1 additions inside a slab, nslab - 1 across the slabs and the closing division, each
at most eps / 2 of a partial sum no larger than sum |term|; the other half of the budget covers forming m * scale^2 back from the scale (the
division by m once, the square root twice: 3 eps / 2), for a slab of 16 rows or more; (b) given the device's OWN means and scales every rewritten entry is two
single rounded operations: `==`.  Column norms after the rewrite on seeded data: (m + 2) eps norms2_j, the bound of tests/test_gpu_screen.py.
A second context that receives the read-back matrix through fh_set_matrix: bit for bit."""
import math
import warnings
from fractions import Fraction

import numpy as np
import pytest

import fasta_python_amd as fa
from fasta_python_amd import certificates as ce
from fasta_python_amd import hip, preprocess
from tests import standardize_cases as SC

pytestmark = pytest.mark.gpu

VECS = ("VEC_X0", "VEC_G0", "VEC_XHAT", "VEC_XPROX", "VEC_X1", "VEC_G1", "VEC_BEST", "VEC_B", "VEC_Z")
EPS = SC.EPS
FORMS = [(storage, m, n, L) for storage, m, n in SC.SHAPES for L in ((0, 3) if storage == "f64" else (0,))]
FORM_IDS = ["%s-%dx%d-L%d" % f for f in FORMS]


def context(A, storage, L):
    c = hip.HipContext(0, storage=storage)
    c.set_matrix(A)
    if L:
        c.set_rhs(L)
    return c


def host_statement(A, storage, center, scale):
    """(rewritten matrix as the storage holds it, means, scales) of preprocess.standardize on the values the context holds."""
    Z, (means, scales, _) = preprocess.standardize(SC.stored(A, storage), center=center, scale=scale)
    return SC.stored(Z, storage), means, scales


def aux_launches(c):
    return c.timing_get(hip.K_AUX)[1]


# ---- 1. exact -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_dyadic_data_gives_the_host_statement_bit_for_bit(form):
    storage, m, n, L = form
    A = SC.balanced_dyadic(m, n, seed=m + n)
    for center, scale in ((True, True), (True, False), (False, True)):
        want_rows, want_means, want_scales = host_statement(A, storage, center, scale)
        with context(A, storage, L) as c:
            means, scales = c.standardize(center=center, scale=scale)
            np.testing.assert_array_equal(means, want_means)
            np.testing.assert_array_equal(scales, want_scales)
            np.testing.assert_array_equal(c.get_matrix_rows(0, m), want_rows)
            assert c.rhs == L and c.shape() == (m, n)
            if scale:
                assert len(set(scales.tolist())) > 3 and scales[SC.CONSTANT if center else SC.ZERO] == 1.0 and scales[SC.ZERO] == 1.0
                assert scales[SC.LARGE] > 1e4 * np.median(scales)
            else:
                np.testing.assert_array_equal(scales, np.ones(n))
            if not center:
                np.testing.assert_array_equal(means, np.zeros(n))
            if not scale:                                # the rewritten values are dyadic again: the norms are exact
                np.testing.assert_array_equal(c.column_norms(), ce.column_norms2(want_rows))


# ---- 2. any data --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_seeded_data_within_the_chains_bound_and_the_rewrite_exactly(form):
    storage, m, n, L = form
    A = SC.stored(SC.seeded(m, n, seed=3 * m + n), storage)
    sh = hip.screen_shape_for(m, n, L, storage, hip.device_cus(0))
    budget = (sh.slab + sh.nslab + 1) * EPS
    with context(A, storage, L) as c:
        means, scales = c.standardize()
        rows = c.get_matrix_rows(0, m)
        norms = c.column_norms()
    worst_mean = worst_ss = 0.0
    for j in range(n):
        col = A[:, j]
        # (a) the mean against the exact sum
        exact = Fraction(0)
        for v in col:
            exact += Fraction(float(v))
        size = math.fsum(abs(v) for v in col)
        err = abs(Fraction(float(means[j])) * m - exact)
        worst_mean = max(worst_mean, float(err) / (budget * size) if size else float(err))
        assert err <= Fraction(budget) * Fraction(size), (j, float(err), budget * size)
        # ... and the centred squares about the device's own mean
        d = col - means[j]
        exact = Fraction(0)
        for v in d:
            exact += Fraction(float(v)) ** 2
        if exact == 0:
            assert scales[j] == 1.0, j
            continue
        err = abs(Fraction(float(scales[j])) ** 2 * m - exact)
        worst_ss = max(worst_ss, float(err / (Fraction(budget) * exact)))
        assert err <= Fraction(budget) * exact, (j, float(err), float(exact))
    print(form, "largest error / bound: mean %.3f, ss %.3f" % (worst_mean, worst_ss))
    assert scales[SC.CONSTANT] == 1.0 and scales[SC.ZERO] == 1.0
    # (b) the rewrite from the device's own statistics
    np.testing.assert_array_equal(rows, SC.stored((A - means) / scales, storage))
    # 3. the norms of the rewritten block
    want = np.array([math.fsum(v * v for v in rows[:, j]) for j in range(n)])
    assert np.all(np.abs(norms - want) <= (m + 2) * EPS * want)
    np.testing.assert_array_equal(norms, norms)          # (no NaN)


# ---- 3. the padding -----------------------------------------------------------------------------------------------------------------------------
def snapshot(c, n_len, m_len):
    return {v: c.get_vector(getattr(hip, v), m_len if v in ("VEC_B", "VEC_Z") else n_len) for v in VECS}


def walk(c, b, x, mu, tau, L):
    """scalars and vectors of fh_init, five one-pass steps (where the shape has the kernel), five K-fwd + K-adj steps, the certificate"""
    c.set_loss_lsq(b)
    c.set_prox(hip.PROX_SHRINK, mu)
    c.set_vector(hip.VEC_X0, x)
    out = [c.init()]
    if c.fused_supported():
        for _ in range(5):
            out.append(c.step(tau))
            c.commit()
    for _ in range(5):
        out.append(c.fwd(tau))
        out.append(c.adj(tau))
        c.commit()
    cert = tuple(c.dual_gap())
    return out, snapshot(c, x.size, b.size), cert


@pytest.mark.parametrize("form", [f for f in FORMS if (f[1], f[2]) in ((33, 530), (40, 1030), (6, 10))], ids=lambda f: "%s-%dx%d-L%d" % f)
def test_a_context_given_the_read_back_matrix_walks_the_same_bits(form):
    storage, m, n, L = form
    A = SC.seeded(m, n, seed=m + 7 * n)
    rng = np.random.RandomState(n)
    cols = () if not L else (L,)
    b, x = rng.randn(*((m,) + cols)), rng.randn(*((n,) + cols)) * (rng.rand(*((n,) + cols)) < 0.2)
    with context(A, storage, L) as c, hip.HipContext(0, storage=storage) as twin:
        c.standardize()
        rows = c.get_matrix_rows(0, m)
        assert np.all(np.isfinite(rows))
        twin.set_matrix(rows)                            # (float32 storage: the rows are float32 values, the upload rounds nothing)
        if L:
            twin.set_rhs(L)
        tau = 0.5 / np.linalg.norm(rows, 2) ** 2
        got = walk(c, b, x, 0.05, tau, L)
        want = walk(twin, b, x, 0.05, tau, L)
        assert len(got[0]) == len(want[0]) >= 11
        for g, w in zip(got[0], want[0]):
            np.testing.assert_array_equal(g, w)
        for v in VECS:
            np.testing.assert_array_equal(got[1][v], want[1][v], err_msg=v)
        assert got[2] == want[2] and np.all(np.isfinite(got[2]))
        np.testing.assert_array_equal(c.column_norms(), twin.column_norms())


# ---- 4. the state -------------------------------------------------------------------------------------------------------------------------------
NO_STATE = "fh_dual_gap: no committed state: call fh_init or fh_setup first (after the operator, the loss and x0 are set)"


def refused(call, status, sentence):
    with pytest.raises(hip.HipError) as err:
        call()
    assert str(err.value) == "[%d] %s" % (status, sentence), str(err.value)


@pytest.mark.parametrize("L", [0, 3])
def test_the_context_is_as_after_a_setter(L):
    m, n = 32, 530
    A = SC.two_level(m, n, seed=9)
    rng = np.random.RandomState(1)
    cols = () if not L else (L,)
    b, x = rng.randn(*((m,) + cols)), rng.randn(*((n,) + cols)) * (rng.rand(*((n,) + cols)) < 0.2)
    with context(A, "f64", L) as c, hip.HipContext(0) as twin:
        c.timing_enable()
        c.set_loss_lsq(b)
        c.set_prox(hip.PROX_SHRINK, 0.25)
        c.set_vector(hip.VEC_X0, x)
        c.init()
        assert c.dual_gap().gap >= 0
        before = c.column_norms()
        held = aux_launches(c)
        c.column_norms()
        assert aux_launches(c) == held                   # kept: a second call launches nothing
        means, scales = c.standardize()
        _, want_means, want_scales = host_statement(A, "f64", True, True)
        np.testing.assert_array_equal(means, want_means)
        np.testing.assert_array_equal(scales, want_scales)
        first_zero = np.zeros(n, dtype=bool)
        first_zero[[SC.CONSTANT, SC.ZERO]] = True        # the columns whose scale was 0 and is reported as 1
        assert set(scales[~first_zero].tolist()) == {0.125, 0.25, 0.5, 0.125 * 2.0 ** 20}
        refused(c.dual_gap, hip.E_ARG, NO_STATE)         # no committed state until fh_init
        refused(c.screen, hip.E_ARG, NO_STATE.replace("fh_dual_gap", "fh_screen"))
        after_call = aux_launches(c)
        norms = c.column_norms()                         # the kept norms were dropped: they are formed again, of the new columns
        assert aux_launches(c) > after_call and np.any(norms != before)
        np.testing.assert_array_equal(norms, np.where(first_zero, 0.0, float(m)))       # columns of +-1, and two of zeros
        assert c.rhs == L
        # the prox kind, the loss, b and x0 stayed: fh_init alone brings the certificate back, the one of a context set up from scratch
        c.init()
        twin.set_matrix(c.get_matrix_rows(0, m))
        if L:
            twin.set_rhs(L)
        twin.set_loss_lsq(b)
        twin.set_prox(hip.PROX_SHRINK, 0.25)
        twin.set_vector(hip.VEC_X0, x)
        twin.init()
        assert tuple(c.dual_gap()) == tuple(twin.dual_gap())
        np.testing.assert_array_equal(c.get_vector(hip.VEC_B, b.size), b.ravel())
        np.testing.assert_array_equal(c.get_vector(hip.VEC_X0, x.size), x.ravel())
        # a second call standardises the standardised matrix: means of exactly zero, scales of exactly one
        means2, scales2 = c.standardize()
        refused(c.dual_gap, hip.E_ARG, NO_STATE)
        np.testing.assert_array_equal(means2, np.zeros(n))
        np.testing.assert_array_equal(scales2, np.ones(n))
        np.testing.assert_array_equal(c.get_matrix_rows(0, m), twin.get_matrix_rows(0, m))
        # the next operator setter works as on any context
        c.set_stencil(4, 5)
        assert c.shape() == (20, 40)


# ---- 5. sparse ----------------------------------------------------------------------------------------------------------------------------------
SPARSE_CENTER = "fh_standardize: centring would fill the sparse matrix: the sparse operator is served with scale alone (center = 0)"


@pytest.mark.parametrize("L", [0, 3])
def test_the_sparse_operator_is_scaled_in_both_copies(L):
    S = SC.long_sparse()
    m, n = S.shape
    Z, (_, want_scales, _) = preprocess.standardize(S, center=False)
    rng = np.random.RandomState(3)
    cols = () if not L else (L,)
    v, w = rng.randn(*((n,) + cols)), rng.randn(*((m,) + cols))
    with hip.HipContext(0) as c, hip.HipContext(0) as twin:
        c.set_matrix_csr(S.indptr, S.indices, S.data, S.shape, rhs=L or None)
        assert c.sparse_lanes(1)[2] >= 1 and c.sparse_lanes(0)[2] >= 1          # a long row in each copy
        assert S.getnnz(axis=0)[5] == 0                                          # an empty column
        refused(lambda: c.standardize(), hip.E_ARG, SPARSE_CENTER)
        refused(lambda: c.standardize(center=True, scale=False), hip.E_ARG, SPARSE_CENTER)
        before = c.column_norms()
        means, scales = c.standardize(center=False)
        np.testing.assert_array_equal(means, np.zeros(n))
        np.testing.assert_array_equal(scales, want_scales)                       # integers: the norms are exact
        assert scales[5] == 1.0 and len(set(scales.tolist())) > 3
        twin.set_matrix_csr(Z.indptr, Z.indices, Z.data, Z.shape, rhs=L or None)
        np.testing.assert_array_equal(c.apply(v), twin.apply(v))                 # the by-rows copy
        np.testing.assert_array_equal(c.apply(w, adjoint=True), twin.apply(w, adjoint=True))      # the by-columns copy
        norms = c.column_norms()
        np.testing.assert_array_equal(norms, twin.column_norms())
        assert np.any(norms != before) and c.rhs == L


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------------------------
SERVED = "(served: the dense and the sparse operator, vector and multi-column)"
IN_FLIGHT = "a step issued by fh_step_begin is still in flight on this context: call fh_step_end first"


def test_what_fh_standardize_refuses():
    rng = np.random.RandomState(1)
    A, b = rng.randn(6, 10), rng.randn(6)
    lib = hip.load_library()
    assert lib.fh_standardize(None, 1, 1, None, None) == hip.E_ARG and lib.fh_last_error().decode() == "fh_standardize: null context"
    with hip.HipContext(0) as c:
        refused(lambda: c.standardize(center=False, scale=False), hip.E_ARG, "fh_standardize: neither center nor scale is asked: nothing to do")
        refused(c.standardize, hip.E_STATE, "fh_standardize: no operator set")
        c.set_matrix(A)
        refused(lambda: c.standardize(center=False, scale=False), hip.E_ARG, "fh_standardize: neither center nor scale is asked: nothing to do")
        c.set_loss_lsq(b)
        c.set_vector(hip.VEC_X0, np.zeros(10))
        c.init()
        c.step_begin(1e-3)
        refused(c.standardize, hip.E_STATE, "fh_standardize: " + IN_FLIGHT)
        c.step_end()
        c.commit()
        np.testing.assert_array_equal(c.get_matrix_rows(0, 6), A)                # nothing of the refused calls reached the matrix
        assert c.standardize()[0].shape == (10,)
    for noun, op in (("identity operator", fa.IdentityMap((4, 5))), ("stencil operator", fa.GradDivMap((4, 5))), ("3-D stencil operator", fa.GradDivMap((2, 4, 5))),
                     ("DCT operator", fa.DCTMap(16)), ("convolution operator", fa.ConvMap((8, 8), rng.randn(3, 3)))):
        try:
            refused(op.ctx.standardize, hip.E_STATE, "fh_standardize: the %s stores no columns %s" % (noun, SERVED))
        finally:
            op.close()
    idm = fa.IdentityMap((2, 3))
    try:
        fa.LeastSquares(np.ones((2, 3)), weights=np.ones((2, 3))).bind(idm.ctx)
        refused(idm.ctx.standardize, hip.E_STATE, "fh_standardize: the context holds observation weights (fh_set_loss_weights), which the identity operator "
                "alone serves: it stores no columns")
    finally:
        idm.close()
    shell = fa.ShardedDenseMatrixMap(A, devices=(0, 0))
    try:
        refused(shell.ctx.standardize, hip.E_STATE, "fh_standardize: a multi-device context holds row blocks of A, not its columns: the columns are "
                "standardised on a plain context")
    finally:
        shell.close()
    with hip.HipContext(0) as c:
        c.set_matrix(A)
        c.comm_init(1, 0, hip.comm_unique_id())
        refused(c.standardize, hip.E_STATE, "fh_standardize: a context with a communicator (row-sharded run) holds a row block of A, not its columns")
        c.comm_destroy()


# ---- 7. the path --------------------------------------------------------------------------------------------------------------------------------
def run_path(A, loss, prox_class, **kw):
    np.random.seed(2)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fa.path(A, loss, prox_class, backend="hip", **SC.PATH_OPTS, **kw)


def assert_same_points(got, want):
    assert len(got) == len(want) == SC.PATH_OPTS["n_mus"]
    for p, q in zip(got, want):
        assert p.mu == q.mu and p.iteration_count == q.iteration_count and tuple(p.certificate) == tuple(q.certificate) and p.gaps == q.gaps
        np.testing.assert_array_equal(p.solution, q.solution)


@pytest.mark.parametrize("screen", [False, True], ids=["plain", "screen"])
def test_the_device_path_is_the_path_on_the_host_standardised_matrix(screen):
    A, b = SC.path_problem()
    kept = A.copy()
    got = run_path(A, fa.LeastSquares(b), fa.Shrink, standardize=True, intercept=True, screen=screen)
    np.testing.assert_array_equal(A, kept)
    st = got[0].standardization
    Z = (A - st.means) / st.scales                       # from the device's own statistics: the bits the context held
    want = run_path(Z, fa.LeastSquares(b - b.mean()), fa.Shrink, screen=screen)
    assert_same_points(got, want)
    for p, q in zip(got, want):
        np.testing.assert_array_equal(p.coefficients, q.solution / st.scales)
        lhs, rhs = A @ p.coefficients + p.intercept, Z @ q.solution + b.mean()
        assert np.max(np.abs(lhs - rhs)) <= 1e-12 * np.max(np.abs(rhs))
        if screen:
            assert p.kept == q.kept and p.rounds == q.rounds
    assert not np.any(got[0].solution) and not np.any(got[0].coefficients) and got[0].intercept == b.mean()
    assert np.count_nonzero(got[-1].coefficients) >= 5 and got[-1].certificate.gap <= SC.PATH_OPTS["gap_tolerance"] * got[-1].certificate.f0
    host_means, host_scales, _ = preprocess.standardize(A)[1]
    assert np.all(np.abs(st.means - host_means) <= 1e-13 * np.abs(A).max(axis=0))      # (two orders of the same 64 additions)
    np.testing.assert_allclose(st.scales, host_scales, rtol=1e-13)
    if screen:
        assert any(p.kept < A.shape[1] for p in got)


@pytest.mark.parametrize("screen", [False, True], ids=["plain", "screen"])
def test_the_sparse_device_path_with_scaling_alone(screen):
    from scipy import sparse as sp
    S, b = SC.sparse_path_problem()
    got = run_path(S, fa.LeastSquares(b), fa.Shrink, standardize=True, screen=screen)
    st = got[0].standardization
    np.testing.assert_array_equal(st.means, np.zeros(S.shape[1]))
    C = S.tocsr()
    Z = sp.csr_matrix((C.data / st.scales[C.indices], C.indices, C.indptr), shape=C.shape)
    want = run_path(Z, fa.LeastSquares(b), fa.Shrink, screen=screen)
    assert_same_points(got, want)
    for p, q in zip(got, want):
        np.testing.assert_array_equal(p.coefficients, q.solution / st.scales)
        assert p.intercept == 0.0
        lhs, rhs = S @ p.coefficients, Z @ q.solution
        assert np.max(np.abs(lhs - rhs)) <= 1e-12 * max(np.max(np.abs(rhs)), 1e-300)
    assert not np.any(got[0].coefficients) and np.count_nonzero(got[-1].coefficients) >= 4


def test_what_the_standardised_path_refuses_on_the_device():
    for kw, words in SC.path_refusals(fa):
        with pytest.raises(TypeError) as err:
            fa.path(kw["A"], kw["loss"], fa.Shrink, n_mus=3, backend="hip", **{k: v for k, v in kw.items() if k not in ("A", "loss")})
        for w in words:
            assert w in str(err.value), (w, str(err.value))


def test_the_example_shows_the_difference(capsys):
    from fasta_python_amd.examples import lasso_path
    out = lasso_path.main(["--backend", "hip", "--rows", "40", "--features", "80", "--standardize", "--intercept"])
    text = capsys.readouterr().out
    assert "intercept" in text
    pts = out["adaptive"]
    assert len(pts) == 10 and all(hasattr(p, "coefficients") for p in pts) and pts[0].intercept != 0.0

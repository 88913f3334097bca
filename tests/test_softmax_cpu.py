"""CPU tier of the softmax loss over a matrix unknown (losses.SoftmaxLoss, fh_set_loss_softmax, csrc/fh_softmax.h): the fixtures
tests/golden/softmax/*.npz were captured from the reference core (scripts/make_softmax_golden.py) with SoftmaxLoss's host closures; the NumPy
oracle and the generic host loop must reproduce them bit for bit, the closures must be the fixed arithmetic, operand recognition must name
what the device does not serve, and a NumPy model of the row kernel's lanes must reproduce the closures.  No GPU."""
import glob
import os
import warnings

import numpy as np
import pytest
from scipy import sparse as sp

import fasta_python_amd as fa
from fasta_python_amd import hip, solver
from fasta_python_amd import stopping as fstop
from oracle import fasta_np as fo
from tests import helpers as H
from tests import softmax_cases as SC

FIELDS = ("residuals", "norm_residuals", "stepsizes", "objectives")


def assert_same_run(c, z):
    assert c.iteration_count == int(z["iteration_count"]) and c.backtracks == int(z["backtracks"])
    for field in FIELDS:
        if field in z.files:
            assert np.array_equal(getattr(c, field), z[field], equal_nan=True), field
    assert np.array_equal(c.solution, z["solution"])


# ---- the fixture set -----------------------------------------------------------------------------------------------------------------------
def test_the_fixture_set_is_the_one_the_script_describes():
    names = [row[0] for row in SC.capture_script().case_table()]
    on_disk = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(SC.GOLDEN, "*.npz")))
    assert sorted(names) == on_disk == sorted(SC.CASES)
    others = [p for p in glob.glob(os.path.join(H.GOLDEN, "**", "*.npz"), recursive=True) if os.path.dirname(p) != SC.GOLDEN]
    biggest = max(os.path.getsize(p) for p in others)                   # the largest fixture the project had before these
    assert all(os.path.getsize(os.path.join(SC.GOLDEN, n + ".npz")) <= biggest for n in SC.CASES)


def test_the_fixtures_have_the_shapes_and_properties_the_script_asserts():
    ms = SC.capture_script()
    for name, prox, ckw, pseed, sseed, opts, setup in ms.case_table():
        meta, z, d = SC.load(name)
        m, n, L = ckw["m"], ckw["n"], ckw["L"]
        assert tuple(ms.matrix_of(d).shape) == (m, n) and d["y"].shape == (m,) and int(d["classes"]) == L and z["solution"].shape == (n, L), name
        assert ("data" in d) == ("density" in ckw) and d["y"].min() >= 0 and d["y"].max() < L
        assert ("L" in meta["options"]) == (setup != "estimated") and meta["setup"] == setup

        class Run:
            iteration_count, backtracks, solution = int(z["iteration_count"]), int(z["backtracks"]), z["solution"]
        ms.check(name, prox, Run, meta["options"], setup)
    _, z, _ = SC.load("group_60x40x3_backtracks")
    assert int(z["backtracks"]) >= 1
    meta, _, d = SC.load("group_60x40x3_backtracks")
    assert meta["options"]["tau0"] == 40.0 * float((2 / ms.lipschitz(d)) / 10)


@pytest.mark.parametrize("name", SC.CASES)
def test_oracle_reproduces_the_reference_run_and_its_row_permuted_twin_never_parts(name):
    """Bit for bit; and the basis for holding the device to the WHOLE history: the stored iteration at which the twin parts is the last one."""
    meta, z, d = SC.load(name)
    ms = SC.capture_script()
    c = ms.run(fo, fo.LinearMap, meta["prox"], d, meta["options"], meta["solver_seed"])
    assert_same_run(c, z)
    assert ms.twin_divergence(meta["prox"], d, meta["options"], meta["solver_seed"]) == meta["twin_divergence"] == int(z["iteration_count"])


@pytest.mark.parametrize("name", SC.CASES)
def test_generic_loop_reproduces_the_reference_run(name):
    """fasta(A, A.T, sm.f, sm.gradf, reg.g, reg.prox, X0, backend="numpy") on the raw matrix, SparseMatrixMap(S, rhs=L) for the sparse cases."""
    meta, z, d = SC.load(name)
    ms = SC.capture_script()
    A = ms.matrix_of(d)
    L = int(d["classes"])
    loss, reg = ms.tags(meta["prox"], d)
    g, proxg = (None, None) if reg is None else (reg.g, reg.prox)
    op = fa.SparseMatrixMap(A, rhs=L) if sp.issparse(A) else A
    At = op.H if sp.issparse(A) else A.T
    np.random.seed(meta["solver_seed"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        c = fa.fasta(op, At, loss.f, loss.gradf, g, proxg, np.zeros((A.shape[1], L)), backend="numpy", verbose=False, **ms.resolve(meta["options"], fstop))
    assert_same_run(c, z)


# ---- the closures --------------------------------------------------------------------------------------------------------------------------
def _random_case(m, L, seed, scale=3.0):
    rng = np.random.RandomState(seed)
    return rng.randn(m, L) * scale, rng.randint(0, L, m)


@pytest.mark.parametrize("L", SC.ALL_L)
def test_f_and_gradf_against_a_longdouble_evaluation(L):
    Z, y = _random_case(97, L, 10 + L, scale=10.0)
    sm = fa.SoftmaxLoss(y, classes=L)
    R, terms, mags = SC.longdouble_rows(Z, y)
    err = np.abs(sm.gradf(Z).astype(np.longdouble) - R).max()
    assert err <= SC.residual_bound(L), (float(err), SC.residual_bound(L))
    assert abs(np.longdouble(sm.f(Z)) - terms.sum()) <= SC.loss_bound(97, L, mags)
    assert sm(Z) == sm.f(Z) and sm.f_from_device(3.25) == np.float64(3.25) and isinstance(sm.f_from_device(1.0), np.float64)


@pytest.mark.parametrize("L", [2, 5, 16])
def test_gradf_against_central_differences_of_f(L):
    """1e-6 relative at step 1e-6 on unit-scale data: truncation O(h^2), rounding about eps |f| / h ~ 1e-9 at f ~ 30."""
    Z, y = _random_case(20, L, 20 + L, scale=1.0)
    sm = fa.SoftmaxLoss(y, classes=L)
    G = sm.gradf(Z)
    h = 1e-6
    num = np.zeros_like(Z)
    for i in range(Z.shape[0]):
        for l in range(L):
            E = np.zeros_like(Z)
            E[i, l] = h
            num[i, l] = (sm.f(Z + E) - sm.f(Z - E)) / (2 * h)
    assert np.abs(num - G).max() <= 1e-6 * np.abs(G).max()


def test_the_800_row_is_finite_and_exact():
    Z = np.array([[800.0, -800.0], [-800.0, 800.0]])
    for y, want in ((np.array([0, 1]), 0.0), (np.array([1, 0]), 3200.0), (np.array([0, 0]), 1600.0)):
        sm = fa.SoftmaxLoss(y, classes=2)
        assert np.array_equal(sm.gradf(Z) + sm.Y, np.array([[1.0, 0.0], [0.0, 1.0]]))
        assert sm.f(Z) == want
    one = fa.SoftmaxLoss(np.array([1]), classes=2)
    assert one.f(Z[:1]) == 1600.0 and np.array_equal(one.gradf(Z[:1]), np.array([[1.0, -1.0]]))


@pytest.mark.parametrize("L", range(2, 17))
def test_constant_rows_give_the_rounded_reciprocal_exactly(L):
    y = np.arange(7) % L
    sm = fa.SoftmaxLoss(y, classes=L)
    for v in (0.0, -3.5, 700.0):
        G = sm.gradf(np.full((7, L), v))
        assert np.array_equal(G, np.float64(1.0) / np.float64(L) - sm.Y), (L, v)
        assert sm.f(np.full((7, L), v)) == np.sum((v + np.log(np.full(7, float(L)))) - v)


def test_the_one_hot_matrix_and_the_device_binding():
    y = np.array([2, 0, 1, 2])
    sm = fa.SoftmaxLoss(y)
    assert sm.classes == 3 and np.array_equal(sm.Y, np.eye(3)[y]) and sm.b is sm.Y and sm.Y.dtype == np.float64
    assert fa.SoftmaxLoss(y, classes=5).Y.shape == (4, 5)

    class Ctx:
        def set_loss_softmax(self, labels):
            self.got = labels
    c = Ctx()
    sm.bind(c)
    assert np.array_equal(c.got, y)
    import fasta
    assert fasta.SoftmaxLoss is fa.SoftmaxLoss is fa.losses.SoftmaxLoss and "SoftmaxLoss" in fa.__all__ and "SoftmaxLoss" in fa.losses.__all__


@pytest.mark.parametrize("y,classes,msg", [
    (np.array([0.0, 1.0]), None, "integer"), (np.array([[0, 1]]), None, "1-D"), (np.array([], dtype=int), None, "non-empty"),
    (np.array([0, -1]), None, ">= 0"), (np.array([0, 0]), None, "2 to 16"), (np.array([0, 16]), None, "2 to 16"), (np.array([0, 1]), 17, "2 to 16"),
    (np.array([0, 1]), 1, "2 to 16"), (np.array([0, 3]), 3, "below classes"),
])
def test_argument_validation(y, classes, msg):
    with pytest.raises(ValueError, match=msg):
        fa.SoftmaxLoss(y, classes=classes)


def test_a_matrix_of_another_shape_is_refused_by_the_closures():
    sm = fa.SoftmaxLoss(np.array([0, 1, 2]))
    with pytest.raises(ValueError, match="shape"):
        sm.f(np.zeros((3, 2)))
    with pytest.raises(ValueError, match="shape"):
        sm.gradf(np.zeros(3))


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------------
def test_the_entry_point_is_in_the_header_the_library_and_the_binding():
    import ctypes as C
    lib = hip.load_library()
    assert hip.SIGNATURES["fh_set_loss_softmax"] == (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_uint64])
    assert hasattr(lib, "fh_set_loss_softmax")
    text = open(os.path.join(SC.ROOT, "include", "fasta_hip.h")).read()
    assert "int fh_set_loss_softmax(fh_ctx* ctx, const int32_t* labels, uint64_t m);" in text
    assert lib.fh_set_loss_softmax(None, None, 0) == hip.E_ARG


# ---- recognition ---------------------------------------------------------------------------------------------------------------------------
def _operands(m=6, n=9, L=3):
    rng = np.random.RandomState(1)
    return rng.randn(m, n), fa.SoftmaxLoss(np.arange(m) % L, classes=L), np.zeros((n, L))


def test_the_matrix_forms_are_recognised():
    A, sm, x0 = _operands()
    S = sp.csr_matrix(A * (np.abs(A) > 0.5))
    for reg in (fa.Shrink(0.1), fa.NonNeg(), fa.Box(-1.0, 1.0), fa.GroupShrink(0.1), None):
        g, proxg = (None, None) if reg is None else (reg.g, reg.prox)
        for op in (A, fa.DenseMatrixMap(A, rhs=3), fa.SparseMatrixMap(S, rhs=3)):
            assert solver._unrecognised(op, None, sm.f, sm.gradf, g, proxg, x0) is None, (type(reg).__name__, type(op).__name__)
    op = fa.SparseMatrixMap(S, rhs=3)
    got, loss, prox = solver._recognise(op, op.H, sm.f, sm.gradf, None, None, x0)
    assert got is op and loss is sm and type(prox) is fa.NoProx and op._ctx is None


def _why(A, sm, x0, reg=None, At=None):
    g, proxg = (None, None) if reg is None else (reg.g, reg.prox)
    return solver._unrecognised(A, At, sm.f, sm.gradf, g, proxg, x0)


def test_every_refusal_names_the_loss_and_the_reason():
    A, sm, x0 = _operands()
    S = sp.csr_matrix(A)
    for why, words in (
            (_why(A, sm, np.zeros(9)), ("MATRIX unknown", "(9,)")),
            (_why(A, fa.SoftmaxLoss(np.arange(6) % 3, classes=4), x0), ("4 classes", "3 columns")),
            (_why(fa.DenseMatrixMap(A, rhs=4), sm, np.zeros((9, 4))), ("3 classes", "4 columns")),
            (_why(fa.DenseMatrixMap(A), sm, x0), ("rhs=3",)),
            (_why(fa.SparseMatrixMap(S), sm, x0), ("rhs=3",)),
            (_why(fa.DenseMatrixMap(A, storage="f32"), sm, x0), ('storage="f32"',)),
            (_why(fa.ShardedDenseMatrixMap(A, devices=(0, 0)), sm, x0), ("row-sharded",)),
            (_why(fa.DCTMap(6, lazy=True), sm, x0), ("DCT",)),
            (_why(object.__new__(fa.GradDivMap), sm, x0), ("stencil",)),      # (its constructor opens a device context: the type alone decides here)
            (_why(fa.IdentityMap((6, 3)), sm, np.zeros((6, 3))), ("identity",)),
            (_why(None, sm, np.zeros((6, 3))), ("identity", "A=None")),
            (_why(lambda X: A @ X, sm, x0, At=lambda Y: A.T @ Y), ("not device-resident",))):
        assert why is not None and "SoftmaxLoss" in why and all(w in why for w in words), why
    for reg in (fa.LinfProx(1.0), fa.L1Ball(1.0), fa.TVDualBall(), fa.RowBall(1.0), fa.RowSplit(3, fa.Shrink(0.1), fa.NonNeg()), fa.NuclearShrink(0.1)):
        why = _why(A, sm, x0, reg)
        assert why is not None and "SoftmaxLoss" in why and type(reg).__name__ in why, why
    other = fa.SoftmaxLoss(np.arange(6) % 3)
    assert "one losses.SoftmaxLoss" in solver._unrecognised(A, None, sm.f, other.gradf, None, None, x0)
    assert "SoftmaxLoss" in solver._unrecognised(A, None, sm.f, sm.gradf, (lambda X: 0.0), (lambda X, t: X), x0)


def test_a_raw_sparse_matrix_with_a_2d_x0_keeps_its_sentence():
    A, sm, x0 = _operands()
    ls = fa.LeastSquares(np.zeros((6, 3)))
    S = sp.csr_matrix(A)
    assert _why(S, sm, x0) == solver._unrecognised(S, None, ls.f, ls.gradf, None, None, x0) and "SparseMatrixMap(S, rhs=L)" in _why(S, sm, x0)


def test_backend_hip_raises_with_the_sentence_and_the_default_backend_takes_the_host_loop():
    A, sm, x0 = _operands()
    reg = fa.L1Ball(1.0)
    with pytest.raises(TypeError, match="L1Ball is not served with losses.SoftmaxLoss"):
        fa.fasta(A, A.T, sm.f, sm.gradf, reg.g, reg.prox, x0, backend="hip", verbose=False)
    with pytest.raises(TypeError, match="MATRIX unknown"):
        fa.fasta(A, A.T, sm.f, sm.gradf, None, None, np.zeros(9), backend="hip", verbose=False)
    shr = fa.Shrink(0.1)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        np.random.seed(3)
        c = fa.fasta(sp.csr_matrix(A), sm.f, sm.gradf, shr.g, shr.prox, x0, verbose=False, max_iters=5)      # refused (raw sparse, 2-D x0): the generic host loop
    assert c.iteration_count >= 1 and c.solution.shape == (9, 3)


def test_the_logistic_sentences_are_still_produced():
    A, _, x0 = _operands()
    lg = fa.LogisticLoss(np.ones((6, 3)))
    assert solver._unrecognised(A, None, lg.f, lg.gradf, None, None, x0) == "losses.LogisticLoss has no matrix (multi-column) form on the device"
    why = solver._unrecognised(fa.SparseMatrixMap(sp.csr_matrix(A), rhs=3), None, lg.f, lg.gradf, None, None, x0)
    assert why == "losses.LogisticLoss has no matrix (multi-column) form over a sparse operator on the device: least squares only"


def test_no_gpu_is_an_error_not_a_fallback():
    try:
        n = hip.device_count()
    except hip.HipError:
        n = 0
    if n:
        return                                           # (with a GPU the same call is tests/test_gpu_softmax.py's business)
    A, sm, x0 = _operands()
    with pytest.raises(hip.HipError):
        fa.fasta(A, A.T, sm.f, sm.gradf, None, None, x0, verbose=False)


# ---- the example ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sparse", [None, 0.2])
def test_the_example_constructs_its_problem_from_its_seed(sparse):
    from fasta_python_amd.examples.multiclass_logistic import MulticlassLogisticProblem as P
    a, x0 = P.construct(M=40, N=24, L=3, K=4, sparse=sparse, group=True, seed=5, backend="numpy")
    b, _ = P.construct(M=40, N=24, L=3, K=4, sparse=sparse, group=True, seed=5, backend="numpy")
    other, _ = P.construct(M=40, N=24, L=3, K=4, sparse=sparse, group=True, seed=6, backend="numpy")
    dense = lambda M: M.toarray() if sp.issparse(M) else M
    assert np.array_equal(dense(a.A), dense(b.A)) and np.array_equal(a.y, b.y) and a.mu == b.mu and np.array_equal(a.X, b.X)
    assert not np.array_equal(dense(a.A), dense(other.A))
    assert a.is_sparse == (sparse is not None) and x0.shape == (24, 3) and a.y.min() >= 0 and a.y.max() < 3 and len(set(a.y)) == 3
    np.random.seed(1)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sol, c = a.solve(x0, dict(tolerance=1e-4, max_iters=300))
    live = np.abs(sol).sum(axis=1) != 0
    assert c.iteration_count < 300 and live.any() and not live.all()


# ---- the kernel's lanes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", SC.ALL_L)
@pytest.mark.parametrize("m", [1, 33, 97])
def test_the_lane_model_of_the_kernel_reproduces_the_closures(m, L):
    """The row sums of the kernel are left to right over the valid columns: residual and per-row terms bit for bit.  The loss adds the rows'
    terms in the workgroup's tree order, the host pairwise: within the bound of the issue."""
    Z, y = _random_case(m, L, 100 * m + L, scale=8.0)
    sm = fa.SoftmaxLoss(y, classes=L)
    R, terms, rec, loss = SC.kernel_model(Z, y, L)
    LB = SC.lb_of(L)
    assert R.shape == (m, LB) and np.array_equal(R[:, :L], sm.gradf(Z)) and not R[:, L:].any()
    mx = Z.max(axis=1)
    s = np.exp(Z - mx[:, None])[:, 0].copy()
    for l in range(1, L):
        s += np.exp(Z - mx[:, None])[:, l]
    assert np.array_equal(terms, (mx + np.log(s)) - Z[np.arange(m), y])
    assert rec.size == (m * (LB // 2) + 255) // 256
    if (m, L) == (97, 16):
        assert rec.size == 4                               # several workgroups: the ordered finaliser sees more than one record
    _, _, mags = SC.longdouble_rows(Z, y)
    assert abs(loss - sm.f(Z)) <= SC.loss_bound(m, L, mags)


def test_the_lane_model_extrapolates_like_the_kernel():
    Z, y = _random_case(33, 5, 7)
    Z0 = np.random.RandomState(8).randn(33, 5)
    sm = fa.SoftmaxLoss(y, classes=5)
    R, _, _, _ = SC.kernel_model(Z, y, 5, zacc0=Z0, coef=0.37)
    assert np.array_equal(R[:, :5], sm.gradf(Z + 0.37 * (Z - Z0)))

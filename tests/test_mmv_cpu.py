"""CPU tier of the matrix-unknown (MMV) form: the fixtures tests/golden/mmv/*.npz were captured from the reference core
(scripts/make_mmv_golden.py); the NumPy oracle, the GroupShrink tag and the generic host loop must reproduce them bit for bit, the
operand recognition must ask the context for `rhs = L`, and the binding must know the two new entry points.  No GPU."""
import ctypes as C
import glob
import json
import os
import warnings

import numpy as np
import pytest
from numpy import linalg as la

import fasta_python_amd as fa
from fasta_python_amd import hip, solver
from oracle import fasta_np as fo
from tests import helpers as H
from tests.fake_ctx import FakeContext

MMV = os.path.join(H.GOLDEN, "mmv")
CASES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(MMV, "*.npz")))
FIELDS = ("residuals", "norm_residuals", "stepsizes", "objectives")


def load(name):
    z = np.load(os.path.join(MMV, name + ".npz"), allow_pickle=False)
    return json.loads(str(z["meta"])), z


def _capture_script():
    """scripts/make_mmv_golden.py as a module: the ONE place that states the closures the fixtures were captured with."""
    import importlib.util
    path = os.path.join(os.path.dirname(H.GOLDEN), os.pardir, "scripts", "make_mmv_golden.py")
    spec = importlib.util.spec_from_file_location("make_mmv_golden", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def closures(A, B, mu):
    """The closures the fixtures were captured with, over the oracle's shrink."""
    return _capture_script().closures(dict(A=A, B=B, mu=mu), fo.shrink)


def oracle_run(z, meta, A=None):
    A = z["in_A"] if A is None else A
    B, mu = z["in_B"], float(z["in_mu"])
    (M, N), L = A.shape, B.shape[1]
    f, gradf, g, proxg = closures(A, B, mu)
    op = fo.LinearMap(lambda X: A @ X, lambda Y: A.T @ Y, (N, L), (M, L))
    np.random.seed(meta["solver_seed"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fo.fasta(op, f, gradf, g, proxg, np.zeros((N, L)), **meta["options"])


def assert_same_run(c, z):
    assert c.iteration_count == int(z["iteration_count"]) and c.backtracks == int(z["backtracks"])
    for field in FIELDS:
        if field in z.files:
            assert np.array_equal(getattr(c, field), z[field], equal_nan=True), field
    assert np.array_equal(c.solution, z["solution"])


def test_the_five_fixtures_are_there():
    assert len(CASES) == 5 and not any(n.startswith("mmv") for n in H.golden_cases())


@pytest.mark.parametrize("name", CASES)
def test_oracle_reproduces_the_reference_bitwise(name):
    meta, z = load(name)
    assert_same_run(oracle_run(z, meta), z)


@pytest.mark.parametrize("name", CASES)
def test_group_shrink_on_host_arrays_is_the_fixtures_closures_bitwise(name):
    meta, z = load(name)
    mu = float(z["in_mu"])
    _, _, g, proxg = closures(z["in_A"], z["in_B"], mu)
    tag = fa.GroupShrink(mu)
    rng = np.random.RandomState(2)
    for X in (z["in_X"], z["solution"], rng.randn(*z["in_X"].shape), np.zeros_like(z["in_X"])):
        for t in (0.01, 0.7, 3.0):
            assert np.array_equal(tag.prox(X, t), proxg(X, t)) and np.array_equal(tag(X, t), proxg(X, t))
        assert tag.g(X) == g(X)
    assert tag.g_from_sums(2.5, 9.0) == mu * 2.5 and tag.kind == hip.PROX_GROUP == 7


@pytest.mark.parametrize("name", CASES)
def test_host_loop_with_group_shrink_reproduces_the_fixtures_bitwise(name):
    meta, z = load(name)
    A, B = z["in_A"], z["in_B"]
    ls, reg = fa.LeastSquares(B), fa.GroupShrink(float(z["in_mu"]))
    np.random.seed(meta["solver_seed"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        c = fa.fasta(A, A.T, ls.f, ls.gradf, reg.g, reg.prox, np.zeros((A.shape[1], B.shape[1])), backend="numpy", verbose=False,
                     **meta["options"])
    assert_same_run(c, z)


def test_backtracking_fixture_records_where_the_oracle_parts_from_a_permuted_copy_of_itself():
    """How far summation order alone lets two correct solvers agree on the backtracking run: the oracle on the problem against the oracle
    on the same problem with its unknowns permuted (columns of A; the rows of X follow).  tests/test_gpu_mmv.py pins the device run up to
    the iteration stored in the fixture's meta; it is recomputed here, not guessed."""
    meta, z = load("mmv_20x30x10_backtracks")
    assert int(z["backtracks"]) >= 10
    a = oracle_run(z, meta)
    perm = np.random.RandomState(7).permutation(z["in_A"].shape[1])
    b = oracle_run(z, meta, A=np.ascontiguousarray(z["in_A"][:, perm]))
    k = min(a.iteration_count, b.iteration_count)
    first = H.first_divergence(b.stepsizes, a.stepsizes, k)
    assert first == meta["permuted_divergence"]
    assert first >= 25                                     # (the vector fixtures of this kind are pinned for 25 iterations)


# ---- recognition -------------------------------------------------------------------------------------------------------------------------
class RecordingContext(FakeContext):
    """Stand-in for hip.HipContext that records what DenseMatrixMap asks of it."""
    made = []

    def __init__(self, device=0, storage="f64", devices=None, rccl_shell=False):
        FakeContext.__init__(self, None, None, (0,), (0,))
        self.matrix, self.rhs_asked = None, None
        RecordingContext.made.append(self)

    def set_tuning(self, key, value):
        pass

    def set_matrix(self, A):
        self.matrix = A

    def set_rhs(self, L):
        self.rhs_asked = L


def test_a_two_dimensional_x0_builds_the_map_with_rhs(monkeypatch):
    monkeypatch.setattr(hip, "HipContext", RecordingContext)
    RecordingContext.made.clear()
    rng = np.random.RandomState(0)
    A, B = rng.randn(12, 9), rng.randn(12, 4)
    ls, reg = fa.LeastSquares(B), fa.GroupShrink(0.5)
    X0 = np.zeros((9, 4))
    assert solver._unrecognised(A, A.T, ls.f, ls.gradf, reg.g, reg.prox, X0) is None
    op, loss, prox = solver._recognise(A, A.T, ls.f, ls.gradf, reg.g, reg.prox, X0)
    assert isinstance(op, fa.DenseMatrixMap) and op.rhs == 4 and op.Vshape == (9, 4) and op.Wshape == (12, 4) and prox is reg
    ctx = op.ctx                                            # first use: the upload, then rhs = L
    assert ctx is RecordingContext.made[-1] and ctx.matrix is A and ctx.rhs_asked == 4
    assert np.array_equal(op(X0 + 1.0), A @ (X0 + 1.0)) and np.array_equal(op.H(B), A.T @ B)      # host closures work on matrices
    # a DenseMatrixMap whose Vshape already matches is taken as it is
    same, _, _ = solver._recognise(op, op.H, ls.f, ls.gradf, reg.g, reg.prox, X0)
    assert same is op
    # a vector x0 keeps the vector form: no set_rhs
    lv, rv = fa.LeastSquares(B[:, 0].copy()), fa.Shrink(0.5)
    opv, _, _ = solver._recognise(A, A.T, lv.f, lv.gradf, rv.g, rv.prox, np.zeros(9))
    assert opv.rhs is None and opv.ctx.rhs_asked is None and opv.Vshape == (9,)
    # any other mismatch keeps today's AssertionError
    with pytest.raises(AssertionError, match="x0 has shape"):
        solver._recognise(A, A.T, ls.f, ls.gradf, reg.g, reg.prox, np.zeros((8, 4)))
    with pytest.raises(AssertionError, match="x0 has shape"):
        solver._recognise(opv, opv.H, ls.f, ls.gradf, reg.g, reg.prox, X0)
    with pytest.raises(AssertionError, match="b has shape"):
        solver._recognise(A, A.T, lv.f, lv.gradf, reg.g, reg.prox, X0)


def test_operands_without_a_matrix_form_take_the_host_loop_or_raise():
    rng = np.random.RandomState(1)
    A, B = rng.randn(14, 10), rng.randn(14, 3)
    X0 = np.zeros((10, 3))
    ls = fa.LeastSquares(B)
    refused = [("LinfProx", A, ls, fa.LinfProx(0.1)), ("L1Ball", A, ls, fa.L1Ball(1.0)),
               ("LogisticLoss", A, fa.LogisticLoss(np.sign(B)), fa.Shrink(0.1)),
               ('storage="f32"', fa.DenseMatrixMap(A, storage="f32"), ls, fa.Shrink(0.1)),
               ("row-sharded", fa.ShardedDenseMatrixMap(A, devices=[0, 0]), ls, fa.Shrink(0.1))]
    for word, op, loss, reg in refused:
        why = solver._unrecognised(op, None, loss.f, loss.gradf, reg.g, reg.prox, X0)
        assert why is not None and word in why, (word, why)
        with pytest.raises(TypeError, match="backend='hip'"):
            fa.fasta(op, loss.f, loss.gradf, reg.g, reg.prox, X0, backend="hip", verbose=False)
    # backend="auto": the generic host loop, as for any unrecognisable operand (no GPU is touched)
    reg = fa.L1Ball(1.0)
    prox_cols = lambda X, t: np.stack([reg.prox(X[:, j], t) for j in range(X.shape[1])], axis=1)
    c = fa.fasta(A, A.T, ls.f, ls.gradf, lambda X: 0, prox_cols, X0, verbose=False, max_iters=5)
    assert c.solution.shape == (10, 3)
    wide = np.zeros((10, 17))                                # more columns than the device keeps per row
    lw = fa.LeastSquares(rng.randn(14, 17))
    assert "at most 16" in solver._unrecognised(A, A.T, lw.f, lw.gradf, None, None, wide)
    gs = fa.GroupShrink(0.2)
    lv = fa.LeastSquares(B[:, 0].copy())
    assert "GroupShrink" in solver._unrecognised(A, A.T, lv.f, lv.gradf, gs.g, gs.prox, np.zeros(10))
    with pytest.raises(ValueError):
        fa.DenseMatrixMap(A, rhs=17)
    with pytest.raises(TypeError):
        fa.DenseMatrixMap(A, rhs=2, storage="f32")


def test_example_constructs_the_fixture_inputs():
    from fasta_python_amd.examples.mmv import MMVProblem
    for name in ("mmv_20x30x10_adaptive", "mmv_64x128x5_objective"):
        meta, z = load(name)
        P, X0 = MMVProblem.construct(seed=meta["problem_seed"], backend="numpy", **meta["construct"])
        assert np.array_equal(P.A, z["in_A"]) and np.array_equal(P.B, z["in_B"]) and np.array_equal(P.X, z["in_X"]) and P.mu == float(z["in_mu"])
        assert X0.shape == z["in_X"].shape and not X0.any()
    P, X0 = MMVProblem.construct(seed=1)
    assert P.A.shape == (20, 30) and P.B.shape == (20, 10) and X0.shape == (30, 10) and int((la.norm(P.X, axis=1) > 0).sum()) == 7
    meta, z = load("mmv_20x30x10_adaptive")
    P, X0 = MMVProblem.construct(seed=meta["problem_seed"], backend="numpy")
    np.random.seed(meta["solver_seed"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sol, c = P.solve(X0, dict(meta["options"]))
    assert_same_run(c, z)
    import fasta
    assert fasta.GroupShrink is fa.GroupShrink and fasta.examples.mmv.MMVProblem is MMVProblem


# ---- C ABI (no device needed) ----------------------------------------------------------------------------------------------------------
def test_binding_knows_the_multi_column_entry_points():
    lib = hip.load_library()
    assert hip.SIGNATURES["fh_set_rhs"] == (C.c_int, [C.c_void_p, C.c_uint32])
    assert hip.SIGNATURES["fh_rhs"] == (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32)])
    text = open(os.path.join(os.path.dirname(H.GOLDEN), os.pardir, "include", "fasta_hip.h")).read()
    assert "FH_PROX_GROUP    = 7" in text and hip.PROX_GROUP == 7 and hip.MAX_RHS == 16
    assert "int fh_set_rhs(fh_ctx* ctx, uint32_t L);" in text and "int fh_rhs(fh_ctx* ctx, uint32_t* L);" in text
    # a null context is refused with a message, not dereferenced
    L = C.c_uint32(99)
    assert lib.fh_set_rhs(None, 4) == hip.E_ARG and lib.fh_last_error()
    assert lib.fh_rhs(None, C.byref(L)) == hip.E_ARG


def test_new_kernels_have_no_scratch_traffic_inside_loops():
    """scripts/loop_spills.py over the default instantiations of both new kernels (make -C fasta_python_amd/csrc multi-spills).  Needs
    hipcc, as the build does: a box without it fails here, it does not skip the only guard on loop spills of these kernels."""
    import subprocess
    import sys
    root = os.path.join(os.path.dirname(H.GOLDEN), os.pardir)
    r = subprocess.run(["make", "-s", "-C", os.path.join(root, "fasta_python_amd", "csrc"), "multi-spills", f"PYTHON={sys.executable}"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "k_mc_fwd" in r.stdout and "k_mc_adj" in r.stdout

"""CPU tier of the sparse operator (fh_set_matrix_csr, csrc/fh_sparse.h): the fixtures tests/golden/sparse/*.npz were captured from the
reference core (scripts/make_sparse_golden.py) with the closure LinearMap `S @ x` / `S.T @ y`; the NumPy oracle and the generic host loop
over a SparseMatrixMap must reproduce them bit for bit, the map must canonicalise what it is given, operand recognition must name what
the device does not serve, and nothing may fall back when there is no GPU.  No GPU."""
import glob
import json
import os
import shutil
import subprocess
import sys
import warnings

import numpy as np
import pytest
from scipy import sparse as sp

import fasta_python_amd as fa
from fasta_python_amd import hip, linalg, solver
from fasta_python_amd import stopping as fstop
from oracle import fasta_np as fo
from tests import helpers as H

SPARSE = os.path.join(H.GOLDEN, "sparse")
CASES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(SPARSE, "*.npz")))
FIELDS = ("residuals", "norm_residuals", "stepsizes", "objectives")


def capture_script():
    """scripts/make_sparse_golden.py as a module: the ONE place that states the closures the fixtures were captured with."""
    import importlib.util
    path = os.path.join(os.path.dirname(H.GOLDEN), os.pardir, "scripts", "make_sparse_golden.py")
    spec = importlib.util.spec_from_file_location("make_sparse_golden", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def load(name):
    z = np.load(os.path.join(SPARSE, name + ".npz"), allow_pickle=False)
    meta = json.loads(str(z["meta"]))
    return meta, z, {k[3:]: z[k] for k in z.files if k.startswith("in_")}


def assert_same_run(c, z):
    assert c.iteration_count == int(z["iteration_count"]) and c.backtracks == int(z["backtracks"])
    for field in FIELDS:
        if field in z.files:
            assert np.array_equal(getattr(c, field), z[field], equal_nan=True), field
    assert np.array_equal(c.solution, z["solution"])


def test_the_fixture_set_is_the_one_the_script_describes():
    names = [row[0] for row in capture_script().case_table()]
    assert sorted(names) == CASES and len(CASES) == 15
    biggest = max(os.path.getsize(p) for p in glob.glob(os.path.join(H.GOLDEN, "*.npz")))
    assert all(os.path.getsize(os.path.join(SPARSE, n + ".npz")) <= biggest for n in CASES)


def test_the_skewed_matrix_is_skewed():
    _, _, d = load("skewed_257x515")
    S = capture_script().matrix_of(d)
    assert S.shape == (257, 515)
    per_row, per_col = np.diff(S.indptr), np.diff(S.tocsc().indptr)
    assert (per_row == 0).sum() == 10 and (per_col == 0).sum() == 10
    assert per_row.max() == 505 and per_col.max() == 247          # every live column / every non-empty row
    assert set(np.delete(per_row, [int(per_row.argmax())])) <= {0, 1, 2, 3}


@pytest.mark.parametrize("name", CASES)
def test_oracle_reproduces_the_reference_run(name):
    meta, z, d = load(name)
    ms = capture_script()
    c = ms.run(fo, fo.LinearMap, fo.shrink, meta["kind"], d, meta["options"], meta["solver_seed"])
    assert_same_run(c, z)


@pytest.mark.parametrize("name", CASES)
def test_generic_loop_over_a_sparse_map_reproduces_the_reference_run(name):
    """fasta(SparseMatrixMap(S), ..., backend="numpy"): the map applied to host arrays is `S @ v` / `S.T @ w`, the reference's closures."""
    meta, z, d = load(name)
    ms = capture_script()
    f, gradf, g, proxg = ms.closures(meta["kind"], d, fa.proximal.shrink)
    op = fa.SparseMatrixMap(ms.matrix_of(d))
    np.random.seed(meta["solver_seed"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        c = fa.fasta(op, f, gradf, g, proxg, np.zeros(op.shape[1]), backend="numpy", verbose=False, **ms.resolve(meta["options"], fstop))
    assert op._ctx is None                                     # the host loop never asked for a device context
    assert_same_run(c, z)


def test_backtracking_fixture_records_where_a_permuted_copy_parts():
    meta, z, d = load("lasso_100x200_backtracks")
    ms = capture_script()
    assert int(z["backtracks"]) >= 5
    assert ms.permuted_divergence(meta["kind"], d, meta["options"], meta["solver_seed"]) == meta["permuted_divergence"]
    assert 10 <= meta["permuted_divergence"] <= int(z["iteration_count"])
    cut = ms.run(fo, fo.LinearMap, fo.shrink, meta["kind"], d, dict(meta["options"], max_iters=meta["permuted_divergence"], tolerance=0.0), meta["solver_seed"])
    assert cut.backtracks == meta["backtracks_at_divergence"] <= int(z["backtracks"])


@pytest.mark.parametrize("name", [n for n in CASES if "backtracks" not in n])
def test_full_length_fixtures_do_not_depend_on_summation_order(name):
    """The basis for holding the device to the WHOLE history of these runs: the oracle and its row-permuted twin never part."""
    meta, z, d = load(name)
    assert capture_script().row_permuted_divergence(meta["kind"], d, meta["options"], meta["solver_seed"]) == int(z["iteration_count"])


# ---- canonicalisation ----------------------------------------------------------------------------------------------------------------------
def _same_csr(a, b):
    return all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(a.csr, b.csr)) and a.shape == b.shape


def test_every_input_format_gives_the_same_canonical_csr():
    rng = np.random.RandomState(3)
    S = sp.random(40, 70, density=0.1, format="csr", random_state=rng, data_rvs=rng.standard_normal)
    S.sort_indices()
    want = fa.SparseMatrixMap(S)
    assert want.csr[0].dtype == np.float64 and want.csr[1].dtype == np.int32 and want.csr[2].dtype == np.int64
    assert want.nnz == S.nnz and want.shape == (40, 70) and want.Vshape == (70,) and want.Wshape == (40,)
    coo = S.tocoo()
    perm = rng.permutation(coo.nnz)
    shuffled = sp.coo_matrix((coo.data[perm], (coo.row[perm], coo.col[perm])), shape=S.shape)
    # duplicated: every entry split into two halves
    dup = sp.coo_matrix((np.concatenate([coo.data / 2, coo.data / 2]), (np.concatenate([coo.row, coo.row]), np.concatenate([coo.col, coo.col]))), shape=S.shape)
    unsorted = S.copy()
    for i in range(S.shape[0]):                                # reverse every row's entries in place: same matrix, unsorted indices
        lo, hi = unsorted.indptr[i], unsorted.indptr[i + 1]
        unsorted.indices[lo:hi] = unsorted.indices[lo:hi][::-1].copy()
        unsorted.data[lo:hi] = unsorted.data[lo:hi][::-1].copy()
    unsorted.has_sorted_indices = False
    for other in (S.tocsc(), shuffled, dup, unsorted, S.tolil(), sp.csr_array(S) if hasattr(sp, "csr_array") else S):
        assert _same_csr(fa.SparseMatrixMap(other), want), type(other).__name__
    assert _same_csr(fa.SparseMatrixMap(((S.data, S.indices, S.indptr), S.shape)), want)
    assert _same_csr(fa.SparseMatrixMap(((S.data, S.indices.astype(np.int64), S.indptr.astype(np.int32)), S.shape)), want)
    assert not unsorted.has_sorted_indices and dup.nnz == 2 * S.nnz      # the caller's matrices are left as they were


def test_explicit_zeros_are_kept_and_the_host_map_is_the_closure_pair():
    S = sp.csr_matrix((np.array([1.0, 0.0, 2.0]), np.array([0, 2, 1]), np.array([0, 2, 3])), shape=(2, 3))
    op = fa.SparseMatrixMap(S)
    assert op.nnz == 3
    v, w = np.array([1.0, 2.0, 3.0]), np.array([-1.0, 4.0])
    assert np.array_equal(op(v), S @ v) and np.array_equal(op.H(w), S.T @ w) and np.array_equal(op.T(w), S.T @ w)
    assert op.H.Vshape == (2,) and op.H.Wshape == (3,)


def test_wide_indices_are_narrowed_or_refused():
    data, indptr = np.ones(2), np.array([0, 2], dtype=np.int64)
    op = fa.SparseMatrixMap(((data, np.array([5, 2 ** 31 - 2], dtype=np.int64), indptr), (1, 2 ** 31 - 1)))
    assert op.csr[1].dtype == np.int32 and op.csr[1][1] == 2 ** 31 - 2
    with pytest.raises(ValueError, match="2\\^31"):
        fa.SparseMatrixMap(((data, np.array([5, 2 ** 31 + 4], dtype=np.int64), indptr), (1, 2 ** 33)))
    with pytest.raises(ValueError, match="out of range"):
        fa.SparseMatrixMap(((data, np.array([5, 9], dtype=np.int64), indptr), (1, 9)))


@pytest.mark.parametrize("triple,shape,what", [
    ((np.ones(2), np.array([1, 0]), np.array([0, 2])), (1, 3), "row 0"),                 # unsorted
    ((np.ones(3), np.array([0, 1, 1]), np.array([0, 1, 3])), (2, 3), "row 1"),           # duplicate
    ((np.ones(2), np.array([0, 1]), np.array([0, 2, 1])), (2, 3), "indptr"),             # decreasing
    ((np.ones(2), np.array([0, 1]), np.array([0, 1])), (1, 3), "indptr"),                # does not end at nnz
    ((np.ones(2), np.array([0, 1]), np.array([0, 1, 2])), (3, 3), "fit"),                # wrong length
])
def test_a_raw_triple_that_is_not_canonical_is_refused(triple, shape, what):
    with pytest.raises(ValueError, match=what):
        fa.SparseMatrixMap((triple, shape))


def test_the_binding_does_not_let_a_wide_column_number_wrap():
    """HipContext.set_matrix_csr checks before it narrows to 32 bits (no library call is reached: no GPU needed)."""
    c = hip.HipContext.__new__(hip.HipContext)
    c._call = lambda *a: pytest.fail("reached the library")
    with pytest.raises(ValueError, match="out of range"):
        c.set_matrix_csr(np.array([0, 1]), np.array([2 ** 32 + 3], dtype=np.int64), np.ones(1), (1, 10))
    with pytest.raises(ValueError, match="out of range"):
        c.set_matrix_csr(np.array([0, 1]), np.array([-1], dtype=np.int64), np.ones(1), (1, 10))
    with pytest.raises(TypeError):
        c.set_matrix_csr(np.array([0, 1]), np.array([1.0]), np.ones(1), (1, 10))


def test_things_that_are_no_sparse_matrix_are_refused():
    with pytest.raises(TypeError):
        fa.SparseMatrixMap(np.eye(3))
    assert not linalg.is_sparse_matrix(np.eye(3)) and linalg.is_sparse_matrix(sp.eye(3))


# ---- recognition ---------------------------------------------------------------------------------------------------------------------------
def _operands(m=6, n=9):
    S = sp.random(m, n, density=0.4, format="csr", random_state=np.random.RandomState(1))
    return S, fa.LeastSquares(np.ones(m)), np.zeros(n)


@pytest.mark.parametrize("make", [lambda S: S, lambda S: S.tocoo(), lambda S: fa.SparseMatrixMap(S)], ids=["csr", "coo", "map"])
def test_a_sparse_matrix_is_recognised(make):
    S, ls, x0 = _operands()
    for reg in (fa.Shrink(0.1), fa.NonNeg(), fa.Box(-1.0, 1.0)):
        assert solver._unrecognised(make(S), None, ls.f, ls.gradf, reg.g, reg.prox, x0) is None
    assert solver._unrecognised(make(S), None, ls.f, ls.gradf, None, None, x0) is None
    lg = fa.LogisticLoss(np.ones(6))
    assert solver._unrecognised(make(S), None, lg.f, lg.gradf, None, None, x0) is None


@pytest.mark.parametrize("reg", [fa.LinfProx(1.0), fa.L1Ball(1.0), fa.TVDualBall(), fa.GroupShrink(0.1)], ids=lambda t: type(t).__name__)
def test_refused_prox_kinds_get_a_sentence(reg):
    S, ls, x0 = _operands()
    for A in (S, fa.SparseMatrixMap(S)):
        why = solver._unrecognised(A, None, ls.f, ls.gradf, reg.g, reg.prox, x0)
        assert why is not None and type(reg).__name__ in why and "sparse" in why
        with pytest.raises(TypeError, match="sparse"):
            fa.fasta(A, ls.f, ls.gradf, reg.g, reg.prox, x0, backend="hip", verbose=False)


def test_matrix_unknown_and_float32_storage_get_a_sentence():
    S, ls, x0 = _operands()
    reg = fa.Shrink(0.1)
    ls2 = fa.LeastSquares(np.ones((6, 2)))
    why = solver._unrecognised(S, None, ls2.f, ls2.gradf, reg.g, reg.prox, np.zeros((9, 2)))
    assert why is not None and "multi-column" in why and "sparse" in why
    with pytest.raises(TypeError, match="f32.*sparse"):             # the one place float32 storage can be asked for
        fa.LinearMap.from_matrix(S, storage="f32")
    assert isinstance(fa.LinearMap.from_matrix(S), fa.SparseMatrixMap)


def test_at_is_checked_for_the_transposed_shape_only():
    S, ls, x0 = _operands()
    reg = fa.Shrink(0.1)
    with pytest.raises(AssertionError, match="transposed"):
        solver._recognise(S, S, ls.f, ls.gradf, reg.g, reg.prox, x0)
    A, loss, prox = solver._recognise(S, S.T, ls.f, ls.gradf, reg.g, reg.prox, x0)
    assert isinstance(A, fa.SparseMatrixMap) and loss is ls and prox is reg and A._ctx is None
    with pytest.raises(AssertionError):
        solver._recognise(S, None, ls.f, ls.gradf, reg.g, reg.prox, np.zeros(8))


def test_fused_true_raises_on_a_sparse_operator():
    S, ls, x0 = _operands()
    with pytest.raises(ValueError, match="one-pass"):
        solver.FBSolver(fa.SparseMatrixMap(S), ls, fa.Shrink(0.1), x0, fused=True)


def test_raw_sparse_matrix_on_the_host_loop_is_the_closure_pair():
    S, ls, x0 = _operands(30, 50)
    reg = fa.Shrink(0.05)
    runs = []
    for A in (S, fa.SparseMatrixMap(S), fa.LinearMap(lambda x: S @ x, lambda y: S.T @ y, (50,), (30,))):
        np.random.seed(5)
        runs.append(fa.fasta(A, ls.f, ls.gradf, reg.g, reg.prox, x0, backend="numpy", verbose=False))
    for c in runs[1:]:
        assert c.iteration_count == runs[0].iteration_count and np.array_equal(c.solution, runs[0].solution)
        assert np.array_equal(c.residuals, runs[0].residuals)


def _gpu_visible():
    try:
        return hip.device_count() > 0
    except hip.HipError:
        return False


@pytest.mark.skipif(_gpu_visible(), reason="a GPU is visible: the device loop runs (tests/test_gpu_sparse.py)")
def test_without_a_gpu_the_device_path_raises():
    S, ls, x0 = _operands()
    reg = fa.Shrink(0.1)
    op = fa.SparseMatrixMap(S)
    with pytest.raises(hip.HipError):
        op.ctx
    for backend in ("auto", "hip"):
        with pytest.raises(hip.HipError):
            fa.fasta(S, ls.f, ls.gradf, reg.g, reg.prox, x0, backend=backend, verbose=False)
    with pytest.raises(hip.HipError):
        op.device_apply(x0)


# ---- binding and build ---------------------------------------------------------------------------------------------------------------------
def test_binding_knows_the_two_new_entry_points():
    assert "fh_set_matrix_csr" in hip.SIGNATURES and "fh_nnz" in hip.SIGNATURES
    assert hasattr(hip.HipContext, "set_matrix_csr") and hasattr(hip.HipContext, "nnz")
    assert len(hip.SIGNATURES["fh_set_matrix_csr"][1]) == 7


def test_no_scratch_in_the_loops_of_the_sparse_kernels():
    """scripts/loop_spills.py over every instantiation of k_sp_fwd and k_sp_adj (make -C fasta_python_amd/csrc sparse-spills).  Needs
    hipcc, as the build does."""
    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("needs hipcc")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run(["make", "-s", "-C", os.path.join(root, "fasta_python_amd", "csrc"), "sparse-spills", f"PYTHON={sys.executable}"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("inside loops: none") == 20, r.stdout

"""CPU tier of a matrix unknown over a sparse operator (fh_set_matrix_csr_rhs, csrc/fh_spmulti.h): the fixtures
tests/golden/sparse_mmv/*.npz were captured from the reference core (scripts/make_sparse_mmv_golden.py) with the closure LinearMap
`S @ X` / `S.T @ Y` over (n, L) / (m, L) arrays; the NumPy oracle and the generic host loop over a SparseMatrixMap(S, rhs=L) must reproduce
them bit for bit, operand recognition must name what the device does not serve, and nothing may fall back when there is no GPU.  No GPU."""
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
from fasta_python_amd import hip, solver
from fasta_python_amd import stopping as fstop
from oracle import fasta_np as fo
from tests import helpers as H

SPARSE_MMV = os.path.join(H.GOLDEN, "sparse_mmv")
CASES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(SPARSE_MMV, "*.npz")))
FIELDS = ("residuals", "norm_residuals", "stepsizes", "objectives")
EXPECTED = ["box_100x60x2_plain", "lasso_120x200x3_adaptive", "mmv_40x60x10_backtracks", "mmv_60x90x5_accelerated", "mmv_60x90x5_adaptive",
            "mmv_60x90x5_plain", "nnls_150x80x16_accelerated", "skewed_257x515x8_adaptive"]


def capture_script():
    """scripts/make_sparse_mmv_golden.py as a module: the ONE place that states the closures the fixtures were captured with."""
    import importlib.util
    path = os.path.join(os.path.dirname(H.GOLDEN), os.pardir, "scripts", "make_sparse_mmv_golden.py")
    spec = importlib.util.spec_from_file_location("make_sparse_mmv_golden", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def load(name):
    z = np.load(os.path.join(SPARSE_MMV, name + ".npz"), allow_pickle=False)
    meta = json.loads(str(z["meta"]))
    return meta, z, {k[3:]: z[k] for k in z.files if k.startswith("in_")}


def assert_same_run(c, z):
    assert c.iteration_count == int(z["iteration_count"]) and c.backtracks == int(z["backtracks"])
    for field in FIELDS:
        if field in z.files:
            assert np.array_equal(getattr(c, field), z[field], equal_nan=True), field
    assert np.array_equal(c.solution, z["solution"])


# ---- the fixture set -----------------------------------------------------------------------------------------------------------------------
def test_the_fixture_set_is_the_one_the_script_describes():
    names = [row[0] for row in capture_script().case_table()]
    assert sorted(names) == CASES == EXPECTED
    others = [p for p in glob.glob(os.path.join(H.GOLDEN, "**", "*.npz"), recursive=True) if os.path.dirname(p) != SPARSE_MMV]
    biggest = max(os.path.getsize(p) for p in others)                   # the largest fixture the project had before these
    assert all(os.path.getsize(os.path.join(SPARSE_MMV, n + ".npz")) <= biggest for n in CASES)


def test_the_fixtures_have_the_shapes_and_prox_kinds_of_their_names():
    want = {"mmv": (60, 90, 5), "lasso": (120, 200, 3), "nnls": (150, 80, 16), "box": (100, 60, 2), "skewed": (257, 515, 8)}
    for name in CASES:
        meta, z, d = load(name)
        m, n, L = (40, 60, 10) if "backtracks" in name else want[meta["kind"]]
        assert tuple(d["shape"]) == (m, n) and d["B"].shape == (m, L) and z["solution"].shape == (n, L), name
    _, _, d = load("mmv_60x90x5_adaptive")
    assert d["data"].size == 540                                          # 10 % density
    _, _, d = load("skewed_257x515x8_adaptive")
    S = capture_script().matrix_of(d)
    per_row, per_col = np.diff(S.indptr), np.diff(S.tocsc().indptr)
    assert (per_row == 0).sum() == 10 and (per_col == 0).sum() == 10 and per_row.max() == 505 and per_col.max() == 247


@pytest.mark.parametrize("name", [n for n in EXPECTED if "backtracks" not in n])
def test_full_length_fixtures_do_not_depend_on_summation_order(name):
    """The basis for holding the device to the WHOLE history of these runs: the oracle and its row-permuted twin never part."""
    meta, z, d = load(name)
    assert capture_script().row_permuted_divergence(meta["kind"], d, meta["options"], meta["solver_seed"]) == int(z["iteration_count"])


def test_backtracking_fixture_records_where_a_permuted_copy_parts():
    meta, z, d = load("mmv_40x60x10_backtracks")
    ms = capture_script()
    assert int(z["backtracks"]) >= 5
    assert ms.permuted_divergence(meta["kind"], d, meta["options"], meta["solver_seed"]) == meta["permuted_divergence"]
    assert 10 <= meta["permuted_divergence"] <= int(z["iteration_count"])
    cut = ms.run(fo, fo.LinearMap, fo.shrink, meta["kind"], d, dict(meta["options"], max_iters=meta["permuted_divergence"], tolerance=0.0), meta["solver_seed"])
    assert cut.backtracks == meta["backtracks_at_divergence"] <= int(z["backtracks"])


# ---- bit-for-bit reproduction --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", EXPECTED)
def test_oracle_reproduces_the_reference_run(name):
    meta, z, d = load(name)
    ms = capture_script()
    c = ms.run(fo, fo.LinearMap, fo.shrink, meta["kind"], d, meta["options"], meta["solver_seed"])
    assert_same_run(c, z)


@pytest.mark.parametrize("name", EXPECTED)
def test_generic_loop_over_a_sparse_map_reproduces_the_reference_run(name):
    """fasta(SparseMatrixMap(S, rhs=L), ..., backend="numpy"): the map applied to host arrays is `S @ X` / `S.T @ Y`, the reference's closures."""
    meta, z, d = load(name)
    ms = capture_script()
    f, gradf, g, proxg = ms.closures(meta["kind"], d, fa.proximal.shrink)
    L = d["B"].shape[1]
    op = fa.SparseMatrixMap(ms.matrix_of(d), rhs=L)
    assert op.Vshape == (op.shape[1], L) and op.Wshape == (op.shape[0], L) and op.rhs == L
    np.random.seed(meta["solver_seed"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        c = fa.fasta(op, f, gradf, g, proxg, np.zeros(op.Vshape), backend="numpy", verbose=False, **ms.resolve(meta["options"], fstop))
    assert op._ctx is None                                     # the host loop never asked for a device context
    assert_same_run(c, z)


# ---- the map -------------------------------------------------------------------------------------------------------------------------------
def _operands(m=6, n=9, L=3):
    S = sp.random(m, n, density=0.4, format="csr", random_state=np.random.RandomState(1))
    return S, fa.LeastSquares(np.ones((m, L))), np.zeros((n, L))


def test_the_host_map_is_the_closure_pair_over_matrices():
    S, _, _ = _operands()
    op = fa.SparseMatrixMap(S, rhs=3)
    rng = np.random.RandomState(2)
    V, W = rng.randn(9, 3), rng.randn(6, 3)
    assert np.array_equal(op(V), S @ V) and np.array_equal(op.H(W), S.T @ W) and np.array_equal(op.T(W), S.T @ W)
    assert op.H.Vshape == (6, 3) and op.H.Wshape == (9, 3) and op.nnz == S.nnz and op._ctx is None
    assert fa.SparseMatrixMap(S).rhs is None and fa.SparseMatrixMap(S).Vshape == (9,)
    with pytest.raises(AssertionError):
        op(np.zeros(9))


@pytest.mark.parametrize("rhs", [0, 17, -1])
def test_a_column_count_outside_1_to_16_is_refused(rhs):
    S, _, _ = _operands()
    with pytest.raises(ValueError, match="1..16"):
        fa.SparseMatrixMap(S, rhs=rhs)
    assert fa.SparseMatrixMap(S, rhs=1).Vshape == (9, 1) and fa.SparseMatrixMap(S, rhs=16).Wshape == (6, 16)


# ---- recognition ---------------------------------------------------------------------------------------------------------------------------
def test_an_explicit_map_with_a_matching_2d_x0_is_recognised():
    S, ls, x0 = _operands()
    op = fa.SparseMatrixMap(S, rhs=3)
    for reg in (fa.Shrink(0.1), fa.NonNeg(), fa.Box(-1.0, 1.0), fa.GroupShrink(0.1)):
        assert solver._unrecognised(op, None, ls.f, ls.gradf, reg.g, reg.prox, x0) is None, type(reg).__name__
        A, loss, prox = solver._recognise(op, op.H, ls.f, ls.gradf, reg.g, reg.prox, x0)
        assert A is op and loss is ls and prox is reg and op._ctx is None
    assert solver._unrecognised(op, None, ls.f, ls.gradf, None, None, x0) is None


def test_the_logistic_loss_gets_a_sentence():
    S, _, x0 = _operands()
    lg = fa.LogisticLoss(np.ones((6, 3)))
    why = solver._unrecognised(fa.SparseMatrixMap(S, rhs=3), None, lg.f, lg.gradf, None, None, x0)
    assert why is not None and "LogisticLoss" in why and "sparse" in why and "multi-column" in why
    with pytest.raises(TypeError, match="LogisticLoss"):
        fa.fasta(fa.SparseMatrixMap(S, rhs=3), lg.f, lg.gradf, None, None, x0, backend="hip", verbose=False)


@pytest.mark.parametrize("reg", [fa.LinfProx(1.0), fa.L1Ball(1.0), fa.TVDualBall()], ids=lambda t: type(t).__name__)
def test_the_level_search_prox_kinds_get_a_sentence(reg):
    S, ls, x0 = _operands()
    op = fa.SparseMatrixMap(S, rhs=3)
    why = solver._unrecognised(op, None, ls.f, ls.gradf, reg.g, reg.prox, x0)
    assert why is not None and type(reg).__name__ in why and "sparse" in why
    with pytest.raises(TypeError, match="sparse"):
        fa.fasta(op, ls.f, ls.gradf, reg.g, reg.prox, x0, backend="hip", verbose=False)


def test_a_shape_mismatch_is_the_x0_has_shape_assertion():
    S, ls, x0 = _operands()
    reg = fa.Shrink(0.1)
    op = fa.SparseMatrixMap(S, rhs=3)
    for bad in (np.zeros((9, 2)), np.zeros(9), np.zeros((8, 3))):
        assert solver._unrecognised(op, None, ls.f, ls.gradf, reg.g, reg.prox, bad) is None
        with pytest.raises(AssertionError, match="x0 has shape"):
            solver._recognise(op, None, ls.f, ls.gradf, reg.g, reg.prox, bad)
    with pytest.raises(AssertionError, match="x0 has shape"):             # a vector map and a 2-D x0 of the right row count
        solver._recognise(fa.SparseMatrixMap(S), None, ls.f, ls.gradf, reg.g, reg.prox, np.zeros((9, 2)))
    ls2 = fa.LeastSquares(np.ones((6, 2)))
    with pytest.raises(AssertionError, match="b has shape"):
        solver._recognise(op, None, ls2.f, ls2.gradf, reg.g, reg.prox, x0)


def test_the_two_pinned_refusals_point_at_the_explicit_map():
    S, ls, x0 = _operands()
    reg = fa.Shrink(0.1)
    why = solver._unrecognised(S, None, ls.f, ls.gradf, reg.g, reg.prox, x0)              # a raw matrix with a 2-D x0
    assert why is not None and "multi-column" in why and "sparse" in why and "SparseMatrixMap(S, rhs=L)" in why
    why = solver._unrecognised(fa.SparseMatrixMap(S), None, ls.f, ls.gradf, reg.g, reg.prox, x0)      # ... and a map that was not told
    assert why is not None and "SparseMatrixMap(S, rhs=L)" in why
    group, lsv = fa.GroupShrink(0.1), fa.LeastSquares(np.ones(6))
    for A in (S, fa.SparseMatrixMap(S)):                                                    # GroupShrink with a vector x0
        why = solver._unrecognised(A, None, lsv.f, lsv.gradf, group.g, group.prox, np.zeros(9))
        assert why is not None and "GroupShrink" in why and "sparse" in why and "SparseMatrixMap(S, rhs=L)" in why


def test_fused_true_raises_on_a_sparse_multi_column_operator():
    S, ls, x0 = _operands()
    with pytest.raises(ValueError, match="one-pass"):
        solver.FBSolver(fa.SparseMatrixMap(S, rhs=3), ls, fa.Shrink(0.1), x0, fused=True)


def _gpu_visible():
    try:
        return hip.device_count() > 0
    except hip.HipError:
        return False


@pytest.mark.skipif(_gpu_visible(), reason="a GPU is visible: the device loop runs (tests/test_gpu_sparse_mmv.py)")
def test_without_a_gpu_the_device_path_raises():
    S, ls, x0 = _operands()
    reg = fa.GroupShrink(0.1)
    op = fa.SparseMatrixMap(S, rhs=3)
    with pytest.raises(hip.HipError):
        op.ctx
    for backend in ("auto", "hip"):
        with pytest.raises(hip.HipError):
            fa.fasta(op, ls.f, ls.gradf, reg.g, reg.prox, x0, backend=backend, verbose=False)
    with pytest.raises(hip.HipError):
        op.device_apply(x0)


# ---- binding and build ---------------------------------------------------------------------------------------------------------------------
def test_binding_knows_the_new_entry_point():
    assert "fh_set_matrix_csr_rhs" in hip.SIGNATURES and hasattr(hip.HipContext, "set_matrix_csr_rhs")
    assert len(hip.SIGNATURES["fh_set_matrix_csr_rhs"][1]) == 8 and len(hip.SIGNATURES["fh_set_matrix_csr"][1]) == 7
    calls = []
    c = hip.HipContext.__new__(hip.HipContext)
    c._call = lambda *a: calls.append(a)
    c.set_matrix_csr_rhs(np.array([0, 1]), np.array([2]), np.ones(1), (1, 10), 5)
    c.set_matrix_csr(np.array([0, 1]), np.array([2]), np.ones(1), (1, 10))
    assert calls[0][0] == "fh_set_matrix_csr_rhs" and calls[0][1:4] == (1, 10, 1) and calls[0][-1] == 5 and len(calls[0]) == 8
    assert calls[1][0] == "fh_set_matrix_csr" and len(calls[1]) == 7


def test_no_scratch_in_the_loops_of_the_sparse_multi_column_kernels():
    """scripts/loop_spills.py over every instantiation of k_spmc_fwd and k_spmc_adj (make -C fasta_python_amd/csrc spmulti-spills): 19
    (G, LB) shapes x 2 load policies x 2 kernels.  Needs hipcc, as the build does."""
    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("needs hipcc")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run(["make", "-s", "-C", os.path.join(root, "fasta_python_amd", "csrc"), "spmulti-spills", f"PYTHON={sys.executable}"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("inside loops: none") == 76, r.stdout

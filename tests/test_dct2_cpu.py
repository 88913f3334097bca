"""CPU tier of the subsampled 2-D DCT operator (fh_set_dct2, csrc/fh_dct2.h): the host face of DCTMap on an image shape, the launch geometry in
its pure form, the NumPy model of the device algorithm against the exact separable transform, the fixtures of scripts/make_dct2_golden.py
against the oracle and the generic host loop, what the solver makes of the map, the example on the host and the loop-spill guard.  No device is
touched."""
import os
import shutil
import subprocess
import sys
import warnings

import numpy as np
import pytest
import scipy.fftpack

import fasta_python_amd as fa
from fasta_python_amd import hip, solver
from tests import dct2_cases as T
from tests import dct_cases as T1

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMOOTH_64 = [L for L in range(1, 65) if not hip.dct_refusal(L)]          # the 5-smooth lengths up to 64


def capture_script():
    """scripts/make_dct2_golden.py as a module: its case table, constructor, closures and twin are the definition of the fixtures."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_dct2_golden", os.path.join(ROOT, "scripts", "make_dct2_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- DCTMap on the host ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (1, 8), (8, 1), (15, 9), (36, 50), (7, 8), (64, 64)], ids=T.ident)
def test_the_host_map_is_the_two_closures_bit_for_bit(shape):
    x, y, _ = T.operands(shape, 1)
    mask = np.random.RandomState(2).randn(*shape)                       # a general float mask
    mask[::3, ::2] = 0.0
    op, full = fa.DCTMap(shape, mask, lazy=True), fa.DCTMap(shape, lazy=True)
    assert op.Vshape == op.Wshape == full.Vshape == shape
    assert np.array_equal(op(x), mask * scipy.fftpack.dctn(x, norm="ortho")) and np.array_equal(op.H(y), scipy.fftpack.idctn(mask * y, norm="ortho"))
    assert np.array_equal(full(x), scipy.fftpack.dctn(x, norm="ortho")) and np.array_equal(full.H(y), scipy.fftpack.idctn(y, norm="ortho"))
    lhs, rhs = float(np.sum(op(x) * y)), float(np.sum(x * op.H(y)))     # <A x, y> = <x, A^H y>
    assert abs(lhs - rhs) <= 1e-12 * np.linalg.norm(x) * np.linalg.norm(y) * max(1.0, np.abs(mask).max())
    assert op._ctx is None and full._ctx is None
    assert (op.refusal is None) == (shape != (7, 8)) and (op.geometry is None) == (shape == (7, 8))
    if op.geometry is not None:
        assert (op.geometry.H, op.geometry.W) == shape


def test_an_int_and_a_one_tuple_are_the_one_dimensional_operator_as_before():
    x, y, mask = T1.operands(60, 60)
    for N in (60, (60,)):
        op = fa.DCTMap(N, mask, lazy=True)
        assert op.Vshape == op.Wshape == (60,) and op.N == 60 and op.geometry == hip.dct_shape(60)
        assert np.array_equal(op(x), mask * scipy.fftpack.dct(x, norm="ortho")) and np.array_equal(op.H(y), scipy.fftpack.idct(mask * y, norm="ortho"))
        assert op._ctx is None
    with pytest.raises(ValueError, match="3 dimensions"):
        fa.DCTMap((4, 4, 4), lazy=True)
    with pytest.raises(ValueError, match="0 dimensions"):
        fa.DCTMap((), lazy=True)
    with pytest.raises(ValueError, match=r"mask has shape \(8, 12\).*\(12, 8\)"):
        fa.DCTMap((12, 8), np.ones((8, 12)), lazy=True)
    with pytest.raises(ValueError, match=r"mask has shape \(96,\).*\(12, 8\)"):
        fa.DCTMap((12, 8), np.ones(96), lazy=True)
    with pytest.raises(hip.HipError, match="DCT_ROW_CAP"):                # a row cap out of range raises, whatever the shape is
        fa.DCTMap((12, 8), lazy=True, tuning={hip.TUNE_DCT_ROW_CAP: 4096})


# ---- the launch geometry ---------------------------------------------------------------------------------------------------------------------
def assert_geometry(sh, shape, cap=0):
    H, W = shape
    assert (sh.served, sh.H, sh.W, sh.cap, sh.threads, sh.launches) == (1, H, W, cap or hip.DCT_ROW_CAP, 256, 4)
    assert int(np.prod(sh.radices_h, dtype=np.int64)) == H and int(np.prod(sh.radices_w, dtype=np.int64)) == W
    assert set(sh.radices_h) | set(sh.radices_w) <= {2, 3, 4, 5}
    for L, rows, lds, rpw, grid in ((H, W, sh.lds_h, sh.rows_h, sh.grid_h), (W, H, sh.lds_w, sh.rows_w, sh.grid_w)):
        assert lds == (128 if L <= 128 else 512 if L <= 512 else 2048) and 1 <= rpw <= 16 and rpw * L <= lds      # the rows of a workgroup fit its LDS buffers
        assert grid == -(-rows // rpw) and (grid - 1) * rpw < rows                                              # every row has exactly one workgroup
    assert sh.tiles == -(-H // 32) * -(-W // 32) and sh.lds_bytes == 32 * max(sh.lds_h, sh.lds_w)


@pytest.mark.parametrize("shape", T.SIZES + [T.FULL_SIZE], ids=T.ident)
def test_the_geometry_rule_over_every_shape_of_the_gpu_tier(shape):
    for ncu in (256, 1, 8):
        assert_geometry(hip.dct2_shape(*shape, 0, ncu), shape)


def test_the_geometry_rule_over_every_smooth_shape_up_to_64():
    assert len(SMOOTH_64) == 27 and 7 not in SMOOTH_64 and 64 in SMOOTH_64
    for H in SMOOTH_64:
        for W in SMOOTH_64:
            assert_geometry(hip.dct2_shape(H, W), (H, W))
    assert_geometry(hip.dct2_shape(16, 12, 16), (16, 12), 16)


def test_the_shapes_reach_what_their_names_promise():
    sh = hip.dct2_shape(18, 40)
    assert sh.rows_h == 7 and 40 % 7 and sh.grid_h == 6                    # 40 rows of length 18 in groups of 7: a ragged last group
    assert 36 % 32 and 50 % 32 and hip.dct2_shape(36, 50).tiles == 4        # ragged tiles on both sides
    assert (hip.dct2_shape(96, 135).lds_h, hip.dct2_shape(96, 135).lds_w) == (128, 512)
    assert (hip.dct2_shape(128, 540).lds_h, hip.dct2_shape(128, 540).lds_w) == (128, 2048)
    assert hip.dct2_shape(2048, 3).rows_w == 16 and hip.dct2_shape(3, 2048).rows_h == 16 and hip.dct2_shape(2048, 3).rows_h == 1
    used = set()
    for shape in T.SIZES:
        sh = hip.dct2_shape(*shape)
        used |= set(sh.radices_h) | set(sh.radices_w)
    assert used == {2, 3, 4, 5}
    assert hip.dct2_shape(1, 8).radices_h == () and hip.dct2_shape(1, 1).radices_w == ()


def test_the_shape_rule_refuses_what_the_operator_refuses():
    for shape, cap, words in T.REFUSED:
        with pytest.raises(hip.HipError, match=words) as e:
            hip.dct2_shape(*shape, cap)
        assert str(e.value).startswith(f"[{hip.E_ARG}]")
        assert hip.dct2_refusal(*shape, cap) is not None
    assert "there is no two-level form per axis" in hip.dct2_refusal(60, 60, 16)
    assert hip.dct2_refusal(16, 16, 16) is None and hip.dct2_refusal(2048, 2048) is None
    with pytest.raises(hip.HipError, match="DCT_ROW_CAP"):
        hip.dct2_shape(8, 8, 4096)
    with pytest.raises(hip.HipError, match="DCT_ROW_CAP"):
        hip.dct2_refusal(8, 8, 4096)


def test_the_binding_the_header_and_the_library_know_the_new_entry_points():
    names = {"fh_set_dct2", "fh_dct2_shape", "fh_dct2_shape_for"}
    assert names <= set(hip.SIGNATURES)
    assert hasattr(hip.HipContext, "set_dct2") and hasattr(hip.HipContext, "dct2_shape") and callable(hip.dct2_refusal)
    text = open(os.path.join(ROOT, "include", "fasta_hip.h")).read()
    lib = hip.load_library()
    for name in names:
        assert f"int {name}(" in text and hasattr(lib, name)


# ---- the model of the device algorithm -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", T.SMALL, ids=T.ident)
def test_the_model_of_the_device_algorithm_is_the_separable_transform(shape):
    """Gather, Stockham passes, post-twiddle, transposes and the adjoint chain, over the radices of the library's own rule: within the GPU tier's
    bound of the exact transform in longdouble, in both directions, masked and not."""
    H, W = shape
    sh = hip.dct2_shape(H, W)
    x, y, mask = T.operands(shape, H * 1000 + W)
    for m in (None, mask):
        d = np.ones(shape) if m is None else m
        zf, za = T.model_fwd(x, m, sh), T.model_adj(y, m, sh)
        ef, ea = float(np.abs(zf - d * T.exact_dct2(x)).max()), float(np.abs(za - T.exact_dct2(d * y, adjoint=True)).max())
        assert ef <= T.bound(H, W, np.linalg.norm(x)) and ea <= T.bound(H, W, np.linalg.norm(d * y)), (ef, ea)
        if m is not None:
            assert np.all(zf[m == 0] == 0.0)
    if shape == (1, 1):
        assert T.model_fwd(x, None, sh)[0, 0] == x[0, 0] and T.model_adj(y, None, sh)[0, 0] == y[0, 0]
    # the host face (scipy.fftpack.dctn / idctn: what the fixtures and the host loop run) lies within the same bound
    assert np.abs(T.host_fwd(x) - T.exact_dct2(x)).max() <= T.bound(H, W, np.linalg.norm(x))
    assert np.abs(T.host_adj(y) - T.exact_dct2(y, adjoint=True)).max() <= T.bound(H, W, np.linalg.norm(y))


def test_the_model_maps_unit_images_to_the_outer_products_of_the_matrices_columns():
    for shape in ((2, 3), (3, 5), (9, 4)):
        H, W = shape
        sh = hip.dct2_shape(H, W)
        CH, CW = T1._exact_matrix(H).astype(np.float64), T1._exact_matrix(W).astype(np.float64)
        for i in range(H):
            for j in range(W):
                e = np.zeros(shape)
                e[i, j] = 1.0
                assert np.abs(T.model_fwd(e, None, sh) - np.outer(CH[:, i], CW[:, j])).max() <= T.bound(H, W, 1.0), (shape, i, j)
                assert np.abs(T.model_adj(e, None, sh) - np.outer(CH[i, :], CW[j, :])).max() <= T.bound(H, W, 1.0), (shape, i, j)


# ---- the fixtures ----------------------------------------------------------------------------------------------------------------------------
def test_the_fixture_set_is_the_capture_scripts_case_table():
    names = [case[0] for case in capture_script().case_table()]
    assert sorted(names) == T.CASES and len(names) == 6
    for name in names:
        meta, z, d = T.load(name)
        assert os.path.getsize(os.path.join(T.GOLDEN, name + ".npz")) < 64 * 1024
        shape = (meta["construct"]["H"], meta["construct"]["W"])
        assert max(shape) <= 64 and d["mask"].shape == d["b"].shape == z["solution"].shape == shape and int(d["mask"].sum()) == meta["construct"]["M"]
        assert ("twin_divergence" in meta) == bool(meta["options"].get("adaptive"))
    counts = {n: (int(T.load(n)[1]["iteration_count"]), int(T.load(n)[1]["backtracks"])) for n in names}
    assert counts == {"dct2_8x12_adaptive": (28, 0), "dct2_8x12_accelerated": (88, 0), "dct2_8x12_plain": (312, 0), "dct2_15x9_adaptive": (31, 0),
                      "dct2_36x50_shrink_accelerated": (409, 0), "dct2_12x8_adaptive": (79, 4)}


def assert_same_run(c, z):
    assert c.iteration_count == int(z["iteration_count"]) and c.backtracks == int(z["backtracks"])
    for f in T.FIELDS:
        assert np.array_equal(getattr(c, f), z[f], equal_nan=True), f
    assert np.array_equal(c.solution, z["solution"])


def tagged(meta, d):
    return fa.LeastSquares(d["b"]), (fa.LinfProx(float(d["mu"])) if meta["prox"] == "linf" else fa.Shrink(float(d["mu"])))


@pytest.mark.parametrize("name", T.CASES)
def test_the_host_loop_reproduces_the_fixture_bit_for_bit(name):
    cap = capture_script()
    meta, z, d = T.load(name)
    np.random.seed(meta["problem_seed"])
    again = cap.construct(**meta["construct"])
    assert np.array_equal(again["mask"], d["mask"]) and np.array_equal(again["b"], d["b"]) and float(again["mu"]) == float(d["mu"])
    shape = d["b"].shape
    # the package's generic host loop over DCTMap's host face and the tagged loss / prox
    op = fa.DCTMap(shape, d["mask"], lazy=True)
    loss, reg = tagged(meta, d)
    np.random.seed(meta["solver_seed"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        c = fa.fasta(op, loss.f, loss.gradf, reg.g, reg.prox, np.zeros(shape), backend="numpy", verbose=False, **meta["options"])
    assert_same_run(c, z)
    assert op._ctx is None                                                                     # no device context was created
    # ... and over the raw closures
    mask = d["mask"]
    A = fa.LinearMap(lambda x: mask * scipy.fftpack.dctn(x, norm="ortho"), lambda w: scipy.fftpack.idctn(mask * w, norm="ortho"), shape, shape)
    f, gradf, g, proxg = cap.closures(d, meta["prox"])
    np.random.seed(meta["solver_seed"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        c = fa.fasta(A, f, gradf, g, proxg, np.zeros(shape), verbose=False, **meta["options"])
    assert_same_run(c, z)


@pytest.mark.parametrize("name", [n for n in T.CASES if "adaptive" in n])
def test_the_twins_parting_iteration_is_the_stored_one(name):
    cap = capture_script()
    meta, z, d = T.load(name)
    k, bt = cap.twin_divergence(d, meta["prox"], meta["options"], meta["solver_seed"])
    assert (k, bt) == (meta["twin_divergence"], meta["backtracks_at_divergence"])
    assert 0 < k <= int(z["iteration_count"])
    if name == "dct2_12x8_adaptive":                       # the run that backtracks
        assert int(z["backtracks"]) > 0 and bt > 0
    x, y, mask = T.operands(d["b"].shape, 3)               # the twin's operator is the closures' to rounding
    (f0, a0), (f1, a1) = cap.fftpack_pair(mask), cap.makhoul_pair(mask)
    H, W = d["b"].shape
    assert np.abs(f0(x) - f1(x)).max() <= T.bound(H, W, np.linalg.norm(x)) and np.abs(a0(y) - a1(y)).max() <= T.bound(H, W, np.linalg.norm(y))


# ---- what the solver makes of the map -----------------------------------------------------------------------------------------------------------
def why(op, loss, reg, x0):
    return solver._unrecognised(op, None, loss.f, loss.gradf, None if reg is None else reg.g, None if reg is None else reg.prox, x0)


def test_what_the_solver_sends_to_the_device_and_what_it_refuses():
    shape = (12, 8)
    op = fa.DCTMap(shape, lazy=True)
    ls = fa.LeastSquares(np.zeros(shape))
    for reg in (None, fa.LinfProx(1.0), fa.L1Ball(1.0), fa.Shrink(0.1), fa.NonNeg(), fa.Box(-1.0, 1.0)):
        assert why(op, ls, reg, np.zeros(shape)) is None
    assert "least squares only" in why(op, fa.LogisticLoss(np.ones(shape)), fa.Shrink(0.1), np.zeros(shape))
    for reg in (fa.TVDualBall(), fa.GroupShrink(0.1)):
        assert "not implemented for a DCT operator" in why(op, ls, reg, np.zeros(shape))
    assert "takes an unknown of that shape" in why(op, ls, fa.Shrink(0.1), np.zeros(96))
    assert "takes an unknown of that shape" in why(op, ls, fa.Shrink(0.1), np.zeros((8, 12)))
    assert op._ctx is None


@pytest.mark.parametrize("shape", [(7, 8), (4, 4096)], ids=T.ident)
def test_a_shape_the_device_refuses_runs_on_the_host_and_raises_under_backend_hip(shape):
    rng = np.random.RandomState(shape[0])
    mask = (rng.rand(*shape) < 0.6).astype(float)
    b = mask * rng.randn(*shape)
    op = fa.DCTMap(shape, mask)                            # (not lazy, and still no device: a refused shape never creates a context)
    words = "prime factor above 5" if shape == (7, 8) else "no two-level form per axis"
    assert op._ctx is None and words in op.refusal
    ls, reg = fa.LeastSquares(b), fa.Shrink(0.1)
    runs = []
    for A in (op, fa.LinearMap(lambda x: mask * scipy.fftpack.dctn(x, norm="ortho"), lambda w: scipy.fftpack.idctn(mask * w, norm="ortho"), shape, shape)):
        np.random.seed(3)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            runs.append(fa.fasta(A, ls.f, ls.gradf, reg.g, reg.prox, np.zeros(shape), verbose=False, max_iters=20))
    assert runs[0].iteration_count == runs[1].iteration_count and np.array_equal(runs[0].solution, runs[1].solution)
    assert np.array_equal(runs[0].residuals, runs[1].residuals)
    with pytest.raises(TypeError, match=words):
        fa.fasta(op, ls.f, ls.gradf, reg.g, reg.prox, np.zeros(shape), backend="hip", verbose=False)
    assert op._ctx is None


def test_a_served_shape_sets_the_operator_on_first_use(monkeypatch):
    calls = []

    class Recorder:
        def __init__(self, *args, **kwargs):
            calls.append(("create",))

        def set_tuning(self, key, value):
            calls.append(("tune", key, value))

        def set_dct(self, N, mask):
            calls.append(("dct", N, mask))

        def set_dct2(self, H, W, mask):
            calls.append(("dct2", H, W, None if mask is None else mask.copy()))

        def close(self):
            pass

    monkeypatch.setattr(hip, "HipContext", Recorder)
    mask = np.arange(96.0).reshape(12, 8)
    op = fa.DCTMap((12, 8), mask, lazy=True, tuning={hip.TUNE_DCT_ROW_CAP: 16})
    assert not calls and op.geometry.cap == 16
    op.ctx
    assert calls[:2] == [("create",), ("tune", hip.TUNE_DCT_ROW_CAP, 16)] and calls[2][:3] == ("dct2", 12, 8) and np.array_equal(calls[2][3], mask)
    fa.DCTMap((4, 6))                                      # not lazy: the context at once
    assert calls[3:] == [("create",), ("dct2", 4, 6, None)]
    fa.DCTMap((6,))                                        # a 1-tuple sets the 1-D operator
    assert calls[5:] == [("create",), ("dct", 6, None)]


def test_the_example_runs_on_the_host(capsys):
    from fasta_python_amd.examples import compressive_imaging as ex
    results = ex.main(["--backend", "numpy", "--shape", "30", "64", "--samples", "900", "--mu", "0.1"])
    assert [x.shape for x, _ in results] == [(30, 64)] * 3 and all(0 < c.iteration_count < 500 for _, c in results)
    objs = [c.objectives[c.iteration_count] for _, c in results]
    assert max(objs) - min(objs) <= 1e-6 * abs(objs[0])                     # the three modes reach the same minimum
    out = capsys.readouterr().out
    assert out.count("Completed in") == 3 and "Constructed compressive imaging problem: 30 x 64, 900 of 1920 DCT coefficients" in out
    import fasta.examples.compressive_imaging as drop_in                    # the drop-in name
    assert drop_in.__file__ == ex.__file__ and hasattr(drop_in, "CompressiveImagingProblem")
    with pytest.raises(ValueError, match="--samples must lie in"):
        ex.CompressiveImagingProblem.construct(shape=(4, 4), samples=17)


def test_no_scratch_in_the_loops_of_the_2d_dct_kernels():
    """scripts/loop_spills.py over every instantiation of the 2-D DCT kernels (make -C fasta_python_amd/csrc dct2-spills).  Needs hipcc, as the
    build does."""
    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("needs hipcc")
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "fasta_python_amd", "csrc"), "dct2-spills", f"PYTHON={sys.executable}"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("inside loops: none") == 15, r.stdout          # 3 LDS classes x four row kernels + three tile kernels

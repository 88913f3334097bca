"""CPU tier of the subsampled DCT operator (fh_set_dct, csrc/fh_dct.h): the NumPy model of the device algorithm against the exact transform, the
fixtures of scripts/make_dct_golden.py against the oracle and the NumPy backend, the host face of DCTMap, the launch geometry in its pure
form, what the solver refuses, and the loop-spill guard.  No device is touched."""
import os
import shutil
import subprocess
import sys
import warnings

import numpy as np
import pytest
import scipy.fft
import scipy.fftpack

import fasta_python_amd as fa
from fasta_python_amd import hip, solver
from tests import dct_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [f"{N}-cap{cap}" for N, cap in T.SIZES]


def capture_script():
    """scripts/make_dct_golden.py as a module: its case table, constructor, closures and twin are the definition of the fixtures."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_dct_golden", os.path.join(ROOT, "scripts", "make_dct_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- the model of the device algorithm -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", T.SIZES, ids=IDS)
def test_the_model_of_the_device_algorithm_is_the_dct(case):
    """Permutation, split, Stockham passes, six-step twiddle, post-twiddle and the adjoint chain, over the radices and the split of the library's
    own rule: within the GPU tier's bound of the exact transform (longdouble, N <= 2048) or, beyond, within twice the bound of scipy."""
    N, cap = case
    sh = hip.dct_shape(N, cap)
    x, y, mask = T.operands(N, N)
    for m in (None, mask):
        zf, za = T.model_fwd(x, m, sh), T.model_adj(y, m, sh)
        if N <= 2048:
            d = np.ones(N) if m is None else m
            want_f, want_a, slack = d * T.exact_dct(x), T.exact_dct(d * y, adjoint=True), 1.0
        else:
            want_f, want_a, slack = T.host_fwd(x, m), T.host_adj(y, m), 2.0
        ef, ea = float(np.abs(zf - want_f).max()), float(np.abs(za - want_a).max())
        assert ef <= slack * T.bound(N, np.linalg.norm(x)) and ea <= slack * T.bound(N, np.linalg.norm(y)), (ef, ea)
        if m is not None:
            assert np.all(zf[m == 0] == 0.0)
    if N == 1:
        assert T.model_fwd(x, None, sh)[0] == x[0] and T.model_adj(y, None, sh)[0] == y[0]


@pytest.mark.parametrize("N", [1, 2, 3, 5, 45, 1000, 2048])
def test_dctmaps_host_face_and_scipy_fft_meet_the_bound(N):
    """The references of the GPU tier: DCTMap on host arrays (scipy.fftpack, what the fixtures and the host loop run) and scipy.fft (the reference of
    the larger sizes) lie within the bound of the exact transform, far inside it at N = 1000."""
    x, y, _ = T.operands(N, N)
    op = fa.DCTMap(N, lazy=True)
    for got, want, v in ((op(x), T.exact_dct(x), x), (op.H(y), T.exact_dct(y, adjoint=True), y),
                         (scipy.fft.dct(x, norm="ortho"), T.exact_dct(x), x), (scipy.fft.idct(y, norm="ortho"), T.exact_dct(y, adjoint=True), y)):
        err = float(np.abs(got - want).max())
        assert err <= T.bound(N, np.linalg.norm(v))
        if N == 1000:
            assert err <= 0.02 * T.bound(N, np.linalg.norm(v))


def test_the_permutation_is_a_bijection_with_the_stated_halves():
    """... and it is the permutation the transform needs: the model over the library's radices maps every unit vector to its column of C."""
    for N in (1, 2, 3, 8, 9, 45, 60):
        src = T.src_index(N)
        assert sorted(src) == list(range(N))
        x = np.arange(N)
        v = x[src]
        half = (N + 1) // 2
        assert np.array_equal(v[:half], x[0::2]) and np.array_equal(v[::-1][:N // 2], x[1::2])
        for cap in (0, 4):
            if hip.dct_refusal(N, cap):                  # (9, 45 and 60 have no split within 4)
                continue
            sh = hip.dct_shape(N, cap)
            C = T._exact_matrix(N).astype(np.float64)
            for i in range(N):
                assert np.abs(T.model_fwd(np.eye(N)[i], None, sh) - C[:, i]).max() <= T.bound(N, 1.0), (N, cap, i)


# ---- the launch geometry ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", T.SIZES + T.FULL_SIZE, ids=IDS + [f"{N}-cap{cap}" for N, cap in T.FULL_SIZE])
def test_the_geometry_rule_over_every_size_of_the_gpu_tier(case):
    N, cap = case
    sh = hip.dct_shape(N, cap)
    limit = cap or hip.DCT_ROW_CAP
    assert sh.cap == limit and sh.N1 * sh.N2 == N and 1 <= sh.N1 <= limit and 1 <= sh.N2 <= limit
    assert int(np.prod(sh.radices1, dtype=np.int64)) == sh.N1 and int(np.prod(sh.radices2, dtype=np.int64)) == sh.N2
    assert set(sh.radices1) | set(sh.radices2) <= {2, 3, 4, 5} and sh.threads == 256
    if N <= limit:
        assert (sh.levels, sh.N1, sh.N2, sh.launches, sh.grid1, sh.rows1) == (1, N, 1, 1, 1, 1)
        assert sh.lds1 >= N and sh.lds_bytes == 32 * sh.lds1
    else:
        assert sh.levels == 2 and sh.launches == 5 and sh.N2 == max(d for d in range(2, limit + 1) if N % d == 0 and N // d <= limit)
        for L, rows, lds, rpw, grid in ((sh.N1, sh.N2, sh.lds1, sh.rows1, sh.grid1), (sh.N2, sh.N1, sh.lds2, sh.rows2, sh.grid2)):
            assert lds in (128, 512, 2048) and L <= lds and 1 <= rpw and rpw * L <= lds            # the rows of a workgroup fit its LDS buffers
            assert grid == -(-rows // rpw)                                                        # every row has exactly one workgroup
        assert sh.tiles == -(-sh.N1 // 32) * -(-sh.N2 // 32) and sh.lds_bytes == 32 * max(sh.lds1, sh.lds2)


def test_the_sizes_reach_what_their_names_promise():
    assert hip.dct_shape(4096)[1:3] == (2, 2048) and hip.dct_shape(6000)[1:3] == (3, 2000) and hip.dct_shape(1000, 40)[1:3] == (25, 40)
    assert hip.dct_shape(1 << 22)[1:3] == (2048, 2048) and hip.dct_shape(3 << 20)[1:3] == (1536, 2048)
    assert 2000 % 32 and 3 % 32                                              # 6000: ragged tiles on both axes
    used = set()
    for N, cap in T.SIZES:
        sh = hip.dct_shape(N, cap)
        used |= set(sh.radices1) | set(sh.radices2)
    assert used == {2, 3, 4, 5}
    sh = hip.dct_shape(1000, 40)
    assert set(sh.radices1) | set(sh.radices2) == {2, 4, 5} and sh.N1 != sh.N2
    assert {hip.dct_shape(N, cap).levels for N, cap in T.ONE_ROW} == {1} and {hip.dct_shape(N, cap).levels for N, cap in T.TWO_LEVEL} == {2}


def test_the_shape_rule_refuses_what_the_operator_refuses():
    assert T.REFUSED == (7, 1001, 3 ** 15, 0)
    for N, words in ((7, "prime factor above 5"), (1001, "prime factor above 5"), (3 ** 15, "both factors at most the row cap"), (0, "N >= 1")):
        with pytest.raises(hip.HipError, match=words):
            hip.dct_shape(N)
    for N, cap in T.REFUSED_AT_CAP:                       # 250 = 2 * 5^3: no two factors of at most 16
        with pytest.raises(hip.HipError, match="both factors at most the row cap"):
            hip.dct_shape(N, cap)
    with pytest.raises(hip.HipError, match="DCT_ROW_CAP"):
        hip.dct_shape(64, 4096)
    assert hip.dct_shape((1 << 22)).levels == 2
    with pytest.raises(hip.HipError, match="both factors"):
        hip.dct_shape(1 << 23)


def test_the_binding_knows_the_new_entry_points():
    assert {"fh_set_dct", "fh_dct_shape", "fh_dct_shape_for"} <= set(hip.SIGNATURES)
    assert hasattr(hip.HipContext, "set_dct") and hasattr(hip.HipContext, "dct_shape") and hip.TUNE_DCT_ROW_CAP == 22
    text = open(os.path.join(ROOT, "include", "fasta_hip.h")).read()
    assert "FH_TUNE_DCT_ROW_CAP = 22" in text and f"#define FH_DCT_SHAPE_LEN {hip.DCT_SHAPE_LEN}" in text
    assert "OP_DCT = 7" in open(os.path.join(ROOT, "fasta_python_amd", "csrc", "fh_host_ctx.h")).read()
    assert f"#define DCT_ROW_CAP {hip.DCT_ROW_CAP}" in open(os.path.join(ROOT, "fasta_python_amd", "csrc", "fh_dct.h")).read()


# ---- DCTMap on the host ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 45, 60, 1000, 1001])
def test_dctmap_host_closures_are_the_references(N):
    x, y, mask = T.operands(N, N)
    op = fa.DCTMap(N, mask, lazy=True)
    assert op.Vshape == op.Wshape == (N,)
    assert np.array_equal(op(x), mask * scipy.fftpack.dct(x, norm="ortho")) and np.array_equal(op.H(y), scipy.fftpack.idct(mask * y, norm="ortho"))
    full = fa.DCTMap(N, lazy=True)
    assert np.array_equal(full(x), scipy.fftpack.dct(x, norm="ortho")) and np.array_equal(full.H(y), scipy.fftpack.idct(y, norm="ortho"))
    assert op._ctx is None and full._ctx is None
    assert (op.refusal is None) == (N != 1001) and (op.geometry is None) == (N == 1001)
    with pytest.raises(ValueError, match="mask has shape"):
        fa.DCTMap(N, np.ones(N + 1), lazy=True)
    # only the library's sentences about N are a refusal: a row cap out of range raises, whatever N is
    with pytest.raises(hip.HipError, match="DCT_ROW_CAP"):
        fa.DCTMap(N, mask, lazy=True, tuning={hip.TUNE_DCT_ROW_CAP: 4096})
    assert (hip.dct_refusal(N) is None) == (N != 1001)


def test_the_fixture_set_is_the_capture_scripts_case_table():
    names = [case[0] for case in capture_script().case_table()]
    assert sorted(names) == T.CASES and len(names) == 8
    for name in names:
        meta, z, d = T.load(name)
        assert os.path.getsize(os.path.join(T.GOLDEN, name + ".npz")) < 64 * 1024
        N = meta["construct"]["N"]
        assert d["mask"].shape == d["b"].shape == z["solution"].shape == (N,) and int(d["mask"].sum()) == meta["construct"]["M"]
        assert ("twin_divergence" in meta) == bool(meta["options"].get("adaptive"))
    counts = {n: (int(T.load(n)[1]["iteration_count"]), int(T.load(n)[1]["backtracks"])) for n in names}
    assert counts == {"dct_60_adaptive": (20, 0), "dct_60_accelerated": (58, 0), "dct_60_plain": (230, 0), "dct_250_accelerated": (48, 0),
                      "dct_1000_adaptive": (22, 0), "dct_96_adaptive": (104, 12), "dct_45_adaptive": (32, 0), "dct_1000_shrink_accelerated": (366, 0)}


def assert_same_run(c, z):
    assert c.iteration_count == int(z["iteration_count"]) and c.backtracks == int(z["backtracks"])
    for f in T.FIELDS:
        assert np.array_equal(getattr(c, f), z[f], equal_nan=True), f
    assert np.array_equal(c.solution, z["solution"])


def tagged(meta, d):
    return fa.LeastSquares(d["b"]), (fa.LinfProx(float(d["mu"])) if meta["prox"] == "linf" else fa.Shrink(float(d["mu"])))


@pytest.mark.parametrize("name", T.CASES)
def test_oracle_and_numpy_backend_reproduce_the_fixture_bit_for_bit(name):
    cap = capture_script()
    meta, z, d = T.load(name)
    np.random.seed(meta["problem_seed"])
    again = cap.construct(**meta["construct"])
    assert np.array_equal(again["mask"], d["mask"]) and np.array_equal(again["b"], d["b"]) and float(again["mu"]) == float(d["mu"])
    assert_same_run(cap.oracle_run(d, meta["prox"], meta["options"], sseed=meta["solver_seed"]), z)
    # the package's generic host loop over DCTMap's host face and the tagged loss / prox
    N = len(d["b"])
    op = fa.DCTMap(N, d["mask"], lazy=True)
    loss, reg = tagged(meta, d)
    np.random.seed(meta["solver_seed"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        c = fa.fasta(op, loss.f, loss.gradf, reg.g, reg.prox, np.zeros(N), backend="numpy", verbose=False, **meta["options"])
    assert_same_run(c, z)
    assert op._ctx is None                                                                     # no device context was created


@pytest.mark.parametrize("name", [n for n in T.CASES if "adaptive" in n])
def test_the_twins_parting_iteration_is_the_stored_one(name):
    cap = capture_script()
    meta, z, d = T.load(name)
    k, bt = cap.twin_divergence(d, meta["prox"], meta["options"], meta["solver_seed"])
    assert (k, bt) == (meta["twin_divergence"], meta["backtracks_at_divergence"])
    if name == "dct_96_adaptive":                          # the run that backtracks parts from its twin before its end
        assert 40 <= k < int(z["iteration_count"]) and 0 < bt <= int(z["backtracks"])
    else:
        assert k == int(z["iteration_count"])
    # ... and up to there the run with L and tau0 passed in IS the fixture's run
    L, tau0 = cap.step_estimate(d, meta["prox"], meta["solver_seed"])
    head = cap.oracle_run(d, meta["prox"], dict(meta["options"], max_iters=max(k, 1), tolerance=0.0), L=L, tau0=tau0)
    assert np.array_equal(head.stepsizes[:k], z["stepsizes"][:k])


def test_the_twins_operator_is_the_references_to_rounding():
    cap = capture_script()
    for N in (45, 60, 1000):
        x, y, mask = T.operands(N, N)
        (f0, a0), (f1, a1) = cap.fftpack_pair(mask), cap.makhoul_pair(mask)
        assert np.abs(f0(x) - f1(x)).max() <= T.bound(N, np.linalg.norm(x)) and np.abs(a0(y) - a1(y)).max() <= T.bound(N, np.linalg.norm(y))


# ---- what the solver makes of a DCTMap --------------------------------------------------------------------------------------------------------
def why(op, loss, reg, x0):
    return solver._unrecognised(op, None, loss.f, loss.gradf, None if reg is None else reg.g, None if reg is None else reg.prox, x0)


def test_what_the_solver_sends_to_the_device_and_what_it_refuses():
    N = 60
    op = fa.DCTMap(N, lazy=True)
    ls = fa.LeastSquares(np.zeros(N))
    for reg in (None, fa.LinfProx(1.0), fa.L1Ball(1.0), fa.Shrink(0.1), fa.NonNeg(), fa.Box(-1.0, 1.0)):
        assert why(op, ls, reg, np.zeros(N)) is None
    assert "least squares only" in why(op, fa.LogisticLoss(np.ones(N)), fa.Shrink(0.1), np.zeros(N))
    for reg in (fa.TVDualBall(), fa.GroupShrink(0.1)):
        assert "not implemented for a DCT operator" in why(op, ls, reg, np.zeros(N))
    assert "vector unknown" in why(op, ls, fa.Shrink(0.1), np.zeros((N, 2)))
    assert op._ctx is None


@pytest.mark.parametrize("N", [7, 1001])
def test_a_length_the_device_refuses_runs_on_the_host_and_raises_under_backend_hip(N):
    """DCTMap keeps the library's sentence; the default backend takes the generic host loop over the reference's closures (the same bits as
    those closures passed by hand), backend="hip" raises with the sentence."""
    rng = np.random.RandomState(N)
    mask = (rng.rand(N) < 0.6).astype(float)
    b = mask * rng.randn(N)
    op = fa.DCTMap(N, mask)                                # (not lazy, and still no device: a refused length never creates a context)
    assert op._ctx is None and "prime factor above 5" in op.refusal
    ls, reg = fa.LeastSquares(b), fa.LinfProx(2.0)
    runs = []
    for A in (op, fa.LinearMap(lambda x: mask * scipy.fftpack.dct(x, norm="ortho"), lambda w: scipy.fftpack.idct(mask * w, norm="ortho"), (N,))):
        np.random.seed(3)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            runs.append(fa.fasta(A, ls.f, ls.gradf, reg.g, reg.prox, np.zeros(N), verbose=False, max_iters=40))
    assert runs[0].iteration_count == runs[1].iteration_count and np.array_equal(runs[0].solution, runs[1].solution)
    assert np.array_equal(runs[0].residuals, runs[1].residuals)
    with pytest.raises(TypeError, match="prime factor above 5"):
        fa.fasta(op, ls.f, ls.gradf, reg.g, reg.prox, np.zeros(N), backend="hip", verbose=False)
    assert op._ctx is None


def test_a_served_length_sets_the_operator_on_first_use(monkeypatch):
    calls = []

    class Recorder:
        def __init__(self, *args, **kwargs):
            calls.append(("create",))

        def set_tuning(self, key, value):
            calls.append(("tune", key, value))

        def set_dct(self, N, mask):
            calls.append(("dct", N, None if mask is None else mask.copy()))

        def close(self):
            pass

    monkeypatch.setattr(hip, "HipContext", Recorder)
    mask = np.array([0.0, 1.0, 2.5] * 20)
    op = fa.DCTMap(60, mask, lazy=True, tuning={hip.TUNE_DCT_ROW_CAP: 16})
    assert not calls and (op.geometry.N1, op.geometry.N2) == (4, 15)
    op.ctx
    assert calls[:2] == [("create",), ("tune", hip.TUNE_DCT_ROW_CAP, 16)] and calls[2][:2] == ("dct", 60) and np.array_equal(calls[2][2], mask)
    fa.DCTMap(64)                                          # not lazy: the context at once
    assert calls[3:] == [("create",), ("dct", 64, None)]


def test_the_example_runs_the_references_problem_on_the_host(capsys):
    from fasta_python_amd.examples import democratic_representation as ex
    results = ex.main(["--backend", "numpy", "--points", "60", "--samples", "30", "--mu", "20"])
    assert [c.iteration_count for _, c in results] == [20, 58, 230]          # the fixtures' runs: same seeds, same data
    for (x, c), name in zip(results, ("dct_60_adaptive", "dct_60_accelerated", "dct_60_plain")):
        assert np.array_equal(x, T.load(name)[1]["solution"])
    out = capsys.readouterr().out
    assert out.count("Completed in") == 3 and "Constructed democratic representation problem." in out
    import fasta.examples.democratic_representation as drop_in            # the drop-in name
    assert drop_in.__file__ == ex.__file__ and hasattr(drop_in, "DemocraticRepresentationProblem")


def test_no_scratch_in_the_loops_of_the_dct_kernels():
    """scripts/loop_spills.py over every instantiation of the DCT kernels (make -C fasta_python_amd/csrc dct-spills).  Needs hipcc, as the
    build does."""
    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("needs hipcc")
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "fasta_python_amd", "csrc"), "dct-spills", f"PYTHON={sys.executable}"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("inside loops: none") == 17, r.stdout          # 3 LDS classes x (two one-row kernels + two row kernels) + five tile kernels

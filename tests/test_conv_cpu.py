"""CPU tier of the periodic convolution operator (linalg.ConvMap, fh_set_conv2d, csrc/fh_conv.h): the host closures against scipy.ndimage and
an FFT product, the exact adjoint identity on integers, the launch rule (every pixel has one owner), the refusals, the fixtures of
scripts/make_conv_golden.py reproduced bit for bit by the oracle and by the package's host loop, and the proof that the exact step of
tests/conv_cases.py is exact.  No GPU."""
import os
import warnings

import numpy as np
import pytest
import scipy.ndimage

import fasta_python_amd as fa
from fasta_python_amd import hip, solver
from tests import conv_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def capture_script():
    """scripts/make_conv_golden.py as a module: its case table, constructor, closures and twin are the definition of the fixtures."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_conv_golden", os.path.join(ROOT, "scripts", "make_conv_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def conv_map(case, K, mask):
    shape, _, origin, _ = case
    return fa.ConvMap(shape, K, origin=origin if origin is None or len(shape) == 2 else origin[0], mask=mask)


# ---- the operator on the host ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", T.SHAPES, ids=T.IDS)
def test_the_host_closures_are_the_definition(case):
    """ConvMap on host arrays == the roll expression of tests/conv_cases.py == the definition written out index by index."""
    shape, kshape, origin, masked = case
    rng = np.random.RandomState(T.SHAPES.index(case))
    x, w, K = rng.randn(*shape), rng.randn(*shape), rng.randn(*kshape)
    mask = (rng.rand(*shape) < 0.6).astype(np.float64) if masked else None
    oh, ow = T.origin2d(kshape, origin)
    op = conv_map(case, K, mask)
    assert op.Vshape == op.Wshape == tuple(shape) and op._ctx is None and op.refusal is None and op.origin == (oh, ow)
    z, g = op(x), op.H(w)
    assert np.array_equal(z, T.conv(x, K, (oh, ow), mask)) and np.array_equal(g, T.conv(w, K, (oh, ow), mask, adjoint=True))
    H, W = T.shape2d(shape)
    if H * W <= 400:
        x2, w2, K2 = x.reshape(H, W), w.reshape(H, W), K.reshape(T.shape2d(kshape))
        d = np.ones((H, W)) if mask is None else mask.reshape(H, W)
        zz, gg = np.zeros((H, W)), np.zeros((H, W))
        for i in range(H):
            for j in range(W):
                for a in range(K2.shape[0]):
                    for b in range(K2.shape[1]):
                        zz[i, j] += K2[a, b] * x2[(i - (a - oh)) % H, (j - (b - ow)) % W]
                        gg[i, j] += K2[a, b] * (d * w2)[(i + (a - oh)) % H, (j + (b - ow)) % W]
        assert np.array_equal(z.reshape(H, W), d * zz) and np.array_equal(g.reshape(H, W), gg)
    assert op._ctx is None                                                  # lazy: no device context on a box without a GPU


@pytest.mark.parametrize("kshape", [(3, 3), (5, 3), (1, 7), (9, 9), (15, 15)])
def test_the_host_closures_against_scipy_ndimage_and_an_fft_product(kshape):
    rng = np.random.RandomState(sum(kshape))
    shape = (37, 41)
    x, w, K = rng.randn(*shape), rng.randn(*shape), rng.randn(*kshape)
    op = fa.ConvMap(shape, K)
    scale = np.abs(K).sum() * np.abs(x).max()
    np.testing.assert_allclose(op(x), scipy.ndimage.convolve(x, K, mode="wrap"), rtol=1e-13, atol=1e-13 * scale)
    np.testing.assert_allclose(op.H(w), scipy.ndimage.correlate(w, K, mode="wrap"), rtol=1e-13, atol=1e-13 * np.abs(K).sum() * np.abs(w).max())
    pad = np.zeros(shape)
    pad[:kshape[0], :kshape[1]] = K
    pad = np.roll(pad, (-(kshape[0] // 2), -(kshape[1] // 2)), axis=(0, 1))
    np.testing.assert_allclose(op(x), np.fft.ifft2(np.fft.fft2(pad) * np.fft.fft2(x)).real, rtol=1e-11, atol=1e-12 * scale)
    np.testing.assert_allclose(op.H(w), np.fft.ifft2(np.conj(np.fft.fft2(pad)) * np.fft.fft2(w)).real, rtol=1e-11, atol=1e-12 * scale)


@pytest.mark.parametrize("case", T.SHAPES, ids=T.IDS)
def test_the_adjoint_identity_is_exact_on_integer_operands(case):
    shape, kshape, origin, masked = case
    rng = np.random.RandomState(40 + T.SHAPES.index(case))
    x, w = rng.randint(-8, 9, size=shape).astype(np.float64), rng.randint(-8, 9, size=shape).astype(np.float64)
    K = rng.randint(-4, 5, size=kshape).astype(np.float64)
    mask = (rng.rand(*shape) < 0.6).astype(np.float64) if masked else None
    op = conv_map(case, K, mask)
    assert float(np.sum(op(x) * w)) == float(np.sum(x * op.H(w)))           # integers far below 2^53: every sum is exact


def test_convmap_refuses_other_ranks_and_bad_arguments():
    with pytest.raises(ValueError, match="image shape \\(H, W\\) or a signal shape \\(N,\\); got 3 dimensions"):
        fa.ConvMap((4, 4, 4), np.ones((3, 3)))
    with pytest.raises(ValueError, match="a 2-D shape takes a 2-D kernel \\(got 1 dimensions\\)"):
        fa.ConvMap((4, 4), np.ones(3))
    with pytest.raises(ValueError, match="a 1-D shape takes a 1-D kernel \\(got 2 dimensions\\)"):
        fa.ConvMap((8,), np.ones((3, 3)))
    with pytest.raises(ValueError, match="a 2-D shape takes a 2-D kernel \\(got 3 dimensions\\)"):
        fa.ConvMap((4, 4), np.ones((3, 3, 3)))
    with pytest.raises(ValueError, match="origin \\(3, 0\\) lies outside the 3 x 3 kernel"):
        fa.ConvMap((4, 4), np.ones((3, 3)), origin=(3, 0))
    with pytest.raises(ValueError, match="mask has shape"):
        fa.ConvMap((4, 4), np.ones((3, 3)), mask=np.ones((4, 5)))
    with pytest.raises(ValueError, match="non-empty"):
        fa.ConvMap((0, 4), np.ones((3, 3)))
    sig = fa.ConvMap((8,), np.arange(3.0), origin=2)
    assert sig.origin == (0, 2) and sig.shape2d == (1, 8) and sig.kernel.shape == (1, 3) and sig(np.arange(8.0)).shape == (8,)
    assert fa.ConvMap(8, np.ones(3)).Vshape == (8,)


# ---- the launch rule -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ncu", [1, 8, 256, 304])
@pytest.mark.parametrize("case", T.SHAPES, ids=T.IDS)
def test_every_pixel_has_exactly_one_owning_workgroup(case, ncu):
    shape, kshape = case[0], case[1]
    H, W = T.shape2d(shape)
    kh, kw = T.shape2d(kshape)
    sh = hip.conv_shape(H, W, kh, kw, ncu=ncu)
    assert np.all(T.owners(shape, sh) == 1)
    assert (sh.tile_h, sh.tile_w) == ((1, T.FLAT_W) if (H == 1 and kh == 1) else (T.TILE_H, T.TILE_W))
    assert sh.grid == sh.tiles_h * sh.tiles_w and sh.run * sh.threads == sh.tile_h * sh.tile_w and sh.threads == 256
    # the tile with the largest halo fits the LDS the kernels declare: rows x pitch, the pitch holding the skewed columns (csrc/fh_conv.h)
    pitch = 2344 if sh.tile_h == 1 else 104
    cols = sh.tile_w + 15
    assert cols - 1 + (cols - 1) // 8 < pitch and pitch % 32 == 8 and (sh.tile_h + (15 if sh.tile_h > 1 else 0)) * pitch * 8 <= sh.lds_bytes <= 64 * 1024


def test_the_shapes_reach_what_they_claim():
    ragged = hip.conv_shape(*T.RAGGED, 7, 9)
    assert ragged.tiles_h >= 3 and ragged.tiles_w >= 3 and T.RAGGED[0] % T.TILE_H and T.RAGGED[1] % T.TILE_W
    kinds = [(T.shape2d(s), T.shape2d(k), T.origin2d(k, o)) for s, k, o, _ in T.SHAPES]
    assert any(kh > H and kw > W for (H, W), (kh, kw), _ in kinds) and ((1, 1), (3, 3), (1, 1)) in kinds and any(kh * kw == 256 for _, (kh, kw), _ in kinds)
    assert any(o == (0, 0) and k == (4, 6) for _, k, o in kinds) and any(o == (3, 5) and k == (4, 6) for _, k, o in kinds)
    assert any(m for *_, m in T.SHAPES) and any(len(s) == 1 for s, *_ in T.SHAPES) and all(int(np.prod(s)) <= 1 << 16 for s, *_ in T.SHAPES)
    assert len(set(T.IDS)) == len(T.SHAPES)


def test_the_shape_rule_refuses_what_the_operator_refuses():
    for args, words in (((0, 5, 3, 3), "H >= 1 and W >= 1"), ((5, 0, 3, 3), "H >= 1 and W >= 1"), ((5, 5, 0, 3), "1 to 16 taps"),
                        ((5, 5, 17, 3), "1 to 16 taps"), ((5, 5, 3, 17), "1 to 16 taps"), ((1 << 16, 1 << 15, 3, 3), "H \\* W < 2\\^31"),
                        ((1 << 31, 1, 3, 3), "H \\* W < 2\\^31")):
        with pytest.raises(hip.HipError, match=words) as e:
            hip.conv_shape(*args)
        assert str(e.value).startswith(f"[{hip.E_ARG}]") and words.replace("\\", "") in hip.conv_refusal(*args)
    assert hip.conv_shape(1 << 15, (1 << 16) - 1, 16, 16).grid == 1024 * 1024 and hip.conv_refusal(8192, 8192, 16, 16) is None


def test_the_binding_knows_the_new_entry_points():
    assert {"fh_set_conv2d", "fh_conv_shape", "fh_conv_shape_for"} <= set(hip.SIGNATURES)
    assert hasattr(hip.HipContext, "set_conv2d") and hasattr(hip.HipContext, "conv_shape")
    text = open(os.path.join(ROOT, "include", "fasta_hip.h")).read()
    assert f"#define FH_CONV_SHAPE_LEN {hip.CONV_SHAPE_LEN}" in text and "int fh_set_conv2d(fh_ctx* ctx, uint64_t H, uint64_t W, uint32_t kh" in text
    assert "OP_CONV = 9" in open(os.path.join(ROOT, "fasta_python_amd", "csrc", "fh_host_ctx.h")).read()
    assert f"#define CONV_MAXK {hip.CONV_MAX_TAPS}" in open(os.path.join(ROOT, "fasta_python_amd", "csrc", "fh_conv.h")).read()
    assert "ConvMap" in fa.__all__ and fa.ConvMap is fa.linalg.ConvMap
    import fasta
    assert fasta.ConvMap is fa.ConvMap


# ---- the exact step is exact -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", T.SHAPES, ids=T.IDS)
def test_the_exact_model_is_exact(case):
    """int64 on the operands scaled by 32 (every division checked to leave no remainder), float64 and longdouble give the same blocks and the same
    vectors, and every integer stays below 2^50: the sums are exact in float64 whatever their order."""
    i = T.SHAPES.index(case)
    kind = T.PROX_KINDS[i % len(T.PROX_KINDS)]
    x0, b, K, origin, mask = T.exact_operands(case, 500 + i)
    assert np.all(np.abs(x0) <= 2) and np.array_equal(2 * x0, np.round(2 * x0)) and np.array_equal(K, np.round(K)) and np.abs(K).max() <= 2
    iops, fops, lops = T.IntOps(), T.FloatOps(np.float64), T.FloatOps(np.longdouble)
    (bi, vi), (bf, vf), (bl, vl) = (T.exact_step(x0, b, K, origin, mask, kind, ops) for ops in (iops, fops, lops))
    for name in vi:
        assert np.array_equal(vi[name] / 32.0, vf[name]) and np.array_equal(vf[name].astype(np.longdouble), vl[name]), name
    for call in bi:
        want = T.block_as_float(bi[call], iops)
        assert np.array_equal(want, T.block_as_float(bf[call], fops)) and np.array_equal(want, T.block_as_float(bl[call], lops)), call
        assert max(abs(int(v)) for v in bi[call]) < 2 ** 50
    # the magnitudes too: with every term's magnitude summed the bound still holds, so no partial sum of any order leaves the exact range
    assert 32 * 32 * max(float(np.sum(np.abs(v / 32.0)) ** 2) for v in vi.values()) < 2.0 ** 62


def test_the_exact_model_at_256_taps():
    case = ((3, 4), (16, 16), None, False)
    assert case in T.SHAPES
    x0, b, K, origin, mask = T.exact_operands(case, 1)
    K = np.random.RandomState(2).randint(-1, 2, size=(16, 16)).astype(np.float64)           # every tap drawn, none thinned out
    assert (K != 0).sum() > 128
    (bi, vi), (bf, vf), (bl, vl) = (T.exact_step(x0, b, K, origin, mask, "shrink", ops) for ops in (T.IntOps(), T.FloatOps(), T.FloatOps(np.longdouble)))
    for call in bi:
        want = T.block_as_float(bi[call], T.IntOps())
        assert np.array_equal(want, T.block_as_float(bf[call], T.FloatOps())) and np.array_equal(want, T.block_as_float(bl[call], T.FloatOps(np.longdouble)))
    for name in vi:
        assert np.array_equal(vi[name] / 32.0, vf[name]), name


# ---- the fixtures ----------------------------------------------------------------------------------------------------------------------------
def test_the_fixture_set_is_the_capture_scripts_case_table():
    table = capture_script().case_table()
    names = [case[0] for case in table]
    assert sorted(names) == T.CASES and len(names) == 12
    for name, ckw, prox, box, opts in table:
        meta, z, d = T.load(name)
        assert os.path.getsize(os.path.join(T.GOLDEN, name + ".npz")) < 64 * 1024
        assert d["b"].shape == z["solution"].shape == tuple(ckw["shape"]) and max(ckw["shape"]) <= 50 or len(ckw["shape"]) == 1
        assert meta["prox"] == prox and ("twin_divergence" in meta) == bool(opts.get("adaptive")) and ("mask" in d) == (ckw.get("missing", 0.0) > 0.0)
        if "twin_divergence" in meta:
            assert meta["twin_divergence"] >= 20
    modes = {(bool(o.get("adaptive")), bool(o.get("accelerate"))) for *_, o in table}
    assert modes == {(True, False), (False, True), (False, False)}
    assert {p for _, _, p, _, _ in table} == {"shrink", "nonneg", "box", "linf", "l1ball", "none"}
    assert any(o.get("L") == 1.0 and o.get("tau0", 0) > 1 for *_, o in table) and int(T.load("conv_24x20_shrink_backtracking")[1]["backtracks"]) > 0
    assert any(np.any(T.load(n)[2].get("mask", np.ones(1)) == 0.0) for n in names) and any(len(c[1]["shape"]) == 1 for c in table)
    even = T.load("conv_20x22_even_offcentre_adaptive")
    assert even[2]["kernel"].shape == (4, 6) and even[0]["origin"] == [0, 1]
    counts = {n: (int(T.load(n)[1]["iteration_count"]), int(T.load(n)[1]["backtracks"])) for n in names}
    assert counts == {"conv_24x20_shrink_adaptive": (86, 4), "conv_24x20_shrink_accelerated": (102, 0), "conv_24x20_shrink_plain": (843, 0),
                      "conv_24x20_shrink_backtracking": (492, 4), "conv_32x40_nonneg_adaptive": (388, 101), "conv_20x24_box_accelerated": (216, 0),
                      "conv_30x30_linf_accelerated": (407, 0), "conv_30x30_l1ball_adaptive": (36, 0), "conv_16x18_noprox_plain": (775, 0),
                      "conv_25x25_masked_shrink_adaptive": (219, 25), "conv_200_signal_shrink_accelerated": (180, 0),
                      "conv_20x22_even_offcentre_adaptive": (40, 1)}


def assert_same_run(c, z):
    assert c.iteration_count == int(z["iteration_count"]) and c.backtracks == int(z["backtracks"])
    for f in T.FIELDS:
        assert np.array_equal(getattr(c, f), z[f], equal_nan=True), f
    assert np.array_equal(c.solution, z["solution"])


@pytest.mark.parametrize("name", T.CASES)
def test_oracle_and_numpy_backend_reproduce_the_fixture_bit_for_bit(name):
    cap = capture_script()
    meta, z, d = T.load(name)
    ckw = dict(meta["construct"])
    again, origin = cap.construct(**ckw)
    assert all(np.array_equal(again[k], d[k]) for k in d) and set(again) == set(d)
    box = meta.get("box")
    assert_same_run(cap.oracle_run(d, origin, meta["prox"], box, meta["options"], sseed=meta["solver_seed"]), z)
    # the package's generic host loop over ConvMap's host face and the tagged loss / prox ...
    kwargs, tag = T.problem_of(meta, d)
    op = fa.ConvMap(**kwargs)
    loss = fa.LeastSquares(d["b"])
    g, prox = (None, None) if tag is None else (tag.g, tag.prox)
    np.random.seed(meta["solver_seed"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        c = fa.fasta(op, loss.f, loss.gradf, g, prox, np.zeros(d["b"].shape), backend="numpy", verbose=False, **meta["options"])
    assert_same_run(c, z)
    assert op._ctx is None                                                                     # no device context was created
    # ... and over plain closures
    fwd, adj, shape = cap.operator_pair(d, origin)
    f, gradf, gg, proxg = cap.closures(d, meta["prox"], box)
    np.random.seed(meta["solver_seed"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        c = fa.fasta(fa.LinearMap(fwd, adj, shape, shape), f, gradf, gg, proxg, np.zeros(shape), verbose=False, **meta["options"])
    assert_same_run(c, z)


@pytest.mark.parametrize("name", [n for n in T.CASES if "adaptive" in n])
def test_the_twins_parting_iteration_is_the_stored_one(name):
    cap = capture_script()
    meta, z, d = T.load(name)
    _, origin = cap.construct(**meta["construct"])
    k, bt, shorter = cap.twin_divergence(d, origin, meta["prox"], meta.get("box"), meta["options"], meta["solver_seed"])
    assert (k, bt) == (meta["twin_divergence"], meta["backtracks_at_divergence"]) and k >= min(cap.MIN_PREFIX, shorter)
    L, tau0 = cap.step_estimate(d, origin, meta["prox"], meta.get("box"), meta["solver_seed"])
    head = cap.oracle_run(d, origin, meta["prox"], meta.get("box"), dict(meta["options"], max_iters=max(k, 1), tolerance=0.0), L=L, tau0=tau0)
    assert np.array_equal(head.stepsizes[:k], z["stepsizes"][:k])


# ---- what the solver makes of a ConvMap ------------------------------------------------------------------------------------------------------
def why(op, loss, reg, x0):
    return solver._unrecognised(op, None, loss.f, loss.gradf, None if reg is None else reg.g, None if reg is None else reg.prox, x0)


def test_what_the_solver_sends_to_the_device_and_what_it_refuses():
    shape = (6, 7)
    op = fa.ConvMap(shape, np.ones((3, 3)))
    ls = fa.LeastSquares(np.zeros(shape))
    for reg in (None, fa.LinfProx(1.0), fa.L1Ball(1.0), fa.Shrink(0.1), fa.NonNeg(), fa.Box(-1.0, 1.0)):
        assert why(op, ls, reg, np.zeros(shape)) is None
    assert "least squares only" in why(op, fa.LogisticLoss(np.ones(shape)), fa.Shrink(0.1), np.zeros(shape))
    for reg in (fa.TVDualBall(), fa.GroupShrink(0.1)):
        assert "not implemented for a convolution operator" in why(op, ls, reg, np.zeros(shape))
    assert "takes an unknown of that shape" in why(op, ls, fa.Shrink(0.1), np.zeros(42))
    sm = fa.SoftmaxLoss(np.zeros(6, dtype=np.int64), 3)
    assert "SoftmaxLoss is not implemented for a convolution operator" in solver._unrecognised(op, None, sm.f, sm.gradf, None, None, np.zeros(shape))
    assert "linalg.ConvMap" in solver._unrecognised(lambda x: x, lambda x: x, ls.f, ls.gradf, None, None, np.zeros(shape))
    assert op._ctx is None


def test_a_kernel_the_device_refuses_runs_on_the_host_and_raises_under_backend_hip():
    rng = np.random.RandomState(5)
    shape, K = (20, 21), rng.rand(17, 3)
    op = fa.ConvMap(shape, K)
    assert op._ctx is None and "1 to 16 taps" in op.refusal and op.geometry is None
    b = rng.randn(*shape)
    ls, reg = fa.LeastSquares(b), fa.Shrink(0.1)
    runs = []
    for A in (op, fa.LinearMap(lambda x: T.conv(x, K, (8, 1)), lambda w: T.conv(w, K, (8, 1), adjoint=True), shape, shape)):
        np.random.seed(3)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            runs.append(fa.fasta(A, ls.f, ls.gradf, reg.g, reg.prox, np.zeros(shape), verbose=False, max_iters=30))
    assert runs[0].iteration_count == runs[1].iteration_count and np.array_equal(runs[0].solution, runs[1].solution)
    with pytest.raises(TypeError, match="1 to 16 taps"):
        fa.fasta(op, ls.f, ls.gradf, reg.g, reg.prox, np.zeros(shape), backend="hip", verbose=False)
    assert op._ctx is None


def test_a_served_kernel_sets_the_operator_on_first_use(monkeypatch):
    calls = []

    class Recorder:
        def __init__(self, *args, **kwargs):
            calls.append(("create",))

        def set_conv2d(self, shape, kernel, origin, diag):
            calls.append(("conv", tuple(shape), kernel.copy(), tuple(origin), None if diag is None else diag.copy()))

        def close(self):
            pass

    monkeypatch.setattr(hip, "HipContext", Recorder)
    mask = np.arange(10.0)
    op = fa.ConvMap((10,), np.arange(4.0), origin=1, mask=mask)
    assert not calls and op.geometry.tile_w == T.FLAT_W
    op.ctx
    assert calls[0] == ("create",) and calls[1][:2] == ("conv", (1, 10)) and calls[1][2].shape == (1, 4) and calls[1][3] == (0, 1)
    assert calls[1][4].shape == (1, 10) and len(calls) == 2


def test_the_example_counts_the_same_with_tags_and_with_plain_closures(capsys):
    from fasta_python_amd.examples import deconvolution as ex
    args = ["--shape", "24", "28", "--psf", "5", "--missing", "0.2"]
    tags = ex.main(["--backend", "numpy"] + args)
    plain = ex.main(["--backend", "numpy", "--closures"] + args)
    assert [(c.iteration_count, c.backtracks) for _, c in tags] == [(c.iteration_count, c.backtracks) for _, c in plain]
    for (x, _), (y, _) in zip(tags, plain):
        assert np.array_equal(x, y)
    nn = ex.main(["--backend", "numpy", "--shape", "16", "16", "--psf", "3", "--nonneg"])
    assert all(np.all(x >= 0.0) for x, _ in nn)
    out = capsys.readouterr().out
    assert out.count("Completed in") == 9 and out.count("Constructed deconvolution problem") == 3 and out.count("relative error") == 9
    import fasta.examples.deconvolution as drop_in                          # the drop-in name
    assert drop_in.__file__ == ex.__file__ and hasattr(drop_in, "DeconvolutionProblem")

"""GPU tests of the periodic convolution operator (fh_set_conv2d, csrc/fh_conv.h): A x = d * (K conv x), A^H w = K corr (d * w) -- through the
C ABI and through fasta().  Every test first asserts, through fh_conv_shape, the geometry it claims to reach.

Tolerances.  The operator's arithmetic is fixed term by term (accumulator from +0.0, a outer, b inner, a rounded product then a rounded sum, the
diagonal last in A and first in A^H), so `fh_apply` in both directions, x-hat and the elementwise prox are held to the NumPy expressions with
`==`; the two level-search prox kinds are held as the dense tests hold them (rtol 1e-12, atol 4e-16 * n * max(1, max|x|): the level is a
quotient of n-term sums).  One exact step (tests/conv_cases.py): every vector and every FH_S_* scalar `==` the integer model.  Whole solves:
those of DESIGN section 2 -- equal iteration and backtrack counts, histories rtol 1e-6, solution rtol 1e-5 / atol 1e-9, an adaptive run on the
prefix on which the oracle agrees with its own transposed twin."""
import warnings

import numpy as np
import pytest

import fasta_python_amd as fa
from fasta_python_amd import hip
from oracle import fasta_np as fo
from tests import conv_cases as T
from tests import gpu_util as G

pytestmark = pytest.mark.gpu


def open_conv(case, K, mask):
    """(map, context) of a SHAPES entry, the geometry asserted: the pure rule's, the tile the one the shape should take."""
    shape, kshape, origin, _ = case
    op = fa.ConvMap(shape, K, origin=origin if origin is None or len(shape) == 2 else origin[0], mask=mask)
    assert op.refusal is None
    c = op.ctx
    sh = c.conv_shape()
    H, W = T.shape2d(shape)
    kh, kw = T.shape2d(kshape)
    flat = H == 1 and kh == 1
    assert sh == hip.conv_shape(H, W, kh, kw, ncu=c.cu_count()[0]) == op.geometry
    assert (sh.tile_h, sh.tile_w) == ((1, T.FLAT_W) if flat else (T.TILE_H, T.TILE_W)) and sh.run * sh.threads == sh.tile_h * sh.tile_w
    assert sh.tiles_h == -(-H // sh.tile_h) and sh.tiles_w == -(-W // sh.tile_w) and sh.grid == sh.tiles_h * sh.tiles_w
    assert c.shape() == (H * W, H * W) and H * W <= 1 << 16
    return op, c


def test_the_shapes_reach_what_they_claim():
    grids = {T.IDS[i]: hip.conv_shape(*T.shape2d(s), *T.shape2d(k)) for i, (s, k, _, _) in enumerate(T.SHAPES)}
    ragged = hip.conv_shape(*T.RAGGED, 7, 9)
    assert ragged.tiles_h >= 3 and ragged.tiles_w >= 3 and T.RAGGED[0] % T.TILE_H and T.RAGGED[1] % T.TILE_W       # several workgroups on both axes, ragged
    assert hip.conv_shape(1, T.FLAT_W + 1, 1, 16).grid == 2 and hip.conv_shape(1, T.FLAT_W, 1, 3).grid == 1
    assert hip.conv_shape(T.TILE_H, T.TILE_W, 3, 5).grid == 1 and hip.conv_shape(T.TILE_H + 1, T.TILE_W + 1, 5, 3).grid == 4
    assert len(grids) == len(T.SHAPES)


# ---- the operator ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", T.SHAPES, ids=T.IDS)
def test_apply_in_both_directions_is_the_numpy_expression_bit_for_bit(case):
    shape, kshape, origin, masked = case
    rng = np.random.RandomState(len(T.IDS) + T.SHAPES.index(case))
    x, y, K = rng.randn(*shape), rng.randn(*shape), rng.randn(*kshape)
    K.flat[rng.randint(K.size)] = 0.0                                       # a zero tap is a tap: not skipped
    mask = (rng.rand(*shape) < 0.6).astype(np.float64) if masked else None
    o2 = T.origin2d(kshape, origin)
    op, c = open_conv(case, K, mask)
    try:
        z, g = op.device_apply(x), op.device_apply(y, adjoint=True)
        assert z.shape == tuple(shape) and g.shape == tuple(shape)
        assert np.array_equal(z, T.conv(x, K, o2, mask)) and np.array_equal(g, T.conv(y, K, o2, mask, adjoint=True))
        assert np.array_equal(z, op(x)) and np.array_equal(g, op.H(y))       # ... which is what the map does on host arrays
        if masked:
            assert np.all(z[mask == 0.0] == 0.0)
        assert np.array_equal(op.device_apply(x), z) and np.array_equal(op.device_apply(y, adjoint=True), g)      # repeatable
    finally:
        op.close()


# ---- the forward launch with every prox kind -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", T.SHAPES, ids=T.IDS)
def test_one_forward_launch_per_prox_kind(case):
    """Same x0, same g0 (set, not computed), same tau: xhat and xprox of one fh_fwd are x0 - tau * g0 and the tag's NumPy prox of it bit for bit
    (LINF / L1BALL: as the dense tests hold the level search), z is the NumPy expression on the device's xprox bit for bit."""
    shape, kshape, origin, masked = case
    n = int(np.prod(shape))
    rng = np.random.RandomState(300 + T.SHAPES.index(case))
    x0, g0, K, tau = rng.randn(n) * 1.5, rng.randn(n), rng.randn(*kshape), 0.9
    mask = (rng.rand(*shape) < 0.6).astype(np.float64) if masked else None
    o2 = T.origin2d(kshape, origin)
    xh = x0 - tau * g0
    l1 = float(np.abs(xh).sum())
    tags = {"identity": fa.NoProx(), "shrink": fa.Shrink(0.3), "nonneg": fa.NonNeg(), "box": fa.Box(-0.4, 0.7),
            "linf": fa.LinfProx(0.3 * l1 / tau), "l1ball": fa.L1Ball(0.3 * l1)}
    op, c = open_conv(case, K, mask)
    try:
        c.set_loss_lsq(np.zeros(n))
        for kind, tag in tags.items():
            c.set_prox(tag.kind, tag.mu, tag.lo, tag.hi)
            c.set_vector(hip.VEC_X0, x0)
            c.init()
            c.set_vector(hip.VEC_G0, g0)
            s = c.fwd(tau)
            got_h, got_p, z = c.get_vector(hip.VEC_XHAT, n), c.get_vector(hip.VEC_XPROX, n), c.get_vector(hip.VEC_Z, n)
            assert np.array_equal(got_h, xh), kind
            if kind in ("linf", "l1ball"):
                want = fo.prox_linf(xh, tau * tag.mu) if kind == "linf" else fo.project_l1(xh, tag.mu)
                np.testing.assert_allclose(got_p, want, rtol=1e-12, atol=4e-16 * n * max(1.0, np.abs(xh).max()), err_msg=kind)
            else:
                assert np.array_equal(got_p, np.asarray(tag.prox(xh, tau)) * np.ones(n)), kind
            assert np.array_equal(z, T.conv(got_p.reshape(shape), K, o2, mask).ravel()), kind
            assert s[hip.S_GMAX] == np.abs(got_p).max() and s[15] == 0.0
            assert np.array_equal(c.get_vector(hip.VEC_X0, n), x0) and np.array_equal(c.get_vector(hip.VEC_G0, n), g0)
    finally:
        op.close()


# ---- one exact step --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", T.SHAPES, ids=T.IDS)
def test_one_exact_step_every_vector_and_every_scalar(case):
    """init -> fwd -> adj -> fwd_adj -> adj(accel) on the exact operands, the prox kinds rotating over the shapes: every vector and every FH_S_*
    scalar `==` the int64 model (tests/test_conv_cpu.py proves the model exact)."""
    shape = case[0]
    i = T.SHAPES.index(case)
    n = int(np.prod(shape))
    kind = T.PROX_KINDS[i % len(T.PROX_KINDS)]
    x0, b, K, o2, mask = T.exact_operands(case, 500 + i)
    ops = T.IntOps()
    blocks, vec = T.exact_step(x0, b, K, o2, mask, kind, ops)
    op, c = open_conv(case, K, mask)
    try:
        c.set_loss_lsq(b.ravel())
        c.set_prox(*T.prox_args(kind))
        c.set_vector(hip.VEC_X0, x0.ravel())
        got = {"init": c.init().copy()}
        dev = {"g0": c.get_vector(hip.VEC_G0, n)}
        got["fwd"] = c.fwd(T.TAU).copy()
        dev.update(xhat=c.get_vector(hip.VEC_XHAT, n), xprox=c.get_vector(hip.VEC_XPROX, n), z=c.get_vector(hip.VEC_Z, n))
        got["adj"] = c.adj(T.TAU).copy()
        dev["g1"] = c.get_vector(hip.VEC_G1, n)
        got["fwd_adj"] = c.fwd_adj(T.TAU).copy()
        assert np.array_equal(c.get_vector(hip.VEC_G1, n), dev["g1"]) and np.array_equal(c.get_vector(hip.VEC_Z, n), dev["z"])
        got["adj_accel"] = c.adj(T.TAU, accel=True, coef=T.COEF).copy()
        dev.update(x1=c.get_vector(hip.VEC_X1, n), g1_accel=c.get_vector(hip.VEC_G1, n))
    finally:
        op.close()
    for name, v in vec.items():
        assert np.array_equal(dev[name], v.ravel() / ops.unit), name
    for call in ("init", "fwd", "adj", "fwd_adj", "adj_accel"):
        want = T.block_as_float(blocks[call], ops)
        assert np.array_equal(got[call][:15], want[:15]) and got[call][15] == 0.0, (call, got[call], want)


# ---- whole solves ----------------------------------------------------------------------------------------------------------------------------
def solve(meta, d, **extra):
    kwargs, tag = T.problem_of(meta, d)
    op = fa.ConvMap(**kwargs)
    try:
        loss = fa.LeastSquares(d["b"])
        g, prox = (None, None) if tag is None else (tag.g, tag.prox)
        np.random.seed(meta["solver_seed"])
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return fa.fasta(op, loss.f, loss.gradf, g, prox, np.zeros(d["b"].shape), verbose=False, backend="hip", **dict(meta["options"], **extra))
    finally:
        op.close()


@pytest.mark.parametrize("name", T.CASES)
def test_fixture_solves_on_the_device(name):
    meta, z, d = T.load(name)
    k = T.prefix_of(meta, z)
    full = k == int(z["iteration_count"])
    extra = {} if full else dict(max_iters=k, tolerance=0.0)
    lib, again = solve(meta, d, **extra), solve(meta, d, **extra)
    assert lib.library_steps == lib.iteration_count and lib.device_steps == 0
    print(f"\n{name}: device {lib.iteration_count} iterations / {lib.backtracks} backtracks, reference {int(z['iteration_count'])} / {int(z['backtracks'])}", end="")
    if full:
        assert lib.iteration_count == int(z["iteration_count"]) and lib.backtracks == int(z["backtracks"])
    else:
        assert lib.iteration_count == k and lib.backtracks == meta["backtracks_at_divergence"]
    worst = G.compare_histories(lib, lambda f: z[f] if f in z.files else None, k, rtol=1e-6, atol=1e-14)
    print(f"; {k} iterations compared, worst relative deviation of a history entry {worst:.2e}")
    if full:
        np.testing.assert_allclose(lib.solution, z["solution"], rtol=1e-5, atol=1e-9)
    # two runs of a solve are bitwise identical
    assert again.iteration_count == lib.iteration_count and again.backtracks == lib.backtracks
    for f in T.FIELDS:
        if getattr(lib, f) is not None:
            assert np.array_equal(getattr(again, f), getattr(lib, f), equal_nan=True), f
    assert np.array_equal(again.solution, lib.solution)


def test_the_drivers_agree_and_the_device_driver_falls_to_the_library_loop():
    """driver="python" takes the same decisions from the same scalars; driver="device" / device_iters=K have no kernel for this form and take the
    library's loop; fused=True has no one-pass kernel to insist on and is refused."""
    name = next(n for n in T.CASES if n.endswith("accelerated"))
    meta, z, d = T.load(name)
    want = solve(meta, d)
    py = solve(meta, d, driver="python")
    assert py.library_steps == 0 and py.iteration_count == want.iteration_count and np.array_equal(py.solution, want.solution)
    for extra in (dict(driver="device"), dict(device_iters=7)):
        c = solve(meta, d, **extra)
        assert c.device_steps == 0 and c.library_steps == c.iteration_count == want.iteration_count
        assert np.array_equal(c.stepsizes, want.stepsizes) and np.array_equal(c.solution, want.solution)
    with pytest.raises(ValueError, match="fused=True needs a dense operator"):
        solve(meta, d, fused=True)


def test_the_example_runs_on_the_device_and_counts_as_its_numpy_twin(capsys):
    from fasta_python_amd.examples import deconvolution as ex
    for args in ([], ["--nonneg"]):                                          # the default problem, and its non-negative variant
        dev = ex.main(["--backend", "hip"] + args)
        host = ex.main(["--backend", "numpy"] + args)
        assert [(c.iteration_count, c.backtracks) for _, c in dev] == [(c.iteration_count, c.backtracks) for _, c in host]
        for (x, _), (y, _) in zip(dev, host):
            np.testing.assert_allclose(x, y, rtol=1e-5, atol=1e-9)
    out = capsys.readouterr().out
    assert out.count("Completed in") == 12 and out.count("Constructed deconvolution problem") == 4 and out.count("relative error") == 12


def test_the_spectral_norm_through_the_gradient_launches():
    """spectral_norm_squared runs fh_gradient_at with a zero target: A^H (A x - 0), the arithmetic of the host closures term by term, so the power
    iteration on the device is the same iteration on the host bit for bit.  A box blur's largest singular value is its DC gain, 1."""
    K = np.ones((3, 3)) / 9.0
    op = fa.ConvMap((20, 24), K)
    try:
        got = op.spectral_norm_squared(iters=60, rtol=0.0, seed=0)
    finally:
        op.close()
    x = np.random.RandomState(0).randn(480)
    x /= np.linalg.norm(x)
    lam = 0.0
    for _ in range(60):
        y = op.H(op(x.reshape(20, 24))).ravel()
        lam = float(np.dot(x, y))
        x = y / float(np.linalg.norm(y))
    assert got == lam and 0.9 < got <= 1.0 + 1e-12


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------
def refused(call, words):
    with pytest.raises(hip.HipError, match=words) as e:
        call()
    return int(str(e.value).split("]")[0][1:])


def test_what_the_convolution_operator_does_not_serve_is_refused_with_its_code_and_sentence():
    shape, K = (9, 11), np.arange(12.0).reshape(3, 4)
    n = 99
    x = np.random.RandomState(1).randn(*shape)
    op = fa.ConvMap(shape, K)
    c = op.ctx
    try:
        c.set_loss_lsq(np.ones(n))
        c.set_prox(hip.PROX_LINF, 0.5)
        c.set_vector(hip.VEC_X0, x.ravel())
        c.init()
        assert c.fused_supported() == 0 and c.fused_agree() == 0 and not c.run_supported() and c.rhs == 0 and c.nnz() == 0
        assert refused(lambda: c.step(0.1), "fh_step: the convolution operator has no one-pass kernel") == hip.E_STATE
        assert refused(lambda: c.step_begin(0.1), "the convolution operator has no one-pass kernel") == hip.E_STATE
        assert refused(lambda: c.step_accel(0.1, 0.5, True), "fh_step_accel: the convolution operator has no one-pass kernel") == hip.E_STATE
        assert refused(lambda: c.run(4, hip.RunOpts(window=10, stepsize_shrink=0.5), hip.RunState(tau_next=0.1, alpha1=1.0)),
                       "fh_run: the convolution operator has no device-side loop") == hip.E_STATE
        assert refused(lambda: c.set_rhs(2), "the convolution operator has no multi-column form") == hip.E_STATE
        assert refused(lambda: c.comm_init(1, 0, bytes(hip.UNIQUE_ID_BYTES)), "a convolution operator cannot be row-sharded") == hip.E_STATE
        assert refused(lambda: c.get_matrix_rows(0, 1), "the convolution operator keeps no dense rows") == hip.E_STATE
        assert refused(lambda: c.stream_read_ms(), "not on the convolution operator") == hip.E_STATE
        assert refused(lambda: c.set_prox(hip.PROX_TVBALL), "\\(TVBALL / GROUP\\) is not implemented for the convolution operator") == hip.E_ARG
        assert refused(lambda: c.set_prox(hip.PROX_GROUP, 0.1), "FH_PROX_GROUP \\(row-wise l2 shrink\\) needs the multi-column form") == hip.E_ARG
        assert refused(lambda: c.set_prox(hip.PROX_ROWBALL, 0.1), "FH_PROX_ROWBALL .* is served by the quadratic operator only") == hip.E_ARG
        assert refused(lambda: c.set_prox(hip.PROX_ROWSPLIT, 0.1), "FH_PROX_ROWSPLIT") == hip.E_ARG
        assert refused(lambda: c.set_prox(hip.PROX_NUCLEAR, 0.1), "\\(NUCLEAR\\) is not implemented for the convolution operator") == hip.E_ARG
        assert refused(lambda: c.set_loss_logistic(np.ones(n)), "the convolution operator serves the least-squares loss only") == hip.E_STATE
        assert refused(lambda: c.set_loss_softmax(np.zeros(n, dtype=np.int64)), "not for the stencil, DCT, convolution,") == hip.E_STATE
        c.fwd(0.1)                                                # ... and the context still works, with the prox and the loss it had
        c.adj(0.1)
        assert refused(lambda: c.set_conv2d((0, 5), K), "H >= 1 and W >= 1") == hip.E_ARG
        assert refused(lambda: c.set_conv2d((5, 0), K), "H >= 1 and W >= 1") == hip.E_ARG
        assert refused(lambda: c.set_conv2d((5, 5), np.ones((17, 3))), "1 to 16 taps") == hip.E_ARG
        assert refused(lambda: c.set_conv2d((5, 5), np.ones((3, 17))), "1 to 16 taps") == hip.E_ARG
        assert refused(lambda: c.set_conv2d((5, 5), K, origin=(3, 0)), "origin \\(3, 0\\) lies outside") == hip.E_ARG
        assert refused(lambda: c.set_conv2d((5, 5), K, origin=(0, 4)), "origin \\(0, 4\\) lies outside") == hip.E_ARG
        assert refused(lambda: c.set_conv2d((1 << 16, 1 << 15), K), "H \\* W < 2\\^31") == hip.E_ARG
        assert c.shape() == (n, n)                                # a refused call leaves the operator in place
        assert np.array_equal(c.apply(x.ravel()), T.conv(x, K, (1, 2)).ravel())
        # another operator leaves the form, fh_set_conv2d brings it back
        c.set_matrix(np.eye(4))
        assert np.array_equal(c.apply(np.arange(4.0)), np.arange(4.0))
        assert refused(lambda: c.conv_shape(), "holds no convolution operator") == hip.E_STATE
        c.set_conv2d(shape, K, origin=(0, 0))
        assert np.array_equal(c.apply(x.ravel()), T.conv(x, K, (0, 0)).ravel())
    finally:
        op.close()
    with hip.HipContext(devices=[0, 0]) as shell:
        assert refused(lambda: shell.set_conv2d((4, 4), K), "a multi-device context has no convolution operator") == hip.E_STATE
    with hip.HipContext(0, "f32") as narrow:
        assert refused(lambda: narrow.set_conv2d((4, 4), K), "float32 storage") == hip.E_STATE
    with hip.HipContext(0) as plain:                              # a context holding a prox kind this form does not serve returns to IDENTITY
        plain.set_stencil(4, 4)
        plain.set_prox(hip.PROX_TVBALL)
        plain.set_conv2d((2, 4), K)
        plain.set_loss_lsq(np.zeros(8))
        plain.set_vector(hip.VEC_X0, np.arange(8.0))
        plain.init()
        plain.fwd(0.5)
        assert np.array_equal(plain.get_vector(hip.VEC_XPROX, 8), plain.get_vector(hip.VEC_XHAT, 8))
    # the solver's word for the same refusals
    ls = fa.LeastSquares(np.zeros((5, 5)))
    big = fa.ConvMap((5, 5), np.ones((17, 3)))
    assert "1 to 16 taps" in big.refusal
    with pytest.raises(TypeError, match="1 to 16 taps"):
        fa.fasta(big, ls.f, ls.gradf, None, None, np.zeros((5, 5)), backend="hip", verbose=False)
    tv = fa.TVDualBall()
    with pytest.raises(TypeError, match="TVDualBall is not implemented for a convolution operator"):
        fa.fasta(fa.ConvMap((5, 5), K), ls.f, ls.gradf, tv.g, tv.prox, np.zeros((5, 5)), backend="hip", verbose=False)
    with pytest.raises(TypeError, match="takes an unknown of that shape"):
        fa.fasta(fa.ConvMap((5, 5), K), ls.f, ls.gradf, None, None, np.zeros(25), backend="hip", verbose=False)

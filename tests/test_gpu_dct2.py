"""GPU tests of the subsampled 2-D DCT operator (fh_set_dct2, csrc/fh_dct2.h): A x = d * (C_H X C_W^T), A^H w = C_H^T (d * w) C_W, C_L the
orthonormal DCT-II of length L -- through the C ABI and through fasta().  Every test first asserts, through fh_dct2_shape, the geometry it
claims to reach.

Tolerances.  The transform: |dev - exact|_inf <= (beta(H) + beta(W)) * |X|_F, beta(L) = (8 ceil(log2 L) + 8) 2^-53 (tests/dct2_cases.py:bound;
the 1-D operator's bound per axis: the first pass errs by at most beta(W) |row|_2 per entry, the orthonormal second pass carries a column of
those errors at no more than its 2-norm, <= beta(W) |X|_F, and adds beta(H) |column|_2 <= beta(H) |X|_F of its own) against the separable
transform in longdouble; at 2048 x 2048 twice the bound against scipy's dctn / idctn, which carry rounding of their own.  The device
transforms ONE real row per complex FFT -- it does not pack two real rows into one transform -- so the first term carries no factor sqrt(2).
Off-mask entries and 1 x 1 are compared with `==`.  The elementwise arithmetic is bit-exact (`==` against the NumPy expressions); the two
level-search prox kinds are held as the 1-D tests hold them (rtol 1e-12, atol 4e-16 * n * max(1, max|x|)).  Scalars of a step: n * 2^-52
relative to the sum of the magnitudes of the n terms, against sums in longdouble over the DEVICE's own vectors.  Whole solves: equal iteration
and backtrack counts, histories rtol 1e-6 with atol 1e-14, solution rtol 1e-5 with a floor of 1e-6 of its largest entry, an adaptive run on
the prefix on which the oracle agrees with its own twin."""
import warnings

import numpy as np
import pytest

import fasta_python_amd as fa
from fasta_python_amd import hip
from oracle import fasta_np as fo
from tests import dct2_cases as T
from tests import gpu_util as G

pytestmark = pytest.mark.gpu


def open_dct2(shape, mask=None):
    """(map, context) of a 2-D DCT on `shape`, the geometry asserted: the pure rule's."""
    op = fa.DCTMap(shape, mask, lazy=True)
    c = op.ctx
    sh = c.dct2_shape()
    assert sh == hip.dct2_shape(*shape, 0, ncu=c.cu_count()[0]) and sh[:6] == op.geometry[:6]
    T.check_geometry(sh)
    assert (sh.served, sh.H, sh.W, sh.launches) == (1, shape[0], shape[1], 4) and c.shape() == (shape[0] * shape[1],) * 2
    return op, c


def assert_transform(got, v, d, adjoint, what):
    """got against d * (C_H v C_W^T) or C_H^T (d * v) C_W in longdouble; returns error / bound."""
    H, W = v.shape
    d = np.ones(v.shape) if d is None else d
    want = T.exact_dct2(d * v, adjoint=True) if adjoint else d * T.exact_dct2(v)
    scale = 1.0 if adjoint else max(1.0, float(np.abs(d).max()))          # (a general diagonal scales the forward error with the output)
    err, lim = float(np.max(np.abs(got.reshape(v.shape) - want))), T.bound(H, W, np.linalg.norm(d * v if adjoint else v)) * scale
    assert err <= lim, (what, err, lim)
    return err / lim


# ---- the operator ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True], ids=["full", "mask"])
@pytest.mark.parametrize("shape", T.SIZES, ids=T.ident)
def test_apply_in_both_directions_is_the_exact_transform(shape, masked):
    x, y, mask = T.operands(shape, shape[0] * 1000 + shape[1])
    d = mask if masked else None
    op, c = open_dct2(shape, d)
    try:
        z, g = op.device_apply(x), op.device_apply(y, adjoint=True)
        assert z.shape == g.shape == shape
        worst = max(assert_transform(z, x, d, False, "forward"), assert_transform(g, y, d, True, "adjoint"))
        if shape == (1, 1):
            dd = 1.0 if d is None else d[0, 0]
            assert z[0, 0] == (0.0 if dd == 0.0 else dd * x[0, 0]) and g[0, 0] == dd * y[0, 0]
        if masked:
            assert np.all(z[mask == 0.0] == 0.0)
        lhs, rhs = float(np.sum(z * y)), float(np.sum(x * g))               # <A x, y> = <x, A^H y>
        assert abs(lhs - rhs) <= 1e-12 * np.linalg.norm(x) * np.linalg.norm(y)
        if not masked:                                                       # orthonormal: A^H A = I
            back = op.device_apply(z, adjoint=True)
            assert float(np.max(np.abs(back - x))) <= 2 * T.bound(*shape, np.linalg.norm(x))
        print(f"\n{shape}: worst error / bound {worst:.3f}, <Ax,y> - <x,A^H y> = {lhs - rhs:.2e}", end="")
        assert np.array_equal(op.device_apply(x), z) and np.array_equal(op.device_apply(y, adjoint=True), g)      # repeatable
    finally:
        op.close()


def test_one_full_size_apply_in_both_directions():
    """2048 x 2048 against scipy's dctn / idctn with twice the bound (both sides lie within the bound of the truth)."""
    shape = T.FULL_SIZE
    rng = np.random.RandomState(48)
    x, y = rng.randn(*shape), rng.randn(*shape)
    mask = (rng.rand(*shape) < 0.5).astype(np.float64)
    op, c = open_dct2(shape, mask)
    try:
        sh = c.dct2_shape()
        assert sh.lds_h == sh.lds_w == 2048 and sh.rows_h == sh.rows_w == 1 and sh.tiles == 4096
        z, g = op.device_apply(x), op.device_apply(y, adjoint=True)
    finally:
        op.close()
    ef, ea = float(np.abs(z - T.host_fwd(x, mask)).max()), float(np.abs(g - T.host_adj(y, mask)).max())
    lf, la = 2 * T.bound(*shape, np.linalg.norm(x)), 2 * T.bound(*shape, np.linalg.norm(mask * y))
    print(f"\n{shape}: error / (2 x bound) forward {ef / lf:.3f}, adjoint {ea / la:.3f}", end="")
    assert ef <= lf and ea <= la and np.all(z[mask == 0.0] == 0.0)


@pytest.mark.parametrize("shape", [(36, 50), (15, 9)], ids=T.ident)
def test_a_general_diagonal_scales_the_outputs(shape):
    x, y, _ = T.operands(shape, 5)
    d = np.random.RandomState(6).randn(*shape)
    d[::3, ::2] = 0.0
    op, c = open_dct2(shape, d)
    try:
        z, g = op.device_apply(x), op.device_apply(y, adjoint=True)
        assert_transform(z, x, d, False, "forward")
        assert_transform(g, y, d, True, "adjoint")
        assert np.all(z[::3, ::2] == 0.0) and np.any(z != 0.0)
    finally:
        op.close()


# ---- the forward launch with every prox kind -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", T.SIZES, ids=T.ident)
def test_one_forward_launch_per_prox_kind(shape):
    """Same x0, same g0 (set, not computed), same tau: xhat and xprox of one fh_fwd are x0 - tau * g0 and the tag's NumPy prox of it bit for bit
    (LINF / L1BALL: as the 1-D tests hold the level search), z is the transform of the device's xprox within the bound."""
    N = shape[0] * shape[1]
    rng = np.random.RandomState(300 + N)
    x0, g0, tau = rng.randn(N) * 1.5, rng.randn(N), 0.9
    xh = x0 - tau * g0
    l1 = float(np.abs(xh).sum())
    tags = {"identity": fa.NoProx(), "shrink": fa.Shrink(0.3), "nonneg": fa.NonNeg(), "box": fa.Box(-0.4, 0.7),
            "linf": fa.LinfProx(0.3 * l1 / tau), "l1ball": fa.L1Ball(0.3 * l1)}
    mask = T.operands(shape, N)[2]
    op, c = open_dct2(shape, mask)
    try:
        c.set_loss_lsq(np.zeros(N))
        for kind, tag in tags.items():
            c.set_prox(tag.kind, tag.mu, tag.lo, tag.hi)
            c.set_vector(hip.VEC_X0, x0)
            c.init()
            c.set_vector(hip.VEC_G0, g0)
            s = c.fwd(tau)
            got_h, got_p, z = c.get_vector(hip.VEC_XHAT, N), c.get_vector(hip.VEC_XPROX, N), c.get_vector(hip.VEC_Z, N)
            assert np.array_equal(got_h, xh), kind
            if kind in ("linf", "l1ball"):
                want = fo.prox_linf(xh, tau * tag.mu) if kind == "linf" else fo.project_l1(xh, tag.mu)
                np.testing.assert_allclose(got_p, want, rtol=1e-12, atol=4e-16 * N * max(1.0, np.abs(xh).max()), err_msg=kind)
            else:
                assert np.array_equal(got_p, np.asarray(tag.prox(xh, tau)) * np.ones(N)), kind
            assert_transform(z.reshape(shape), got_p.reshape(shape), mask, False, kind)
            assert np.all(z.reshape(shape)[mask == 0.0] == 0.0)
            assert s[hip.S_GMAX] == np.abs(got_p).max() and s[15] == 0.0
            assert np.array_equal(c.get_vector(hip.VEC_X0, N), x0) and np.array_equal(c.get_vector(hip.VEC_G0, N), g0)
    finally:
        op.close()


# ---- the scalars of one step -----------------------------------------------------------------------------------------------------------------
def ld_sum(terms):
    return np.sum(np.asarray(terms, dtype=np.longdouble).ravel())


def prod(a, b):
    return np.asarray(a, dtype=np.longdouble) * np.asarray(b, dtype=np.longdouble)


@pytest.mark.parametrize("shape", T.SIZES, ids=T.ident)
def test_the_scalars_of_one_step_against_a_longdouble_model_of_the_devices_own_vectors(shape):
    """init -> fwd -> adj -> fwd_adj -> adj(accel) on random data, the prox kinds rotating over the shapes: every scalar within n * 2^-52 of the
    longdouble sum of its n float64 terms (formed from the vectors the device wrote), relative to the sum of their magnitudes; maxima `==`."""
    N = shape[0] * shape[1]
    i = T.SIZES.index(shape)
    rng = np.random.RandomState(400 + i)
    x0, b, mask = rng.randn(N), rng.randn(N), T.operands(shape, N)[2]
    tau, coef = 0.5, 0.25
    prox = [(hip.PROX_LINF, 0.2 * N, 0.0, 0.0), (hip.PROX_SHRINK, 0.3, 0.0, 0.0), (hip.PROX_L1BALL, 0.4 * N, 0.0, 0.0), (hip.PROX_BOX, 0.0, -0.4, 0.7),
            (hip.PROX_IDENTITY, 0.0, 0.0, 0.0), (hip.PROX_NONNEG, 0.0, 0.0, 0.0)][i % 6]
    op, c = open_dct2(shape, mask)
    try:
        c.set_loss_lsq(b)
        c.set_prox(*prox)
        c.set_vector(hip.VEC_X0, x0)
        blocks = {"init": c.init().copy()}
        g0, z0 = c.get_vector(hip.VEC_G0, N), c.apply(x0)
        blocks["fwd"] = c.fwd(tau).copy()
        xh, xp, z1 = c.get_vector(hip.VEC_XHAT, N), c.get_vector(hip.VEC_XPROX, N), c.get_vector(hip.VEC_Z, N)
        blocks["adj"] = c.adj(tau).copy()
        g1 = c.get_vector(hip.VEC_G1, N)
        blocks["fwd_adj"] = c.fwd_adj(tau).copy()
        assert np.array_equal(c.get_vector(hip.VEC_G1, N), g1) and np.array_equal(c.get_vector(hip.VEC_Z, N), z1)          # the same launches again
        blocks["adj_accel"] = c.adj(tau, accel=True, coef=coef).copy()
        x1, g1a = c.get_vector(hip.VEC_X1, N), c.get_vector(hip.VEC_G1, N)
    finally:
        op.close()
    assert np.array_equal(xh, x0 - tau * g0) and np.array_equal(x1, xp + coef * (xp - x0))
    # the gradients are the adjoint of the residuals the device formed
    zq = z1 + coef * (z1 - z0)
    for g, r in ((g0, z0 - b), (g1, z1 - b), (g1a, zq - b)):
        assert_transform(g.reshape(shape), r.reshape(shape), mask, True, "gradient")
    dx = xp - x0

    def adj_terms(g, zz, xx):
        dg = g + (xh - x0) / tau
        return {hip.S_DXDG: prod(dx, dg), hip.S_DG2: prod(dg, dg), hip.S_FSQ_ADJ: prod(zz - b, zz - b), hip.S_XH2_ADJ: prod(xx - xh, xx - xh),
                hip.S_GSUM_ADJ: np.abs(xx)}
    fwd_terms = {hip.S_FSQ: prod(z1 - b, z1 - b), hip.S_DXG0: prod(dx, g0), hip.S_DX2: prod(dx, dx), hip.S_XH2: prod(xp - xh, xp - xh),
                 hip.S_G02: prod(g0, g0), hip.S_GSUM: np.abs(xp), hip.S_RDOT: prod(x0 - xp, xp - x0)}
    checks = [("init", {hip.S_FSQ: prod(z0 - b, z0 - b), hip.S_GSUM: np.abs(x0), hip.S_FSQ_ADJ: prod(z0 - b, z0 - b)}),
              ("fwd", fwd_terms), ("adj", adj_terms(g1, z1, xp)), ("fwd_adj", {**fwd_terms, **adj_terms(g1, z1, xp)}),
              ("adj_accel", adj_terms(g1a, zq, x1))]
    worst = 0.0
    for call, terms in checks:
        for k, t in terms.items():
            want, mag = ld_sum(t), ld_sum(np.abs(np.asarray(t, dtype=np.longdouble)))
            err, lim = abs(np.longdouble(blocks[call][k]) - want), N * 2.0 ** -52 * mag
            worst = max(worst, float(err / lim) if lim else 0.0)
            assert err <= lim, (call, k, float(err), float(lim))
        assert blocks[call][15] == 0.0
    print(f"\n{shape}, prox kind {prox[0]}: worst |error| / (n 2^-52 sum of magnitudes) = {worst:.3e}", end="")
    assert blocks["init"][hip.S_GMAX] == np.abs(x0).max() and blocks["fwd"][hip.S_GMAX] == np.abs(xp).max()
    assert blocks["adj"][hip.S_GMAX_ADJ] == np.abs(xp).max() and blocks["adj_accel"][hip.S_GMAX_ADJ] == np.abs(x1).max()


# ---- whole solves ----------------------------------------------------------------------------------------------------------------------------
def solve(meta, d, **extra):
    shape = d["b"].shape
    op, c = open_dct2(shape, d["mask"])
    try:
        loss = fa.LeastSquares(d["b"])
        reg = fa.LinfProx(float(d["mu"])) if meta["prox"] == "linf" else fa.Shrink(float(d["mu"]))
        np.random.seed(meta["solver_seed"])
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return fa.fasta(op, loss.f, loss.gradf, reg.g, reg.prox, np.zeros(shape), verbose=False, backend="hip", **dict(meta["options"], **extra))
    finally:
        op.close()


@pytest.mark.parametrize("name", T.CASES)
def test_fixture_solves_on_the_device(name):
    meta, z, d = T.load(name)
    k = T.prefix_of(meta, z)
    full = k == int(z["iteration_count"])
    extra = {} if full else dict(max_iters=k, tolerance=0.0)
    lib, py = solve(meta, d, driver="library", **extra), solve(meta, d, driver="python", **extra)
    assert lib.library_steps == lib.iteration_count and lib.device_steps == 0 and py.library_steps == 0
    print(f"\n{name}: device {lib.iteration_count} iterations / {lib.backtracks} backtracks, reference {int(z['iteration_count'])} / {int(z['backtracks'])}", end="")
    if full:
        assert lib.iteration_count == int(z["iteration_count"]) and lib.backtracks == int(z["backtracks"])
    else:
        assert lib.iteration_count == k and lib.backtracks == meta["backtracks_at_divergence"]
    worst = G.compare_histories(lib, lambda f: z[f] if f in z.files else None, k, rtol=1e-6, atol=1e-14)
    print(f"; {k} iterations compared, worst relative deviation of a history entry {worst:.2e}")
    assert lib.solution.shape == d["b"].shape
    if full:
        np.testing.assert_allclose(lib.solution, z["solution"], rtol=1e-5, atol=1e-6 * float(np.max(np.abs(z["solution"]))))
    # the two drivers take the same decisions from the same scalars: bit-identical
    assert py.iteration_count == lib.iteration_count and py.backtracks == lib.backtracks
    for f in T.FIELDS:
        if getattr(lib, f) is not None:
            assert np.array_equal(getattr(py, f), getattr(lib, f), equal_nan=True), f
    assert np.array_equal(py.solution, lib.solution)


def test_two_fresh_contexts_run_the_same_solve_bit_for_bit():
    """36 x 50 (ragged tiles, several workgroups per launch, so the finalisers' arrival order varies): 20 accelerated iterations twice."""
    meta, z, d = T.load("dct2_36x50_shrink_accelerated")
    a, b = solve(meta, d, max_iters=20, tolerance=0.0), solve(meta, d, max_iters=20, tolerance=0.0)
    assert a.iteration_count == b.iteration_count == 20
    for f in T.FIELDS:
        assert np.array_equal(getattr(a, f), getattr(b, f), equal_nan=True), f
    assert np.array_equal(a.solution, b.solution)


def test_the_example_runs_on_the_device_with_its_host_twins_counts(capsys):
    from fasta_python_amd.examples import compressive_imaging as ex
    args = ["--shape", "30", "64", "--samples", "900", "--mu", "0.1"]
    host = ex.main(["--backend", "numpy"] + args)
    dev = ex.main(["--backend", "hip"] + args)
    assert [c.iteration_count for _, c in dev] == [c.iteration_count for _, c in host]
    for (x, _), (want, _) in zip(dev, host):
        assert x.shape == (30, 64)
        np.testing.assert_allclose(x, want, rtol=1e-5, atol=1e-6 * float(np.max(np.abs(want))))
    out = capsys.readouterr().out
    assert out.count("Completed in") == 6 and out.count("Constructed compressive imaging problem") == 2


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------
def refused(call, words):
    with pytest.raises(hip.HipError, match=words) as e:
        call()
    return int(str(e.value).split("]")[0][1:])


def test_what_the_2d_dct_operator_does_not_serve_is_refused_with_its_code_and_sentence():
    shape = (12, 8)
    N = 96
    x, y, mask = T.operands(shape, N)
    op, c = open_dct2(shape, mask)
    try:
        c.set_loss_lsq(np.ones(N))
        c.set_prox(hip.PROX_LINF, 0.5)
        c.set_vector(hip.VEC_X0, x)
        c.init()
        assert c.fused_supported() == 0 and c.fused_agree() == 0 and not c.run_supported() and c.rhs == 0 and c.nnz() == 0
        assert refused(lambda: c.step(0.1), "fh_step: the DCT operator has no one-pass kernel") == hip.E_STATE
        assert refused(lambda: c.step_accel(0.1, 0.5, True), "fh_step_accel: the DCT operator has no one-pass kernel") == hip.E_STATE
        assert refused(lambda: c.run(4, hip.RunOpts(window=10, stepsize_shrink=0.5), hip.RunState(tau_next=0.1, alpha1=1.0)),
                       "fh_run: the DCT operator has no device-side loop") == hip.E_STATE
        assert refused(lambda: c.set_rhs(2), "the DCT operator has no multi-column form") == hip.E_STATE
        assert refused(lambda: c.comm_init(1, 0, bytes(hip.UNIQUE_ID_BYTES)), "a DCT operator cannot be row-sharded") == hip.E_STATE
        assert refused(lambda: c.get_matrix_rows(0, 1), "the DCT operator keeps no dense rows") == hip.E_STATE
        assert refused(lambda: c.set_prox(hip.PROX_TVBALL), "\\(TVBALL / GROUP\\) is not implemented for the DCT operator") == hip.E_ARG
        assert refused(lambda: c.set_loss_logistic(np.ones(N)), "the DCT operator serves the least-squares loss only") == hip.E_STATE
        assert refused(lambda: c.dct_shape(), "2-D geometry \\(fh_set_dct2\\): fh_dct2_shape reports it") == hip.E_STATE
        c.fwd(0.1)                                                # ... and the context still works, with the prox and the loss it had
        c.adj(0.1)
        for bad, cap, words in T.REFUSED:
            if cap == 0:
                assert refused(lambda: c.set_dct2(*bad), words) == hip.E_ARG
        assert c.shape() == (N, N)                                # a refused call leaves the operator in place
        z = c.apply(x)
        assert_transform(z.reshape(shape), x, mask, False, "forward")
        # the row cap is read when the operator is set: a later change waits for the next fh_set_dct2
        c.set_tuning(hip.TUNE_DCT_ROW_CAP, 8)
        assert np.array_equal(c.apply(x), z)
        assert refused(lambda: c.set_dct2(12, 8, mask), "row cap \\(8\\).*axis 0 \\(H = 12\\).*no two-level form per axis") == hip.E_ARG
        c.set_tuning(hip.TUNE_DCT_ROW_CAP, 0)
        # replacing operators: the 1-D form, a matrix, and back
        c.set_dct(N)
        assert refused(lambda: c.dct2_shape(), "holds no 2-D DCT operator") == hip.E_STATE and c.dct_shape().levels == 1
        c.set_matrix(np.eye(4))
        assert np.array_equal(c.apply(np.arange(4.0)), np.arange(4.0))
        assert refused(lambda: c.dct2_shape(), "holds no 2-D DCT operator") == hip.E_STATE
        c.set_dct2(8, 12)
        assert (c.dct2_shape().H, c.dct2_shape().W) == (8, 12)
        assert_transform(c.apply(x).reshape(8, 12), x.reshape(8, 12), None, False, "forward")
    finally:
        op.close()
    with hip.HipContext(devices=[0, 0]) as shell:
        assert refused(lambda: shell.set_dct2(8, 8), "a multi-device context has no 2-D DCT operator") == hip.E_STATE
    with hip.HipContext(0, "f32") as narrow:
        assert refused(lambda: narrow.set_dct2(8, 8), "fh_set_dct2: float32 storage") == hip.E_STATE
    # the solver's word for a refused shape
    ls = fa.LeastSquares(np.zeros((7, 8)))
    with pytest.raises(TypeError, match="prime factor above 5"):
        fa.fasta(fa.DCTMap((7, 8)), ls.f, ls.gradf, None, None, np.zeros((7, 8)), backend="hip", verbose=False)

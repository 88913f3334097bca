"""GPU tests of the subsampled DCT operator (fh_set_dct, csrc/fh_dct.h): A = diag(d) * C, A^H = C^T * diag(d), C the orthonormal DCT-II -- through
the C ABI and through fasta().  Every test first asserts, through fh_dct_shape, the geometry it claims to reach.

Tolerances.  The transform: |dev - exact|_inf <= (8 * ceil(log2 N) + 8) * 2^-53 * |x|_2 (tests/dct_cases.py:bound: 8 roundings per radix pass of a
generic butterfly over at most ceil(log2 N) passes, 8 more for the two twiddles and the scale) against a longdouble O(N^2) transform up to
N = 2048, and twice that against scipy.fft beyond (both sides lie within the bound of the truth); N = 1 and off-mask entries are compared with
`==`.  The elementwise arithmetic is bit-exact (`==` against the NumPy expressions); the two level-search prox kinds are held as the dense
tests hold them (rtol 1e-12, atol 4e-16 * n * max(1, max|x|): the level is a quotient of n-term sums).  Scalars of a step: n * 2^-52 relative
to the sum of the magnitudes of the n terms, against sums in longdouble over the DEVICE's own vectors.  Whole solves those of DESIGN section 2:
equal iteration and backtrack counts, histories rtol 1e-6, solution rtol 1e-5 with a floor of 1e-6 of its largest entry, an adaptive run on
the prefix on which the oracle agrees with its own twin."""
import warnings

import numpy as np
import pytest
import scipy.fft

import fasta_python_amd as fa
from fasta_python_amd import hip
from oracle import fasta_np as fo
from tests import dct_cases as T
from tests import gpu_util as G

pytestmark = pytest.mark.gpu
IDS = [f"{N}-cap{cap}" for N, cap in T.SIZES]


def open_dct(N, cap=0, mask=None):
    """(map, context) of a DCT of length N under FH_TUNE_DCT_ROW_CAP = cap (0: the default), the geometry asserted: the pure rule's."""
    op = fa.DCTMap(N, mask, lazy=True, tuning={hip.TUNE_DCT_ROW_CAP: cap} if cap else None)
    c = op.ctx
    sh = c.dct_shape()
    limit = cap or hip.DCT_ROW_CAP
    assert sh == hip.dct_shape(N, cap, ncu=c.cu_count()[0]) and sh[:4] == op.geometry[:4]
    assert sh.N1 * sh.N2 == N and sh.levels == (1 if N <= limit else 2) and max(sh.N1, sh.N2) <= limit and sh.launches == (1 if N <= limit else 5)
    assert c.shape() == (N, N)
    return op, c


LEVEL_RTOL = 1e-12                  # how the suites hold the output of the level search (LINF, L1BALL) against the sort-based host prox


def level_atol(n, xh):
    return 4e-16 * n * max(1.0, np.abs(xh).max())


def reference(v, d, adjoint):
    """(d * C v or C^T (d * v), slack): exact in longdouble up to N = 2048, scipy.fft with twice the bound beyond."""
    N = len(v)
    d = np.ones(N) if d is None else d
    if N <= 2048:
        return (T.exact_dct(d * v, adjoint=True) if adjoint else d * T.exact_dct(v)), 1.0
    return (scipy.fft.idct(d * v, norm="ortho") if adjoint else d * scipy.fft.dct(v, norm="ortho")), 2.0


def assert_transform(got, v, d, adjoint, what):
    want, slack = reference(v, d, adjoint)
    err, lim = float(np.max(np.abs(got - want))), slack * T.bound(len(v), np.linalg.norm(v))
    assert err <= lim, (what, err, lim)
    return err / lim


# ---- the operator ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True], ids=["full", "mask"])
@pytest.mark.parametrize("case", T.SIZES, ids=IDS)
def test_apply_in_both_directions_is_the_exact_transform(case, masked):
    N, cap = case
    x, y, mask = T.operands(N, N)
    d = mask if masked else None
    op, c = open_dct(N, cap, d)
    try:
        z, g = op.device_apply(x), op.device_apply(y, adjoint=True)
        worst = max(assert_transform(z, x, d, False, "forward"), assert_transform(g, y, d, True, "adjoint"))
        if N == 1:
            dd = 1.0 if d is None else d[0]
            assert z[0] == (0.0 if dd == 0.0 else dd * x[0]) and g[0] == dd * y[0]
        if masked:
            assert np.all(z[mask == 0.0] == 0.0)
        lhs, rhs = float(np.dot(z, y)), float(np.dot(x, g))                 # <A x, y> = <x, A^H y>
        assert abs(lhs - rhs) <= 1e-12 * np.linalg.norm(x) * np.linalg.norm(y)
        if not masked:                                                       # orthonormal: A^H A = I
            back = op.device_apply(z, adjoint=True)
            assert float(np.max(np.abs(back - x))) <= 2 * T.bound(N, np.linalg.norm(x))
        print(f"\nN = {N}, cap {cap}: worst error / bound {worst:.3f}, <Ax,y> - <x,A^H y> = {lhs - rhs:.2e}", end="")
        assert np.array_equal(op.device_apply(x), z) and np.array_equal(op.device_apply(y, adjoint=True), g)      # repeatable
    finally:
        op.close()


def test_a_general_diagonal_scales_the_rows():
    N = 96
    x, y, _ = T.operands(N, 5)
    d = np.random.RandomState(6).randn(N)
    d[::7] = 0.0
    for cap in (0, 16):
        op, c = open_dct(N, cap, d)
        try:
            z, g = op.device_apply(x), op.device_apply(y, adjoint=True)
            want_z, want_g = d * T.exact_dct(x), T.exact_dct(d * y, adjoint=True)
            assert np.max(np.abs(z - want_z)) <= T.bound(N, np.linalg.norm(x)) * np.abs(d).max()
            assert np.max(np.abs(g - want_g)) <= T.bound(N, np.linalg.norm(d * y))
            assert np.all(z[::7] == 0.0)
        finally:
            op.close()


@pytest.mark.parametrize("case", T.FULL_SIZE, ids=[str(N) for N, _ in T.FULL_SIZE])
def test_one_full_size_apply_in_both_directions(case):
    N, cap = case
    rng = np.random.RandomState(N % 1000)
    x, y = rng.randn(N), rng.randn(N)
    mask = (rng.rand(N) < 0.5).astype(np.float64)
    op, c = open_dct(N, cap, mask)
    try:
        sh = c.dct_shape()
        assert sh.N2 == 2048 and sh.N1 == N // 2048 and sh.lds1 == sh.lds2 == 2048 and sh.rows1 == sh.rows2 == 1
        z, g = op.device_apply(x), op.device_apply(y, adjoint=True)
        worst = max(assert_transform(z, x, mask, False, "forward"), assert_transform(g, y, mask, True, "adjoint"))
        assert np.all(z[mask == 0.0] == 0.0)
        print(f"\nN = {N}: worst error / (2 x bound) {worst:.3f}", end="")
    finally:
        op.close()


# ---- the forward launch with every prox kind -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", T.SIZES, ids=IDS)
def test_one_forward_launch_per_prox_kind(case):
    """Same x0, same g0 (set, not computed), same tau: xhat and xprox of one fh_fwd are x0 - tau * g0 and the tag's NumPy prox of it bit for bit
    (LINF / L1BALL: as the dense tests hold the level search), z is the transform of the device's xprox within the bound."""
    N, cap = case
    rng = np.random.RandomState(300 + N)
    x0, g0, tau = rng.randn(N) * 1.5, rng.randn(N), 0.9
    xh = x0 - tau * g0
    l1 = float(np.abs(xh).sum())
    tags = {"identity": fa.NoProx(), "shrink": fa.Shrink(0.3), "nonneg": fa.NonNeg(), "box": fa.Box(-0.4, 0.7),
            "linf": fa.LinfProx(0.3 * l1 / tau), "l1ball": fa.L1Ball(0.3 * l1)}
    mask = T.operands(N, N)[2]
    op, c = open_dct(N, cap, mask)
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
                np.testing.assert_allclose(got_p, want, rtol=LEVEL_RTOL, atol=level_atol(N, xh), err_msg=kind)
            else:
                assert np.array_equal(got_p, np.asarray(tag.prox(xh, tau)) * np.ones(N)), kind
            assert_transform(z, got_p, mask, False, kind)
            assert np.all(z[mask == 0.0] == 0.0)
            assert s[hip.S_GMAX] == np.abs(got_p).max() and s[15] == 0.0
            assert np.array_equal(c.get_vector(hip.VEC_X0, N), x0) and np.array_equal(c.get_vector(hip.VEC_G0, N), g0)
    finally:
        op.close()


@pytest.mark.parametrize("kind", ["linf", "l1ball"])
def test_the_level_search_prox_kinds_at_a_length_beyond_the_dense_operators(kind):
    """N = 2^20: above 262144 entries the level search takes its one-workgroup path, which no dense test reaches with this operator.  One fh_fwd,
    xhat bit for bit, xprox held as at the other lengths, z the transform of the device's xprox."""
    N, tau = 1 << 20, 0.9
    rng = np.random.RandomState(20)
    x0, g0 = rng.randn(N) * 1.5, rng.randn(N)
    mask = (rng.rand(N) < 0.5).astype(np.float64)
    xh = x0 - tau * g0
    l1 = float(np.abs(xh).sum())
    tag = fa.LinfProx(0.3 * l1 / tau) if kind == "linf" else fa.L1Ball(0.3 * l1)
    op, c = open_dct(N, 0, mask)
    try:
        assert c.dct_shape()[1:3] == (512, 2048)
        c.set_loss_lsq(np.zeros(N))
        c.set_prox(tag.kind, tag.mu, tag.lo, tag.hi)
        c.set_vector(hip.VEC_X0, x0)
        c.init()
        c.set_vector(hip.VEC_G0, g0)
        s = c.fwd(tau)
        got_h, got_p, z = c.get_vector(hip.VEC_XHAT, N), c.get_vector(hip.VEC_XPROX, N), c.get_vector(hip.VEC_Z, N)
    finally:
        op.close()
    assert np.array_equal(got_h, xh)
    want = fo.prox_linf(xh, tau * tag.mu) if kind == "linf" else fo.project_l1(xh, tag.mu)
    np.testing.assert_allclose(got_p, want, rtol=LEVEL_RTOL, atol=level_atol(N, xh))
    assert_transform(z, got_p, mask, False, kind)
    assert np.all(z[mask == 0.0] == 0.0) and s[hip.S_GMAX] == np.abs(got_p).max() and s[15] == 0.0


# ---- the scalars of one step -----------------------------------------------------------------------------------------------------------------
def ld_sum(terms):
    return np.sum(np.asarray(terms, dtype=np.longdouble).ravel())


def prod(a, b):
    return np.asarray(a, dtype=np.longdouble) * np.asarray(b, dtype=np.longdouble)


@pytest.mark.parametrize("case", T.SIZES, ids=IDS)
def test_the_scalars_of_one_step_against_a_longdouble_model_of_the_devices_own_vectors(case):
    """init -> fwd -> adj -> fwd_adj -> adj(accel) on random data, the prox kinds rotating over the sizes: every scalar within n * 2^-52 of the
    longdouble sum of its n float64 terms (formed from the vectors the device wrote), relative to the sum of their magnitudes; maxima `==`."""
    N, cap = case
    i = T.SIZES.index(case)
    rng = np.random.RandomState(400 + i)
    x0, b, mask = rng.randn(N), rng.randn(N), T.operands(N, N)[2]
    tau, coef = 0.5, 0.25
    prox = [(hip.PROX_LINF, 0.2 * N, 0.0, 0.0), (hip.PROX_SHRINK, 0.3, 0.0, 0.0), (hip.PROX_L1BALL, 0.4 * N, 0.0, 0.0), (hip.PROX_BOX, 0.0, -0.4, 0.7),
            (hip.PROX_IDENTITY, 0.0, 0.0, 0.0), (hip.PROX_NONNEG, 0.0, 0.0, 0.0)][i % 6]
    op, c = open_dct(N, cap, mask)
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
        assert_transform(g, r, mask, True, "gradient")
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
    print(f"\nN = {N}, cap {cap}, prox kind {prox[0]}: worst |error| / (n 2^-52 sum of magnitudes) = {worst:.3e}", end="")
    assert blocks["init"][hip.S_GMAX] == np.abs(x0).max() and blocks["fwd"][hip.S_GMAX] == np.abs(xp).max()
    assert blocks["adj"][hip.S_GMAX_ADJ] == np.abs(xp).max() and blocks["adj_accel"][hip.S_GMAX_ADJ] == np.abs(x1).max()


# ---- whole solves ----------------------------------------------------------------------------------------------------------------------------
def solve(meta, d, cap=0, **extra):
    N = len(d["b"])
    op, c = open_dct(N, cap, d["mask"])
    try:
        loss = fa.LeastSquares(d["b"])
        reg = fa.LinfProx(float(d["mu"])) if meta["prox"] == "linf" else fa.Shrink(float(d["mu"]))
        np.random.seed(meta["solver_seed"])
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return fa.fasta(op, loss.f, loss.gradf, reg.g, reg.prox, np.zeros(N), verbose=False, backend="hip", **dict(meta["options"], **extra))
    finally:
        op.close()


@pytest.mark.parametrize("name", T.CASES)
def test_fixture_solves_on_the_device(name):
    meta, z, d = T.load(name)
    k = T.prefix_of(meta, z)
    full = k == int(z["iteration_count"])
    extra = {} if full else dict(max_iters=k, tolerance=0.0)
    lib, py, again = solve(meta, d, driver="library", **extra), solve(meta, d, driver="python", **extra), solve(meta, d, **extra)
    assert lib.library_steps == lib.iteration_count and lib.device_steps == 0 and py.library_steps == 0
    print(f"\n{name}: device {lib.iteration_count} iterations / {lib.backtracks} backtracks, reference {int(z['iteration_count'])} / {int(z['backtracks'])}", end="")
    if full:
        assert lib.iteration_count == int(z["iteration_count"]) and lib.backtracks == int(z["backtracks"])
    else:
        assert lib.iteration_count == k and lib.backtracks == meta["backtracks_at_divergence"]
    worst = G.compare_histories(lib, lambda f: z[f] if f in z.files else None, k, rtol=1e-6, atol=1e-14)
    print(f"; {k} iterations compared, worst relative deviation of a history entry {worst:.2e}")
    if full:
        np.testing.assert_allclose(lib.solution, z["solution"], rtol=1e-5, atol=1e-6 * float(np.max(np.abs(z["solution"]))))
    # the two drivers take the same decisions from the same scalars, and a second run is the first: bit-identical
    for other in (py, again):
        assert other.iteration_count == lib.iteration_count and other.backtracks == lib.backtracks
        for f in T.FIELDS:
            if getattr(lib, f) is not None:
                assert np.array_equal(getattr(other, f), getattr(lib, f), equal_nan=True), f
        assert np.array_equal(other.solution, lib.solution)


def test_a_fixture_through_the_two_level_transform_and_the_device_driver():
    """N = 60 as 4 x 15 (a row cap of 16): the same run to the same tolerances; driver="device" has no kernel for this form and takes the library's loop."""
    meta, z, d = T.load("dct_60_accelerated")
    want = solve(meta, d)
    two = solve(meta, d, cap=16)
    assert two.iteration_count == int(z["iteration_count"]) and two.backtracks == int(z["backtracks"])
    G.compare_histories(two, lambda f: z[f] if f in z.files else None, two.iteration_count, rtol=1e-6, atol=1e-14)
    np.testing.assert_allclose(two.solution, z["solution"], rtol=1e-5, atol=1e-6 * float(np.max(np.abs(z["solution"]))))
    for extra in (dict(driver="device"), dict(device_iters=7)):
        c = solve(meta, d, **extra)
        assert c.device_steps == 0 and c.library_steps == c.iteration_count == want.iteration_count
        assert np.array_equal(c.stepsizes, want.stepsizes) and np.array_equal(c.solution, want.solution)


def test_the_example_runs_on_the_device_with_the_fixtures_counts(capsys):
    from fasta_python_amd.examples import democratic_representation as ex
    results = ex.main(["--backend", "hip", "--points", "60", "--samples", "30", "--mu", "20"])
    assert [c.iteration_count for _, c in results] == [20, 58, 230]
    for (x, c), name in zip(results, ("dct_60_adaptive", "dct_60_accelerated", "dct_60_plain")):
        want = T.load(name)[1]["solution"]
        np.testing.assert_allclose(x, want, rtol=1e-5, atol=1e-6 * float(np.max(np.abs(want))))
    results = ex.main(["--backend", "hip"])                                # the reference's construct(M=500, N=1000, mu=300.0)
    assert results[0][1].iteration_count == int(T.load("dct_1000_adaptive")[1]["iteration_count"]) == 22
    assert all(x.shape == (1000,) for x, _ in results)
    out = capsys.readouterr().out
    assert out.count("Completed in") == 6 and out.count("Constructed democratic representation problem.") == 2


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------
def refused(call, words):
    with pytest.raises(hip.HipError, match=words) as e:
        call()
    return int(str(e.value).split("]")[0][1:])


def test_what_the_dct_operator_does_not_serve_is_refused_with_its_code_and_sentence():
    N = 60
    x, y, mask = T.operands(N, N)
    op, c = open_dct(N, 0, mask)
    try:
        c.set_loss_lsq(np.ones(N))
        c.set_prox(hip.PROX_LINF, 0.5)
        c.set_vector(hip.VEC_X0, x)
        c.init()
        assert c.fused_supported() == 0 and c.fused_agree() == 0 and not c.run_supported() and c.rhs == 0 and c.nnz() == 0
        assert refused(lambda: c.step(0.1), "fh_step: the DCT operator has no one-pass kernel") == hip.E_STATE
        assert refused(lambda: c.step_begin(0.1), "the DCT operator has no one-pass kernel") == hip.E_STATE
        assert refused(lambda: c.step_accel(0.1, 0.5, True), "fh_step_accel: the DCT operator has no one-pass kernel") == hip.E_STATE
        assert refused(lambda: c.run(4, hip.RunOpts(window=10, stepsize_shrink=0.5), hip.RunState(tau_next=0.1, alpha1=1.0)),
                       "fh_run: the DCT operator has no device-side loop") == hip.E_STATE
        assert refused(lambda: c.set_rhs(2), "the DCT operator has no multi-column form") == hip.E_STATE
        assert refused(lambda: c.comm_init(1, 0, bytes(hip.UNIQUE_ID_BYTES)), "a DCT operator cannot be row-sharded") == hip.E_STATE
        assert refused(lambda: c.get_matrix_rows(0, 1), "the DCT operator keeps no dense rows") == hip.E_STATE
        assert refused(lambda: c.stream_read_ms(), "not on the DCT operator") == hip.E_STATE
        assert refused(lambda: c.set_prox(hip.PROX_TVBALL), "\\(TVBALL / GROUP\\) is not implemented for the DCT operator") == hip.E_ARG
        assert refused(lambda: c.set_prox(hip.PROX_GROUP, 0.1), "FH_PROX_GROUP \\(row-wise l2 shrink\\) needs the multi-column form") == hip.E_ARG
        assert refused(lambda: c.set_prox_split(3, hip.PROX_SHRINK, 0.1), "FH_PROX_ROWSPLIT .* is served by the bilinear operator only") == hip.E_STATE
        assert refused(lambda: c.set_loss_logistic(np.ones(N)), "the DCT operator serves the least-squares loss only") == hip.E_STATE
        c.fwd(0.1)                                                # ... and the context still works, with the prox and the loss it had
        c.adj(0.1)
        assert refused(lambda: c.set_dct(0), "N >= 1") == hip.E_ARG
        assert refused(lambda: c.set_dct(7), "prime factor above 5") == hip.E_ARG
        assert refused(lambda: c.set_dct(1001), "prime factor above 5") == hip.E_ARG
        assert refused(lambda: c.set_dct(3 ** 15), "both factors at most the row cap") == hip.E_ARG
        assert c.shape() == (N, N)                                # a refused call leaves the operator in place
        z = c.apply(x)
        assert_transform(z, x, mask, False, "forward")
        # the row cap is read when the operator is set: a later change waits for the next fh_set_dct
        c.set_tuning(hip.TUNE_DCT_ROW_CAP, 16)
        assert c.dct_shape().levels == 1 and np.array_equal(c.apply(x), z)
        c.set_dct(N, mask)
        assert (c.dct_shape().levels, c.dct_shape().N1, c.dct_shape().N2) == (2, 4, 15)
        assert refused(lambda: c.set_dct(250), "both factors at most the row cap \\(16\\)") == hip.E_ARG
        assert refused(lambda: c.set_tuning(hip.TUNE_DCT_ROW_CAP, 4096), "DCT_ROW_CAP") == hip.E_ARG
        # another operator leaves the form, fh_set_dct brings it back
        c.set_matrix(np.eye(4))
        assert np.array_equal(c.apply(np.arange(4.0)), np.arange(4.0))
        assert refused(lambda: c.dct_shape(), "holds no DCT operator") == hip.E_STATE
        c.set_dct(N)
        assert_transform(c.apply(x), x, None, False, "forward")
    finally:
        op.close()
    with hip.HipContext(devices=[0, 0]) as shell:
        assert refused(lambda: shell.set_dct(60), "a multi-device context has no DCT operator") == hip.E_STATE
    with hip.HipContext(0, "f32") as narrow:
        assert refused(lambda: narrow.set_dct(60), "float32 storage") == hip.E_STATE
    with hip.HipContext(0) as plain:                              # a context holding a prox kind this form does not serve returns to IDENTITY
        plain.set_stencil(4, 4)
        plain.set_prox(hip.PROX_TVBALL)
        plain.set_dct(8)
        plain.set_loss_lsq(np.zeros(8))
        plain.set_vector(hip.VEC_X0, np.arange(8.0))
        plain.init()
        plain.fwd(0.5)
        assert np.array_equal(plain.get_vector(hip.VEC_XPROX, 8), plain.get_vector(hip.VEC_XHAT, 8))
    # the solver's word for the same refusals
    ls = fa.LeastSquares(np.zeros(7))
    with pytest.raises(TypeError, match="prime factor above 5"):
        fa.fasta(fa.DCTMap(7), ls.f, ls.gradf, None, None, np.zeros(7), backend="hip", verbose=False)

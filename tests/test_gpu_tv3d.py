"""GPU tests of the 3-D stencil operator (fh_set_stencil3d, csrc/fh_tv3d.h): A = div : (D, H, W, 3) -> (D, H, W), A^H = grad, periodic -- through
the C ABI and through fasta().  Every test first asserts, through fh_tv3d_shape, the launch geometry it claims to reach.

Tolerances: the stencil and the elementwise arithmetic are bit-exact (`==` against the NumPy expressions); on the exact operands of
tests/tv3d_cases.py every scalar is compared with `==` too; a TV-ball step (a root and divisions: no exact operands) holds its scalars at
n * 2^-52 relative to the sum of the magnitudes of the n terms, against sums in longdouble; whole solves those of DESIGN section 2: equal
iteration and backtrack counts, histories rtol 1e-6, solution rtol 1e-5 with a floor of 1e-6 of its largest entry, an adaptive run on the
prefix on which the oracle agrees with its own twin.
(The padding behind a vector is not addressable through the C ABI, so "no kernel writes padding" cannot be read back here: it follows from
the kernels' index bounds -- every n-side store is at 3 * p + c with p a voxel of the volume, every m-side store at p.)"""
import warnings

import numpy as np
import pytest

import fasta_python_amd as fa
from fasta_python_amd import hip
from tests import gpu_util as G
from tests import tv3d_cases as T

pytestmark = pytest.mark.gpu
IDS = [str(s) for s in T.ALL_SHAPES]


def open_volume(shape, planes=T.PLANES, nt=None):
    """(map, context) of a volume with FH_TUNE_TV3_PLANES forced small (0: the automatic rule), the geometry asserted: the pure rule's, `planes` planes per workgroup."""
    op = fa.GradDivMap(shape)
    c = op.ctx
    c.set_tuning(hip.TUNE_TV3_PLANES, planes)
    if nt is not None:
        c.set_tuning(hip.TUNE_NT_LOADS, nt)
    sh = c.tv3d_shape()
    assert sh[:7] == hip.tv3d_shape(*shape, planes=planes, ncu=c.cu_count()[0])[:7] and sh.NT == (1 if nt else 0)
    assert sh.planes == (min(planes, shape[0]) if planes else sh.planes) and sh.chunks == -(-shape[0] // sh.planes) and (sh.tile_h, sh.tile_w) == (T.TILE_H, T.TILE_W)
    assert np.all(T.owners(shape, sh) == 1)
    assert c.shape() == (int(np.prod(shape)), 3 * int(np.prod(shape)))
    return op, c


def test_the_ragged_shape_reaches_several_workgroups_on_every_axis():
    op, c = open_volume(T.RAGGED)
    try:
        sh = c.tv3d_shape()
        assert sh.chunks >= 2 and sh.tiles_h >= 2 and sh.tiles_w >= 2 and sh.grid == sh.chunks * sh.tiles_h * sh.tiles_w
        assert T.RAGGED[0] % sh.planes and T.RAGGED[1] % sh.tile_h and T.RAGGED[2] % sh.tile_w
    finally:
        op.close()
    for shape in ((17, 9, 130), (9, 40, 257), (4, 33, 65)):             # ... and these reach several on the axes their names promise
        sh = hip.tv3d_shape(*shape, planes=T.PLANES)
        assert sh.chunks >= 2 and sh.tiles_h >= 2 and sh.tiles_w >= 2


@pytest.mark.parametrize("nt", [0, 1], ids=["plain", "nt"])
@pytest.mark.parametrize("shape", T.ALL_SHAPES, ids=IDS)
def test_apply_is_numpys_div_and_grad_bit_for_bit(shape, nt):
    rng = np.random.RandomState(11)
    Y, X = rng.randn(*shape, 3), rng.randn(*shape)
    op, c = open_volume(shape, nt=nt)
    try:
        z, g = op.device_apply(Y), op.device_apply(X, adjoint=True)
        assert np.array_equal(z, T.div(Y)) and np.array_equal(g, T.grad(X))
        lhs, rhs = float(np.sum(z * X)), float(np.sum(Y * g))            # <div Y, X> = <Y, grad X>
        print(f"\n{shape}: <div Y, X> - <Y, grad X> = {lhs - rhs:.3e} of {lhs:.6e}", end="")
        assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs), 1e-300)
        assert np.array_equal(op.device_apply(Y), z) and np.array_equal(op.device_apply(X, adjoint=True), g)      # repeatable
    finally:
        op.close()
    op, c = open_volume(shape, planes=0, nt=nt)                          # the automatic geometry: the same bits
    try:
        assert np.array_equal(op.device_apply(Y), z) and np.array_equal(op.device_apply(X, adjoint=True), g)
    finally:
        op.close()


TAGS = {"tvball": fa.TVDualBall(), "identity": fa.NoProx(), "shrink": fa.Shrink(0.3), "nonneg": fa.NonNeg(), "box": fa.Box(-0.4, 0.7)}


@pytest.mark.parametrize("nt", [0, 1], ids=["plain", "nt"])
@pytest.mark.parametrize("kind", list(TAGS))
def test_prox_outputs_of_one_forward_launch_are_the_numpy_expression_bit_for_bit(kind, nt):
    """Same x0, same g0 (set, not computed), same tau: xhat and xprox of one fh_fwd == x0 - tau * g0 and the tag's NumPy prox of it, on every shape."""
    tag, tau = TAGS[kind], 0.9
    for i, shape in enumerate(T.ALL_SHAPES):
        rng = np.random.RandomState(17 + i)
        x0, g0 = rng.randn(*shape, 3) * 1.5, rng.randn(*shape, 3)
        op, c = open_volume(shape, nt=nt)
        try:
            n = x0.size
            c.set_loss_lsq(np.zeros(shape))
            c.set_prox(tag.kind, tag.mu, tag.lo, tag.hi)
            c.set_vector(hip.VEC_X0, x0)
            c.init()
            c.set_vector(hip.VEC_G0, g0)
            s = c.fwd(tau)
            xh = x0 - tau * g0
            xp = np.asarray(tag.prox(xh, tau)) * np.ones(xh.shape)
            assert np.array_equal(c.get_vector(hip.VEC_XHAT, n).reshape(xh.shape), xh), shape
            assert np.array_equal(c.get_vector(hip.VEC_XPROX, n).reshape(xh.shape), xp), shape
            assert np.array_equal(c.get_vector(hip.VEC_Z, n // 3).reshape(shape), T.div(xp)), shape
            assert s[hip.S_GMAX] == np.abs(xp).max()
            assert np.array_equal(c.get_vector(hip.VEC_X0, n).reshape(xh.shape), x0) and np.array_equal(c.get_vector(hip.VEC_G0, n).reshape(xh.shape), g0)
        finally:
            op.close()


def run_step(c, shape, x0, b, prox, tau, coef):
    """init -> fwd -> adj -> fwd_adj -> adj(accel) through the C ABI: (blocks, vectors) as tests/tv3d_cases.py:exact_step names them."""
    n, m = x0.size, b.size
    vs, ms = tuple(shape) + (3,), tuple(shape)
    c.set_loss_lsq(b)
    c.set_prox(*prox)
    c.set_vector(hip.VEC_X0, x0)
    blocks, vec = {}, {}
    blocks["init"] = c.init().copy()
    vec["g0"] = c.get_vector(hip.VEC_G0, n).reshape(vs)
    blocks["fwd"] = c.fwd(tau).copy()
    vec.update(xhat=c.get_vector(hip.VEC_XHAT, n).reshape(vs), xprox=c.get_vector(hip.VEC_XPROX, n).reshape(vs), z=c.get_vector(hip.VEC_Z, m).reshape(ms))
    blocks["adj"] = c.adj(tau).copy()
    vec["g1"] = c.get_vector(hip.VEC_G1, n).reshape(vs)
    blocks["fwd_adj"] = c.fwd_adj(tau).copy()
    blocks["adj_accel"] = c.adj(tau, accel=True, coef=coef).copy()
    vec.update(x1=c.get_vector(hip.VEC_X1, n).reshape(vs), g1_accel=c.get_vector(hip.VEC_G1, n).reshape(vs))
    return blocks, vec


@pytest.mark.parametrize("nt", [0, 1], ids=["plain", "nt"])
@pytest.mark.parametrize("case", list(enumerate(T.ALL_SHAPES)), ids=IDS)
def test_one_exact_step_every_vector_and_every_scalar(case, nt):
    """Operands that make every sum exactly representable in any order (tests/test_tv3d_cpu.py checks that they do): every vector and each of the
    16 scalars of every call `==` the NumPy model."""
    i, shape = case
    kind = T.PROX_KINDS[i % len(T.PROX_KINDS)]
    x0, b = T.exact_operands(shape, 100 + i)
    ops = T.FloatOps(np.float64)
    want_blocks, want_vec = T.exact_step(x0, b, kind, ops)
    op, c = open_volume(shape, nt=nt)
    try:
        blocks, vec = run_step(c, shape, x0, b, T.prox_args(kind), T.TAU, T.COEF)
        for name, v in want_vec.items():
            assert np.array_equal(vec[name], v), (name, kind)
        for call, block in want_blocks.items():
            want = T.block_as_float(block, ops)
            got = blocks[call]
            assert np.array_equal(got[:15], want[:15]), (call, kind, [(k, got[k], want[k]) for k in range(15) if got[k] != want[k]])
            assert got[15] == 0.0                                           # the one-pass kernels' timeout word: never set by this form
        c.timing_enable(True)                                                # timing runs under the existing kernel ids
        c.fwd(T.TAU), c.adj(T.TAU)
        assert c.timing_get(hip.K_FWD)[1] >= 1 and c.timing_get(hip.K_ADJ)[1] >= 1 and c.timing_get(hip.K_FUSED)[1] == 0
    finally:
        op.close()


def ld_sum(terms):
    return np.sum(np.asarray(terms, dtype=np.longdouble).ravel())


@pytest.mark.parametrize("case", list(enumerate(T.ALL_SHAPES)), ids=IDS)
def test_one_tv_ball_step_against_a_longdouble_model(case):
    """The TV-ball step has a root and divisions, so no exact operands: vectors are bit-equal to the float64 NumPy expressions, every scalar is within
    n * 2^-52 of the longdouble sum of its n float64 terms, relative to the sum of their magnitudes."""
    i, shape = case
    rng = np.random.RandomState(200 + i)
    x0, b = rng.randn(*shape, 3), rng.randn(*shape)
    tau, coef = 0.5, 0.25
    op, c = open_volume(shape)
    try:
        blocks, vec = run_step(c, shape, x0, b, (hip.PROX_TVBALL, 0.0, 0.0, 0.0), tau, coef)
    finally:
        op.close()
    z0 = T.div(x0)
    g0 = T.grad(z0 - b)
    xh = x0 - tau * g0
    xp = xh / np.maximum(np.linalg.norm(xh, axis=-1), 1)[..., np.newaxis]
    z1 = T.div(xp)
    g1 = T.grad(z1 - b)
    x1, zq = xp + coef * (xp - x0), z1 + coef * (z1 - z0)
    g1a = T.grad(zq - b)
    for name, v in dict(g0=g0, xhat=xh, xprox=xp, z=z1, g1=g1, x1=x1, g1_accel=g1a).items():
        assert np.array_equal(vec[name], v), name
    dx = xp - x0

    def sums(terms):
        return {k: (ld_sum(t), ld_sum(np.abs(np.asarray(t, dtype=np.longdouble))), np.asarray(t).size) for k, t in terms.items()}

    def prod(a, b_):
        return np.asarray(a, dtype=np.longdouble) * np.asarray(b_, dtype=np.longdouble)

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
        for k, (want, mag, n) in sums(terms).items():
            err, bound = abs(np.longdouble(blocks[call][k]) - want), n * 2.0 ** -52 * mag
            worst = max(worst, float(err / bound) if bound else 0.0)
            assert err <= bound, (call, k, float(err), float(bound))
    print(f"\n{shape}: worst |error| / (n 2^-52 sum of magnitudes) = {worst:.3e}", end="")
    assert blocks["init"][hip.S_GMAX] == np.abs(x0).max() and blocks["fwd"][hip.S_GMAX] == np.abs(xp).max()
    assert blocks["adj"][hip.S_GMAX_ADJ] == np.abs(xp).max() and blocks["adj_accel"][hip.S_GMAX_ADJ] == np.abs(x1).max()


# ---- whole solves --------------------------------------------------------------------------------------------------------------------------
def solve(meta, d, **extra):
    M, mu = d["M"], float(d["mu"])
    op, c = open_volume(M.shape)
    try:
        loss, reg = fa.LeastSquares(M / mu), (fa.TVDualBall() if meta["prox"] == "ball" else fa.Box(-1.0, 1.0))
        np.random.seed(meta["solver_seed"])
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            conv = fa.fasta(op, op.H, loss.f, loss.gradf, reg.g, reg.prox, np.zeros(M.shape + (3,)), verbose=False, backend="hip", **dict(meta["options"], **extra))
        return conv, M - mu * op(conv.solution)
    finally:
        op.close()


@pytest.mark.parametrize("name", T.CASES)
def test_fixture_solves_on_the_device(name):
    meta, z, d = T.load(name)
    k = T.prefix_of(meta, z)
    full = k == int(z["iteration_count"])
    extra = {} if full else dict(max_iters=k, tolerance=0.0)
    (lib, primal), (py, _), (again, _) = solve(meta, d, driver="library", **extra), solve(meta, d, driver="python", **extra), solve(meta, d, **extra)
    assert lib.library_steps == lib.iteration_count and lib.device_steps == 0 and py.library_steps == 0
    print(f"\n{name}: device {lib.iteration_count} iterations / {lib.backtracks} backtracks, reference {int(z['iteration_count'])} / {int(z['backtracks'])}", end="")
    if full:
        assert lib.iteration_count == int(z["iteration_count"]) and lib.backtracks == int(z["backtracks"])
    else:
        assert k >= 40 and lib.iteration_count == k and lib.backtracks == meta["backtracks_at_divergence"]
    worst = G.compare_histories(lib, lambda f: z[f] if f in z.files else None, k, rtol=1e-6, atol=1e-14)
    print(f"; {k} iterations compared, worst relative deviation of a history entry {worst:.2e}")
    if full:
        np.testing.assert_allclose(lib.solution, z["solution"], rtol=1e-5, atol=1e-6 * float(np.max(np.abs(z["solution"]))))
        np.testing.assert_allclose(primal, z["primal"], rtol=1e-5, atol=1e-6 * float(np.max(np.abs(z["primal"]))))
    # the two drivers take the same decisions from the same scalars, and a second run is the first: bit-identical
    for other in (py, again):
        assert other.iteration_count == lib.iteration_count and other.backtracks == lib.backtracks
        for f in T.FIELDS:
            if getattr(lib, f) is not None:
                assert np.array_equal(getattr(other, f), getattr(lib, f), equal_nan=True), f
        assert np.array_equal(other.solution, lib.solution)


def test_device_driver_falls_to_the_library_loop():
    meta, z, d = T.load("tv3d_6x10x12_accelerated")
    want, _ = solve(meta, d, driver="library")
    for extra in (dict(driver="device"), dict(device_iters=7)):
        c, _ = solve(meta, d, **extra)
        assert c.device_steps == 0 and c.library_steps == c.iteration_count == want.iteration_count
        assert np.array_equal(c.stepsizes, want.stepsizes) and np.array_equal(c.solution, want.solution)


def test_the_example_runs_on_the_device_and_counts_as_the_numpy_backend_does(capsys):
    from fasta_python_amd.examples import tv_denoising3d as ex
    counts = {}
    for backend in ("numpy", "hip"):
        results = ex.main(["--backend", backend, "--shape", "16", "16", "16"])
        counts[backend] = [c.iteration_count for _, c in results]
        assert all(X.shape == (16, 16, 16) for X, _ in results)
    out = capsys.readouterr().out
    assert out.count("Completed in") == 6 and "16 x 16 x 16" in out
    assert counts["hip"][1] == counts["numpy"][1], counts               # the accelerated mode (the adaptive one amplifies summation order)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def status_of(call):
    with pytest.raises(hip.HipError) as e:
        call()
    assert len(str(e.value)) > 20                             # a sentence, not just a code
    return int(str(e.value).split("]")[0][1:])


def test_what_the_3d_stencil_does_not_serve_is_refused_with_its_code():
    shape = (3, 4, 5)
    op, c = open_volume(shape)
    try:
        n = 3 * 60
        c.set_loss_lsq(np.ones(60))
        c.set_prox(hip.PROX_TVBALL)
        c.set_vector(hip.VEC_X0, np.zeros(n))
        c.init()
        assert c.fused_supported() == 0 and c.fused_agree() == 0 and not c.run_supported() and c.rhs == 0 and c.nnz() == 0
        assert status_of(lambda: c.step(0.1)) == hip.E_STATE
        assert status_of(lambda: c.step_begin(0.1)) == hip.E_STATE
        assert status_of(lambda: c.step_accel(0.1, 0.5, True)) == hip.E_STATE
        assert status_of(lambda: c.run(4, hip.RunOpts(window=10, stepsize_shrink=0.5), hip.RunState(tau_next=0.1, alpha1=1.0))) == hip.E_STATE
        assert status_of(lambda: c.set_rhs(2)) == hip.E_STATE
        assert status_of(lambda: c.comm_init(1, 0, bytes(hip.UNIQUE_ID_BYTES))) == hip.E_STATE
        assert status_of(lambda: c.get_matrix_rows(0, 1)) == hip.E_STATE
        assert status_of(lambda: c.stream_read_ms()) == hip.E_STATE
        for kind in (hip.PROX_LINF, hip.PROX_L1BALL, hip.PROX_GROUP):
            assert status_of(lambda: c.set_prox(kind, 0.1)) == hip.E_ARG
        assert status_of(lambda: c.set_loss_logistic(np.ones(60))) == hip.E_STATE
        c.fwd(0.1)                                                # ... and the context still works, with the prox and the loss it had
        c.adj(0.1)
        assert status_of(lambda: c.set_stencil3d(895, 895, 895)) == hip.E_ARG          # 3 * P >= 2^31
        for bad in ((0, 4, 5), (3, 0, 5), (3, 4, 0)):
            assert status_of(lambda: c.set_stencil3d(*bad)) == hip.E_ARG
        assert c.shape() == (60, n)                               # a refused call leaves the operator in place
        rng = np.random.RandomState(3)
        Y = rng.randn(*shape, 3)
        assert np.array_equal(c.apply(Y).reshape(shape), T.div(Y))
        # fh_set_stencil returns the context to the 2-D form (one 2-D apply, still bit-exact), fh_set_stencil3d brings it back
        c.set_stencil(6, 7)
        assert c.shape() == (42, 84)
        assert status_of(lambda: c.tv3d_shape()) == hip.E_STATE
        Y2, X2 = rng.randn(6, 7, 2), rng.randn(6, 7)
        assert np.array_equal(c.apply(Y2).reshape(6, 7), T.div(Y2)) and np.array_equal(c.apply(X2, adjoint=True).reshape(6, 7, 2), T.grad(X2))
        c.set_matrix(np.eye(4))
        assert np.array_equal(c.apply(np.arange(4.0)), np.arange(4.0))
        c.set_stencil3d(*shape)
        assert np.array_equal(c.apply(Y).reshape(shape), T.div(Y))
    finally:
        op.close()
    with hip.HipContext(devices=[0, 0]) as shell:
        assert status_of(lambda: shell.set_stencil3d(3, 4, 5)) == hip.E_STATE
    with hip.HipContext(0) as plain:                              # a context holding a prox kind this form does not serve returns to IDENTITY
        plain.set_matrix(np.eye(4))
        plain.set_prox(hip.PROX_LINF, 0.5)
        plain.set_stencil3d(2, 2, 2)
        plain.set_loss_lsq(np.zeros(8))
        plain.set_vector(hip.VEC_X0, np.arange(24.0))
        plain.init()
        plain.fwd(0.5)
        assert np.array_equal(plain.get_vector(hip.VEC_XPROX, 24), plain.get_vector(hip.VEC_XHAT, 24))

"""One map, many solves: a *Map object keeps ONE context across fasta() calls, and proximal.device_prox switches prox kinds on a cached scratch
context.  Solve P, then Q -- another loss, another prox tag, the other mode -- then P again on the same map: the third Convergence equals the
first bit for bit, and -- for the map classes that have golden fixtures -- equals the home suite's own solve of the fixture on a map of its own, which
the home suite's fixture test (called here) holds to the recorded run; fasta.path twice on one map gives the same grid twice; device_prox
alternating tags on one cached shape equals fresh scratch contexts.  (The C-ABI form of the same question, on
every operator form: tests/test_gpu_carry.py.)"""
import warnings

import numpy as np
import pytest

import fasta_python_amd as fa
from fasta_python_amd import proximal

pytestmark = pytest.mark.gpu
FIELDS = ("residuals", "norm_residuals", "stepsizes", "objectives", "solution")
COUNTERS = ("iteration_count", "backtracks")


def assert_same_convergence(a, b):
    for name in COUNTERS:
        assert getattr(a, name) == getattr(b, name), name
    for name in FIELDS:
        assert np.array_equal(np.asarray(getattr(a, name)), np.asarray(getattr(b, name))), name


def test_device_prox_alternates_tags_on_one_cached_shape():
    """shrink, the l1 ball (a level search that starts from the level the scratch context last held) and l-infinity in turn, twice, on one
    cached shape: the elementwise kind bit for bit what fresh scratch contexts give; the level-search kinds as the suites hold the level search"""
    from tests.test_gpu_dct import LEVEL_RTOL, level_atol
    rng = np.random.RandomState(4)
    x = rng.randn(20001) * 1.5
    tags = (fa.Shrink(0.3), fa.L1Ball(0.3 * float(np.abs(x).sum())), fa.LinfProx(0.3 * float(np.abs(x).sum())))
    fresh = []
    for tag in tags:
        proximal.release_scratch()
        fresh.append(proximal.device_prox(tag, x, 1.0))
    proximal.release_scratch()
    try:
        for rep in range(2):
            for tag, want in zip(tags, fresh):
                got = proximal.device_prox(tag, x, 1.0)
                if isinstance(tag, fa.Shrink):
                    assert np.array_equal(got, want), (rep, tag)
                else:
                    np.testing.assert_allclose(got, want, rtol=LEVEL_RTOL, atol=level_atol(x.size, x))
                    np.testing.assert_allclose(got, np.asarray(tag.prox(x, 1.0)), rtol=LEVEL_RTOL, atol=level_atol(x.size, x))
    finally:
        proximal.release_scratch()


# ---- the map classes with golden fixtures: P is the fixture, through the home suite's loader, solve and fixture comparison -----------------------------
def _fasta(seed, args, options):
    np.random.seed(seed)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fa.fasta(*args, verbose=False, backend="hip", **options)


def _other_mode(options, gap, device=True):
    """Q's options: adaptive and accelerate swapped, a short run; the device loop in calls of 4 iterations (forms it does not serve fall to the library
    loop), and the duality-gap stop rule where the form serves the certificate and the run is not accelerated"""
    o = dict(options, adaptive=not options.get("adaptive", True), accelerate=not options.get("accelerate", False), max_iters=24)
    if device:                                                                      # (the identity operator refuses the device driver by name)
        o["device_iters"] = 4
    if gap and not o["accelerate"]:
        o["stop_rule"] = fa.DualityGap(1e-3)
    return o


def _linear(G, T, name, make_op, tag_of, x0_of, six, gap, b_of=lambda d: d["b"]):
    """(run P on op, run Q on op, the home solve on a map of its own, the home fixture test) of a map class whose home solve builds its own map"""
    meta, z, d = T.load(name)
    op = make_op(meta, d)
    head = (lambda: (op,)) if six else (lambda: (op, op.H))
    tag = tag_of(meta, d)
    g, prox = (None, None) if tag is None else (tag.g, tag.prox)
    loss, other = fa.LeastSquares(b_of(d)), fa.LeastSquares(np.flip(b_of(d)).copy() * 0.5)
    shrink = fa.Shrink(0.25)
    run_p = lambda: _fasta(meta["solver_seed"], head() + (loss.f, loss.gradf, g, prox, x0_of(d)), meta["options"])
    run_q = lambda: _fasta(3, head() + (other.f, other.gradf, shrink.g, shrink.prox, x0_of(d)), _other_mode(meta["options"], gap))
    first = lambda c: c[0] if isinstance(c, tuple) else c
    return op, run_p, run_q, (lambda: first(G.solve(meta, d))), (lambda: G.test_fixture_solves_on_the_device(name))


def conv_map():
    from tests import conv_cases as T, test_gpu_conv as G
    return _linear(G, T, T.CASES[0], lambda meta, d: fa.ConvMap(**T.problem_of(meta, d)[0]), lambda meta, d: T.problem_of(meta, d)[1],
                   lambda d: np.zeros(d["b"].shape), six=True, gap=True)


def dct_map():
    from tests import dct_cases as T, test_gpu_dct as G
    return _linear(G, T, T.CASES[0], lambda meta, d: fa.DCTMap(len(d["b"]), d["mask"], lazy=True),
                   lambda meta, d: fa.LinfProx(float(d["mu"])) if meta["prox"] == "linf" else fa.Shrink(float(d["mu"])), lambda d: np.zeros(len(d["b"])), six=True, gap=True)


def dct2_map():
    from tests import dct2_cases as T, test_gpu_dct2 as G
    return _linear(G, T, T.CASES[0], lambda meta, d: fa.DCTMap(d["b"].shape, d["mask"], lazy=True),
                   lambda meta, d: fa.LinfProx(float(d["mu"])) if meta["prox"] == "linf" else fa.Shrink(float(d["mu"])), lambda d: np.zeros(d["b"].shape), six=True, gap=True)


def tv3d_map():
    from tests import test_gpu_tv3d as G, tv3d_cases as T
    return _linear(G, T, T.CASES[0], lambda meta, d: fa.GradDivMap(d["M"].shape), lambda meta, d: fa.TVDualBall() if meta["prox"] == "ball" else fa.Box(-1.0, 1.0),
                   lambda d: np.zeros(d["M"].shape + (3,)), six=False, gap=False, b_of=lambda d: d["M"] / float(d["mu"]))


def sparse_map():
    from tests import test_gpu_sparse as G
    name = next(n for n in G.CASES if G.load(n)[0]["kind"] == "lasso")
    meta, z, d = G.load(name)
    op = fa.SparseMatrixMap(G.capture_script().matrix_of(d))
    other, shrink = fa.LogisticLoss(np.where(d["b"] >= 0, 1.0, -1.0)), fa.Shrink(0.25)
    run_q = lambda: _fasta(3, (op, op.H, other.f, other.gradf, shrink.g, shrink.prox, np.zeros(op.shape[1])), _other_mode(G.H.resolve_options(dict(meta["options"]), G.fstop), True))
    return op, (lambda: G.solve(meta, d, op=op)), run_q, (lambda: G.solve(meta, d)), (lambda: G.test_fixture_solves_on_the_device(name))


def _tagged(G, C, name, device=True):
    """the operators that bring their smooth term (quadratic, bilinear, identity): the map lives in the tagged closures, built ONCE here.  P is the
    home suite's library_run of the fixture (its compared prefix), which its fixture test holds to the recording."""
    meta, z, d = C.load(name)
    k, whole = C.compared_prefix(meta, z)
    ms = C.capture_script()
    f, gradf, g, proxg, x0 = ms.operands(fa, meta["kind"], d)
    o = ms.resolve(meta["options"], G.fstop)
    o_p = dict(o, driver="library", **({} if whole else dict(max_iters=k, tolerance=0.0)))
    run_p = lambda: _fasta(1, (None, None, f, gradf, g, proxg, x0), o_p)
    run_q = lambda: _fasta(3, (None, None, f, gradf, None, None, x0), _other_mode(o, False, device))
    return None, run_p, run_q, (lambda: G.library_run(name)[0]), (lambda: G.test_fixture_solves_on_the_device(name))


def _recorded(G, name, gap):
    """the dense and the 2-D stencil map: P is a recorded reference run, solved as tests/gpu_util.py:run_hip solves it but on a map that stays"""
    from fasta_python_amd import stopping as fstop
    from tests import gpu_util as U, helpers as H
    meta, z = H.load_case(name)
    data = H.case_data(meta, z)
    A, loss, reg, x0 = U.hip_operands(meta["kind"], data)
    o = H.resolve_options(meta["options"], fstop)
    o.pop("g_none", None)
    b = data["M"] / float(data["mu"]) if meta["kind"] == "tv" else np.asarray(data["b"])
    other = fa.LeastSquares(0.5 * np.flip(b).copy())
    other_reg = fa.NoProx() if meta["kind"] == "tv" else fa.Shrink(0.5 * float(data["mu"]))
    run_p = lambda: _fasta(meta["solver_seed"], (A, A.H, loss.f, loss.gradf, reg.g, reg.prox, x0), o)
    run_q = lambda: _fasta(3, (A, A.H, other.f, other.gradf, other_reg.g, other_reg.prox, x0), _other_mode(o, gap))
    return A, run_p, run_q, (lambda: U.run_hip(meta["kind"], data, meta["options"], meta["solver_seed"])), (lambda: G.test_golden_parity_full_solve(name))


def dense_map():
    from tests import test_gpu_dense as G
    return _recorded(G, "sparse_ls_64x128_accelerated", gap=True)                  # (Q: adaptive, not accelerated, under the duality-gap rule, device driver)


def graddiv2d_map():
    from tests import test_gpu_prox_tv as G
    return _recorded(G, "tv_32x32_plain", gap=False)                               # (Q: adaptive and accelerated: the lazily-kept iterate)


def quad_map():
    from tests import quad_cases as C, test_gpu_quad as G
    return _tagged(G, C, C.FIXTURES[1])


def factor_map():
    from tests import factor_cases as C, test_gpu_factor as G
    return _tagged(G, C, C.FIXTURES[1])


def identity_map():
    from tests import nuclear_cases as C, test_gpu_nuclear as G
    return _tagged(G, C, C.FIXTURES[1], device=False)


MAPS = {"dense": dense_map, "graddiv2d": graddiv2d_map, "sparse": sparse_map, "quadratic": quad_map, "bilinear": factor_map, "identity": identity_map, "graddiv3d": tv3d_map, "dct": dct_map, "dct2": dct2_map,
        "conv": conv_map}


@pytest.mark.parametrize("kind", list(MAPS))
def test_a_fixture_solved_again_after_another_problem_on_the_same_map(kind):
    op, run_p, run_q, home, fixture_test = MAPS[kind]()
    try:
        first = run_p()
        other = run_q()
        third = run_p()
        assert first.iteration_count >= 2 and other.iteration_count >= 1
        assert_same_convergence(third, first)
        assert_same_convergence(home(), first)                                      # the home suite's own solve, on a map of its own: the same bits ...
    finally:
        if op is not None:
            op.close()
        proximal.release_scratch()
    fixture_test()                                                                  # ... which the home suite's fixture test holds to the recorded run


def test_the_path_twice_on_one_map_gives_the_same_grid():
    rng = np.random.RandomState(8)
    A = rng.randn(64, 128) / 8.0                                                    # (the problem of tests/test_gpu_gap.py:test_the_path_on_the_device)
    xt = np.zeros(128)
    xt[rng.permutation(128)[:5]] = 2.0 * rng.randn(5)
    loss = fa.LeastSquares(A @ xt + 0.01 * rng.randn(64))
    op = fa.DenseMatrixMap(A)
    try:
        grids = []
        for _ in range(2):
            np.random.seed(2)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                grids.append(fa.path(op, loss, fa.Shrink, n_mus=5, ratio=1e-2, gap_tolerance=1e-7, backend="hip", max_iters=5000))
        assert len(grids[0]) == len(grids[1]) == 5 and grids[0][-1].solution.any()
        for a, b in zip(*grids):
            assert a.mu == b.mu and a.iteration_count == b.iteration_count and tuple(a.certificate) == tuple(b.certificate)
            assert np.array_equal(a.solution, b.solution) and np.array_equal(a.residuals, b.residuals)
    finally:
        op.close()

"""CPU tier of matrix completion from partial observations: observation weights on the two elementwise losses (losses.LeastSquares /
LogisticLoss(B, weights=W), fh_set_loss_weights) and the nuclear-norm ball (proximal.NuclearBall, FH_PROX_NUCBALL).  The fixtures
tests/golden/completion/*.npz were captured from the reference core (scripts/make_completion_golden.py) with the tags' host closures and the
identity operator; the NumPy oracle and `fasta(None, None, ..., backend="numpy")` must reproduce them bit for bit, the closures must be the
written forms, `weights=None` must be the tags as they were, an unobserved entry must contribute exactly zero, the NumPy restatement of the
device's level rule must equal project_L1_ball bit for bit on every GPU-tier case, operand recognition must serve what the device serves and
name what it does not, and nothing may fall back.  No GPU."""
import os
import warnings

import numpy as np
import pytest
from numpy import linalg as la

import fasta_python_amd as fa
from fasta_python_amd import hip
from fasta_python_amd.solver import _unrecognised as why
from tests import completion_cases as CC


def assert_same_run(c, z):
    assert c.iteration_count == int(z["iteration_count"]) and c.backtracks == int(z["backtracks"])
    for field in CC.HISTORIES:
        assert np.array_equal(getattr(c, field), z[field], equal_nan=True), field
    assert np.array_equal(c.solution, z["solution"])


# ---- the fixture set ---------------------------------------------------------------------------------------------------------------------------
def test_the_fixture_set_is_the_one_the_script_describes():
    names = [row[0] for row in CC.capture_script().case_table()]
    assert sorted(names) == CC.FIXTURES == CC.EXPECTED
    assert all(os.path.getsize(os.path.join(CC.GOLDEN, n + ".npz")) < 100 << 10 for n in CC.FIXTURES)


def test_the_fixtures_cover_what_the_issue_lists_and_hold_the_scripts_assertions():
    seen = set()
    for name in CC.EXPECTED:
        meta, z, d = CC.load(name)
        o = meta["options"]
        shape = d["B"].shape
        assert o["evaluate_objective"] and o["L"] > 0 and o["tau0"] > 0 and z["solution"].shape == d["x0"].shape == d["W"].shape == shape, name
        assert (d["W"] >= 0).all() and np.isfinite(d["W"]).all() and 0.5 < np.mean(d["W"] != 0) < 0.8, name      # partial observations
        seen.add((meta["kind"], "adaptive" if o["adaptive"] else "accelerated" if o["accelerate"] else "plain", shape))
        s = la.svd(z["solution"], compute_uv=False)
        if meta["kind"] != "wlsq_shrink":                # a rank strictly between 0 and p
            assert 0 < meta["solution_rank"] < min(shape) and int(np.sum(s > 1e-3 * s[0])) == meta["solution_rank"], name
        if meta["kind"].endswith("ball"):                # the constraint is active at the solution
            assert abs(s.sum() - float(d["radius"])) <= 1e-6 * float(d["radius"]), name
        if meta["kind"].startswith("wlog"):
            assert set(np.unique(d["B"])) <= {-1.0, 1.0}, name
    assert {("wlsq_nuc", "adaptive", (12, 20)), ("wlsq_nuc", "accelerated", (12, 20)), ("wlsq_nuc", "plain", (12, 20)), ("wlsq_nuc", "adaptive", (20, 12)),
            ("wlsq_ball", "adaptive", (12, 20)), ("wlsq_ball", "accelerated", (12, 20)), ("wlog_nuc", "adaptive", (12, 20)),
            ("wlog_ball", "adaptive", (12, 20)), ("wlsq_shrink", "adaptive", (9, 7))} <= seen
    meta, z, _ = CC.load("wlsq_nuc_12x20_backtracks")
    assert int(z["backtracks"]) >= 2 and meta["options"]["tau0"] == 40 * (2 / meta["options"]["L"]) / 10
    assert len(set(np.unique(CC.load("wlsq_shrink_9x7_adaptive")[2]["W"]))) > 2                                  # real weights, not a mask


@pytest.mark.parametrize("name", CC.EXPECTED)
def test_twin_parting_iteration_is_recomputed(name):
    """The oracle and a twin of itself with permuted rows and columns (B, W and x0 alike; same L, same tau0) agree on every step size up to the
    stored iteration; a prefix must have at least 30 iterations or be the whole run."""
    meta, z, d = CC.load(name)
    assert CC.capture_script().twin_divergence(meta["kind"], d, meta["options"]) == meta["twin_divergence"]
    k, whole = CC.compared_prefix(meta, z)
    assert whole or k >= CC.MIN_PREFIX


# ---- bit-for-bit reproduction ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CC.EXPECTED)
def test_oracle_reproduces_the_reference_run(name):
    meta, z, d = CC.load(name)
    assert_same_run(CC.capture_script().run_oracle(meta["kind"], d, meta["options"]), z)


@pytest.mark.parametrize("name", CC.EXPECTED)
def test_host_loop_reproduces_the_reference_run(name):
    meta, z, d = CC.load(name)
    ms = CC.capture_script()
    f, gradf, g, proxg, x0 = ms.operands(fa, meta["kind"], d)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        c = fa.fasta(None, None, f, gradf, g, proxg, x0, backend="numpy", verbose=False, **ms.resolve(meta["options"], fa.stopping))
    assert_same_run(c, z)


# ---- the tags ------------------------------------------------------------------------------------------------------------------------------------
def _seeded(shape=(7, 9), seed=3):
    rng = np.random.RandomState(seed)
    return rng.randn(*shape), np.sign(rng.randn(*shape)), rng.randn(*shape), (rng.rand(*shape) < 0.6)


def test_weights_none_is_the_tag_as_it_was():
    Z, B, Bv, _ = _seeded()
    ls = fa.LeastSquares(Bv)
    assert ls.weights is None and ls.f(Z) == .5 * la.norm((Z - Bv).ravel()) ** 2 == ls(Z) and np.array_equal(ls.gradf(Z), Z - Bv)
    assert ls.f.__func__ is fa.LeastSquares.f and ls.gradf.__func__ is fa.LeastSquares.gradf                    # the class's own methods, not the weighted ones
    ll = fa.LogisticLoss(B)
    assert ll.weights is None and ll.f(Z) == np.sum(np.log(1 + np.exp(Z)) - (B == 1) * Z) == ll(Z)
    assert np.array_equal(ll.gradf(Z), -B / (1 + np.exp(B * Z))) and ll.f.__func__ is fa.LogisticLoss.f
    assert fa.LeastSquares(Bv, weights=None).f(Z) == ls.f(Z) and fa.LogisticLoss(B, None).f(Z) == ll.f(Z)

    class Recorder:
        calls = []

        def __getattr__(self, name):
            return lambda *a: self.calls.append(name)

    ls.bind(Recorder())
    ll.bind(Recorder())
    assert Recorder.calls == ["set_loss_lsq", "set_loss_logistic"]                                                # fh_set_loss_weights is never called


def test_the_weighted_closures_are_the_written_forms():
    Z, B, Bv, mask = _seeded()
    W = mask * np.random.RandomState(4).choice([0.25, 1.0, 3.5], size=Z.shape)
    ls = fa.LeastSquares(Bv, weights=W)
    sqrtW = np.sqrt(W)
    assert ls.f(Z) == .5 * la.norm((sqrtW * (Z - Bv)).ravel()) ** 2 == ls(Z) and np.array_equal(ls.gradf(Z), W * (Z - Bv))
    ll = fa.LogisticLoss(B, weights=W)
    assert ll.f(Z) == np.sum(W * (np.log(1 + np.exp(Z)) - (B == 1) * Z)) == ll(Z)
    assert np.array_equal(ll.gradf(Z), W * (-B / (1 + np.exp(B * Z))))
    assert ls.f.__self__ is ls and ll.gradf.__self__ is ll                                                        # still recognisable as the tag's own
    calls = []

    class Recorder:
        def __getattr__(self, name):
            return lambda *a: calls.append((name, a[0]))

    ls.bind(Recorder())
    assert [c[0] for c in calls] == ["set_loss_lsq", "set_loss_weights"] and calls[1][1] is ls.weights            # the loss, then the weights


def test_all_ones_weights_give_the_unweighted_bits_and_a_mask_restricts_the_loss():
    Z, B, Bv, mask = _seeded()
    ones = np.ones(Z.shape)
    assert fa.LeastSquares(Bv, weights=ones).f(Z) == fa.LeastSquares(Bv).f(Z) and np.array_equal(fa.LeastSquares(Bv, weights=ones).gradf(Z), Z - Bv)
    assert fa.LogisticLoss(B, weights=ones).f(Z) == fa.LogisticLoss(B).f(Z)
    assert np.array_equal(fa.LogisticLoss(B, weights=ones).gradf(Z), fa.LogisticLoss(B).gradf(Z))
    for W in (mask, mask.astype(np.float64), mask.astype(np.int32)):                                              # a boolean mask becomes 0.0 / 1.0
        ls, ll = fa.LeastSquares(Bv, weights=W), fa.LogisticLoss(B, weights=W)
        assert ls.weights.dtype == np.float64 and set(np.unique(ls.weights)) == {0.0, 1.0}
        n = int(mask.sum())
        # (the restricted sum adds the same terms without the zeros between them: the same value up to the order of a sum of n terms)
        assert abs(ls.f(Z) - fa.LeastSquares(Bv[mask]).f(Z[mask])) <= n * CC.EPS * ls.f(Z)
        assert abs(ll.f(Z) - fa.LogisticLoss(B[mask]).f(Z[mask])) <= n * CC.EPS * np.sum(np.abs(np.log(1 + np.exp(Z)) - (B == 1) * Z)[mask])
        for loss, plain in ((ls, fa.LeastSquares(Bv)), (ll, fa.LogisticLoss(B))):
            G = loss.gradf(Z)
            assert np.array_equal(G[mask], plain.gradf(Z)[mask]) and not G[~mask].any()


def test_an_unobserved_entry_contributes_exactly_zero_whatever_z_is():
    Z, B, Bv, mask = _seeded()
    mask[0, 0] = mask[1, 2] = False
    for far in (800.0, -800.0):
        Zf = Z.copy()
        Zf[~mask] = far
        with warnings.catch_warnings():
            warnings.simplefilter("error")                 # ... and without a warning from the host closures
            for sign in (1.0, -1.0):
                ll = fa.LogisticLoss(sign * B, weights=mask)
                G = ll.gradf(Zf)
                assert np.isfinite(ll.f(Zf)) and ll.f(Zf) == ll.f(np.where(mask, Z, 0.0)) - 0.0 * np.log(2) and np.isfinite(G).all()
                assert np.array_equal(G[~mask], np.zeros(int((~mask).sum()))) and np.array_equal(G[mask], fa.LogisticLoss(sign * B).gradf(Z)[mask])
            ls = fa.LeastSquares(Bv, weights=mask)
            assert ls.f(Zf) == ls.f(Z) and not ls.gradf(Zf)[~mask].any()


def test_validation_errors_name_the_first_offender():
    B = np.zeros((3, 4))
    for cls in (fa.LeastSquares, fa.LogisticLoss):
        with pytest.raises(ValueError, match=r"weights must have B's shape \(3, 4\) \(got \(4, 3\)\)"):
            cls(B, weights=np.ones((4, 3)))
        W = np.ones((3, 4))
        W[1, 2], W[2, 0] = -0.5, np.nan
        with pytest.raises(ValueError, match=r"finite and >= 0 \(entry \(1, 2\) is -0\.5\)"):
            cls(B, weights=W)
        W[1, 2] = 1.0
        with pytest.raises(ValueError, match=r"entry \(2, 0\) is nan"):
            cls(B, weights=W)
        W[2, 0] = np.inf
        with pytest.raises(ValueError, match=r"entry \(2, 0\) is inf"):
            cls(B, weights=W)
        with pytest.raises(ValueError, match="real numbers or a boolean mask"):
            cls(B, weights=np.ones((3, 4), dtype=complex))
    with pytest.raises(ValueError, match=r"entry 1 is -1\.0"):
        fa.LeastSquares(np.zeros(3), weights=[1.0, -1.0, -2.0])
    for bad in (-1.0, np.nan, np.inf):
        with pytest.raises(ValueError, match="finite radius >= 0"):
            fa.NuclearBall(bad)


def test_the_ball_tag_is_the_projection():
    rng = np.random.RandomState(8)
    for shape in ((6, 9), (9, 6), (5, 5), (1, 4)):
        X = rng.randn(*shape)
        s = la.svd(X, compute_uv=False)
        for radius in (0.0, 0.3 * s.sum(), 2.0 * s.sum()):
            reg = fa.NuclearBall(radius)
            U, sv, Vh = la.svd(X, full_matrices=False)
            want = (U * fa.proximal.project_L1_ball(sv, radius)) @ Vh
            assert np.array_equal(reg.prox(X, 0.1), want) and np.array_equal(reg.prox(X, 7.0), want) and np.array_equal(reg(X, 1.0), want)   # independent of t
            assert np.array_equal(fa.proximal.project_nuclear_ball(X, radius), want)
            got = la.svd(want, compute_uv=False)
            assert got.sum() <= radius + 1e-12 * s.sum() + 1e-300
            if radius >= s.sum():
                assert la.norm(want - X) <= 1e-13 * la.norm(X)
            if radius == 0.0:
                assert not want.any()
        assert reg.g(X) == 0 and reg.g_from_sums(3.0, 9.0) == 0 and reg.nuclear_norm_from_sums(3.0, 9.0) == 3.0
        assert reg.kind == hip.PROX_NUCBALL == 11 and reg.step_scaled is False and reg.mu == reg.radius
    # idempotent, and non-expansive: what carries the thresholding's bound over
    X, Y = rng.randn(6, 8), rng.randn(6, 8)
    P = fa.proximal.project_nuclear_ball
    assert la.norm(P(P(X, 2.0), 2.0) - P(X, 2.0)) <= 1e-14 * la.norm(X) and la.norm(P(X, 2.0) - P(Y, 2.0)) <= la.norm(X - Y)


# ---- the level rule restated ---------------------------------------------------------------------------------------------------------------------
def test_exact_ball_input_is_exact():
    X, want = CC.ball_exact_input()
    theta, phi, kept = CC.model_level(CC.NC.EXACT_SIGMA, CC.BALL_RADIUS)
    assert theta == CC.BALL_THETA and tuple(kept) == CC.BALL_KEPT and tuple(phi) == CC.BALL_FACTORS
    assert kept.sum() == CC.BALL_GSUM == CC.BALL_RADIUS and kept.max() == CC.BALL_GMAX and int(np.sum(np.array(CC.NC.EXACT_SIGMA) > theta)) == CC.BALL_RANK
    assert la.norm(fa.proximal.project_nuclear_ball(X, CC.BALL_RADIUS) - want) <= 1e-13 * la.norm(X)
    assert np.array_equal(CC.model_order([2.0, 8.0, 2.0, 0.0, 8.0]), [8.0, 8.0, 2.0, 2.0, 0.0])
    X, want = CC.ball_tie_input()                        # two equal non-zero sigma
    assert np.array_equal(X @ X.T, np.diag(np.square(CC.TIE_SIGMA)))
    theta, phi, kept = CC.model_level(CC.TIE_SIGMA, CC.BALL_RADIUS)
    assert theta == CC.TIE_THETA and tuple(kept) == CC.TIE_KEPT and tuple(phi) == CC.TIE_FACTORS and kept.sum() == CC.TIE_GSUM
    assert np.array_equal(kept, fa.proximal.project_L1_ball(np.array(CC.TIE_SIGMA), CC.BALL_RADIUS))
    assert la.norm(fa.proximal.project_nuclear_ball(X, CC.BALL_RADIUS) - want) <= 1e-13 * la.norm(X)


@pytest.mark.parametrize("case", CC.BALL_CASES + [CC.FULL_WIDTH], ids=lambda c: c.name)
def test_restated_level_equals_project_l1_ball_bit_for_bit(case):
    X, radius = CC.ball_input(case)
    sigma = la.svd(X, compute_uv=False)                  # descending
    theta, phi, kept = CC.model_level(sigma, radius)
    assert np.array_equal(kept, fa.proximal.project_L1_ball(sigma, radius))
    # the ordering is the rule's own: the same values in any other index order give the same level and the same kept values
    perm = np.random.RandomState(1).permutation(len(sigma))
    theta_p, _, kept_p = CC.model_level(sigma[perm], radius)
    assert theta_p == theta and np.array_equal(kept_p, kept[perm]) and np.array_equal(kept_p, fa.proximal.project_L1_ball(sigma[perm], radius))
    assert np.array_equal(phi * sigma == 0, kept == 0) and (phi <= 1).all() and (phi >= 0).all()
    if case.kind in ("r0", "zero"):
        assert not kept.any()
    if case.kind == "outside":
        assert theta == 0.0 and np.array_equal(kept, sigma)
    if case.kind in ("random", "duplicated", "rank8") and len(sigma) > 1:
        assert theta > 0 and abs(kept.sum() - radius) <= len(sigma) * CC.EPS * sigma.sum()


def test_ties_enter_the_running_sums_in_index_order():
    sigma = np.array([0.1, 0.7, 0.1, 0.3, 0.7, 0.1, 0.0, 0.0])
    assert np.array_equal(CC.model_order(sigma), np.sort(sigma)[::-1])
    for radius in (0.05, 0.5, 1.0, 1.9):
        assert np.array_equal(CC.model_level(sigma, radius)[2], fa.proximal.project_L1_ball(sigma, radius))


# ---- recognition -----------------------------------------------------------------------------------------------------------------------------------
def _operands(shape=(4, 6)):
    rng = np.random.RandomState(1)
    B = np.sign(rng.randn(*shape))
    W = rng.rand(*shape) < 0.5
    return fa.LogisticLoss(B, weights=W), fa.LeastSquares(B, weights=W), fa.LogisticLoss(B), np.zeros(shape)


def test_served_operands_are_recognised():
    wl, ws, plain, X0 = _operands()
    for loss in (wl, ws, plain):
        for reg in (fa.NuclearShrink(1.0), fa.NuclearBall(2.0), fa.Shrink(0.1), fa.NonNeg(), fa.Box(-1, 1)):
            assert why(None, None, loss.f, loss.gradf, reg.g, reg.prox, X0) is None
            assert why(fa.IdentityMap(X0.shape), None, loss.f, loss.gradf, reg.g, reg.prox, X0) is None
        assert why(None, None, loss.f, loss.gradf, None, None, X0) is None
    A, loss, prox = fa.solver._recognise(None, None, ws.f, ws.gradf, None, None, X0)
    assert isinstance(A, fa.IdentityMap) and A._ctx is None and loss is ws and type(prox) is fa.NoProx
    ball = fa.NuclearBall(2.0)
    assert fa.solver._recognise(None, None, wl.f, wl.gradf, ball.g, ball.prox, X0)[1:] == (wl, ball)


def test_refusals_name_what_is_not_served_and_nothing_falls_back():
    wl, ws, plain, X0 = _operands()
    ball, box = fa.NuclearBall(1.0), fa.Box(0, 1)
    # the two halves of one weighted tag, not a weighted and an unweighted one
    assert "not device-resident" in why(None, None, ws.f, plain.gradf, box.g, box.prox, X0)
    assert "B must have x0's shape" in why(None, None, ws.f, ws.gradf, ball.g, ball.prox, np.zeros((6, 4)))
    # weights over any other operator: named, on the host loop under the default backend, an error under backend="hip"
    b = fa.LeastSquares(np.zeros(3), weights=[1.0, 0.0, 2.0])
    shr = fa.Shrink(0.1)
    for A in (np.eye(3), fa.DenseMatrixMap(np.eye(3))):
        for g, proxg in ((shr.g, shr.prox), (None, None)):
            assert "observation weights" in why(A, None, b.f, b.gradf, g, proxg, np.zeros(3)) and "identity operator" in why(A, None, b.f, b.gradf, g, proxg, np.zeros(3))
    with pytest.raises(TypeError, match=r"fasta\(backend='hip'\): observation weights .* are served on the device by the identity operator only"):
        fa.fasta(np.eye(3), np.eye(3), b.f, b.gradf, shr.g, shr.prox, np.zeros(3), backend="hip", verbose=False)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        c = fa.fasta(np.eye(3), np.eye(3), b.f, b.gradf, None, None, np.ones(3), verbose=False, max_iters=5)           # the default backend: the host loop, WEIGHTED
    assert not hasattr(c, "library_steps") and c.solution[1] == 1.0 and abs(c.solution[0]) < 1.0                       # (the unobserved entry has a zero gradient: it never moves)
    # NuclearBall over any other operator
    u = fa.LeastSquares(np.zeros(3))
    assert "proximal.NuclearBall is served on the device by the identity operator only" in why(np.eye(3), None, u.f, u.gradf, ball.g, ball.prox, np.zeros(3))
    q = fa.Quadratic(np.eye(3))
    assert "proximal.NuclearBall is served on the device by the identity operator only" in why(None, None, q.f, q.gradf, ball.g, ball.prox, np.zeros((3, 2)))
    with pytest.raises(TypeError, match="NuclearBall is served on the device by the identity operator only"):
        fa.fasta(np.eye(3), np.eye(3), u.f, u.gradf, ball.g, ball.prox, np.zeros(3), backend="hip", verbose=False)
    # the size limit is NuclearShrink's
    wide = fa.LogisticLoss(np.ones((1025, 1026)), weights=np.ones((1025, 1026)))
    assert "proximal.NuclearBall serves min(M, N) <= 1024" in why(None, None, wide.f, wide.gradf, ball.g, ball.prox, np.zeros((1025, 1026)))
    assert why(None, None, wide.f, wide.gradf, box.g, box.prox, np.zeros((1025, 1026))) is None
    with pytest.raises(ValueError, match="NuclearBall needs a 2-D array"):
        fa.proximal.device_prox(ball, np.ones(5), 1.0)


def test_no_gpu_is_an_error_not_a_fallback():
    try:
        n = hip.device_count()
    except hip.HipError:
        n = 0
    wl, ws, _, X0 = _operands()
    reg = fa.NuclearBall(0.5)
    if n == 0:
        for loss in (wl, ws):
            with pytest.raises(hip.HipError):
                fa.fasta(None, None, loss.f, loss.gradf, reg.g, reg.prox, X0, verbose=False)
        with pytest.raises(hip.HipError):
            fa.proximal.device_prox(reg, np.ones((3, 4)), 1.0)
    else:
        c = fa.fasta(None, None, ws.f, ws.gradf, reg.g, reg.prox, X0, verbose=False)
        assert c.solution.shape == X0.shape and c.library_steps == c.iteration_count


def test_the_example_runs_on_the_host_in_every_form(capsys):
    from fasta_python_amd.examples import matrix_completion as ex
    for extra in ([], ["--radius", "30"], ["--one-bit"], ["--one-bit", "--radius", "10"]):
        results = ex.main(["--backend", "numpy", "--rows", "10", "--cols", "14", "--rank", "2", "--observed", "0.7"] + extra)
        assert len(results) == 3
        for solution, conv in results:
            assert solution.shape == (10, 14) and np.isfinite(solution).all() and conv.iteration_count > 0
        out = capsys.readouterr().out
        assert out.count("relative error on the unobserved entries") == 3 and "rank kept" in out and "objective" in out
    with pytest.raises(SystemExit):
        ex.main(["--backend", "numpy", "--mu", "1", "--radius", "2"])

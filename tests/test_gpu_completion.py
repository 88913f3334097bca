"""GPU tests of matrix completion from partial observations: observation weights on the identity operator (fh_set_loss_weights, the weighted
instantiations of k_id_fwd / k_id_adj) and the nuclear-norm ball (FH_PROX_NUCBALL, k_nuc_ball; csrc/fh_nuclear.h) -- through the C ABI and
through fasta().

Tolerances.  Least squares on dyadic data with dyadic weights: every vector `==` NumPy.  Every scalar: within n * 2^-52 * sum|terms| of the
extended-precision sum of its terms formed from the device's OWN vectors (the project's standing rule for a fixed-order reduction of n terms).
The logistic loss sum has no device vector of its terms: they are formed by NumPy from the device's vectors, and the device's exp and log are
each within 2 ulp of NumPy's, an error relative to |log(1 + e^z)| + |z| (the subtraction cancels for large z), so that sum is held to
(n + 8) * 2^-52 * sum w (|log(1 + e^z)| + |z|).  The ball's prox: ||xprox_dev - project_nuclear_ball(xhat, r)||_F <= 32 * p * eps * ||xhat||_F
against float64 LAPACK -- the thresholding's bound (tests/test_gpu_nuclear.py), which carries over because the projection onto a convex set
is non-expansive; the sum of the kept values against LAPACK's p times that (Weyl: every value moves by at most the perturbation's norm).  The
CONSTRAINT itself, FH_S_GSUM <= radius, is held to the bound alone: the level comes from the device's own sigma, so the sum of the kept values
misses the radius only by the rounding of p terms, whatever the decomposition's error is.  The exact input is compared with np.array_equal.  Whole solves: histories
rtol 1e-6, atol 1e-14, solutions rtol 1e-5 with a floor of 1e-6 of the largest entry, as for every other operator."""
import warnings

import numpy as np
import pytest
from numpy import linalg as la

import fasta_python_amd as fa
from fasta_python_amd import hip
from fasta_python_amd import stopping as fstop
from tests import completion_cases as CC
from tests import gpu_util as G
from tests import nuclear_cases as NC

pytestmark = pytest.mark.gpu

TAGS = {"identity": fa.NoProx(), "shrink": fa.Shrink(0.5), "nonneg": fa.NonNeg(), "box": fa.Box(-0.5, 0.75), "nuclear": fa.NuclearShrink(0.5),
        "nucball": fa.NuclearBall(2.0)}


def open_identity(M, N, loss, B, W=None, Bk=0):
    op = fa.IdentityMap((M, N), tuning={hip.TUNE_NUC_BLOCK_ROWS: Bk} if Bk else None)
    c = op.ctx
    (c.set_loss_lsq if loss == "lsq" else c.set_loss_logistic)(B)
    if W is not None:
        c.set_loss_weights(W)
    return op, c


def bind(c, tag):
    if isinstance(tag, fa.NuclearShrink):
        tag.bind_prox(c, True)
    else:
        c.set_prox(tag.kind, tag.mu, tag.lo, tag.hi)


def vec(c, which, shape):
    return c.get_vector(which, shape[0] * shape[1]).reshape(shape)


def host_loss(loss, B, W):
    return (fa.LeastSquares if loss == "lsq" else fa.LogisticLoss)(B, weights=W)


def loss_terms(loss, Z, B, W):
    """(terms of the device's loss sum, their magnitudes for the bound, ulps of slack): least squares sums w * (z - b)^2."""
    if loss == "lsq":
        t = np.where(W == 0, 0.0, W * ((Z - B) * (Z - B)))
        return t, np.abs(t), 0
    with np.errstate(over="ignore", invalid="ignore"):
        soft = np.log(1 + np.exp(Z))
        t = np.where(W == 0, 0.0, W * (soft - (B == 1) * Z))
        return t, np.where(W == 0, 0.0, W * (np.abs(soft) + np.abs(Z))), 8


def assert_scalar(got, terms, what, mags=None, slack=0):
    terms = np.asarray(terms, dtype=np.longdouble).ravel()
    mags = np.abs(terms) if mags is None else np.asarray(mags, dtype=np.longdouble).ravel()
    want, bound = np.sum(terms), (terms.size + slack) * 2.0 ** -52 * np.sum(mags)
    assert abs(np.longdouble(got) - want) <= bound, (what, float(got), float(want), float(bound))


def one_step(c, shape, loss, B, W, X0, tag, tau=0.25, coef=0.5, exact=True):
    """init -> fwd -> adj -> fwd_adj -> adj(accel) -> commit on a context whose loss, weights and prox are set; every vector and scalar checked
    against NumPy on the device's own vectors.  Returns everything read, for bitwise comparisons between contexts."""
    Wf = np.ones(shape) if W is None else W
    ld = lambda a: np.asarray(a, dtype=np.longdouble)
    hl = host_loss(loss, B, Wf)
    jacobi = tag.kind in (hip.PROX_NUCLEAR, hip.PROX_NUCBALL)
    seen = []
    c.set_vector(hip.VEC_X0, X0)
    s = c.init()
    g0 = vec(c, hip.VEC_G0, shape)
    with np.errstate(over="ignore", invalid="ignore"):
        want_g0 = hl.gradf(X0)
    if loss == "lsq":
        assert np.array_equal(g0, want_g0)
    else:
        np.testing.assert_allclose(g0, want_g0, rtol=1e-14, atol=1e-16)
    assert not g0[Wf == 0].any()
    t, mags, slack = loss_terms(loss, X0, B, Wf)
    assert_scalar(s[hip.S_FSQ], t, "init f", mags, slack)
    s = c.fwd(tau)
    xhat, xp, z = vec(c, hip.VEC_XHAT, shape), vec(c, hip.VEC_XPROX, shape), vec(c, hip.VEC_Z, shape)
    assert np.array_equal(xhat, X0 - tau * g0) and np.array_equal(z, xp)
    if not jacobi:
        assert np.array_equal(xp, tag.prox(xhat, tau))
    else:
        want = tag.prox(xhat, tau) if tag.kind == hip.PROX_NUCBALL else fa.proximal.project_Lnuc_ball(xhat, tau * tag.mu)
        assert la.norm(xp - want) <= CC.tolerance(xhat)
        if tag.kind == hip.PROX_NUCBALL:
            assert s[hip.S_GSUM] <= tag.radius + CC.tolerance(xhat)
    t, mags, slack = loss_terms(loss, xp, B, Wf)
    assert_scalar(s[hip.S_FSQ], t, "fwd f", mags, slack)
    assert_scalar(s[hip.S_DXG0], (ld(xp) - ld(X0)) * ld(g0), "dxg0")
    assert_scalar(s[hip.S_DX2], (ld(xp) - ld(X0)) ** 2, "dx2")
    assert_scalar(s[hip.S_XH2], (ld(xp) - ld(xhat)) ** 2, "xh2")
    assert_scalar(s[hip.S_G02], ld(g0) ** 2, "g02")
    if not jacobi:
        assert_scalar(s[hip.S_GSUM], np.abs(xp), "gsum")
        assert s[hip.S_GMAX] == np.max(np.abs(xp))
    seen += [s, xhat, xp]
    a = c.adj(tau)
    g1 = vec(c, hip.VEC_G1, shape)
    with np.errstate(over="ignore", invalid="ignore"):
        want_g1 = hl.gradf(xp)
    if loss == "lsq":
        assert np.array_equal(g1, want_g1)
    else:
        np.testing.assert_allclose(g1, want_g1, rtol=1e-14, atol=1e-16)
    assert not g1[Wf == 0].any()
    dg = ld(g1) + (ld(xhat) - ld(X0)) / np.longdouble(tau)
    assert_scalar(a[hip.S_DXDG], (ld(xp) - ld(X0)) * dg, "dxdg")
    assert_scalar(a[hip.S_DG2], dg * dg, "dg2")
    assert_scalar(a[hip.S_FSQ_ADJ], t, "adj f", mags, slack)
    assert_scalar(a[hip.S_XH2_ADJ], (ld(xp) - ld(xhat)) ** 2, "xh2 adj")
    if jacobi:
        assert a[hip.S_GSUM_ADJ] == s[hip.S_GSUM] and a[hip.S_GMAX_ADJ] == s[hip.S_GMAX]            # x1 is xprox: the decomposition's own
    seen += [a, g1]
    both = c.fwd_adj(tau)
    assert np.array_equal(both[:8], s[:8]) and np.array_equal(both[8:15], a[8:15])
    a = c.adj(tau, True, coef)
    x1, g1a = vec(c, hip.VEC_X1, shape), vec(c, hip.VEC_G1, shape)
    assert np.array_equal(x1, xp + coef * (xp - X0))
    with np.errstate(over="ignore", invalid="ignore"):
        want_g1a = hl.gradf(x1)
    if loss == "lsq":
        assert np.array_equal(g1a, want_g1a)
    else:
        np.testing.assert_allclose(g1a, want_g1a, rtol=1e-14, atol=1e-16)
    t, mags, slack = loss_terms(loss, x1, B, Wf)
    assert_scalar(a[hip.S_FSQ_ADJ], t, "accelerated f", mags, slack)
    if tag.kind == hip.PROX_NUCBALL:                                                                # g = 0: never evaluated where it is not free
        assert np.isnan(a[hip.S_GSUM_ADJ]) and a[hip.S_GMAX_ADJ] == 0.0 and np.isfinite(np.delete(a, hip.S_GSUM_ADJ)).all()
    seen += [a, x1, g1a]
    c.commit(True)
    assert np.array_equal(vec(c, hip.VEC_X0, shape), x1) and np.array_equal(vec(c, hip.VEC_BEST, shape), x1) and np.array_equal(vec(c, hip.VEC_G0, shape), g1a)
    assert np.array_equal(c.apply(X0), X0.ravel()) and np.array_equal(c.apply(X0, adjoint=True), X0.ravel())      # fh_apply: the plain operator, a copy
    return seen


def labels_of(B):
    return np.where(B >= 0, 1.0, -1.0)


# ---- weights -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", CC.STEP_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kind", CC.STEP_KINDS)
@pytest.mark.parametrize("loss", ["lsq", "logistic"])
def test_one_weighted_step(loss, kind, shape):
    X0, B, W = CC.step_problem(*shape)
    if loss == "logistic":
        B = labels_of(B)
    op, c = open_identity(*shape, loss, B, W)
    try:
        bind(c, TAGS[kind])
        one_step(c, shape, loss, B, W, X0, TAGS[kind])
    finally:
        op.close()


@pytest.mark.parametrize("loss", ["lsq", "logistic"])
def test_one_weighted_step_past_the_grid_cap(loss):
    """725 x 725 = 525 625 entries > 2048 x 256: the grid-stride loop of both kernels makes a second trip."""
    shape = CC.SECOND_TRIP
    assert shape[0] * shape[1] > 2048 * 256
    X0, B, W = CC.step_problem(*shape)
    if loss == "logistic":
        B = labels_of(B)
    op, c = open_identity(*shape, loss, B, W)
    try:
        bind(c, TAGS["shrink"])
        one_step(c, shape, loss, B, W, X0, TAGS["shrink"])
    finally:
        op.close()


@pytest.mark.parametrize("kind", ["shrink", "nuclear", "nucball"])
@pytest.mark.parametrize("loss", ["lsq", "logistic"])
def test_all_ones_weights_are_the_unweighted_context_bit_for_bit(loss, kind):
    shape = (33, 130)
    X0, B, _ = CC.step_problem(*shape)
    if loss == "logistic":
        B = labels_of(B)
    runs = []
    for W in (None, np.ones(shape)):
        op, c = open_identity(*shape, loss, B, W)
        try:
            bind(c, TAGS[kind])
            runs.append(one_step(c, shape, loss, B, W, X0, TAGS[kind]))
        finally:
            op.close()
    assert len(runs[0]) == len(runs[1]) and all(np.array_equal(a, b, equal_nan=True) for a, b in zip(*runs))


def test_unobserved_entries_at_plus_minus_800_contribute_exactly_zero():
    shape = (33, 130)
    X0, B, W = CC.step_problem(*shape)
    B, mask = labels_of(B), W != 0
    X0 = np.where(mask, X0, np.where(B > 0, 800.0, -800.0) * np.where(np.arange(X0.size).reshape(shape) % 2, 1.0, -1.0))
    assert (np.abs(X0[~mask]) == 800.0).all() and (~mask).sum() > 100
    op, c = open_identity(*shape, "logistic", B, mask)
    try:
        c.set_prox(hip.PROX_IDENTITY)
        c.set_vector(hip.VEC_X0, X0)
        s = c.init()
        assert np.isfinite(s[hip.S_FSQ]) and not vec(c, hip.VEC_G0, shape)[~mask].any()
        s = c.fwd(0.5)
        xp = vec(c, hip.VEC_XPROX, shape)
        assert np.isfinite(s).all() and (np.abs(xp[~mask]) == 800.0).all()                          # a zero gradient: the entry never moves
        a = c.adj(0.5)
        g1 = vec(c, hip.VEC_G1, shape)
        assert np.isfinite(a).all() and np.array_equal(g1[~mask], np.zeros(int((~mask).sum()))) and g1[mask].all()
        t, mags, slack = loss_terms("logistic", xp, B, mask.astype(np.float64))
        assert_scalar(a[hip.S_FSQ_ADJ], t, "f", mags, slack)
        a = c.adj(0.5, True, 0.25)
        assert np.isfinite(a).all() and not vec(c, hip.VEC_G1, shape)[~mask].any()
        # the unweighted context does see them: the loss sum overflows there
        c.set_loss_weights(None)
        c.set_vector(hip.VEC_X0, X0)
        assert np.isinf(c.init()[hip.S_FSQ])
    finally:
        op.close()


@pytest.mark.parametrize("loss", ["lsq", "logistic"])
def test_gradient_at_and_setup_are_weighted_and_apply_is_not(loss):
    shape = (9, 14)
    X0, B, W = CC.step_problem(*shape)
    if loss == "logistic":
        B = labels_of(B)
    hl = host_loss(loss, B, W)
    op, c = open_identity(*shape, loss, B, W)
    try:
        P1, P2 = X0 + 0.5, X0 * 0.5 - 1.0
        c.set_vector(hip.VEC_T0, P1)
        c.gradient_at(hip.VEC_T0, hip.VEC_T2)
        got = vec(c, hip.VEC_T2, shape)
        assert np.array_equal(got, hl.gradf(P1)) if loss == "lsq" else np.allclose(got, hl.gradf(P1), rtol=1e-14, atol=1e-16)
        assert not got[W == 0].any() and got[W != 0].any()
        c.set_vector(hip.VEC_T1, P2)
        c.set_vector(hip.VEC_X0, X0)
        s = c.setup()                                      # the Lipschitz probes and init() in one call
        np.testing.assert_allclose(s[hip.S_DG2], np.sum((hl.gradf(P1) - hl.gradf(P2)) ** 2), rtol=1e-12)
        np.testing.assert_allclose(s[hip.S_DX2], np.sum((P1 - P2) ** 2), rtol=1e-13)
        t, mags, slack = loss_terms(loss, X0, B, W)
        assert_scalar(s[hip.S_FSQ], t, "setup f", mags, slack)
        assert np.array_equal(c.apply(P1), P1.ravel()) and np.array_equal(c.apply(P1, adjoint=True), P1.ravel())
    finally:
        op.close()


def refusal(code, text):
    return pytest.raises(hip.HipError, match=rf"\[{code}\].*{text}")


def test_weight_refusals_by_code_and_sentence_and_the_loss_owns_the_weights():
    shape = (4, 6)
    X0, B, W = CC.step_problem(*shape)
    op, c = open_identity(*shape, "lsq", B)
    try:
        for at, bad in ((7, -0.25), (11, np.nan), (3, np.inf)):
            Wb = W.copy().ravel()
            Wb[at] = bad
            with refusal(hip.E_ARG, rf"finite and >= 0 \(entry {at} is"):
                c.set_loss_weights(Wb)
        with pytest.raises(ValueError, match="weights have 23 entries"):
            c.set_loss_weights(np.ones(23))
        c.set_prox(hip.PROX_IDENTITY)
        c.set_loss_weights(W)
        c.set_vector(hip.VEC_X0, X0)
        c.init()
        assert np.array_equal(vec(c, hip.VEC_G0, shape), W * (X0 - B))
        # weights, then another operator: a weighted problem never silently runs unweighted
        for setter in (lambda: c.set_matrix(np.eye(3)), lambda: c.set_stencil(4, 4), lambda: c.set_quadratic(np.eye(3), None, 1)):
            with refusal(hip.E_STATE, "holds observation weights"):
                setter()
        c.init()
        assert np.array_equal(vec(c, hip.VEC_G0, shape), W * (X0 - B))                              # ... and the refusal changed nothing
        # fh_set_loss_lsq / fh_set_loss_logistic drop them; NULL removes them
        c.set_loss_lsq(B)
        c.init()
        assert np.array_equal(vec(c, hip.VEC_G0, shape), X0 - B)
        c.set_loss_weights(W)
        c.set_loss_weights(None)
        c.init()
        assert np.array_equal(vec(c, hip.VEC_G0, shape), X0 - B)
        c.set_loss_weights(W)
        c.set_loss_logistic(labels_of(B))
        c.init()
        np.testing.assert_allclose(vec(c, hip.VEC_G0, shape), fa.LogisticLoss(labels_of(B)).gradf(X0), rtol=1e-14)
        # another operator, then weights
        c.set_matrix(np.eye(24))
        c.set_loss_lsq(np.zeros(24))
        with refusal(hip.E_STATE, "identity operator only"):
            c.set_loss_weights(W)
        # the identity operator again: the loss first
        c.set_identity(*shape)
        with refusal(hip.E_STATE, "set the loss first"):
            c.set_loss_weights(W)
    finally:
        op.close()


# ---- the ball --------------------------------------------------------------------------------------------------------------------------------------
def device_ball(X, radius, Bk, tau=1.0):
    """(xprox, forward scalars, NuclearInfo, xhat, launches booked under FH_K_LEVEL) of one forward launch with x0 = X, g0 = 0; the geometry asserted."""
    M, N = X.shape
    op, c = open_identity(M, N, "lsq", np.zeros((M, N)), None, Bk)
    try:
        c.set_prox(hip.PROX_NUCBALL, radius)
        assert c.nuclear_shape()._asdict() == NC.shape_of(M, N, Bk) == hip.nuclear_shape(M, N, Bk)._asdict()
        c.timing_enable(True)
        c.set_vector(hip.VEC_X0, X)
        c.set_vector(hip.VEC_G0, np.zeros(M * N))
        s = c.fwd(tau)
        return vec(c, hip.VEC_XPROX, X.shape), s, c.nuclear_info(), vec(c, hip.VEC_XHAT, X.shape), c.timing_get(hip.K_LEVEL)[1]
    finally:
        op.close()


@pytest.mark.parametrize("transposed", [False, True], ids=["5x16", "16x5"])
@pytest.mark.parametrize("Bk", [1, 2, 8])
def test_exact_ball_input_bit_for_bit(Bk, transposed):
    X, want = CC.ball_exact_input()
    if transposed:
        X, want = np.ascontiguousarray(X.T), np.ascontiguousarray(want.T)
    runs = [device_ball(X, CC.BALL_RADIUS, Bk, tau) for tau in (1.0, 0.125)]                        # independent of the step
    out, s, info, xhat, levels = runs[0]
    assert np.array_equal(out, want) and np.array_equal(xhat, X) and levels == 1
    assert info == hip.NuclearInfo(1, NC.shape_of(*X.shape, Bk)["steps_per_sweep"], 0, CC.BALL_RANK)       # one sweep, zero rotations
    assert s[hip.S_GSUM] == CC.BALL_GSUM and s[hip.S_GMAX] == CC.BALL_GMAX and s[hip.S_ALPHA] == CC.BALL_RANK
    assert s[hip.S_FSQ] == float(np.sum(want * want)) and s[hip.S_XH2] == float(np.sum((want - X) ** 2))
    assert np.array_equal(runs[1][0], out) and np.array_equal(runs[1][1], s) and runs[1][2] == info        # repeatable bit for bit


@pytest.mark.parametrize("transposed", [False, True], ids=["5x16", "16x5"])
@pytest.mark.parametrize("Bk", [1, 2, 8])
def test_equal_singular_values_are_ordered_by_their_index(Bk, transposed):
    """sigma = {16, 16, 2, 8, 0}: the kernel's tie-break on two equal NON-ZERO values (without it theta is 4, not 10)."""
    X, want = CC.ball_tie_input()
    if transposed:
        X, want = np.ascontiguousarray(X.T), np.ascontiguousarray(want.T)
    runs = [device_ball(X, CC.BALL_RADIUS, Bk) for _ in range(2)]
    out, s, info, xhat, _ = runs[0]
    assert np.array_equal(out, want) and np.array_equal(xhat, X) and info.rotations == 0 and info.rank == CC.TIE_RANK
    assert s[hip.S_GSUM] == CC.TIE_GSUM == CC.BALL_RADIUS and s[hip.S_GMAX] == CC.TIE_GMAX and s[hip.S_ALPHA] == CC.TIE_RANK
    assert np.array_equal(runs[1][0], out) and np.array_equal(runs[1][1], s) and runs[1][2] == info


@pytest.mark.parametrize("case", CC.BALL_CASES, ids=lambda c: c.name)
def test_ball_cases_against_lapack(case):
    X, radius = CC.ball_input(case)
    runs = [device_ball(X, radius, case.Bk) for _ in range(2)]
    out, s, info, xhat, _ = runs[0]
    want = fa.proximal.project_nuclear_ball(X, radius)
    sv = la.svd(X, compute_uv=False)
    kept = fa.proximal.project_L1_ball(sv, radius)
    err, lim = float(la.norm(out - want)), CC.tolerance(X)
    unit = lim / CC.TOL_FACTOR
    print(f"\n{case.name}: {info}, error {err / unit if unit else err:.2f} p eps |X|_F", end="")
    assert np.array_equal(xhat, X) and np.isfinite(out).all() and info.sweeps < NC.MAX_SWEEPS
    assert err <= lim
    print(f", nuclear norm of xprox minus the radius {(s[hip.S_GSUM] - radius) / unit if unit else s[hip.S_GSUM] - radius:+.3f} of those units", end="")
    assert s[hip.S_GSUM] <= radius + lim                                                           # the constraint: the bound alone
    assert abs(s[hip.S_GSUM] - float(kept.sum())) <= min(X.shape) * lim                             # against LAPACK's kept values: Weyl, p terms
    if case.kind in ("random", "duplicated") and min(X.shape) > 1:
        assert abs(s[hip.S_GSUM] - radius) <= lim                                                   # an active ball is met, not only respected
    assert abs(s[hip.S_GMAX] - float(kept.max())) <= lim and abs(la.svd(out, compute_uv=False).sum() - s[hip.S_GSUM]) <= min(X.shape) * lim
    assert s[hip.S_ALPHA] == info.rank
    if case.kind in ("random", "duplicated"):
        assert info.rank == int(np.sum(kept > 0)) or min(X.shape) == 1
    if case.kind in ("r0", "zero"):
        assert not out.any() and s[hip.S_GSUM] == 0.0 and s[hip.S_GMAX] == 0.0 and info.rank == 0       # exact zeros, no NaN
    if case.kind == "outside":                             # theta = 0: xprox is xhat up to the decomposition's own error
        assert la.norm(out - X) <= lim and abs(s[hip.S_GSUM] - sv.sum()) <= min(X.shape) * lim
    if case.kind == "duplicated":
        assert la.matrix_rank(out) <= case.M // 2
    assert np.array_equal(runs[1][0], out) and np.array_equal(runs[1][1], s) and runs[1][2] == info        # two runs, bit-identical


def test_ball_at_the_full_ordering_width():
    case = CC.FULL_WIDTH
    X, radius = CC.ball_input(case)
    out, s, info, xhat, _ = device_ball(X, radius, case.Bk)
    assert c_shape_p(X) == 1024 and info.sweeps < NC.MAX_SWEEPS
    want = fa.proximal.project_nuclear_ball(X, radius)
    err, lim = float(la.norm(out - want)), CC.tolerance(X)
    print(f"\n{case.name}: {info}, error {err / (lim / CC.TOL_FACTOR):.2f} p eps |X|_F", end="")
    print(f", nuclear norm of xprox minus the radius {(s[hip.S_GSUM] - radius) / (lim / CC.TOL_FACTOR):+.3f} of those units", end="")
    assert err <= lim and abs(s[hip.S_GSUM] - radius) <= lim and 0 < info.rank <= 16               # (the ball is active: the radius is met up to the bound alone)


def c_shape_p(X):
    return hip.nuclear_shape(*X.shape).p


def test_the_ball_never_runs_a_values_only_decomposition():
    rng = np.random.RandomState(21)
    shape = (7, 12)
    X0, B = rng.randn(*shape), rng.randn(*shape)
    for objective_first in (True, False):                  # whatever a NuclearShrink before it left behind
        op, c = open_identity(*shape, "lsq", B)
        try:
            fa.NuclearShrink(1.0).bind_prox(c, objective_first)
            c.set_prox(hip.PROX_NUCBALL, 3.0)
            c.timing_enable(True)
            c.set_vector(hip.VEC_X0, X0)
            s = c.init()
            assert np.isnan(s[hip.S_GSUM]) and np.isfinite(np.delete(s, hip.S_GSUM)).all() and c.timing_get(hip.K_LEVEL)[1] == 0
            s = c.fwd(0.5)
            assert np.isfinite(s).all() and c.timing_get(hip.K_LEVEL)[1] == 1 and s[hip.S_GSUM] <= 3.0 + CC.tolerance(vec(c, hip.VEC_XHAT, shape))
            a = c.adj(0.5)
            assert a[hip.S_GSUM_ADJ] == s[hip.S_GSUM] and c.timing_get(hip.K_LEVEL)[1] == 1
            a = c.adj(0.5, True, 0.25)
            assert np.isnan(a[hip.S_GSUM_ADJ]) and a[hip.S_GMAX_ADJ] == 0.0 and c.timing_get(hip.K_LEVEL)[1] == 1
            assert c.nuclear_info().sweeps > 0 and c.nuclear_shape().p == 7
        finally:
            op.close()


def test_ball_refusals():
    op, c = open_identity(4, 6, "lsq", np.zeros((4, 6)))
    try:
        for bad in (-1.0, np.nan, np.inf):
            with refusal(hip.E_ARG, "radius"):
                c.set_prox(hip.PROX_NUCBALL, bad)
        c.set_prox(hip.PROX_NUCBALL, 0.0)
        c.set_matrix(np.eye(3))                            # a context holding NUCBALL returns to IDENTITY when another operator is set
        c.set_loss_lsq(np.zeros(3))
        c.set_vector(hip.VEC_X0, np.ones(3))
        c.init()
        c.fwd(0.5)
        assert np.array_equal(c.get_vector(hip.VEC_XPROX, 3), np.full(3, 0.5))
        with refusal(hip.E_STATE, "FH_PROX_NUCBALL .* identity operator only"):
            c.set_prox(hip.PROX_NUCBALL, 1.0)
        with refusal(hip.E_STATE, "fh_nuclear_shape"):
            c.nuclear_shape()
        c.set_identity(1025, 1030)
        with refusal(hip.E_ARG, "<= 1024"):
            c.set_prox(hip.PROX_NUCBALL, 1.0)
    finally:
        op.close()


def test_device_prox_of_the_ball_is_the_forward_path():
    case = CC.BALL_CASES[0]
    X, radius = CC.ball_input(case)
    reg = fa.NuclearBall(radius)
    got = fa.proximal.device_prox(reg, X, 0.5)
    want = device_ball(X, radius, 0)[0]
    assert np.array_equal(got, want) and np.array_equal(reg.prox_on_device(X, 3.0), want)
    assert la.norm(got - reg.prox(X, 0.5)) <= CC.tolerance(X)
    fa.proximal.release_scratch()


# ---- solves ----------------------------------------------------------------------------------------------------------------------------------------
def solve(meta, d, **extra):
    ms = CC.capture_script()
    f, gradf, g, proxg, x0 = ms.operands(fa, meta["kind"], d)
    o = ms.resolve(meta["options"], fstop)
    o.update(extra)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fa.fasta(None, None, f, gradf, g, proxg, x0, verbose=False, backend="hip", **o)


_runs = {}


def library_run(name):
    """The library-driven device solve of a fixture (its compared prefix), computed once and shared by the tests below; never modified."""
    if name not in _runs:
        meta, z, d = CC.load(name)
        k, whole = CC.compared_prefix(meta, z)
        extra = {} if whole else dict(max_iters=k, tolerance=0.0)
        _runs[name] = (solve(meta, d, driver="library", **extra), k, whole, extra)
    return _runs[name]


@pytest.mark.parametrize("name", CC.EXPECTED)
def test_fixture_solves_on_the_device(name):
    meta, z, d = CC.load(name)
    lib, k, whole, extra = library_run(name)
    assert lib.library_steps == lib.iteration_count and lib.device_steps == 0
    print(f"\n{name}: device {lib.iteration_count} iterations / {lib.backtracks} backtracks, reference {int(z['iteration_count'])} / {int(z['backtracks'])}", end="")
    if whole:
        assert lib.iteration_count == int(z["iteration_count"]) and lib.backtracks == int(z["backtracks"])
    else:
        assert k >= CC.MIN_PREFIX and lib.iteration_count == k and lib.backtracks == meta["backtracks_at_divergence"]
    worst = G.compare_histories(lib, lambda f: z[f], k, rtol=1e-6, atol=1e-14)
    print(f"; {k} iterations compared, worst relative deviation of a history entry {worst:.2e}")
    if whole:
        np.testing.assert_allclose(lib.solution, z["solution"], rtol=1e-5, atol=1e-6 * float(np.max(np.abs(z["solution"]))))
    if meta["kind"].endswith("ball"):
        r = float(d["radius"])
        assert abs(la.svd(lib.solution, compute_uv=False).sum() - r) <= 1e-6 * r                    # the constraint is active on the device too


@pytest.mark.parametrize("name", CC.EXPECTED)
def test_library_and_python_drivers_are_bit_identical(name):
    meta, z, d = CC.load(name)
    lib, k, whole, extra = library_run(name)
    py = solve(meta, d, driver="python", **extra)
    assert py.library_steps == 0 and py.iteration_count == lib.iteration_count and py.backtracks == lib.backtracks
    for f in CC.HISTORIES:
        assert np.array_equal(getattr(py, f), getattr(lib, f), equal_nan=True), f
    assert np.array_equal(py.solution, lib.solution)


@pytest.mark.parametrize("extra", [[], ["--radius", "60"], ["--one-bit"], ["--one-bit", "--radius", "25"]], ids=["mu", "radius", "one-bit", "one-bit-radius"])
def test_the_example_runs_on_the_device(extra, capsys):
    from fasta_python_amd.examples import matrix_completion as ex
    results = ex.main(["--backend", "hip", "--rows", "24", "--cols", "60", "--rank", "3", "--observed", "0.6"] + extra)
    assert len(results) == 3
    for solution, conv in results:
        assert solution.shape == (24, 60) and np.isfinite(solution).all() and conv.iteration_count > 0 and conv.library_steps == conv.iteration_count
        assert 0 < la.matrix_rank(solution, tol=1e-3 * la.norm(solution, 2)) <= 24
    out = capsys.readouterr().out
    assert out.count("relative error on the unobserved entries") == 3

"""CPU tier of the duality-gap certificates (fasta_python_amd/certificates.py), the stop rule stopping.DualityGap on the generic loop and on
FBSolver (over a stand-in context whose `dual_gap` is the host statement), and fasta.path on host operands.

Bounds.  eps = 2^-52.  Weak duality holds exactly in real arithmetic; P and D are each a sum of a few rounded terms of the size of |P| and |D|,
so gap >= -64 eps (|P| + |D|).  For A = I the soft-threshold solution is the minimiser, gap = 0 in real arithmetic: gap <= 64 eps P.  On dyadic
data (entries k/8, small shapes) every product and sum of the least-squares record is exact in float64, so the record equals the rational
evaluation with `==`.  The path's last point against a tight stand-alone solve: f is 1-strongly convex in z, so .5 ||A (x - x*)||^2 <= gap(x),
and with the triangle inequality over the tight solve's own gap, .5 ||A (x - xt)||^2 <= (sqrt(gap) + sqrt(gap_t))^2."""
import math
from fractions import Fraction

import numpy as np
import pytest

import fasta
import fasta_python_amd as fa
from fasta_python_amd import certificates as ce
from fasta_python_amd import hip, stopping
from fasta_python_amd.linalg import LinearMap, _DeviceMap
from tests.fake_ctx import FakeContext

EPS = 2.0 ** -52


def problem(seed, m=12, n=20, L=None, logistic=False):
    rng = np.random.RandomState(seed)
    A = rng.randn(m, n)
    shape = (m,) if L is None else (m, L)
    b = np.sign(rng.randn(*shape)) if logistic else rng.randn(*shape)
    b[b == 0] = 1.0
    return A, (fa.LogisticLoss(b) if logistic else fa.LeastSquares(b)), rng


COMBOS = [(False, fa.Shrink, None), (False, fa.GroupShrink, 3), (True, fa.Shrink, None), (True, fa.GroupShrink, 2)]
COMBO_IDS = ["lsq-shrink", "lsq-group", "logistic-shrink", "logistic-group"]


# ---- the certificate ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logistic,prox_class,L", COMBOS, ids=COMBO_IDS)
def test_the_gap_at_zero_is_exactly_zero_from_the_critical_mu_on_and_positive_below(logistic, prox_class, L):
    A, loss, _ = problem(1, L=L, logistic=logistic)
    shape = (A.shape[1],) if L is None else (A.shape[1], L)
    mu_c = ce.critical_mu(A, loss, prox_class, shape)
    assert mu_c > 0
    for mu in (mu_c, 1.5 * mu_c, 100.0 * mu_c):
        c = ce.duality_gap(A, loss, prox_class(mu), np.zeros(shape))
        assert c.gap == 0.0 and c.scale == 1.0 and c.omega == 0.0 and c.dual_norm == mu_c and c.primal == c.f == c.f0 and c.relative == 0.0
    for mu in (0.999 * mu_c, 0.5 * mu_c, 1e-3 * mu_c):
        c = ce.duality_gap(A, loss, prox_class(mu), np.zeros(shape))
        assert c.gap > 0.0 and c.scale == mu / mu_c < 1.0


@pytest.mark.parametrize("seed", range(5))
def test_on_the_identity_the_soft_threshold_solution_closes_the_gap(seed):
    rng = np.random.RandomState(seed)
    n, mu = 50, 0.7
    b = 2.0 * rng.randn(n)
    x = np.sign(b) * np.maximum(np.abs(b) - mu, 0.0)
    c = ce.duality_gap(np.eye(n), fa.LeastSquares(b), fa.Shrink(mu), x)
    assert 0 < np.count_nonzero(x) < n
    print("gap", c.gap, "bound", 64 * EPS * c.primal)
    assert abs(c.gap) <= 64 * EPS * c.primal
    B = 2.0 * rng.randn(n, 3)                               # rows: the group soft-threshold
    nu = np.sqrt(np.sum(B * B, axis=1))
    X = B * (np.maximum(nu - mu, 0.0) / nu)[:, None]
    c = ce.duality_gap(np.eye(n), fa.LeastSquares(B), fa.GroupShrink(mu), X)
    print("gap", c.gap, "bound", 64 * EPS * c.primal)
    assert abs(c.gap) <= 64 * EPS * c.primal


@pytest.mark.parametrize("logistic,prox_class,L", COMBOS, ids=COMBO_IDS)
def test_weak_duality_at_a_hundred_random_points(logistic, prox_class, L):
    worst = 0.0
    for seed in range(100):
        A, loss, rng = problem(100 + seed, L=L, logistic=logistic)
        shape = (A.shape[1],) if L is None else (A.shape[1], L)
        x = rng.randn(*shape) * (rng.rand(*shape) < 0.3) * 10.0 ** rng.randint(-3, 2)
        mu = 10.0 ** rng.uniform(-3, 1)
        c = ce.duality_gap(A, loss, prox_class(mu), x)
        assert c.gap >= -64 * EPS * (abs(c.primal) + abs(c.dual)), (seed, c)
        assert 0.0 < c.scale <= 1.0 and c.gap == c.primal - c.dual and c.primal == c.f + mu * c.omega
        worst = min(worst, c.gap / (abs(c.primal) + abs(c.dual)))
    print("most negative gap / (|P| + |D|):", worst)


def frac(a):
    return [Fraction(float(v)) for v in np.ravel(a)]


def exact_lsq_record(A, b, x, mu, group):
    """The least-squares record in rational arithmetic (the dual norm of a group: the square of it), from rational A, b, x."""
    m, n = A.shape
    L = 1 if x.ndim == 1 else x.shape[1]
    Af, X, B = [frac(A[i]) for i in range(m)], [frac(np.reshape(x, (n, L))[j]) for j in range(n)], [frac(np.reshape(b, (m, L))[i]) for i in range(m)]
    Z = [[sum(Af[i][j] * X[j][l] for j in range(n)) for l in range(L)] for i in range(m)]
    R = [[Z[i][l] - B[i][l] for l in range(L)] for i in range(m)]
    G = [[sum(Af[i][j] * R[i][l] for i in range(m)) for l in range(L)] for j in range(n)]
    rr = sum(v * v for row in R for v in row)
    rb = sum(R[i][l] * B[i][l] for i in range(m) for l in range(L))
    bb = sum(v * v for row in B for v in row)
    if group:
        omega_sq_rows = [sum(v * v for v in row) for row in X]
        dn_sq = max(sum(v * v for v in row) for row in G)
        return rr, rb, bb, omega_sq_rows, dn_sq
    return rr, rb, bb, sum(abs(v) for row in X for v in row), max(abs(v) for row in G for v in row)


@pytest.mark.parametrize("seed", range(6))
def test_the_least_squares_record_on_dyadic_data_is_the_rational_evaluation_exactly(seed):
    rng = np.random.RandomState(seed)
    m, n = 5 + seed, 7 + 2 * seed
    A = rng.randint(-8, 9, size=(m, n)) / 8.0
    b = rng.randint(-16, 17, size=m) / 8.0
    x = rng.randint(-8, 9, size=n) / 8.0 * (rng.rand(n) < 0.5)
    rr, rb, bb, omega, dn = exact_lsq_record(A, b, x, None, False)
    for mu, s in ((float(dn), Fraction(1)), (float(dn) * 4.0, Fraction(1)), (float(dn) / 4.0, Fraction(1, 4)), (float(dn) / 32.0, Fraction(1, 32))):
        c = ce.duality_gap(A, fa.LeastSquares(b), fa.Shrink(mu), x)
        P = rr / 2 + Fraction(mu) * omega
        D = -s * s * rr / 2 - s * rb
        assert (Fraction(c.primal), Fraction(c.dual), Fraction(c.gap), Fraction(c.f), Fraction(c.omega), Fraction(c.dual_norm), Fraction(c.scale),
                Fraction(c.f0)) == (P, D, P - D, rr / 2, omega, dn, s, bb / 2)
        assert P - D >= 0
    # rows of a matrix unknown with rational norms: multiples of (3, 4, 0), (0, 0, 5), (2, 3, 6) / 8; mu at or above the dual norm, so s = 1
    base = np.array([[3, 4, 0], [0, 0, 5], [2, 3, 6], [0, 0, 0]]) / 8.0
    X = base[rng.randint(0, 4, size=n)] * rng.randint(-3, 4, size=(n, 1))
    B = rng.randint(-16, 17, size=(m, 3)) / 8.0
    rr, rb, bb, om_rows, dn_sq = exact_lsq_record(A, B, X, None, True)
    omega = sum(Fraction(math.isqrt(v.numerator)) / math.isqrt(v.denominator) for v in om_rows)
    assert all(math.isqrt(v.numerator) ** 2 == v.numerator and math.isqrt(v.denominator) ** 2 == v.denominator for v in om_rows)
    dn = math.sqrt(float(dn_sq))                               # (an exact float64 under a correctly rounded square root)
    for mu in (math.ceil(dn * 8.0) / 8.0, math.ceil(dn) * 2.0):      # (dyadic, so that mu * Omega is exact)
        c = ce.duality_gap(A, fa.LeastSquares(B), fa.GroupShrink(mu), X)
        P = rr / 2 + Fraction(mu) * omega
        D = -rr / 2 - rb
        assert (Fraction(c.primal), Fraction(c.dual), Fraction(c.gap), Fraction(c.f), Fraction(c.omega), c.dual_norm, c.scale, Fraction(c.f0)) \
            == (P, D, P - D, rr / 2, omega, dn, 1.0, bb / 2)


def test_maps_and_sparse_matrices_give_the_matrix_record():
    from scipy import sparse as sp
    A, loss, rng = problem(7)
    x = rng.randn(A.shape[1])
    want = ce.duality_gap(A, loss, fa.Shrink(0.3), x)
    got_map = ce.duality_gap(LinearMap(lambda v: A @ v, lambda w: A.T @ w, (A.shape[1],), (A.shape[0],)), loss.f, fa.Shrink(0.3).prox, x)
    got_sp = ce.duality_gap(sp.csr_matrix(A), loss, fa.Shrink(0.3), x)
    assert got_map == want
    np.testing.assert_allclose(got_sp, want, rtol=1e-13)
    assert fasta.certificates is ce and fasta.duality_gap is ce.duality_gap and fasta.path is fa.path and fasta.DualityGap is stopping.DualityGap


def test_every_refusal_is_a_type_error_with_its_sentence():
    A, loss, rng = problem(3)
    x = np.zeros(A.shape[1])
    for bad_loss, bad_prox, sentence in (
            (fa.SoftmaxLoss(np.array([0, 1, 1] * 4), classes=2), fa.Shrink(0.1), "stated for losses.LeastSquares and losses.LogisticLoss (got SoftmaxLoss)"),
            (lambda z: 0.0, fa.Shrink(0.1), "stated for losses.LeastSquares and losses.LogisticLoss (got function)"),
            (loss, fa.NonNeg(), "stated for proximal.Shrink and proximal.GroupShrink (got NonNeg)"),
            (loss, fa.L1Ball(1.0), "stated for proximal.Shrink and proximal.GroupShrink (got L1Ball)"),
            (fa.LeastSquares(loss.b, weights=np.ones_like(loss.b)), fa.Shrink(0.1), "a loss with observation weights has no certificate"),
            (loss, fa.Shrink(0.0), "needs mu > 0 (got mu = 0.0)"),
            (loss, fa.GroupShrink(-1.0), "needs mu > 0 (got mu = -1.0)"),
            (fa.LeastSquares(np.zeros(5)), fa.Shrink(0.1), "A x has shape (12,), the loss holds b of shape (5,)")):
        with pytest.raises(TypeError) as err:
            ce.duality_gap(A, bad_loss, bad_prox, x)
        assert sentence in str(err.value), str(err.value)
    with pytest.raises(TypeError, match="A must be an ndarray, a scipy.sparse matrix or a map"):
        ce.duality_gap("A", loss, fa.Shrink(0.1), x)
    with pytest.raises(TypeError, match="critical_mu: the certificate is stated for proximal.Shrink and proximal.GroupShrink"):
        ce.critical_mu(A, loss, fa.NonNeg, A.shape[1])
    with pytest.raises(ValueError, match="tolerance must be >= 0"):
        stopping.DualityGap(-1.0)
    with pytest.raises(ValueError, match="every must be a positive integer"):
        stopping.DualityGap(1e-6, every=0)


# ---- the stop rule on the generic loop -------------------------------------------------------------------------------------------------------------
def lasso(seed=0, m=30, n=50, mu=0.4):
    rng = np.random.RandomState(seed)
    A = rng.randn(m, n) / np.sqrt(m)
    xt = np.zeros(n)
    xt[rng.permutation(n)[:5]] = rng.randn(5) * 3
    b = A @ xt + 0.01 * rng.randn(m)
    return A, fa.LeastSquares(b), fa.Shrink(mu)


@pytest.mark.parametrize("every", [1, 7, 10])
def test_the_rule_on_the_generic_loop_stops_on_a_chunk_boundary_with_a_certified_solution(every):
    A, ls, reg = lasso()
    np.random.seed(5)
    c = fa.fasta(A, A.T, ls.f, ls.gradf, reg.g, reg.prox, np.zeros(A.shape[1]), backend="numpy", verbose=False, max_iters=2000,
                 stop_rule=fa.DualityGap(1e-9, every=every), tolerance=123.0)            # (tolerance: unused under the tag)
    assert [i for i, _ in c.gaps] == list(range(0, c.iteration_count + 1, every)) and 0 < c.iteration_count < 2000
    assert all(g > 1e-9 * c.certificate.f0 for _, g in c.gaps[:-1]) and c.gaps[-1][1] == c.certificate.gap <= 1e-9 * c.certificate.f0
    assert ce.duality_gap(A, ls, reg, c.solution) == c.certificate                      # the solution is the certified iterate
    np.random.seed(5)
    plain = fa.fasta(A, A.T, ls.f, ls.gradf, reg.g, reg.prox, np.zeros(A.shape[1]), backend="numpy", verbose=False, max_iters=c.iteration_count,
                     stop_rule=stopping.residual, tolerance=0.0)
    assert not hasattr(plain, "certificate") and not hasattr(plain, "gaps")            # without the tag nothing changes
    np.testing.assert_array_equal(plain.residuals[:c.iteration_count], c.residuals[:c.iteration_count])


def test_the_rule_on_the_generic_loop_ends_at_max_iters_with_the_last_certificate_and_needs_tags():
    A, ls, reg = lasso()
    np.random.seed(5)
    c = fa.fasta(A, A.T, ls.f, ls.gradf, reg.g, reg.prox, np.zeros(A.shape[1]), backend="numpy", verbose=False, max_iters=25, stop_rule=fa.DualityGap(0.0))
    assert c.iteration_count == 25 and [i for i, _ in c.gaps] == [0, 10, 20, 25] and c.certificate.gap > 0
    with pytest.raises(TypeError, match="stated for losses.LeastSquares"):
        fa.fasta(A, A.T, lambda z: .5 * np.sum((z - ls.b) ** 2), lambda z: z - ls.b, reg.g, reg.prox, np.zeros(A.shape[1]), backend="numpy", verbose=False,
                 stop_rule=fa.DualityGap(1e-6))


# ---- the stop rule on FBSolver, over a stand-in context whose dual_gap is the host statement --------------------------------------------------
class GapContext(FakeContext):
    """tests/fake_ctx.py's context plus `dual_gap`: certificates.duality_gap at the committed x0, and a log of where it was asked."""
    matrix = None

    def dual_gap(self):
        loss = fa.LogisticLoss(self.b) if self.loss == "logistic" else fa.LeastSquares(self.b)
        self.asked = getattr(self, "asked", []) + [int(getattr(self, "committed", 0))]
        return ce.duality_gap(self.matrix, loss, fa.Shrink(self.mu), self.x0)

    def init(self):
        self.committed = 0
        return FakeContext.init(self)

    def commit(self, save_best=False):
        self.committed += 1
        FakeContext.commit(self, save_best)


class GapDenseMap(_DeviceMap):
    def __init__(self, A, controller="numpy"):
        A = np.asarray(A, dtype=float)
        self.matrix, self.shape = A, A.shape
        self.ctx = GapContext(lambda x: A @ x, lambda y: A.T @ y, (A.shape[1],), (A.shape[0],), 0, controller)
        self.ctx.matrix = A
        LinearMap.__init__(self, self.ctx.fwd_op, self.ctx.adj_op, (A.shape[1],), (A.shape[0],))


@pytest.mark.parametrize("driver", ["library", "device", "python"])
@pytest.mark.parametrize("every", [4, 10])
def test_the_rule_on_fbsolver_under_the_three_drivers(driver, every):
    A, ls, reg = lasso(1)
    op = GapDenseMap(A)
    np.random.seed(2)
    solver = fa.FBSolver(op, ls, reg, np.zeros(A.shape[1]), verbose=False, max_iters=3000, stop_rule=fa.DualityGap(1e-8, every=every), tolerance=55.0,
                         driver=driver, device_iters=3 if driver != "python" else None).setup()
    c = solver.run()
    k = c.iteration_count
    assert 0 < k < 3000 and k % every == 0
    assert [i for i, _ in c.gaps] == list(range(0, k + 1, every)) == op.ctx.asked                 # every check sits on a chunk boundary of the loop
    assert c.certificate.gap == c.gaps[-1][1] <= 1e-8 * c.certificate.f0 and all(g > 1e-8 * c.certificate.f0 for _, g in c.gaps[:-1])
    np.testing.assert_array_equal(c.solution, op.ctx.x0)                                           # x0 of the committed state, not the best iterate
    assert ce.duality_gap(A, ls, reg, c.solution) == c.certificate == solver.certificate()
    np.random.seed(2)
    host = fa.fasta(A, A.T, ls.f, ls.gradf, reg.g, reg.prox, np.zeros(A.shape[1]), backend="numpy", verbose=False, max_iters=3000,
                    stop_rule=fa.DualityGap(1e-8, every=every))
    assert host.iteration_count == k
    np.testing.assert_allclose(c.solution, host.solution, rtol=1e-6, atol=1e-9)


def test_fbsolver_without_the_tag_is_unchanged_and_certifies_on_demand_and_refuses_acceleration_under_the_tag():
    A, ls, reg = lasso(1)
    op = GapDenseMap(A)
    np.random.seed(2)
    solver = fa.FBSolver(op, ls, reg, np.zeros(A.shape[1]), verbose=False, max_iters=40).setup()
    c = solver.run()
    assert not hasattr(c, "certificate") and not hasattr(c, "gaps") and not hasattr(op.ctx, "asked")
    assert solver.certificate() == ce.duality_gap(A, ls, reg, op.ctx.x0)
    with pytest.raises(ValueError, match="needs accelerate=False"):
        fa.FBSolver(op, ls, reg, np.zeros(A.shape[1]), verbose=False, accelerate=True, stop_rule=fa.DualityGap(1e-6))
    np.random.seed(2)
    capped = fa.FBSolver(op, ls, reg, np.zeros(A.shape[1]), verbose=False, max_iters=25, stop_rule=fa.DualityGap(0.0)).setup().run()
    assert capped.iteration_count == 25 and [i for i, _ in capped.gaps] == [0, 10, 20, 25]


# ---- the path --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logistic,prox_class,L", COMBOS[:3], ids=COMBO_IDS[:3])
def test_the_path_on_host_operands(logistic, prox_class, L):
    rng = np.random.RandomState(4)
    A = rng.randn(40, 60) / np.sqrt(40)
    shape = (60,) if L is None else (60, L)
    xt = np.zeros(shape)
    xt[rng.permutation(60)[:6]] = 3.0
    z = A @ xt + 0.01 * rng.randn(*((40,) if L is None else (40, L)))
    loss = fa.LogisticLoss(np.where(z > 0, 1.0, -1.0)) if logistic else fa.LeastSquares(z)
    np.random.seed(0)
    pts = fa.path(A, loss, prox_class, n_mus=6, ratio=1e-2, gap_tolerance=1e-7, backend="numpy", max_iters=5000)
    mu_c = ce.critical_mu(A, loss, prox_class, shape)
    np.testing.assert_allclose([p.mu for p in pts], mu_c * np.geomspace(1.0, 1e-2, 6), rtol=1e-15)
    assert pts[0].mu == mu_c and pts[0].iteration_count == 0 and not pts[0].solution.any() and pts[0].certificate.gap == 0.0
    support = [int(np.count_nonzero(np.abs(np.reshape(p.solution, (60, -1))).sum(axis=1))) for p in pts]
    assert support == sorted(support) and support[-1] > support[0] == 0
    for p in pts:
        assert p.certificate.relative <= 1e-7 and p.iteration_count < 5000
        assert ce.duality_gap(A, loss, prox_class(p.mu), p.solution) == p.certificate
    cold = fa.path(A, loss, prox_class, mus=[pts[-1].mu], gap_tolerance=1e-7, backend="numpy", max_iters=5000, L=1.0, tau0=0.1)
    assert len(cold) == 1 and cold[0].mu == pts[-1].mu and cold[0].certificate.relative <= 1e-7


def test_the_last_point_of_the_path_agrees_with_a_tight_solve_to_the_accuracy_its_gap_implies():
    A, ls, _ = lasso(3, m=40, n=60)
    np.random.seed(0)
    pts = fa.path(A, ls, fa.Shrink, n_mus=5, ratio=1e-2, gap_tolerance=1e-6, backend="numpy", max_iters=5000)
    last = pts[-1]
    reg = fa.Shrink(last.mu)
    np.random.seed(1)
    tight = fa.fasta(A, A.T, ls.f, ls.gradf, reg.g, reg.prox, np.zeros(60), backend="numpy", verbose=False, max_iters=20000, stop_rule=fa.DualityGap(1e-14))
    assert tight.certificate.relative <= 1e-14 < last.certificate.relative <= 1e-6
    d = A @ (last.solution - tight.solution)
    lhs, bound = 0.5 * float(d @ d), (math.sqrt(last.certificate.gap) + math.sqrt(max(tight.certificate.gap, 0.0))) ** 2
    print("half squared image distance", lhs, "bound", bound)
    assert lhs <= bound


def test_path_refuses_what_it_does_not_serve():
    A, ls, _ = lasso()
    with pytest.raises(TypeError, match="prox_class must be proximal.Shrink or proximal.GroupShrink"):
        fa.path(A, ls, fa.NonNeg, backend="numpy")
    with pytest.raises(TypeError, match="stopped by its duality gap"):
        fa.path(A, ls, fa.Shrink, backend="numpy", stop_rule=stopping.residual)
    with pytest.raises(ValueError, match="the solution is zero for every mu"):
        fa.path(A, fa.LeastSquares(np.zeros(A.shape[0])), fa.Shrink, backend="numpy")
    with pytest.raises(TypeError, match="not device-resident"):
        fa.path(LinearMap(lambda v: A @ v, lambda w: A.T @ w, (A.shape[1],), (A.shape[0],)), ls, fa.Shrink, backend="hip")


def test_the_binding_declares_the_entry_point():
    assert hip.SIGNATURES["fh_dual_gap"][1][0] is hip.SIGNATURES["fh_commit"][1][0] and len(hip.SIGNATURES["fh_dual_gap"][1]) == 2
    assert hip.GAP_NOUT == 8 == len(ce.Certificate._fields) and hasattr(hip.HipContext, "dual_gap")

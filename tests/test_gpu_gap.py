"""GPU tests of the duality-gap certificate (fh_dual_gap, csrc/fh_gap.h) against its host statement (fasta_python_amd/certificates.py), of the stop
rule stopping.DualityGap on the device loop and of fasta.path.  Shapes, dyadic data and the geometry they reach: tests/gap_cases.py.

Bounds.  Least squares on dyadic data: every product and sum of the record is exact (tests/gap_cases.py), all eight outputs `==`.  Logistic: each
of the two sums (f and -D) within 32 eps sum |term| of math.fsum over the host's terms -- a few roundings per term, exp / log to an ulp, a tree of
depth <= 32 -- with s, a quotient of two exactly equal operands, `==`; the host's terms are formed from the device's own z (read after the forward
launch whose commit makes it Z[zc]) and g0.  At a committed state reached by a solve the device reads its own z = A x0
while the host statement forms A x0 itself: both are inner products of at most n = 256 terms, so every output is held to 4 n eps = 1024 eps relative
(the gap, a difference, to 1024 eps (|P| + |D|)); a stale image -- the previous iterate's -- would be off by the size of a step, orders above that.
What a committed state holds: Z[zc] = A x0 after fh_init / fh_setup and after every step without acceleration, under every driver and after a
one-pass step; an accelerated step commits the extrapolated x1 whose image the adjoint launch forms on the fly and never stores, and the call
refuses that state with a sentence."""
import math
import warnings

import numpy as np
import pytest

import fasta_python_amd as fa
from fasta_python_amd import certificates as ce
from fasta_python_amd import hip, stopping
from tests import gap_cases as T
from tests import helpers as H

pytestmark = pytest.mark.gpu

VECS = ("VEC_X0", "VEC_G0", "VEC_XHAT", "VEC_XPROX", "VEC_X1", "VEC_G1", "VEC_BEST", "VEC_B", "VEC_Z", "VEC_T0", "VEC_T1", "VEC_T2", "VEC_T3")


def snapshot(c, n_len, m_len):
    return {v: c.get_vector(getattr(hip, v), m_len if v in ("VEC_B", "VEC_Z") else n_len) for v in VECS}


def at_init(op, loss, reg, x):
    c = op.ctx
    loss.bind(c)
    c.set_prox(reg.kind, reg.mu, 0.0, 0.0)
    c.set_vector(hip.VEC_X0, x)
    c.init()
    return c


# ---- the record against the host statement -----------------------------------------------------------------------------------------------------
# (the sparse operator at every shape whose dense host twin stays small; the long sides are the dense operator's)
DYADIC = [(s, False) for s in T.SHAPES] + [(s, True) for s in T.SHAPES if s[0] * s[1] <= 1 << 18]
DYADIC_IDS = [("csr-" if sparse else "dense-") + "%dx%dx%d" % s for s, sparse in DYADIC]


@pytest.mark.parametrize("shape,sparse", DYADIC, ids=DYADIC_IDS)
def test_least_squares_on_dyadic_data_gives_the_host_record_bit_for_bit(shape, sparse):
    m, n, L = shape
    if sparse:
        from scipy import sparse as sp
    for group in ((False, True) if L > 1 else (False,)):
        A, b, x = T.dyadic_problem(m, n, L, seed=m + 3 * n + L, group=group)
        if sparse:
            A = A * (np.random.RandomState(L).rand(m, n) < 0.3)
        rhs = None if L == 1 else L
        op = fa.SparseMatrixMap(sp.csr_matrix(A), rhs=rhs) if sparse else fa.DenseMatrixMap(A, rhs=rhs)
        try:
            loss = fa.LeastSquares(b)
            probe = at_init(op, loss, fa.Shrink(1.0), x)
            dn = probe.dual_gap().dual_norm
            assert dn > 0
            for mu in (dn, 4.0 * dn, dn / 4.0, math.ceil(dn) / 64.0):
                reg = (fa.GroupShrink if group else fa.Shrink)(mu)
                c = at_init(op, loss, reg, x)
                got = c.dual_gap()
                want = ce.duality_gap(A, loss, reg, x)
                assert tuple(got) == tuple(want), (shape, group, mu)
                assert got == c.dual_gap()                                           # two calls: bit-identical
                x0, g0 = c.get_vector(hip.VEC_X0, x.size).reshape(x.shape), c.get_vector(hip.VEC_G0, x.size).reshape(x.shape)
                assert tuple(ce.certificate_from_parts(x0, g0, A @ x0, loss, reg)) == tuple(got)      # ... and from the vectors read back
                assert got.gap >= 0.0 and (got.scale == 1.0) == (mu >= got.dual_norm)
        finally:
            op.close()


def test_at_zero_the_record_holds_the_critical_mu_and_the_gap_vanishes_from_there_on():
    A, b, _ = T.dyadic_problem(257, 1000, 1, seed=5)
    labels = np.where(b > 0, 1.0, -1.0)
    op = fa.DenseMatrixMap(A)
    try:
        for loss in (fa.LeastSquares(b), fa.LogisticLoss(labels)):
            mu_c = ce.critical_mu(A, loss, fa.Shrink, 1000)
            for mu, zero in ((mu_c, True), (2.0 * mu_c, True), (0.5 * mu_c, False)):
                got = at_init(op, loss, fa.Shrink(mu), np.zeros(1000)).dual_gap()
                assert got.dual_norm == mu_c and got.omega == 0.0 and got.scale == (1.0 if zero else 0.5)
                if type(loss) is fa.LeastSquares:
                    assert (got.gap == 0.0) == zero and got.primal == got.f == got.f0
                else:                                   # the device's log / log1p are good to an ulp: the two sums of m equal terms agree to the logistic bound
                    assert got.f0 == 257 * ce.LN2 and abs(got.f - got.f0) <= 32 * T.EPS * got.f0
                    assert abs(got.gap) <= 64 * T.EPS * got.f0 if zero else got.gap > 0
    finally:
        op.close()


@pytest.mark.parametrize("m,n", [(s[0], s[1]) for s in T.SHAPES if s[2] == 1], ids=[i for i, s in zip(T.IDS, T.SHAPES) if s[2] == 1])
def test_logistic_sums_are_within_the_bound_of_the_hosts_exact_sum(m, n):
    A, labels, x = T.logistic_problem(m, n, seed=m + n)
    op = fa.DenseMatrixMap(A)
    try:
        loss = fa.LogisticLoss(labels)
        probe = at_init(op, loss, fa.Shrink(1.0), x)
        dn = probe.dual_gap().dual_norm
        tau = 1.0 / np.linalg.norm(A, 2) ** 2
        for mu in (2.0 * dn, dn / 3.0, dn / 50.0):
            reg = fa.Shrink(mu)
            c = at_init(op, loss, reg, x)
            c.fwd(tau)
            z = c.get_vector(hip.VEC_Z, m)              # the image of the prox output, as the device formed it: Z[zc] once the step is committed
            c.adj(tau)
            c.commit()
            got = c.dual_gap()
            assert got == c.dual_gap()
            x0, g0 = c.get_vector(hip.VEC_X0, n), c.get_vector(hip.VEC_G0, n)
            s = 1.0 if float(np.max(np.abs(g0))) <= mu else mu / float(np.max(np.abs(g0)))
            assert got.dual_norm == float(np.max(np.abs(g0))) and got.scale == s
            f_sum, f_bound = T.fsum_bound(ce.logistic_loss_terms(z, labels))
            h_sum, h_bound = T.fsum_bound(ce.logistic_dual_terms(z, labels, s))
            om_sum, om_bound = T.fsum_bound(np.abs(x0))
            print(f"m={m} n={n} mu={mu:.3e}: f {got.f - f_sum:+.3e} (bound {f_bound:.3e})  D {-got.dual - h_sum:+.3e} (bound {h_bound:.3e})")
            assert abs(got.f - f_sum) <= f_bound
            assert abs(-got.dual - h_sum) <= h_bound
            assert abs(got.omega - om_sum) <= om_bound
            assert got.f0 == m * ce.LN2 and got.primal == got.f + mu * got.omega and got.gap == got.primal - got.dual
            assert got.gap >= -64 * T.EPS * (abs(got.primal) + abs(got.dual))
    finally:
        op.close()


def test_the_call_changes_no_vector_and_no_state_of_the_context():
    A, b, x = T.dyadic_problem(257, 255, 2, seed=9)
    rng = np.random.RandomState(0)
    A, b = A + rng.randn(*A.shape) / 64, b + rng.randn(*b.shape)          # (not exact: the step below moves)
    op = fa.DenseMatrixMap(A, rhs=2)
    try:
        c = at_init(op, fa.LeastSquares(b), fa.GroupShrink(0.3), x)
        for q in range(4):
            c.set_vector(getattr(hip, "VEC_T%d" % q), rng.randn(255, 2))
        tau = 1.0 / np.linalg.norm(A, 2) ** 2
        first = c.fwd(tau)
        before = snapshot(c, 255 * 2, 257 * 2)
        cert = c.dual_gap()
        after = snapshot(c, 255 * 2, 257 * 2)
        for v in VECS:
            np.testing.assert_array_equal(before[v], after[v], err_msg=v)
        np.testing.assert_array_equal(c.fwd(tau), first)                     # the same forward launch from the same state gives the same scalars
        c.adj(tau)
        c.commit()
        moved = c.dual_gap()
        assert moved != cert and moved == c.dual_gap()
    finally:
        op.close()


# ---- committed states: Z[zc] = A x0 ------------------------------------------------------------------------------------------------------------------
def committed_operators():
    from scipy import sparse as sp
    rng = np.random.RandomState(12)
    ops = {}
    for m, n in ((9, 100), (64, 128)):
        A = rng.randn(m, n) / math.sqrt(m)
        ops["dense%dx%d" % (m, n)] = (lambda A=A: fa.DenseMatrixMap(A), A, (n,), (m,))
    S = sp.random(40, 60, density=0.2, format="csr", random_state=rng, data_rvs=rng.standard_normal)
    ops["csr40x60"] = (lambda: fa.SparseMatrixMap(S), S, (60,), (40,))
    mask = (rng.rand(64) < 0.6).astype(float)
    ops["dct64"] = (lambda: fa.DCTMap(64, mask=mask), None, (64,), (64,))
    mask2 = (rng.rand(8, 12) < 0.7).astype(float)
    ops["dct8x12"] = (lambda: fa.DCTMap((8, 12), mask=mask2), None, (8, 12), (8, 12))
    K = rng.randn(3, 3)
    ops["conv16x16"] = (lambda: fa.ConvMap((16, 16), K), None, (16, 16), (16, 16))
    return ops


OPERATORS = ["dense9x100", "dense64x128", "csr40x60", "dct64", "dct8x12", "conv16x16"]


def assert_close_records(got, want, n_terms=256):
    tol = 4 * n_terms * T.EPS
    for name in ("primal", "dual", "f", "omega", "dual_norm", "scale", "f0"):
        g, w = getattr(got, name), getattr(want, name)
        assert abs(g - w) <= tol * max(abs(w), abs(want.primal) if name == "dual" else 0.0), (name, g, w)
    assert abs(got.gap - want.gap) <= tol * (abs(want.primal) + abs(want.dual)), (got.gap, want.gap)


@pytest.mark.parametrize("name", OPERATORS)
def test_every_committed_state_without_acceleration_holds_the_image_of_its_iterate(name):
    make, host, V, W = committed_operators()[name]
    rng = np.random.RandomState(3)
    op = make()
    try:
        A = host if host is not None else op
        xt = rng.randn(*V) * (rng.rand(*V) < 0.1)
        b = np.asarray(A @ xt if host is not None else op(xt)) + 0.05 * rng.randn(*W)
        loss = fa.LeastSquares(b)
        mu = 0.2 * ce.critical_mu(A, loss, fa.Shrink, V)
        reg = fa.Shrink(mu)
        c = at_init(op, loss, reg, np.zeros(V))                              # after fh_init
        assert_close_records(c.dual_gap(), ce.duality_gap(A, loss, reg, np.zeros(V)))
        seen = []
        for driver in ("python", "library", "device"):
            for adaptive in (False, True):
                np.random.seed(4)
                solver = fa.FBSolver(op, loss, reg, np.zeros(V), verbose=False, max_iters=7, tolerance=0.0, stop_rule=stopping.residual,
                                     adaptive=adaptive, driver=driver).setup()      # after fh_setup
                assert_close_records(solver.certificate(), ce.duality_gap(A, loss, reg, np.zeros(V)))
                solver.advance(3)
                x3 = op.ctx.get_vector(hip.VEC_X0, int(np.prod(V))).reshape(V)
                assert_close_records(solver.certificate(), ce.duality_gap(A, loss, reg, x3))
                solver.advance(4)
                x7 = op.ctx.get_vector(hip.VEC_X0, int(np.prod(V))).reshape(V)
                got = solver.certificate()
                assert_close_records(got, ce.duality_gap(A, loss, reg, x7))
                assert solver.i == 7 and np.any(x7 != x3) and got.gap > 0
                # the iterate still moves: the previous iterate's image would not pass
                stale = ce.duality_gap(A, loss, reg, x3)
                assert abs(stale.f - got.f) > 1e3 * 1024 * T.EPS * got.f
                seen.append(tuple(got))
        assert seen[0] == seen[2] and seen[1] == seen[3] and seen[0] != seen[1]      # step() and the library's loop hold the same state, bit for bit
        # an accelerated step: refused, with the sentence
        np.random.seed(4)
        solver = fa.FBSolver(op, loss, reg, np.zeros(V), verbose=False, max_iters=3, tolerance=0.0, stop_rule=stopping.residual, adaptive=False,
                             accelerate=True).setup()
        solver.certificate()                                                  # (the state of fh_setup is served)
        solver.advance(2)
        with pytest.raises(hip.HipError) as err:
            solver.certificate()
        assert "[10001]" in str(err.value) and "the latest step was accelerated" in str(err.value)
    finally:
        op.close()


@pytest.mark.parametrize("m,n,logistic", [(9, 100, False), (64, 128, False), (64, 128, True)])
def test_a_one_pass_step_commits_the_image_of_its_iterate(m, n, logistic):
    rng = np.random.RandomState(m)
    A = rng.randn(m, n) / math.sqrt(m)
    b = np.where(rng.rand(m) < 0.5, 1.0, -1.0) if logistic else rng.randn(m)
    loss = fa.LogisticLoss(b) if logistic else fa.LeastSquares(b)
    reg = fa.Shrink(0.1 * ce.critical_mu(A, loss, fa.Shrink, n))
    op = fa.DenseMatrixMap(A)
    try:
        c = at_init(op, loss, reg, np.zeros(n))
        assert c.fused_supported() in (1, 3)
        tau = (1.0 if not logistic else 4.0) / np.linalg.norm(A, 2) ** 2
        for _ in range(3):
            c.step(tau)
            c.commit()
            x0 = c.get_vector(hip.VEC_X0, n)
            assert np.any(x0 != 0)
            assert_close_records(c.dual_gap(), ce.duality_gap(A, loss, reg, x0))
    finally:
        op.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------
def refused(c, sentence):
    with pytest.raises(hip.HipError) as err:
        c.dual_gap()
    text = str(err.value)
    assert text.startswith("[%d] fh_dual_gap: " % hip.E_ARG) and sentence in text, text


def test_every_refusal_answers_fh_e_arg_with_its_sentence():
    rng = np.random.RandomState(1)
    A, b = rng.randn(6, 10), rng.randn(6)
    ls = fa.LeastSquares(b)
    op = fa.DenseMatrixMap(A)
    try:
        c = op.ctx
        refused(c, "no loss set")
        ls.bind(c)
        c.set_prox(hip.PROX_SHRINK, 0.5)
        refused(c, "no committed state: call fh_init or fh_setup first")
        c.set_vector(hip.VEC_X0, np.zeros(10))
        c.init()
        assert c.dual_gap().gap >= 0
        for kind in (hip.PROX_IDENTITY, hip.PROX_NONNEG, hip.PROX_LINF, hip.PROX_L1BALL, hip.PROX_BOX):
            c.set_prox(kind, 0.5, -1.0, 1.0)
            refused(c, "implemented for FH_PROX_SHRINK and FH_PROX_GROUP (the context holds prox kind %d)" % kind)
        for mu in (0.0, -1.0):
            c.set_prox(hip.PROX_SHRINK, mu)
            refused(c, "needs mu > 0 (the context holds mu = %g)" % mu)
        c.set_prox(hip.PROX_SHRINK, 0.5)
        assert c.dual_gap().gap >= 0
        c.set_vector(hip.VEC_X0, np.ones(10))                    # a vector set from outside: the state is lost until the next fh_init
        refused(c, "no committed state")
        c.init()
        ls.bind(c)                                               # ... and so it is with the loss
        refused(c, "no committed state")
        c.init()
        c.step_begin(1e-3)
        refused(c, "a step issued by fh_step_begin is still in flight")
        c.step_end()
        c.commit()
        assert c.dual_gap().gap >= 0
        c.fwd(1e-3)
        c.adj(1e-3, accel=True, coef=0.3)
        c.commit()
        refused(c, "the latest step was accelerated")
        c.init()
        assert c.dual_gap().gap >= 0
    finally:
        op.close()
    op = fa.DenseMatrixMap(A, rhs=2)                             # the softmax loss
    try:
        c = op.ctx
        fa.SoftmaxLoss(np.array([0, 1, 1, 0, 1, 0]), classes=2).bind(c)
        c.set_prox(hip.PROX_SHRINK, 0.5)
        c.set_vector(hip.VEC_X0, np.zeros((10, 2)))
        c.init()
        refused(c, "implemented for the least-squares and the logistic loss")
    finally:
        op.close()
    B = rng.randn(4, 5)
    for op, loss, kind, x0, sentence in (
            (fa.IdentityMap((4, 5)), fa.LeastSquares(B), hip.PROX_SHRINK, np.zeros((4, 5)), "the identity operator has no duality-gap certificate"),
            (fa.IdentityMap((4, 5)), fa.LeastSquares(B, weights=np.ones((4, 5))), hip.PROX_SHRINK, np.zeros((4, 5)), "a context that holds observation weights"),
            (fa.GradDivMap((4, 5)), fa.LeastSquares(B), hip.PROX_TVBALL, np.zeros((4, 5, 2)), "the stencil operator has no duality-gap certificate"),
            (fa.GradDivMap((2, 4, 5)), fa.LeastSquares(rng.randn(2, 4, 5)), hip.PROX_SHRINK, np.zeros((2, 4, 5, 3)), "the 3-D stencil operator has no duality-gap certificate")):
        try:
            c = op.ctx
            loss.bind(c)
            c.set_prox(kind, 0.5)
            c.set_vector(hip.VEC_X0, x0)
            c.init()
            refused(c, sentence)
        finally:
            op.close()
    Q = rng.randn(5, 5)
    quad = fa.Quadratic(Q + Q.T)
    op = fa.QuadraticMap(quad, (5,))
    try:
        c = op.ctx
        quad.bind(c)
        c.set_prox(hip.PROX_SHRINK, 0.5)
        c.set_vector(hip.VEC_X0, np.zeros(5))
        c.init()
        refused(c, "the quadratic operator has no duality-gap certificate")
    finally:
        op.close()
    fz = fa.Factorization(np.abs(rng.randn(3, 4)))
    op = fa.BilinearMap(fz, (7, 2))
    try:
        c = op.ctx
        fz.bind(c)
        c.set_prox(hip.PROX_SHRINK, 0.5)
        c.set_vector(hip.VEC_X0, np.ones((7, 2)))
        c.init()
        refused(c, "the bilinear operator has no duality-gap certificate")
    finally:
        op.close()
    op = fa.ShardedDenseMatrixMap(A, devices=(0, 0))
    try:
        c = op.ctx
        ls.bind(c)
        c.set_prox(hip.PROX_SHRINK, 0.5)
        c.set_vector(hip.VEC_X0, np.zeros(10))
        c.init()
        refused(c, "a multi-device context or a context with a communicator holds a row block")
    finally:
        op.close()
    c = hip.HipContext()
    try:
        refused(c, "the operator has no duality-gap certificate")
    finally:
        c.close()


# ---- the stop rule and the path on the device ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["logistic_100x160_adaptive", "sparse_ls_64x128_adaptive", "logistic_100x160_plain", "sparse_ls_64x128_plain"])
@pytest.mark.parametrize("driver", ["library", "device", "python"])
def test_fasta_under_the_gap_rule_on_the_fixture_problems(name, driver):
    meta, z = H.load_case(name)
    d = H.case_data(meta, z)
    A = np.asarray(d["A"])
    loss = fa.LogisticLoss(d["b"]) if meta["kind"] == "logistic" else fa.LeastSquares(d["b"])
    reg = fa.Shrink(float(d["mu"]))
    opts = dict(verbose=False, adaptive=meta["options"]["adaptive"], max_iters=5000, stop_rule=fa.DualityGap(1e-8))
    runs = {}
    for backend in ("hip", "numpy"):
        np.random.seed(meta["solver_seed"])
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            extra = dict(driver=driver) if backend == "hip" else {}
            runs[backend] = fa.fasta(A, A.T, loss.f, loss.gradf, reg.g, reg.prox, np.zeros(A.shape[1]), backend=backend, **opts, **extra)
    got, want = runs["hip"], runs["numpy"]
    host = ce.duality_gap(A, loss, reg, got.solution)
    print(name, driver, "iterations", got.iteration_count, want.iteration_count, "relative gap: device", got.certificate.relative, "host", host.relative)
    assert host.relative <= 1e-8 and got.certificate.relative <= 1e-8
    assert got.iteration_count == want.iteration_count and got.iteration_count % 10 == 0 and 0 < got.iteration_count < 5000
    assert [i for i, _ in got.gaps] == list(range(0, got.iteration_count + 1, 10))
    assert_close_records(got.certificate, host, n_terms=256)
    np.testing.assert_allclose(got.solution, want.solution, rtol=1e-5, atol=1e-9)


@pytest.mark.parametrize("sparse", [False, True], ids=["dense64x128", "csr40x60"])
def test_the_path_on_the_device(sparse):
    from scipy import sparse as sp
    rng = np.random.RandomState(8)
    if sparse:
        A = sp.random(40, 60, density=0.2, format="csr", random_state=rng, data_rvs=rng.standard_normal)
        n = 60
    else:
        A = rng.randn(64, 128) / 8.0
        n = 128
    xt = np.zeros(n)
    xt[rng.permutation(n)[:5]] = 2.0 * rng.randn(5)
    loss = fa.LeastSquares(A @ xt + 0.01 * rng.randn(A.shape[0]))
    runs = {}
    for backend in ("hip", "numpy"):
        np.random.seed(2)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            runs[backend] = fa.path(A, loss, fa.Shrink, n_mus=6, ratio=1e-2, gap_tolerance=1e-7, backend=backend, max_iters=5000)
    got, want = runs["hip"], runs["numpy"]
    assert len(got) == len(want) == 6
    assert got[0].iteration_count == 0 and not got[0].solution.any() and got[0].certificate.gap == 0.0      # at the critical mu: identically zero
    np.testing.assert_allclose([p.mu for p in got], [p.mu for p in want], rtol=1e-13)
    supports = [set(np.flatnonzero(p.solution)) for p in got]
    host_supports = [set(np.flatnonzero(p.solution)) for p in want]
    assert supports == host_supports
    assert [len(s) for s in supports] == sorted(len(s) for s in supports) and len(supports[-1]) > 0
    for p, w in zip(got, want):
        assert p.certificate.relative <= 1e-7 and ce.duality_gap(A, loss, fa.Shrink(p.mu), p.solution).relative <= 1e-7
        assert p.iteration_count == w.iteration_count
        np.testing.assert_allclose(p.solution, w.solution, rtol=1e-5, atol=1e-9)


@pytest.mark.parametrize("argv", [[], ["--sparse", "0.1", "--columns", "3"], ["--logistic"]], ids=["lasso", "sparse-mmv", "logistic"])
def test_the_example_runs_in_its_three_modes(argv, capsys):
    from fasta_python_amd.examples import lasso_path
    out = lasso_path.main(["--backend", "hip", "--rows", "40", "--features", "80"] + argv)
    text = capsys.readouterr().out
    assert "relative gap" in text and set(out) == {"adaptive", "accelerated", "plain"}
    for mode in ("adaptive", "plain"):
        pts = out[mode]
        assert len(pts) == 10 and not pts[0].solution.any() and pts[0].iteration_count == 0
        assert all(p.certificate.relative <= 1e-6 or p.iteration_count == 5000 for p in pts) and pts[1].certificate.relative <= 1e-6
    assert "needs accelerate=False" in out["accelerated"] and "not served on the device" in text      # the device does not certify an extrapolated iterate
    host = lasso_path.main(["--backend", "numpy", "--rows", "40", "--features", "80"] + argv)
    assert len(host["accelerated"]) == 10                                                               # the host loop does
    assert [p.mu for p in host["adaptive"]] == pytest.approx([p.mu for p in out["adaptive"]], rel=1e-12)

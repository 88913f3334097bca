"""GPU tests of the identity operator with an elementwise loss and the nuclear-norm prox (fh_set_identity, FH_PROX_NUCLEAR, csrc/fh_nuclear.h) --
through the C ABI and through fasta().  Every thresholding test first asserts, through fh_nuclear_shape, the geometry it claims to reach.

Tolerances.  The prox: ||xprox_dev - project_Lnuc_ball(xhat, tau*mu)||_F <= 32 * p * eps * ||xhat||_F against float64 LAPACK (thresholding is
non-expansive, so the decomposition's backward error is not amplified; the NumPy restatement of the rule stays within 0.5 - 4.5 of those
units, tests/test_nuclear_cpu.py, and 32 is that worst case times 8 for FMA contraction and the device's summation order); the sum of the kept
singular values p times that (Weyl: every value moves by at most the perturbation's norm).  The exact input is compared with np.array_equal.
The elementwise kinds are bit-exact (`==` against the NumPy expressions) on exact inputs.  Whole solves: histories rtol 1e-6, atol 1e-14 over
the recorded twin-divergence prefix, solutions rtol 1e-5 with a floor of 1e-6 of the largest entry -- what tests/test_gpu_quad.py holds the
quadratic form to.  Every case asserts sweeps < 30."""
import warnings

import numpy as np
import pytest
from numpy import linalg as la

import fasta_python_amd as fa
from fasta_python_amd import hip
from fasta_python_amd import stopping as fstop
from tests import gpu_util as G
from tests import nuclear_cases as NC

pytestmark = pytest.mark.gpu


def open_identity(M, N, Bk=0, loss="lsq", B=None):
    """(map, context) of the identity operator on (M, N) under FH_TUNE_NUC_BLOCK_ROWS = Bk, a loss set."""
    op = fa.IdentityMap((M, N), tuning={hip.TUNE_NUC_BLOCK_ROWS: Bk} if Bk else None)
    c = op.ctx
    assert c.shape() == (M * N, M * N) and c.fused_supported() == 0 and c.fused_agree() == 0 and not c.run_supported()
    B = np.zeros((M, N)) if B is None else B
    (c.set_loss_lsq if loss == "lsq" else c.set_loss_logistic)(B)
    return op, c


def device_threshold(X, thr, Bk, objective=True):
    """(xprox, forward scalars, NuclearInfo) of one forward launch with x0 = X, g0 = 0, tau = 1, mu = thr; the geometry asserted."""
    M, N = X.shape
    op, c = open_identity(M, N, Bk)
    try:
        c.set_prox_nuclear(thr, objective)
        assert c.nuclear_shape()._asdict() == NC.shape_of(M, N, Bk) == hip.nuclear_shape(M, N, Bk)._asdict()
        c.set_vector(hip.VEC_X0, X)
        c.set_vector(hip.VEC_G0, np.zeros(M * N))
        s = c.fwd(1.0)
        return c.get_vector(hip.VEC_XPROX, M * N).reshape(M, N), s, c.nuclear_info(), c.get_vector(hip.VEC_XHAT, M * N).reshape(M, N)
    finally:
        op.close()


# ---- exact ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("transposed", [False, True], ids=["5x16", "16x5"])
@pytest.mark.parametrize("Bk", [1, 2, 8])
def test_exact_input_bit_for_bit(Bk, transposed):
    X, want = NC.exact_input()
    if transposed:
        X, want = np.ascontiguousarray(X.T), np.ascontiguousarray(want.T)
    runs = [device_threshold(X, NC.EXACT_THR, Bk) for _ in range(2)]
    out, s, info, xhat = runs[0]
    assert np.array_equal(out, want) and np.array_equal(xhat, X)                                            # (the zero rows that pad p to P added nothing)
    assert info == hip.NuclearInfo(1, NC.shape_of(*X.shape, Bk)["steps_per_sweep"], 0, NC.EXACT_RANK)       # one sweep, zero rotations: J = I
    assert s[hip.S_GSUM] == NC.EXACT_GSUM and s[hip.S_ALPHA] == NC.EXACT_RANK
    assert s[hip.S_FSQ] == float(np.sum(want * want)) and s[hip.S_XH2] == float(np.sum((want - X) ** 2)) and s[hip.S_GMAX] == 12.0
    assert np.array_equal(runs[1][0], out) and np.array_equal(runs[1][1], s) and runs[1][2] == info        # repeatable bit for bit


# ---- rotating cases --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", NC.CASES, ids=lambda c: c.name)
def test_rotating_cases_against_lapack(case):
    X, thr = NC.case_input(case)
    out, s, info, xhat = device_threshold(X, thr, case.Bk)
    want = fa.proximal.project_Lnuc_ball(X, thr)
    sv = la.svd(X, compute_uv=False)
    err, lim = float(la.norm(out - want)), NC.tolerance(X)
    unit = lim / NC.TOL_FACTOR
    print(f"\n{case.name}: {info}, error {err / unit if unit else err:.2f} p eps |X|_F", end="")
    assert np.array_equal(xhat, X) and np.isfinite(out).all()
    assert info.sweeps < NC.MAX_SWEEPS and info.steps == info.sweeps * NC.shape_of(case.M, case.N, case.Bk)["steps_per_sweep"]
    assert err <= lim
    assert abs(s[hip.S_GSUM] - float(np.sum(np.maximum(sv - thr, 0)))) <= min(X.shape) * lim
    assert abs(s[hip.S_GMAX] - max(float(sv[0]) - thr, 0.0)) <= lim and s[hip.S_ALPHA] == info.rank == int(np.sum(sv > thr))
    if case.kind in ("zero", "below"):
        assert not out.any() and s[hip.S_GSUM] == 0.0 and s[hip.S_GMAX] == 0.0 and info.rank == 0                                    # exact zeros, no NaN
    if case.kind == "mu0":
        assert la.norm(out - X) <= lim
    if case.kind == "duplicated":
        assert la.matrix_rank(out) <= case.M // 2


def test_device_prox_is_the_forward_path():
    case = NC.CASES[0]
    X, thr = NC.case_input(case)
    reg = fa.NuclearShrink(thr)
    got = fa.proximal.device_prox(reg, X, 0.5)
    want = device_threshold(X, 0.5 * thr, 0)[0]
    assert np.array_equal(got, want) and np.array_equal(reg.prox_on_device(X, 0.5), want)
    assert la.norm(got - reg.prox(X, 0.5)) <= NC.tolerance(X)
    fa.proximal.release_scratch()


# ---- steps -----------------------------------------------------------------------------------------------------------------------------------------
def _exact_problem(M=6, N=10):
    """Dyadic data: every elementwise expression of a step is exact in float64 (the least-squares loss; tau and coef powers of two)."""
    rng = np.random.RandomState(5)
    X0 = rng.randint(-8, 9, (M, N)) / 4.0
    B = rng.randint(-8, 9, (M, N)) / 8.0
    return X0, B


@pytest.mark.parametrize("kind", ["identity", "shrink", "nonneg", "box"])
def test_one_step_of_the_elementwise_kinds_is_bit_exact(kind):
    X0, B = _exact_problem()
    M, N = X0.shape
    tag = {"identity": fa.NoProx(), "shrink": fa.Shrink(0.5), "nonneg": fa.NonNeg(), "box": fa.Box(-0.5, 0.75)}[kind]
    op, c = open_identity(M, N, 0, "lsq", B)
    try:
        c.set_prox(tag.kind, tag.mu, tag.lo, tag.hi)
        c.set_vector(hip.VEC_X0, X0)
        s = c.init()
        g0 = X0 - B
        assert np.array_equal(c.get_vector(hip.VEC_G0, M * N).reshape(M, N), g0) and s[hip.S_FSQ] == float(np.sum(g0 * g0))
        assert s[hip.S_GSUM] == float(np.sum(np.abs(X0))) and s[hip.S_GMAX] == float(np.max(np.abs(X0)))
        tau, coef = 0.25, 0.5
        s = c.fwd(tau)
        xhat = X0 - tau * g0
        xp = tag.prox(xhat, tau)
        assert np.array_equal(c.get_vector(hip.VEC_XHAT, M * N).reshape(M, N), xhat)
        assert np.array_equal(c.get_vector(hip.VEC_XPROX, M * N).reshape(M, N), xp) and np.array_equal(c.get_vector(hip.VEC_Z, M * N).reshape(M, N), xp)
        want = {hip.S_FSQ: np.sum((xp - B) ** 2), hip.S_DXG0: np.sum((xp - X0) * g0), hip.S_DX2: np.sum((xp - X0) ** 2), hip.S_XH2: np.sum((xp - xhat) ** 2),
                hip.S_G02: np.sum(g0 * g0), hip.S_GSUM: np.sum(np.abs(xp)), hip.S_GMAX: np.max(np.abs(xp)), hip.S_RDOT: np.sum((X0 - xp) * (xp - X0)), hip.S_ALPHA: 0.0}
        for slot, v in want.items():
            assert s[slot] == float(v), slot
        a = c.adj(tau)
        g1 = xp - B
        assert np.array_equal(c.get_vector(hip.VEC_G1, M * N).reshape(M, N), g1)
        dg = g1 + (xhat - X0) / tau
        want = {hip.S_DXDG: np.sum((xp - X0) * dg), hip.S_DG2: np.sum(dg * dg), hip.S_FSQ_ADJ: np.sum(g1 * g1), hip.S_XH2_ADJ: np.sum((xp - xhat) ** 2),
                hip.S_GSUM_ADJ: np.sum(np.abs(xp)), hip.S_GMAX_ADJ: np.max(np.abs(xp))}
        for slot, v in want.items():
            assert a[slot] == float(v), slot
        assert np.array_equal(c.fwd_adj(tau)[:14], np.concatenate((s[:8], a[8:14])))                        # the pair under one synchronisation
        a = c.adj(tau, True, coef)                                                                          # accelerated: x_accel0 = x0 after init
        x1 = xp + coef * (xp - X0)
        assert np.array_equal(c.get_vector(hip.VEC_X1, M * N).reshape(M, N), x1) and np.array_equal(c.get_vector(hip.VEC_G1, M * N).reshape(M, N), x1 - B)
        assert a[hip.S_FSQ_ADJ] == float(np.sum((x1 - B) ** 2)) and a[hip.S_GSUM_ADJ] == float(np.sum(np.abs(x1)))
        c.commit(True)
        assert np.array_equal(c.get_vector(hip.VEC_X0, M * N).reshape(M, N), x1) and np.array_equal(c.get_vector(hip.VEC_BEST, M * N).reshape(M, N), x1)
        assert np.array_equal(c.apply(X0), X0.ravel()) and np.array_equal(c.apply(X0, adjoint=True), X0.ravel())   # fh_apply: a copy
    finally:
        op.close()


@pytest.mark.parametrize("loss", ["lsq", "logistic"])
def test_one_step_with_the_nuclear_prox_on_both_losses(loss):
    rng = np.random.RandomState(11)
    M, N, mu, tau, coef = 7, 12, 5.0, 0.5, 0.25
    B = np.sign(rng.randn(M, N))
    X0 = rng.randn(M, N)
    ll = fa.LogisticLoss(B) if loss == "logistic" else fa.LeastSquares(B)
    reg = fa.NuclearShrink(mu)
    op, c = open_identity(M, N, 2, loss, B)
    try:
        reg.bind_prox(c, True)
        c.set_vector(hip.VEC_X0, X0)
        s = c.init()
        lim = NC.tolerance(X0)
        f0 = ll.f(X0) if loss == "logistic" else 2 * ll.f(X0)
        np.testing.assert_allclose(s[hip.S_FSQ], f0, rtol=1e-13)
        assert abs(s[hip.S_GSUM] - la.svd(X0, compute_uv=False).sum()) <= min(M, N) * lim and abs(s[hip.S_GMAX] - la.norm(X0, 2)) <= lim
        g0 = c.get_vector(hip.VEC_G0, M * N).reshape(M, N)
        np.testing.assert_allclose(g0, ll.gradf(X0), rtol=1e-14, atol=1e-16)
        s = c.fwd(tau)
        info = c.nuclear_info()
        xhat = c.get_vector(hip.VEC_XHAT, M * N).reshape(M, N)
        xp = c.get_vector(hip.VEC_XPROX, M * N).reshape(M, N)
        assert np.array_equal(xhat, X0 - tau * g0) and info.sweeps < NC.MAX_SWEEPS and 0 < info.rank == s[hip.S_ALPHA] < min(M, N)
        assert la.norm(xp - fa.proximal.project_Lnuc_ball(xhat, tau * mu)) <= NC.tolerance(xhat)
        assert abs(s[hip.S_GSUM] - la.svd(xp, compute_uv=False).sum()) <= min(M, N) * NC.tolerance(xhat) and abs(s[hip.S_GMAX] - la.norm(xp, 2)) <= NC.tolerance(xhat)
        np.testing.assert_allclose(s[hip.S_FSQ], ll.f(xp) if loss == "logistic" else 2 * ll.f(xp), rtol=1e-13)
        np.testing.assert_allclose(s[hip.S_DX2], np.sum((xp - X0) ** 2), rtol=1e-13)
        a = c.adj(tau)
        assert a[hip.S_GSUM_ADJ] == s[hip.S_GSUM] and a[hip.S_GMAX_ADJ] == s[hip.S_GMAX]                                                           # x1 is xprox: the thresholding's sum
        np.testing.assert_allclose(c.get_vector(hip.VEC_G1, M * N).reshape(M, N), ll.gradf(xp), rtol=1e-14, atol=1e-16)
        both = c.fwd_adj(tau)
        assert np.array_equal(both[:8], s[:8]) and np.array_equal(both[8:15], a[8:15])
        a = c.adj(tau, True, coef)
        x1 = c.get_vector(hip.VEC_X1, M * N).reshape(M, N)
        assert np.array_equal(x1, xp + coef * (xp - X0))
        assert abs(a[hip.S_GMAX_ADJ] - la.norm(x1, 2)) <= NC.tolerance(x1) and abs(a[hip.S_GSUM_ADJ] - la.svd(x1, compute_uv=False).sum()) <= min(M, N) * NC.tolerance(x1)   # a values-only decomposition of x1
        assert c.nuclear_info() == info                                                                     # ... which is not "the last prox"
        # objective = 0: NaN in exactly the two slots
        reg.bind_prox(c, False)
        s0 = c.init()
        assert np.isnan(s0[hip.S_GSUM]) and np.isfinite(np.delete(s0, hip.S_GSUM)).all() and s0[hip.S_GMAX] == 0.0
        sf = c.fwd(tau)
        assert np.isfinite(sf).all() and sf[hip.S_GSUM] == s[hip.S_GSUM]
        assert np.isfinite(c.adj(tau)).all()
        aa = c.adj(tau, True, coef)
        assert np.isnan(aa[hip.S_GSUM_ADJ]) and np.isfinite(np.delete(aa, hip.S_GSUM_ADJ)).all() and aa[hip.S_GMAX_ADJ] == 0.0
    finally:
        op.close()


# ---- solves ----------------------------------------------------------------------------------------------------------------------------------------
def solve(meta, d, **extra):
    ms = NC.capture_script()
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
        meta, z, d = NC.load(name)
        k, whole = NC.compared_prefix(meta, z)
        extra = {} if whole else dict(max_iters=k, tolerance=0.0)
        _runs[name] = (solve(meta, d, driver="library", **extra), k, whole, extra)
    return _runs[name]


@pytest.mark.parametrize("name", NC.EXPECTED)
def test_fixture_solves_on_the_device(name):
    meta, z, d = NC.load(name)
    lib, k, whole, extra = library_run(name)
    assert lib.library_steps == lib.iteration_count and lib.device_steps == 0
    print(f"\n{name}: device {lib.iteration_count} iterations / {lib.backtracks} backtracks, reference {int(z['iteration_count'])} / {int(z['backtracks'])}", end="")
    if whole:
        assert lib.iteration_count == int(z["iteration_count"]) and lib.backtracks == int(z["backtracks"])
    else:
        assert k >= NC.MIN_PREFIX and lib.iteration_count == k and lib.backtracks == meta["backtracks_at_divergence"]
    worst = G.compare_histories(lib, lambda f: z[f], k, rtol=1e-6, atol=1e-14)
    print(f"; {k} iterations compared, worst relative deviation of a history entry {worst:.2e}")
    if whole:
        np.testing.assert_allclose(lib.solution, z["solution"], rtol=1e-5, atol=1e-6 * float(np.max(np.abs(z["solution"]))))


@pytest.mark.parametrize("name", NC.EXPECTED)
def test_library_and_python_drivers_are_bit_identical(name):
    meta, z, d = NC.load(name)
    lib, k, whole, extra = library_run(name)
    py = solve(meta, d, driver="python", **extra)
    assert py.library_steps == 0 and py.iteration_count == lib.iteration_count and py.backtracks == lib.backtracks
    for f in NC.HISTORIES:
        assert np.array_equal(getattr(py, f), getattr(lib, f), equal_nan=True), f
    assert np.array_equal(py.solution, lib.solution)


def test_least_squares_solution_is_the_closed_form():
    meta, z, d = NC.load("lsq_10x14_plain")
    lib = library_run("lsq_10x14_plain")[0]
    want = fa.proximal.project_Lnuc_ball(d["B"], float(d["mu"]))
    np.testing.assert_allclose(lib.solution, z["solution"], rtol=1e-5, atol=1e-6 * float(np.max(np.abs(want))))
    assert la.norm(lib.solution - want) <= 1e-3 * la.norm(want)


def test_an_explicit_identity_map_is_equivalent():
    meta, z, d = NC.load("lmc_12x20_adaptive")
    ms = NC.capture_script()
    f, gradf, g, proxg, x0 = ms.operands(fa, meta["kind"], d)
    op = fa.IdentityMap(x0.shape)
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            c = fa.fasta(op, f, gradf, g, proxg, x0, verbose=False, backend="hip", **ms.resolve(meta["options"], fstop))
    finally:
        op.close()
    lib = library_run("lmc_12x20_adaptive")[0]
    assert np.array_equal(c.solution, lib.solution) and np.array_equal(c.stepsizes, lib.stepsizes)


def test_the_example_runs_on_the_device(capsys):
    from fasta_python_amd.examples import logistic_matrix_completion as ex
    results = ex.main(["--backend", "hip", "--rows", "24", "--cols", "60", "--rank", "3", "--mu", "4.0"])
    assert len(results) == 3
    for solution, conv in results:
        assert solution.shape == (24, 60) and np.isfinite(solution).all() and conv.iteration_count > 0
        assert 0 < la.matrix_rank(solution, tol=1e-3 * la.norm(solution, 2)) < 24


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------------
def refusal(code, text):
    return pytest.raises(hip.HipError, match=rf"\[{code}\].*{text}")


def test_what_the_identity_operator_does_not_serve_is_refused_with_its_code_and_sentence():
    op, c = open_identity(4, 6)
    try:
        for kind in (hip.PROX_LINF, hip.PROX_L1BALL, hip.PROX_TVBALL, hip.PROX_GROUP, hip.PROX_ROWBALL):
            with pytest.raises(hip.HipError, match=r"\[10001\]"):
                c.set_prox(kind, 1.0)
        with refusal(hip.E_ARG, "fh_set_prox_split"):
            c.set_prox(hip.PROX_ROWSPLIT, 1.0)
        with refusal(hip.E_STATE, "bilinear operator only"):
            c.set_prox_split(2, hip.PROX_SHRINK, 1.0)
        c.set_prox(hip.PROX_NUCLEAR, 1.0)
        c.set_vector(hip.VEC_X0, np.zeros(24))
        c.init()
        for call, text in ((lambda: c.step(0.1), "no one-pass kernel"), (lambda: c.step_accel(0.1, 0.0, False), "no one-pass kernel"),
                           (lambda: c.step_begin(0.1), "no one-pass kernel"), (lambda: c.set_rhs(2), "no multi-column form"),
                           (lambda: c.get_matrix_rows(0, 1), "keeps no matrix"), (lambda: c.stream_read_ms(), "dense matrix"),
                           (lambda: c.comm_init(1, 0, bytes(128)), "cannot be row-sharded")):
            with refusal(hip.E_STATE, text):
                call()
        with refusal(hip.E_STATE, "no device-side loop"):
            c.run(1, hip.RunOpts(window=1), hip.RunState())
        with refusal(hip.E_ARG, "entries"):
            c.set_loss_logistic(np.ones(23))
        with refusal(hip.E_ARG, "NUC_BLOCK_ROWS"):
            c.set_tuning(hip.TUNE_NUC_BLOCK_ROWS, 3)
        for M, N in ((0, 4), (4, 0), (1 << 13, (1 << 13) + 1)):
            with pytest.raises(hip.HipError, match=r"\[10001\]"):
                c.set_identity(M, N)
        # a context holding NUCLEAR returns to IDENTITY when another operator is set, and every other operator refuses it
        c.set_matrix(np.eye(3))
        c.set_loss_lsq(np.zeros(3))
        c.set_vector(hip.VEC_X0, np.ones(3))
        c.init()
        c.fwd(0.5)
        assert np.array_equal(c.get_vector(hip.VEC_XPROX, 3), np.full(3, 0.5))
        for setter in (lambda: c.set_prox(hip.PROX_NUCLEAR, 1.0), lambda: c.set_prox_nuclear(1.0)):
            with refusal(hip.E_STATE, "identity operator only"):
                setter()
        with refusal(hip.E_STATE, "fh_nuclear_shape"):
            c.nuclear_shape()
        c.set_identity(1025, 1030)
        with refusal(hip.E_ARG, "<= 1024"):
            c.set_prox_nuclear(1.0)
    finally:
        op.close()
    with hip.HipContext(0, "f32") as c32:
        with refusal(hip.E_STATE, "float32 storage"):
            c32.set_identity(4, 6)
    with hip.HipContext(devices=[0, 0]) as shell:
        with refusal(hip.E_STATE, "multi-device"):
            shell.set_identity(4, 6)

"""CPU tier of the quadratic smooth term (fh_set_quadratic, csrc/fh_quad.h; losses.Quadratic, proximal.RowBall): the fixtures
tests/golden/quad/*.npz were captured from the reference core (scripts/make_quad_golden.py) with the tags' closures and the identity operator;
the NumPy oracle and `fasta(None, None, ..., backend="numpy")` must reproduce them bit for bit, the closures must be the reference examples'
own, operand recognition must name what the device does not serve, the exported launch geometry must hold what every GPU-tier case claims of
it, the exact inputs must be exact, and nothing may fall back when there is no GPU.  No GPU."""
import os
import warnings

import numpy as np
import pytest
from numpy import linalg as la

import fasta_python_amd as fa
from fasta_python_amd import hip, solver
from fasta_python_amd import stopping as fstop
from oracle import fasta_np as fo
from tests import quad_cases as QC


def assert_same_run(c, z):
    assert c.iteration_count == int(z["iteration_count"]) and c.backtracks == int(z["backtracks"])
    for field in QC.HISTORIES:
        assert np.array_equal(getattr(c, field), z[field], equal_nan=True), field
    assert np.array_equal(c.solution, z["solution"])


# ---- the fixture set ---------------------------------------------------------------------------------------------------------------------------
def test_the_fixture_set_is_the_one_the_script_describes():
    names = [row[0] for row in QC.capture_script().case_table()]
    assert sorted(names) == QC.FIXTURES == QC.EXPECTED
    assert all(os.path.getsize(os.path.join(QC.QUAD, n + ".npz")) < 100 << 10 for n in QC.FIXTURES)


def test_the_fixtures_cover_the_prox_kinds_the_column_layouts_and_a_missing_prox_term():
    kinds, lbs = set(), set()
    for name in QC.FIXTURES:
        meta, z, d = QC.load(name)
        kinds.add(meta["kind"])
        lbs.add(QC.lb_of(1 if d["x0"].ndim == 1 else d["x0"].shape[1]))
        assert np.array_equal(d["Q"], d["Q"].T) and d["Q"].dtype == np.float64, name
        assert z["solution"].shape == d["x0"].shape and meta["options"]["L"] > 0 and meta["options"]["tau0"] > 0, name
    assert kinds == {"maxnorm", "svm", "shrink", "nonneg", "group", "gnone"} and lbs == {2, 4, 8, 16}
    _, _, d = QC.load("maxnorm_60x5_adaptive")
    assert la.eigvalsh(d["Q"])[0] < -1                                    # max-norm's Q has negative eigenvalues: no .5 ||A x - b||^2 has it
    _, _, d = QC.load("shrink_90_adaptive")
    assert la.eigvalsh(d["Q"])[0] > 0 and np.count_nonzero(d["xstar"]) <= 9 and np.array_equal(d["c"], -(d["Q"] @ d["xstar"]))


@pytest.mark.parametrize("name", QC.EXPECTED)
def test_twin_parting_iteration_is_recomputed(name):
    """The basis for what the device is held to: the oracle and a twin of itself with permuted unknowns (same L, same tau0) agree on every step
    size up to the stored iteration -- the whole run, except for the forced-backtracking fixture."""
    meta, z, d = QC.load(name)
    ms = QC.capture_script()
    assert ms.twin_divergence(meta["kind"], d, meta["options"]) == meta["twin_divergence"]
    k, whole = QC.compared_prefix(meta, z)
    assert whole == ("backtracks" not in name)
    if not whole:
        assert k >= QC.MIN_PREFIX and int(z["backtracks"]) >= 5
        cut = ms.run_oracle(meta["kind"], d, dict(meta["options"], max_iters=k, tolerance=0.0))
        assert cut.backtracks == meta["backtracks_at_divergence"] <= int(z["backtracks"])


def test_every_mode_has_a_fixture_that_is_compared_whole():
    whole = set()
    for name in QC.EXPECTED:
        meta, z, _ = QC.load(name)
        if QC.compared_prefix(meta, z)[1]:
            o = meta["options"]
            whole.add("adaptive" if o["adaptive"] else "accelerated" if o["accelerate"] else "plain")
    assert whole == {"adaptive", "accelerated", "plain"}
    assert any(int(QC.load(n)[1]["backtracks"]) > 0 and QC.compared_prefix(*QC.load(n)[:2])[1] for n in QC.EXPECTED)      # ... one of them with backtracks


# ---- bit-for-bit reproduction ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", QC.EXPECTED)
def test_oracle_reproduces_the_reference_run(name):
    meta, z, d = QC.load(name)
    assert_same_run(QC.capture_script().run_oracle(meta["kind"], d, meta["options"]), z)


@pytest.mark.parametrize("name", QC.EXPECTED)
def test_generic_loop_on_the_tags_closures_reproduces_the_reference_run(name):
    """fasta(None, None, q.f, q.gradf, g, prox, x0, backend="numpy"): the generic loop on the tags' closures, no device context anywhere."""
    meta, z, d = QC.load(name)
    ms = QC.capture_script()
    f, gradf, g, proxg, x0 = ms.operands(fa, meta["kind"], d)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        c = fa.fasta(None, None, f, gradf, g, proxg, x0, backend="numpy", verbose=False, **ms.resolve(meta["options"], fstop))
        six = fa.fasta(None, f, gradf, g, proxg, x0, backend="numpy", verbose=False, **ms.resolve(meta["options"], fstop))
    assert_same_run(c, z)
    assert_same_run(six, z)


# ---- the closures are the reference examples' own ------------------------------------------------------------------------------------------------
def rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(float(np.max(np.abs(b))), 1e-300))


@pytest.mark.parametrize("name", [n for n in QC.EXPECTED if n.startswith("maxnorm")])
def test_quadratic_closures_are_max_norms(name):
    """examples/max_norm.py:49-50: f = sum(S * (X @ X.T)), gradf = (S + S.T) @ X -- at x0 and at the solution."""
    _, z, d = QC.load(name)
    S, q = d["S"], fa.Quadratic(d["Q"])
    assert np.array_equal(d["Q"], S + S.T)
    for X in (d["x0"], z["solution"]):
        assert rel(q.f(X), np.sum(S * (X @ X.T))) <= 1e-12
        assert rel(q.gradf(X), (S + S.T) @ X) <= 1e-12


def test_quadratic_closures_are_the_svm_duals():
    """examples/svm.py:68-69 on the fixture's points with the LINEAR kernel, Q = (l l^T) * (D D^T), c = -1."""
    from fasta_python_amd.examples.svm import kernel_matrix
    _, _, d = QC.load("svm_rbf_80_adaptive")
    D, l = d["D"], d["l"]
    Q = np.outer(l, l) * kernel_matrix(D, "linear")
    assert np.array_equal(Q, Q.T)
    q = fa.Quadratic(Q, -np.ones(len(l)))
    rng = np.random.RandomState(3)
    for y in (rng.rand(len(l)), np.zeros(len(l)), rng.randn(len(l))):
        f_ref = .5 * la.norm((D.T @ (l * y)).ravel()) ** 2 - np.sum(y)
        assert abs(q.f(y) - f_ref) <= 1e-12 * max(abs(f_ref), .5 * la.norm(D.T @ (l * y)) ** 2)
        assert rel(q.gradf(y), l * (D @ (D.T @ (l * y))) - 1) <= 1e-12
    assert np.array_equal(fa.Quadratic(Q).gradf(rng.rand(len(l), 3)).shape, (len(l), 3))


def test_quadratic_refuses_what_is_not_a_symmetric_float64_square():
    Q = np.arange(9.0).reshape(3, 3)
    with pytest.raises(ValueError, match=r"symmetric.*Q\[0,1\] = 1\.0 but Q\[1,0\] = 3\.0"):
        fa.Quadratic(Q)
    with pytest.raises(ValueError, match="square"):
        fa.Quadratic(np.zeros((3, 4)))
    with pytest.raises(ValueError, match="float64"):
        fa.Quadratic(np.eye(3, dtype=np.float32))
    tiny = np.eye(3)
    tiny[0, 2] = np.nextafter(0.0, 1.0)
    with pytest.raises(ValueError, match=r"Q\[0,2\]"):
        fa.Quadratic(tiny)
    assert fa.Quadratic(np.eye(3)).c is None


def test_rowball_is_the_reference_expression_bit_for_bit():
    """examples/max_norm.py:53-59; a zero row stays zero."""
    rng = np.random.RandomState(5)
    for mu in (1.0, 0.3):
        X = rng.randn(40, 7) * rng.choice([0.05, 1.0, 30.0], size=(40, 1))
        X[3] = 0.0
        norms = la.norm(X, axis=1)
        scale = np.maximum(norms, mu) + (norms == 0)
        want = mu * X / scale[:, np.newaxis]
        tag = fa.RowBall(mu)
        got = tag.prox(X, 0.37)
        assert np.array_equal(got, want) and np.array_equal(got, tag(X, 99.0)) and not got[3].any()
        assert la.norm(got, axis=1).max() <= mu * (1 + 1e-15) and tag.g(X) == 0 and tag.g_from_sums(3.0, 2.0) == 0
        inside = norms <= mu
        assert np.array_equal(got[inside], (mu * X / mu)[inside])
    assert fa.RowBall(2.0).kind == hip.PROX_ROWBALL == 8 and not fa.RowBall(2.0).step_scaled


# ---- recognition ---------------------------------------------------------------------------------------------------------------------------------
def test_recognition_names_what_the_device_does_not_serve():
    Q = np.eye(4)
    q, other = fa.Quadratic(Q), fa.Quadratic(Q)
    box, rb, gs = fa.Box(0, 1), fa.RowBall(1.0), fa.GroupShrink(1.0)
    why = lambda *a: solver._unrecognised(*a)
    x1, x2 = np.zeros(4), np.zeros((4, 3))
    assert why(None, None, q.f, q.gradf, box.g, box.prox, x1) is None
    assert why(None, None, q.f, q.gradf, None, None, x2) is None
    assert why(None, None, q.f, q.gradf, rb.g, rb.prox, x2) is None and why(None, None, q.f, q.gradf, gs.g, gs.prox, x2) is None
    assert "A must be None with a quadratic loss" in why(Q, None, q.f, q.gradf, box.g, box.prox, x1)
    assert "A must be None with a quadratic loss" in why(None, Q, q.f, q.gradf, box.g, box.prox, x1)
    assert "one losses.Quadratic" in why(None, None, q.f, other.gradf, box.g, box.prox, x1)
    assert "one losses.Quadratic" in why(None, None, q.f, (lambda x: x), box.g, box.prox, x1)
    assert "c must have x0's shape" in why(None, None, *(lambda t: (t.f, t.gradf))(fa.Quadratic(Q, np.zeros(4))), box.g, box.prox, x2)
    assert "at most 16 columns" in why(None, None, q.f, q.gradf, box.g, box.prox, np.zeros((4, 17)))
    assert "x0 has shape (5,)" in why(None, None, q.f, q.gradf, box.g, box.prox, np.zeros(5))
    for tag in (rb, gs):
        assert "RowBall and GroupShrink need a 2-D x0" in why(None, None, q.f, q.gradf, tag.g, tag.prox, x1)
    for tag in (fa.LinfProx(1.0), fa.L1Ball(1.0), fa.TVDualBall()):
        assert "LinfProx, L1Ball and TVDualBall have no quadratic form" in why(None, None, q.f, q.gradf, tag.g, tag.prox, x1)
    assert "one proximal.* tag" in why(None, None, q.f, q.gradf, (lambda x: 0), box.prox, x1)
    # RowBall is served with a quadratic loss only; a closure loss with A = None stays on the host loop
    ls = fa.LeastSquares(np.zeros(4))
    assert "quadratic loss only" in why(np.eye(4), None, ls.f, ls.gradf, rb.g, rb.prox, np.zeros((4, 2)))
    assert "not device-resident" in why(None, None, (lambda x: 0.0), (lambda x: x), box.g, box.prox, x1)
    with pytest.raises(TypeError, match="A must be None"):
        fa.fasta(Q, None, q.f, q.gradf, box.g, box.prox, x1, backend="hip", verbose=False)
    with pytest.raises(ValueError, match="quadratic loss only"):
        fa.proximal.device_prox(rb, x2, 1.0)


def test_no_gpu_is_an_error_not_a_fallback():
    try:
        n = hip.device_count()
    except hip.HipError:
        n = 0
    q, box = fa.Quadratic(np.eye(3), -np.ones(3)), fa.Box(0, 0.5)
    if n == 0:
        for form in ((None, None), (None,)):
            with pytest.raises(hip.HipError):
                fa.fasta(*form, q.f, q.gradf, box.g, box.prox, np.zeros(3), verbose=False)
    else:
        c = fa.fasta(None, None, q.f, q.gradf, box.g, box.prox, np.zeros(3), verbose=False)
        assert np.allclose(c.solution, 0.5)


def test_the_map_is_the_identity_on_host_arrays_and_lazy():
    q = fa.Quadratic(np.eye(5))
    op = fa.QuadraticMap(q, (5, 3))
    X = np.arange(15.0).reshape(5, 3)
    assert op(X) is X and op.H(X) is X and op._ctx is None and op.shape == (5, 5) and op.rhs == 3 and fa.QuadraticMap(q, (5,)).rhs == 1
    for bad in ((4,), (5, 17), (5, 0), (5, 2, 2)):
        with pytest.raises(ValueError):
            fa.QuadraticMap(q, bad)
    with pytest.raises(ValueError, match="linear term"):
        fa.QuadraticMap(fa.Quadratic(np.eye(5), np.zeros(5)), (5, 3))


# ---- geometry --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", QC.cases(), ids=QC.case_id)
def test_every_gpu_case_reaches_the_path_it_claims(case):
    """fh_quad_shape_for -- the one rule both launchers call -- under the case's tuning: the instantiation, the trips, the live lanes of the
    last trip and the (un)even passes are what the case's name says."""
    sh = hip.quad_shape(case.n, case.L, grid_cap=case.cap, nt_loads=case.nt)
    assert sh == QC.expected_shape(case)
    trips, trips16, live, uneven = QC.claimed_path(case)
    assert sh.ntrip == (trips16 if case.LB == 16 else trips) and sh.last_live == live
    assert (sh.pass_max != sh.pass_min) == uneven and (sh.CH, sh.R) == QC.MC_FOR_EACH[sh.LB] and sh.LB == QC.lb_of(case.L)
    if uneven:
        assert sh.fwd_grid == case.cap in (3, 4, 5) and sh.nrg % sh.fwd_grid != 0 and sh.pass_max >= 2
    lanes = QC.FH_WG * sh.CH // sh.LB
    assert (sh.ntrip - 1) * lanes < QC.round_up(case.n, 16) // 2 <= sh.ntrip * lanes


def test_the_cases_cover_every_instantiation_and_every_column_count_of_the_issue():
    seen = {(c.n, c.LB, c.L, c.nt) for c in QC.cases()}
    for LB in QC.ALL_LB:
        for L in QC.columns_of(LB):
            assert {(QC.N_WIDE, LB, L, 0), (QC.N_WIDE, LB, L, 1)} <= seen
        assert {(QC.N_NARROW, LB, LB, 0), (QC.N_NARROW, LB, LB - 1, 1)} <= seen and any(c.n == QC.N_CONTROL and c.LB == LB and not c.cap for c in QC.cases())
    assert QC.columns_of(2) == [2, 1] and QC.columns_of(16) == [16, 15, 9]
    for LB in QC.ALL_LB:
        assert {c.kind for c in QC.cases() if c.LB == LB} == set(QC.PROX_KINDS)
    assert {c.n for c in QC.cases()} == {1030, 24, 200, 1, 17}


def test_geometry_rule_refuses_what_no_kernel_serves():
    import ctypes as C
    lib = hip.load_library()
    out = (C.c_uint32 * hip.QUAD_SHAPE_LEN)()
    for n, L, cap, nt, text in ((0, 1, 0, -1, "dimension"), (5, 0, 0, -1, "1 to 16 columns"), (5, 17, 0, -1, "1 to 16 columns"),
                                (5, 1, -1, -1, "FWD_GRID_CAP"), (5, 1, 0, 2, "nt_loads")):
        assert lib.fh_quad_shape_for(n, L, cap, nt, out) == hip.E_ARG and text in lib.fh_last_error().decode()
    assert hip.quad_shape(16384, 10).NT == 1 and hip.quad_shape(4096, 10).NT == 0       # 2 GiB streams, 128 MiB stays in the last-level cache
    assert hip.quad_shape(16384, 1).fwd_grid == 512


# ---- exactness of the exact inputs ------------------------------------------------------------------------------------------------------------------
UNIT = {"init": 2.0 ** -4, "fwd": 2.0 ** -6, "adj": 2.0 ** -6, "adja": 2.0 ** -10}      # granularity of a block's terms (the CPU tier checks it)


@pytest.mark.parametrize("n,L,kind", sorted({(c.n, c.L, c.kind) for c in QC.cases()}))
def test_the_exact_step_is_exact(n, L, kind):
    """float64 == longdouble == integer arithmetic for every matrix product and every sum of the model, and every sum of magnitudes stays
    below 2^53 units: the order of summation cannot matter, so the kernels are compared with ==."""
    Q, c, X0 = QC.exact_inputs(n, L)
    assert np.array_equal(Q, Q.T) and set(np.unique(Q)) <= {-1.0, 0.0, 1.0} and (n < 100 or 0.7 < np.mean(Q == 0) < 0.8)
    assert np.array_equal(2 * c, np.round(2 * c)) and np.array_equal(2 * X0, np.round(2 * X0))
    tag, terms = QC.prox_tag(kind), {}
    a = QC.model_step(Q, c, X0, tag, terms=terms)
    b = QC.model_step(Q, c, X0, tag, dtype=np.longdouble)
    for name in QC.MATRICES:
        assert np.array_equal(a[name], b[name].astype(np.float64)) and np.array_equal(a[name].astype(np.longdouble), b[name]), name
    Qi = Q.astype(np.int64)
    for product, operand, scale in ((a["G0"] - c, X0, 2), (a["W"], a["XPROX"], 4)):
        Vi = operand * scale
        assert np.array_equal(Vi, np.round(Vi)) and np.array_equal((Qi @ Vi.astype(np.int64)) / scale, product)
        assert float(np.max(np.abs(Qi) @ np.abs(Vi))) < 2.0 ** 53
    for blk in QC.BLOCKS:
        for slot, value in a[blk].items():
            assert value == float(b[blk][slot]), (blk, slot)
            t = terms[(blk, slot)] / UNIT[blk]
            assert np.array_equal(t, np.round(t)) and float(np.sum(np.abs(t))) < 2.0 ** 53, (blk, slot)
            if slot not in (hip.S_GMAX, hip.S_GMAX_ADJ):
                assert int(np.sum(t.astype(np.int64))) * UNIT[blk] == value, (blk, slot)
    assert a["fwd"][hip.S_RDOT] == -a["fwd"][hip.S_DX2]                     # x_accel0 = x0 right after fh_init
    if kind != "none" and n >= 17:
        assert not np.array_equal(a["XPROX"], a["XHAT"])                  # the prox does something at this scale


def test_the_rownorm_problems_exercise_both_branches():
    for n, L, kind, nt in QC.rownorm_cases():
        Q, c, X0, tau, tag = QC.rownorm_problem(n, L, kind)
        norms = la.norm(X0 - tau * (Q @ X0 + c), axis=1)
        thr = tau * tag.mu if kind == "group" else tag.mu
        assert 0.1 < np.mean(norms <= thr) < 0.9 or n < 20, (n, L, kind)
    assert {r[2] for r in QC.rownorm_cases()} == {"group", "rowball"} and {QC.lb_of(r[1]) for r in QC.rownorm_cases()} == set(QC.ALL_LB)


# ---- the examples on the host loop --------------------------------------------------------------------------------------------------------------------
@pytest.mark.filterwarnings("ignore::RuntimeWarning")
def test_examples_run_the_reference_closures_on_the_host():
    from fasta_python_amd.examples.max_norm import MaxNormProblem
    from fasta_python_amd.examples.svm import SVMProblem
    opts = dict(tolerance=1e-5, evaluate_objective=True, max_iters=60)
    problem, X0 = MaxNormProblem.construct(N=40, K=3, seed=11, backend="numpy")
    np.random.seed(1)
    _, c = problem.solve(X0, opts)
    q, rb = fa.Quadratic(problem.S + problem.S.T), fa.RowBall(problem.mu)
    np.random.seed(1)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        t = fa.fasta(None, None, q.f, q.gradf, rb.g, rb.prox, X0, backend="numpy", verbose=False, **opts)
    assert c.iteration_count == t.iteration_count and np.allclose(c.solution, t.solution, rtol=1e-9, atol=1e-12)
    assert la.norm(c.solution, axis=1).max() <= problem.mu * (1 + 1e-12)
    # the RNG order of construct() is the reference's: points' noise first, then X0 (examples/max_norm.py:90-93)
    np.random.seed(11)
    noise = np.random.randn(40, 2)
    assert np.array_equal(X0, np.random.randn(40, 3) / np.sqrt(3) / 10) and noise.shape == (40, 2)
    svm, y0 = SVMProblem.construct(M=30, N=4, C=0.1, seed=12, backend="numpy")
    np.random.seed(1)
    w, c = svm.solve(y0, opts)
    q, box = fa.Quadratic(svm.Q, -np.ones(30)), fa.Box(0.0, 0.1)
    np.random.seed(1)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        t = fa.fasta(None, None, q.f, q.gradf, box.g, box.prox, y0, backend="numpy", verbose=False, **opts)
    assert np.allclose(c.solution, t.solution, rtol=1e-6, atol=1e-9) and np.array_equal(w, svm.D.T @ (svm.l * c.solution))
    rbf, y0 = SVMProblem.construct(M=30, N=4, C=0.1, kernel="rbf", seed=12, backend="numpy")
    assert np.array_equal(rbf.Q, rbf.Q.T) and np.all(np.diag(rbf.Q) == 1.0)
    _, c = rbf.solve(y0, opts)
    assert 0.0 <= c.solution.min() and c.solution.max() <= 0.1

"""CPU tier of the identity operator with an elementwise loss and the nuclear-norm prox (fh_set_identity, FH_PROX_NUCLEAR, csrc/fh_nuclear.h;
linalg.IdentityMap, proximal.NuclearShrink): the fixtures tests/golden/nuclear/*.npz were captured from the reference core
(scripts/make_nuclear_golden.py) with the tags' closures and the identity operator; the NumPy oracle and `fasta(None, None, ...,
backend="numpy")` must reproduce them bit for bit, the closures must be the reference example's own, operand recognition must serve what the
device serves and name what it does not, the exported launch geometry must hold what every GPU-tier case claims of it, the NumPy restatement
of the block-Jacobi rule must stay inside a quarter of the device's tolerance, the exact inputs must be exact, and nothing may fall back when
there is no GPU.  No GPU."""
import os
import warnings

import numpy as np
import pytest
from numpy import linalg as la

import fasta_python_amd as fa
from fasta_python_amd import hip
from fasta_python_amd.solver import _unrecognised as why
from oracle import fasta_np as fo
from tests import nuclear_cases as NC


def assert_same_run(c, z):
    assert c.iteration_count == int(z["iteration_count"]) and c.backtracks == int(z["backtracks"])
    for field in NC.HISTORIES:
        assert np.array_equal(getattr(c, field), z[field], equal_nan=True), field
    assert np.array_equal(c.solution, z["solution"])


# ---- the fixture set ---------------------------------------------------------------------------------------------------------------------------
def test_the_fixture_set_is_the_one_the_script_describes():
    names = [row[0] for row in NC.capture_script().case_table()]
    assert sorted(names) == NC.FIXTURES == NC.EXPECTED
    assert all(os.path.getsize(os.path.join(NC.NUCLEAR, n + ".npz")) < 100 << 10 for n in NC.FIXTURES)


def test_the_fixtures_cover_the_modes_both_orientations_both_losses_and_backtracks():
    seen = set()
    for name in NC.EXPECTED:
        meta, z, d = NC.load(name)
        o = meta["options"]
        assert o["evaluate_objective"] and o["L"] > 0 and o["tau0"] > 0 and z["solution"].shape == d["x0"].shape == d["B"].shape, name
        seen.add((meta["kind"], "adaptive" if o["adaptive"] else "accelerated" if o["accelerate"] else "plain", d["B"].shape[0] > d["B"].shape[1]))
        if meta["kind"] != "shrink":                     # mu leaves a rank strictly between 0 and p
            assert 0 < meta["solution_rank"] < min(d["B"].shape), name
            s = la.svd(z["solution"], compute_uv=False)
            assert int(np.sum(s > 1e-3 * s[0])) == meta["solution_rank"], name
        if meta["kind"] != "lsq":
            assert set(np.unique(d["B"])) <= {-1.0, 1.0}, name
    assert {("lmc", "adaptive", False), ("lmc", "accelerated", False), ("lmc", "plain", False), ("lmc", "adaptive", True), ("lsq", "plain", False),
            ("shrink", "adaptive", True)} <= seen
    assert int(NC.load("lmc_12x20_backtracks")[1]["backtracks"]) >= 2


@pytest.mark.parametrize("name", NC.EXPECTED)
def test_twin_parting_iteration_is_recomputed(name):
    """The basis for what the device is held to: the oracle and a twin of itself with permuted rows and columns (same L, same tau0) agree on
    every step size up to the stored iteration; a prefix must have at least 30 iterations or be the whole run."""
    meta, z, d = NC.load(name)
    assert NC.capture_script().twin_divergence(meta["kind"], d, meta["options"]) == meta["twin_divergence"]
    k, whole = NC.compared_prefix(meta, z)
    assert whole or k >= NC.MIN_PREFIX


# ---- bit-for-bit reproduction ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NC.EXPECTED)
def test_oracle_reproduces_the_reference_run(name):
    meta, z, d = NC.load(name)
    assert_same_run(NC.capture_script().run_oracle(meta["kind"], d, meta["options"]), z)


@pytest.mark.parametrize("name", NC.EXPECTED)
def test_host_loop_reproduces_the_reference_run(name):
    meta, z, d = NC.load(name)
    ms = NC.capture_script()
    f, gradf, g, proxg, x0 = ms.operands(fa, meta["kind"], d)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        c = fa.fasta(None, None, f, gradf, g, proxg, x0, backend="numpy", verbose=False, **ms.resolve(meta["options"], fa.stopping))
    assert_same_run(c, z)


def test_least_squares_limit_is_the_closed_form():
    meta, z, d = NC.load("lsq_10x14_plain")
    want = fa.proximal.project_Lnuc_ball(d["B"], float(d["mu"]))       # argmin mu ||X||_* + .5 ||X - B||^2
    assert la.norm(z["solution"] - want) <= 1e-3 * la.norm(want)


def test_the_tag_is_the_examples_closures():
    rng = np.random.RandomState(3)
    for shape in ((6, 9), (9, 6), (5, 5)):
        X, mu, t = rng.randn(*shape), 0.7, 0.3
        reg = fa.NuclearShrink(mu)
        U, s, V = la.svd(X)
        S = np.zeros(X.shape)
        S[:len(s), :len(s)] = np.diag(np.sign(s) * np.maximum(np.abs(s) - t * mu, 0))
        assert np.array_equal(reg.prox(X, t), U @ S @ V) and np.array_equal(reg(X, t), U @ S @ V)
        assert reg.g(X) == mu * la.norm(np.diag(la.svd(X)[1]), 1)
        # (the example's g: the induced 1-norm of diag(s) is the LARGEST singular value; the device's sums are mapped to the same thing)
        assert reg.g(X) == mu * s[0] and reg.g_from_sums(3.0, 9.0) == mu * 9.0 and reg.nuclear_norm_from_sums(3.0, 9.0) == 3.0 and reg.kind == hip.PROX_NUCLEAR == 10
        assert la.norm(reg.prox(X, t) - fa.proximal.project_Lnuc_ball(X, t * mu)) <= 1e-13 * la.norm(X)


# ---- recognition ---------------------------------------------------------------------------------------------------------------------------------
def _operands(shape=(4, 6)):
    B = np.sign(np.random.RandomState(1).randn(*shape))
    return fa.LogisticLoss(B), fa.LeastSquares(B), np.zeros(shape)


def test_served_operands_are_recognised():
    ll, ls, X0 = _operands()
    for loss in (ll, ls):
        for reg in (fa.NuclearShrink(1.0), fa.Shrink(0.1), fa.NonNeg(), fa.Box(-1, 1)):
            assert why(None, None, loss.f, loss.gradf, reg.g, reg.prox, X0) is None
            assert why(fa.IdentityMap(X0.shape), None, loss.f, loss.gradf, reg.g, reg.prox, X0) is None
        assert why(None, None, loss.f, loss.gradf, None, None, X0) is None
    A, loss, prox = fa.solver._recognise(None, None, ll.f, ll.gradf, None, None, X0)
    assert isinstance(A, fa.IdentityMap) and A._ctx is None and loss is ll and type(prox) is fa.NoProx
    op = fa.IdentityMap((4, 6))
    assert fa.solver._recognise(op, None, ll.f, ll.gradf, None, None, X0)[0] is op


def test_refusals_name_what_is_not_served():
    ll, ls, X0 = _operands()
    nuc, box = fa.NuclearShrink(1.0), fa.Box(0, 1)
    assert "not device-resident" in why(None, None, (lambda x: 0.0), (lambda x: x), box.g, box.prox, X0)
    assert "not device-resident" in why(None, None, ll.f, ls.gradf, box.g, box.prox, X0)               # two different tags
    assert "not device-resident" in why(None, np.eye(4), ll.f, ll.gradf, box.g, box.prox, X0)          # an At without an A
    assert "x0 must be 2-D" in why(None, None, ll.f, ll.gradf, nuc.g, nuc.prox, np.zeros(24))
    assert "B must have x0's shape" in why(None, None, ll.f, ll.gradf, nuc.g, nuc.prox, np.zeros((6, 4)))
    assert "IdentityMap was built for" in why(fa.IdentityMap((6, 4)), None, ll.f, ll.gradf, nuc.g, nuc.prox, X0)
    for reg in (fa.LinfProx(1.0), fa.L1Ball(1.0), fa.GroupShrink(1.0), fa.RowBall(1.0), fa.TVDualBall()):
        assert "not implemented for the identity operator" in why(None, None, ll.f, ll.gradf, reg.g, reg.prox, X0)
    assert "one proximal.* tag object" in why(None, None, ll.f, ll.gradf, (lambda x: 0.0), nuc.prox, X0)
    # NuclearShrink over any other operator
    b = fa.LeastSquares(np.zeros(3))
    assert "identity operator only" in why(np.eye(3), None, b.f, b.gradf, nuc.g, nuc.prox, np.zeros(3))
    q = fa.Quadratic(np.eye(3))
    assert "identity operator only" in why(None, None, q.f, q.gradf, nuc.g, nuc.prox, np.zeros((3, 2)))
    # the size limits
    wide = fa.LogisticLoss(np.ones((1025, 1026)))
    assert "min(M, N) <= 1024" in why(None, None, wide.f, wide.gradf, nuc.g, nuc.prox, np.zeros((1025, 1026)))
    assert why(None, None, wide.f, wide.gradf, box.g, box.prox, np.zeros((1025, 1026))) is None
    with pytest.raises(ValueError, match="2\\^26"):
        fa.IdentityMap((1 << 13, (1 << 13) + 1))
    for bad in ((4,), (4, 0), (2, 3, 4)):
        with pytest.raises(ValueError):
            fa.IdentityMap(bad)


def test_one_pass_and_device_loop_are_refused():
    ll, _, X0 = _operands()
    op = fa.IdentityMap(X0.shape)
    with pytest.raises(ValueError, match="no one-pass kernel"):
        fa.FBSolver(op, ll, fa.NuclearShrink(1.0), X0, fused=True)
    for kw in (dict(driver="device"), dict(device_iters=4)):
        with pytest.raises(ValueError, match="no device-side loop"):
            fa.FBSolver(op, ll, fa.NuclearShrink(1.0), X0, **kw)
    assert op._ctx is None


def test_the_map_is_the_identity_on_host_arrays_and_lazy():
    op = fa.IdentityMap((5, 3))
    X = np.arange(15.0).reshape(5, 3)
    assert op(X) is X and op.H(X) is X and op._ctx is None and op.shape == (15, 15) and op.Vshape == op.Wshape == (5, 3)


def test_no_gpu_is_an_error_not_a_fallback():
    try:
        n = hip.device_count()
    except hip.HipError:
        n = 0
    ll, _, X0 = _operands()
    reg = fa.NuclearShrink(0.5)
    if n == 0:
        for form in ((None, None), (None,)):
            with pytest.raises(hip.HipError):
                fa.fasta(*form, ll.f, ll.gradf, reg.g, reg.prox, X0, verbose=False)
        with pytest.raises(hip.HipError):
            fa.proximal.device_prox(reg, np.ones((3, 4)), 1.0)
    else:
        c = fa.fasta(None, None, ll.f, ll.gradf, reg.g, reg.prox, X0, verbose=False)
        assert c.solution.shape == X0.shape and c.library_steps == c.iteration_count


# ---- the launch geometry -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", NC.CASES, ids=lambda c: c.name)
def test_shape_rule_holds_what_the_gpu_cases_claim(case):
    assert hip.nuclear_shape(case.M, case.N, case.Bk)._asdict() == NC.shape_of(case.M, case.N, case.Bk)


def test_shape_rule_reaches_every_path_the_cases_are_named_for():
    by = {c.name: hip.nuclear_shape(c.M, c.N, c.Bk) for c in NC.CASES}
    sh = by["three_blocks_bye"]
    assert (sh.nb, sh.steps_per_sweep, sh.wgs_per_step, sh.P) == (3, 3, 2, 6) and len(NC.step_pairs(3, 0)) == 1       # a bye in every step
    assert (by["self_pair"].nb, by["self_pair"].steps_per_sweep, by["self_pair"].wgs_per_step) == (1, 1, 1)
    assert (by["one_pair"].nb, by["one_pair"].steps_per_sweep, by["one_pair"].wgs_per_step) == (2, 1, 1)
    sh = by["padding_odd_ragged"]
    assert sh.P == 36 > sh.p == 33 and sh.nb == 9 and sh.nb % 2 == 1 and sh.q % sh.column_chunk != 0
    assert by["transposed"].transposed == 1 and by["transposed"].p == 16 and by["transposed"].q == 40
    assert by["p1_row"].p == by["p1_col"].p == 1 and by["p1_col"].transposed == 1
    assert by["several_chunks"].chunks_per_row == 3
    assert hip.nuclear_shape(200, 1000, 8).steps_per_sweep == 25 and hip.nuclear_shape(200, 1000, 1).steps_per_sweep == 199
    assert hip.nuclear_shape(200, 1000) == hip.nuclear_shape(200, 1000, NC.AUTO_BLOCK_ROWS)            # 0 = auto
    for Bk in (1, 2, 8):                                  # the exact input, both orientations
        for M, N in ((5, 16), (16, 5)):
            assert hip.nuclear_shape(M, N, Bk)._asdict() == NC.shape_of(M, N, Bk)
    assert hip.nuclear_shape(200, 1000).lds_bytes < 64 << 10


def test_every_schedule_meets_every_pair_of_blocks_once_per_sweep():
    for nb in (2, 3, 4, 5, 8, 9, 25, 128):
        steps = 1 if nb == 1 else nb + (nb & 1) - 1
        seen = []
        for r in range(steps):
            pairs = NC.step_pairs(nb, r)
            blocks = [b for pr in pairs for b in pr]
            assert len(blocks) == len(set(blocks))       # disjoint within a step
            seen += pairs
        assert sorted(seen) == [(a, b) for a in range(nb) for b in range(a + 1, nb)]
    assert NC.step_pairs(1, 0) == [(0, -1)]


def test_limits_are_refused_with_a_sentence():
    for args, text in (((0, 5, 0), "non-empty"), ((5, 0, 0), "non-empty"), ((1025, 1025, 0), "min\\(M, N\\) <= 1024"),
                       ((1 << 13, (1 << 13) + 1, 0), "2\\^26"), ((5, 7, 3), "NUC_BLOCK_ROWS")):
        with pytest.raises(hip.HipError, match=text):
            hip.nuclear_shape(*args)
    assert hip.nuclear_shape(1024, 65536).p == 1024


# ---- the restatement and the exact inputs ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", NC.CASES, ids=lambda c: c.name)
def test_restatement_stays_inside_a_quarter_of_the_tolerance(case):
    X, thr = NC.case_input(case)
    out, info = NC.model_svt(X, thr, case.Bk)
    want = fa.proximal.project_Lnuc_ball(X, thr)
    assert info.converged and info.sweeps < NC.MAX_SWEEPS
    assert la.norm(out - want) <= NC.tolerance(X, NC.MODEL_FACTOR)
    # (Weyl: every singular value moves by at most the perturbation's norm, which the bound above stands for; the sum has at most p terms)
    assert abs(info.gsum - np.sum(np.maximum(la.svd(X, compute_uv=False) - thr, 0))) <= min(X.shape) * NC.tolerance(X, NC.MODEL_FACTOR)
    if case.kind in ("zero", "below"):
        assert not out.any() and info.rank == 0


def test_exact_inputs_are_exact():
    X, want = NC.exact_input()
    assert np.array_equal(X @ X.T, np.diag(np.square(NC.EXACT_SIGMA)))                 # mutually orthogonal rows, sigma = 16, 4, 2, 8, 0
    for Bk in (1, 2, 8):
        for T in (False, True):
            out, info = NC.model_svt(X.T.copy() if T else X, NC.EXACT_THR, Bk)
            assert np.array_equal(out, want.T if T else want)
            assert (info.sweeps, info.rotations, info.rank, info.gsum) == (1, 0, NC.EXACT_RANK, NC.EXACT_GSUM)

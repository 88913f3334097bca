"""GPU tests of the quadratic smooth term f(X) = .5 <X, Q X> + <c, X> (fh_set_quadratic; csrc/fh_quad.h: k_qd_prologue / k_qd_fwd / k_qd_grad),
every one through the C ABI.

Shapes, column counts and tuning are those of tests/quad_cases.py (the smallest at which each loop of k_qd_fwd exists: several trips with a
masked last one, a single trip of clamped lanes, unequal numbers of passes, every LB with and without padding columns, both load policies);
every test first asks the library what it is about to launch (fh_quad_shape) and compares that with what the case claims.  The exact step runs
on operands for which every product and every sum is exactly representable whatever the order of summation (tests/test_quad_cpu.py proves it
without a device): np.array_equal / ==, no tolerance.  GroupShrink and RowBall (a square root and a division per row) are compared against
an np.longdouble model at the tolerances the project holds those quantities to (tests/quad_cases.py says where f, which
unlike a sum of squares may cancel, needs the summation bound as well)."""
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

import fasta_python_amd as fa
from fasta_python_amd import hip, proximal
from fasta_python_amd import stopping as fstop
from tests import gpu_util as G
from tests import quad_cases as QC

pytestmark = pytest.mark.gpu
VECS = {"G0": hip.VEC_G0, "XHAT": hip.VEC_XHAT, "XPROX": hip.VEC_XPROX, "W": hip.VEC_Z, "G1": hip.VEC_G1, "X1": hip.VEC_X1}
EPS = float(np.finfo(np.float64).eps)


@pytest.fixture(autouse=True)
def no_scratch_contexts_left_behind():
    yield
    proximal.release_scratch()


def first_bad(name, got, want):
    bad = np.argwhere(got != want)
    if bad.size:
        i = tuple(bad[0])
        return f"{name}: {len(bad)} wrong entries, first at {bad[0]}: {got[i]!r} != {want[i]!r}"
    return None


def padding_is_zero(c, which, n, L, scratch=hip.VEC_T0):
    """fh_diff_norm adds up the WHOLE device buffers -- padding columns and rows -- so against a buffer that holds the same logical entries and
    untouched (zero) padding the norm is exactly zero only if the padding of `which` is.  scratch = VEC_B for the m-side W (overwrites c)."""
    c.set_vector(scratch, c.get_vector(which, n * L))
    return c.diff_norm(which, scratch) == 0.0


def context(Q, cvec, L, tuning):
    c = hip.HipContext(0)
    for key, value in tuning.items():
        c.set_tuning(key, value)
    c.set_quadratic(Q, cvec, L)
    return c


def run_step(c, n, L, X0, tag, tau, coef):
    """init -> fwd -> adj -> fwd_adj -> adj(accel): what the device returned, keyed as tests/quad_cases.py:model_step keys its model."""
    mat = lambda name: c.get_vector(VECS[name], n * L).reshape(n, L)
    got = {}
    c.set_prox(tag.kind, tag.mu, tag.lo, tag.hi)
    c.set_vector(hip.VEC_X0, X0)
    got["init"] = c.init()
    got["G0"] = mat("G0")
    got["fwd"] = c.fwd(tau)
    got["XHAT"], got["XPROX"], got["W"] = mat("XHAT"), mat("XPROX"), mat("W")
    got["adj"] = c.adj(tau)
    got["G1"] = mat("G1")
    got["pair"] = c.fwd_adj(tau)
    got["G1_pair"], got["W_pair"] = mat("G1"), mat("W")
    got["adja"] = c.adj(tau, accel=True, coef=coef)
    got["G1A"], got["X1"] = mat("G1"), mat("X1")
    return got


def assert_shape(c, case):
    sh = c.quad_shape()
    print(f"\n{QC.case_id(case)}: {sh}", end="")
    assert sh == QC.expected_shape(case) == hip.quad_shape(case.n, case.L, grid_cap=case.cap, nt_loads=case.nt), (sh, QC.expected_shape(case))
    trips, trips16, live, uneven = QC.claimed_path(case)
    assert sh.ntrip == (trips16 if case.LB == 16 else trips) and sh.last_live == live and (sh.pass_max != sh.pass_min) == uneven
    return sh


# ---- apply -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", QC.cases(), ids=QC.case_id)
def test_apply_matches_numpy_and_ignores_the_adjoint_flag(case):
    """out = Q in on unit-scale data within 1e-12 * (|Q| |V|), and on the exact operands bit for bit; both adjoint flags give the same bits."""
    rng = np.random.RandomState(11 + case.n + case.L)
    U = np.triu(rng.randn(case.n, case.n))
    Q = U + np.triu(U, 1).T
    V = rng.randn(case.n, case.L)
    c = context(Q, None, case.L, QC.tuning_of(case))
    try:
        assert_shape(c, case)
        assert c.shape() == (case.n, case.n) and c.rhs == case.L
        a, b = c.apply(V).reshape(V.shape), c.apply(V, adjoint=True).reshape(V.shape)
        assert np.array_equal(a, b)
        assert np.all(np.abs(a - Q @ V) <= 1e-12 * (np.abs(Q) @ np.abs(V)) + 1e-300)
        Qe, _, X0 = QC.exact_inputs(case.n, case.L)
        c.set_quadratic(Qe, None, case.L)
        msg = first_bad("Q X0", c.apply(X0).reshape(X0.shape), Qe @ X0)
        assert msg is None, msg
        assert padding_is_zero(c, hip.VEC_T3, case.n, case.L)
    finally:
        c.close()


# ---- one exact step ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", QC.cases(), ids=QC.case_id)
def test_one_step_is_exact(case):
    """init -> fwd -> adj -> fwd_adj -> adj(accel, coef = 1/4) with tau = 1/2: every matrix, every scalar and the padding, bit for bit."""
    Q, cvec, X0 = QC.exact_inputs(case.n, case.L)
    want = QC.exact_model(case.n, case.L, case.kind)
    c = context(Q, cvec, case.L, QC.tuning_of(case))
    try:
        assert_shape(c, case)
        got = run_step(c, case.n, case.L, X0, QC.prox_tag(case.kind), QC.TAU, QC.COEF)
        for name in QC.MATRICES:
            msg = first_bad(name, got[name], want[name])
            assert msg is None, msg
        for block in QC.BLOCKS:
            for slot, v in want[block].items():
                assert got[block][slot] == v, f"{block} scalar {slot}: {got[block][slot]!r} != {v!r}"
        # the elementwise launch leaves the forward half of the block alone; fh_fwd_adj is both launches under one synchronisation
        assert np.array_equal(got["adj"][:hip.S_DXDG], got["fwd"][:hip.S_DXDG])
        assert np.array_equal(got["pair"][:hip.S_ALPHA], np.concatenate([got["fwd"][:hip.S_DXDG], got["adj"][hip.S_DXDG:hip.S_ALPHA]]))
        assert np.array_equal(got["G1_pair"], want["G1"]) and np.array_equal(got["W_pair"], want["W"])
        for which in (hip.VEC_G0, hip.VEC_XHAT, hip.VEC_XPROX, hip.VEC_X1, hip.VEC_G1):
            assert padding_is_zero(c, which, case.n, case.L), which
        assert padding_is_zero(c, hip.VEC_Z, case.n, case.L, scratch=hip.VEC_B)        # (last: it overwrites c)
    finally:
        c.close()


def test_the_step_is_bitwise_repeatable_and_timed():
    case = next(k for k in QC.cases() if k.n == QC.N_WIDE and k.L == 10 - 1 and k.nt == 1)
    Q, cvec, X0 = QC.rownorm_problem(case.n, case.L, "rowball")[:3]
    runs = []
    for _ in range(2):
        c = context(Q, cvec, case.L, QC.tuning_of(case))
        try:
            c.timing_enable(True)
            got = run_step(c, case.n, case.L, X0, proximal.RowBall(0.5), 0.25, 0.25)
            assert c.timing_get(hip.K_FWD)[1] >= 3 and c.timing_get(hip.K_ADJ)[1] >= 3 and c.timing_get(hip.K_FUSED)[1] == 0
            runs.append(got)
        finally:
            c.close()
    for key in runs[0]:
        assert np.array_equal(runs[0][key], runs[1][key]), key


def assert_rownorm_step(got, want, terms, n, L, kind, tag):
    """what run_step returned against the np.longdouble model of a GroupShrink / RowBall step, at the tolerances of tests/quad_cases.py (shared with
    the stations of tests/carry_cases.py)"""
    for name in QC.MATRICES:
        rtol, atol = QC.ROWNORM_TOL[name]
        np.testing.assert_allclose(got[name], want[name].astype(np.float64), rtol=rtol, atol=atol, err_msg=name)
    worst = 0.0
    for block in QC.BLOCKS:
        for slot, v in want[block].items():
            rtol, atol = QC.scalar_tol(block, slot)
            if slot in (hip.S_FSQ, hip.S_FSQ_ADJ, hip.S_DXG0, hip.S_DXDG, hip.S_RDOT):
                # a signed sum: the bound of a summation of depth <= 64 on the magnitudes of its terms
                atol += 64 * EPS * float(np.sum(np.abs(terms[(block, slot)])))
            dev = abs(got[block][slot] - float(v))
            print(f"\n{kind} n={n} L={L} {block}[{slot}]: device {got[block][slot]!r}, model {float(v)!r}", end="")
            assert dev <= rtol * abs(float(v)) + atol, (block, slot, got[block][slot], float(v))
            worst = max(worst, dev / max(abs(float(v)), 1e-300))
    zero_rows = np.all(got["XPROX"] == 0, axis=1).mean()
    print(f"\n{kind} n={n} L={L}: worst relative deviation of a scalar {worst:.2e}; rows brought to zero {zero_rows:.2f}", end="")
    if kind == "rowball":
        assert np.linalg.norm(got["XPROX"], axis=1).max() <= tag.mu * (1 + 4 * EPS)


# ---- GroupShrink and RowBall -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,L,kind,nt", QC.rownorm_cases(), ids=lambda v: str(v))
def test_rownorm_step_matches_the_extended_precision_model(n, L, kind, nt):
    Q, cvec, X0, tau, tag = QC.rownorm_problem(n, L, kind)
    terms = {}
    want = QC.model_step(Q, cvec, X0, tag, tau=tau, coef=QC.COEF, dtype=np.longdouble, terms=terms)
    case = QC.Case(n, QC.lb_of(L), L, QC.uneven_cap(QC.round_up(n, 16) // QC.MC_FOR_EACH[QC.lb_of(L)][1]) if n == QC.N_WIDE else 0, nt, kind)
    c = context(Q, cvec, L, QC.tuning_of(case))
    try:
        assert c.quad_shape() == QC.expected_shape(case)
        got = run_step(c, n, L, X0, tag, tau, QC.COEF)
        assert_rownorm_step(got, want, terms, n, L, kind, tag)
        for which in (hip.VEC_XPROX, hip.VEC_X1, hip.VEC_G1):
            assert padding_is_zero(c, which, n, L), which
    finally:
        c.close()


def test_a_zero_row_stays_zero_under_both_row_kinds():
    n, L = 17, 3
    Q, cvec, X0 = QC.exact_inputs(n, L)
    X0, cvec = X0.copy(), cvec.copy()
    X0[5] = 0.0
    cvec[5] = 0.0
    Q = Q.copy()
    Q[5, :] = Q[:, 5] = 0.0                          # row 5 of the gradient is zero: xhat's row 5 is zero
    for tag in (proximal.RowBall(1.0), proximal.GroupShrink(1.0)):
        c = context(Q, cvec, L, {})
        try:
            got = run_step(c, n, L, X0, tag, 0.5, 0.25)
            assert not got["XHAT"][5].any() and not got["XPROX"][5].any() and np.isfinite(got["XPROX"]).all()
        finally:
            c.close()


# ---- elementwise kinds: the bits of the multi-column dense form ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 2, 3, 5, 8, 9, 16])
def test_elementwise_prox_outputs_are_those_of_the_multi_column_dense_form(L):
    n = 203
    rng = np.random.RandomState(40 + L)
    Q = np.eye(n)
    X0, G0 = rng.randn(n, L), rng.randn(n, L)
    tau = 0.37
    quad = context(Q, None, L, {})
    dense = fa.DenseMatrixMap(np.zeros((1, n)), rhs=L)
    try:
        dense.ctx.set_loss_lsq(np.zeros((1, L)))
        for kind in QC.PROX_KINDS:
            tag = {"shrink": proximal.Shrink(0.8)}.get(kind) or QC.prox_tag(kind)
            outs = []
            for c in (quad, dense.ctx):
                c.set_prox(tag.kind, tag.mu, tag.lo, tag.hi)
                c.set_vector(hip.VEC_X0, X0)
                c.set_vector(hip.VEC_G0, G0)
                s = c.fwd(tau)
                outs.append((c.get_vector(hip.VEC_XHAT, n * L), c.get_vector(hip.VEC_XPROX, n * L), s[hip.S_DXG0:hip.S_RDOT + 1]))
            for a, b in zip(*outs):
                assert np.array_equal(a, b), kind
            assert np.array_equal(outs[0][1].reshape(n, L), tag.prox(X0 - tau * G0, tau)), kind
    finally:
        quad.close()
        dense.close()


# ---- fixtures ------------------------------------------------------------------------------------------------------------------------------------------
def solve(meta, d, **extra):
    ms = QC.capture_script()
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
        meta, z, d = QC.load(name)
        k, whole = QC.compared_prefix(meta, z)
        extra = {} if whole else dict(max_iters=k, tolerance=0.0)
        _runs[name] = (solve(meta, d, driver="library", **extra), k, whole, extra)
    return _runs[name]


def assert_same_bits(a, b):
    assert a.iteration_count == b.iteration_count and a.backtracks == b.backtracks
    for f in QC.HISTORIES:
        assert np.array_equal(getattr(a, f), getattr(b, f), equal_nan=True), f
    assert np.array_equal(a.solution, b.solution)


@pytest.mark.parametrize("name", QC.EXPECTED)
def test_fixture_solves_on_the_device(name):
    meta, z, d = QC.load(name)
    lib, k, whole, extra = library_run(name)
    assert lib.library_steps == lib.iteration_count and lib.device_steps == 0
    print(f"\n{name}: device {lib.iteration_count} iterations / {lib.backtracks} backtracks, reference {int(z['iteration_count'])} / {int(z['backtracks'])}", end="")
    if whole:
        assert lib.iteration_count == int(z["iteration_count"]) and lib.backtracks == int(z["backtracks"])
    else:
        assert k >= QC.MIN_PREFIX and lib.iteration_count == k and lib.backtracks == meta["backtracks_at_divergence"]
    worst = G.compare_histories(lib, lambda f: z[f], k, rtol=1e-6, atol=1e-14)
    print(f"; {k} iterations compared, worst relative deviation of a history entry {worst:.2e}")
    if whole:
        np.testing.assert_allclose(lib.solution, z["solution"], rtol=1e-5, atol=1e-6 * float(np.max(np.abs(z["solution"]))))


@pytest.mark.parametrize("name", QC.EXPECTED)
def test_library_and_python_drivers_are_bit_identical_and_runs_repeat(name):
    meta, z, d = QC.load(name)
    lib, k, whole, extra = library_run(name)
    py = solve(meta, d, driver="python", **extra)
    assert py.library_steps == 0
    assert_same_bits(py, lib)
    assert_same_bits(solve(meta, d, driver="library", device_iters=7, **extra), lib)          # cut elsewhere, run again: the same bits


def test_the_six_argument_form_the_pair_policy_and_the_fallbacks_of_device_iters():
    meta, z, d = QC.load("svm_rbf_80_adaptive")
    ms = QC.capture_script()
    f, gradf, g, proxg, x0 = ms.operands(fa, meta["kind"], d)
    o = ms.resolve(meta["options"], fstop)
    lib = library_run("svm_rbf_80_adaptive")[0]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        six = fa.fasta(None, f, gradf, g, proxg, x0, verbose=False, **o)                          # operand types decide: the device loop
        dev = fa.fasta(None, None, f, gradf, g, proxg, x0, verbose=False, driver="device", **o)   # no device-side loop: the library's
        sep = fa.fasta(None, None, f, gradf, g, proxg, x0, verbose=False, fused=False, **o)       # fh_fwd / fh_adj instead of the pair
    for other in (six, dev, sep):
        assert_same_bits(other, lib)
    assert dev.device_steps == 0 and dev.library_steps == dev.iteration_count
    with pytest.raises(ValueError, match="fused=True"):
        fa.fasta(None, None, f, gradf, g, proxg, x0, verbose=False, fused=True, **o)


# ---- examples ------------------------------------------------------------------------------------------------------------------------------------------
def test_examples_agree_between_the_backends():
    from fasta_python_amd.examples.max_norm import MaxNormProblem
    from fasta_python_amd.examples.svm import SVMProblem
    """Three modes each, with L and tau0 given (the probes are random): the first 40 iterations -- a permuted twin of the adaptive SVM runs
    parts from the oracle after 54 to 57, of every other run never -- or the whole run, and then the solution, where it is shorter."""
    modes = (dict(adaptive=True, accelerate=False), dict(adaptive=False, accelerate=True), dict(adaptive=False, accelerate=False))
    problems = []
    ctor = lambda backend: MaxNormProblem.construct(N=90, K=10, seed=21, backend=backend)
    (pn, X0), (ph, _) = ctor("numpy"), ctor("hip")
    L = float(np.linalg.norm(pn.S + pn.S.T, 2))
    problems.append(("max_norm", pn, ph, X0, L))
    for kernel in ("linear", "rbf"):
        ctor = lambda backend: SVMProblem.construct(M=120, N=6, C=0.05 if kernel == "linear" else 0.5, kernel=kernel, gamma=0.01, seed=22, backend=backend)
        (pn, y0), (ph, _) = ctor("numpy"), ctor("hip")
        problems.append((f"svm {kernel}", pn, ph, y0, float(np.linalg.norm(pn.Q, 2))))
    for label, pn, ph, x0, L in problems:
        for mode in modes:
            opts = dict(tolerance=1e-5, evaluate_objective=True, L=L, tau0=(2 / L) / 10, max_iters=120, **mode)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                (sn, cn), (sh, ch) = pn.solve(x0, opts), ph.solve(x0, opts)
            print(f"\n{label} {mode}: numpy {cn.iteration_count} iterations, hip {ch.iteration_count}", end="")
            k = min(cn.iteration_count, ch.iteration_count, 40)
            assert k == 40 or cn.iteration_count == ch.iteration_count, (label, mode)
            G.compare_histories(ch, lambda f: getattr(cn, f), k, rtol=1e-6, atol=1e-12)
            if k < 40:
                np.testing.assert_allclose(sh, sn, rtol=1e-5, atol=1e-6 * float(np.max(np.abs(sn))) + 1e-12)


def test_example_command_lines_run_on_the_device():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for module, args in (("fasta.examples.max_norm", ["--points", "150", "--rank", "4"]), ("fasta.examples.svm", ["--points", "120", "--kernel", "rbf"])):
        out = subprocess.run([sys.executable, "-m", module, "--backend", "hip"] + args, cwd=root, capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr[-2000:]
        assert "Iterations (adaptive, accelerated, plain):" in out.stdout


# ---- the C ABI says no with a sentence -------------------------------------------------------------------------------------------------------------------
def refusal(code, text):
    return pytest.raises(hip.HipError, match=rf"^\[{code}\].*{text}")


def test_refusals_of_the_c_abi():
    import ctypes as C
    Q = np.eye(6)
    pd = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    with hip.HipContext(0) as c:
        with refusal(hip.E_STATE, "no quadratic operator"):
            c.quad_shape()
        for L in (0, 17):
            with refusal(hip.E_ARG, "1 to 16 columns"):
                c.set_quadratic(Q, None, L)
        bad = Q.copy()
        bad[4, 1], bad[2, 5] = 0.5, 0.25
        with refusal(hip.E_ARG, r"not symmetric: Q\[1,4\] = 0 but Q\[4,1\] = 0\.5"):
            c.set_quadratic(bad, None, 1)
        assert c.lib.fh_set_quadratic(c._h, pd(Q), 6, 5, None, 1) == hip.E_ARG and b"ld_host" in c.lib.fh_last_error()
        assert c.lib.fh_set_quadratic(c._h, None, 6, 6, None, 1) == hip.E_ARG
        with refusal(hip.E_ARG, "quadratic operator only"):
            c.set_prox(hip.PROX_ROWBALL, 1.0)
        c.set_matrix(np.eye(6))
        c.set_rhs(2)
        with refusal(hip.E_ARG, "quadratic operator only"):
            c.set_prox(hip.PROX_ROWBALL, 1.0)
        c.set_quadratic(Q, np.ones((6, 3)), 3)
        assert c.rhs == 3 and c.shape() == (6, 6) and c.fused_supported() == 0 and c.fused_agree() == 0 and not c.run_supported()
        for kind in (hip.PROX_LINF, hip.PROX_L1BALL, hip.PROX_TVBALL):
            with refusal(hip.E_ARG, "has no quadratic form"):
                c.set_prox(kind, 1.0)
        with refusal(hip.E_ARG, "unknown prox kind"):
            c.set_prox(9, 1.0)
        for call in (lambda: c.set_loss_lsq(np.zeros(18)), lambda: c.set_loss_logistic(np.ones(18))):
            with refusal(hip.E_STATE, "carries its own loss"):
                call()
        with refusal(hip.E_STATE, "fixed when it is set"):
            c.set_rhs(2)
        c.set_prox(hip.PROX_ROWBALL, 1.0)
        c.set_vector(hip.VEC_X0, np.ones((6, 3)))
        c.init()
        for call, who in ((lambda: c.step(0.1), "fh_step"), (lambda: c.step_begin(0.1), "fh_step"), (lambda: c.step_accel(0.1, 0.1, True), "fh_step_accel")):
            with refusal(hip.E_STATE, who + ": the quadratic operator has no one-pass kernel"):
                call()
        with refusal(hip.E_STATE, "fh_run: the quadratic operator has no device-side loop"):
            c.run(1, hip.RunOpts(window=1), hip.RunState())
        with refusal(hip.E_STATE, "cannot be row-sharded"):
            c.comm_init(1, 0, bytes(hip.UNIQUE_ID_BYTES))
        with refusal(hip.E_STATE, "not read back"):
            c.get_matrix_rows(0, 1)
        with refusal(hip.E_STATE, "stream-read"):
            c.stream_read_ms()
        # any other operator returns the context to its previous form: vector layout, least squares, and ROWBALL gives way to IDENTITY
        c.set_matrix(np.eye(6))
        assert c.rhs == 0
        c.set_loss_lsq(np.zeros(6))
        c.set_vector(hip.VEC_X0, np.full(6, 3.0))
        c.set_vector(hip.VEC_G0, np.zeros(6))
        c.fwd(1.0)
        assert np.array_equal(c.get_vector(hip.VEC_XPROX, 6), np.full(6, 3.0))
        with refusal(hip.E_STATE, "no quadratic operator"):
            c.quad_shape()
    for kwargs in (dict(storage="f32"), dict(devices=[0, 0])):
        with hip.HipContext(0, **kwargs) as c:
            with refusal(hip.E_STATE, "float32 storage has no quadratic operator" if "storage" in kwargs else "multi-device context has no quadratic operator"):
                c.set_quadratic(Q, None, 1)


def test_gradient_at_and_setup_take_the_three_pass_route():
    n, L = 70, 5
    rng = np.random.RandomState(9)
    U = np.triu(rng.randn(n, n))
    Q, cvec = U + np.triu(U, 1).T, rng.randn(n, L)
    T0, T1, X0 = rng.randn(n, L), rng.randn(n, L), rng.randn(n, L)
    with context(Q, cvec, L, {}) as c:
        c.set_vector(hip.VEC_T0, T0)
        c.set_vector(hip.VEC_T1, T1)
        c.set_vector(hip.VEC_X0, X0)
        s = c.setup()
        g0 = c.get_vector(hip.VEC_T2, n * L).reshape(n, L)
        np.testing.assert_allclose(g0, Q @ T0 + cvec, rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(np.sqrt(s[hip.S_DG2]), np.linalg.norm(Q @ (T0 - T1)), rtol=1e-12)
        np.testing.assert_allclose(np.sqrt(s[hip.S_DX2]), np.linalg.norm(T0 - T1), rtol=1e-12)
        want_f = .5 * np.sum(X0 * (Q @ X0)) + np.sum(cvec * X0)
        assert abs(s[hip.S_FSQ] - want_f) <= 1e-12 * np.sum(np.abs(X0) * (np.abs(Q) @ np.abs(X0) + np.abs(cvec)))
        np.testing.assert_allclose(c.get_vector(hip.VEC_G0, n * L).reshape(n, L), Q @ X0 + cvec, rtol=1e-12, atol=1e-12)
        assert np.array_equal(c.get_vector(hip.VEC_B, n * L).reshape(n, L), cvec)                 # FH_VEC_B holds c

"""GPU tests of EVERY instantiation and path of the one-pass dense kernels (csrc/fh_fused.h + fh_fused_body.inc: k_fused_dense, what fh_step /
fh_step_accel launch; csrc/fh_setup.h: k_setup_dense, fh_setup's one-read launch), each against exact arithmetic.

tests/fused_paths.py pins the geometry of every case (FH_TUNE_FUSED_CUS, both halves of FH_TUNE_FUSED_VARIANT), and every test here first asks
the library what it is about to launch (fh_fused_launch_shape / fh_setup_shape, the rule the launchers themselves call).  The operands are such that
every product and every sum of a launch is exactly representable in float64 whatever the order of summation (tests/test_fused_paths_cpu.py proves
it in integer arithmetic, without a device), so all fourteen scalars, the vectors a launch writes and the padding behind them are compared with
== / np.array_equal: a last column pair masked wrongly, a padding row counted, a team's last row skipped, a member's partial left out of a row
sum, a team's partial left out of the gradient or the wrong acceleration history cannot hide inside a tolerance.  Only the logistic loss (exp, log, a
division per row) is not exact: it is compared with an np.longdouble model at the tolerances of
tests/test_gpu_run_paths.py::test_the_first_logistic_iteration_against_longdouble; its Z, XHAT, XPROX and X1 stay exact."""
import numpy as np
import pytest

from fasta_python_amd import hip
from tests import fused_paths as FP
from tests import run_paths as RP
from tests.test_gpu_run_paths import first_bad, padding_is_zero

pytestmark = pytest.mark.gpu
EXACT, LOGISTIC, SETUP = FP.exact_step_cases(), FP.logistic_cases(), FP.setup_cases()
VECTORS = {"xhat": hip.VEC_XHAT, "xprox": hip.VEC_XPROX, "x1": hip.VEC_X1, "g1": hip.VEC_G1, "z": hip.VEC_Z}


def ids(cases):
    return [FP.case_id(c) for c in cases]


def context(case, A, b_or_labels):
    c = hip.HipContext(0, storage=case.storage)
    for key, value in FP.tuning_of(case).items():
        c.set_tuning(key, value)
    c.set_matrix(A)
    (c.set_loss_lsq if case.loss == "lsq" else c.set_loss_logistic)(b_or_labels)
    kind, mu, lo, hi = RP.PROX[case.kind]
    c.set_prox(kind, mu, lo, hi)
    return c


def check_geometry(c, case):
    """the library is about to launch what the case expects (a whole-device case: from the CU count the device reports)"""
    device_cus, used = c.cu_count()
    assert device_cus >= max(64, case.cus) and used == (case.cus or device_cus), (device_cus, used)
    got = c.fused_launch_shape() if case.what == "step" else c.setup_shape()
    assert got == FP.expected_shape(case, device_cus), (got, FP.expected_shape(case, device_cus))
    assert c.fused_supported() in (1, 3)
    return got


def enter(c, case, st):
    """The entering state with the existing entry points: fh_init forms z0 and g0 from x0; an accelerated (or logistic) case then takes one accelerated
    launch -- so that the context addresses x1 and the prox output separately -- overwrites what it left with the state the case enters with (x0 and
    g0 as the next iterate and gradient, x_accel0 and z_accel0 as the prox output and z) and commits it."""
    c.set_vector(hip.VEC_X0, st.x0)
    c.init()
    if case.mode == "plain" and case.loss == "lsq":
        assert np.array_equal(c.get_vector(hip.VEC_G0, case.n), st.g0)          # (exact too: the CPU tier proves the sums of fh_init)
        return
    c.step_accel(FP.TAU, 0.0, False)
    for which, v in ((hip.VEC_XPROX, st.xacc0), (hip.VEC_Z, st.zacc0), (hip.VEC_X1, st.x0), (hip.VEC_G1, st.g0)):
        c.set_vector(which, v)
    c.commit()
    assert np.array_equal(c.get_vector(hip.VEC_X0, case.n), st.x0) and np.array_equal(c.get_vector(hip.VEC_G0, case.n), st.g0)


def launch(c, case):
    if case.mode == "plain":
        scal = c.step(FP.TAU)
    else:
        scal = c.step_accel(FP.TAU, FP.COEF, case.mode in ("restart_hi", "restart_lo"))
    out = {"sums": scal[:14].copy(), "tail": scal[14:].copy()}
    for name, which in VECTORS.items():
        out[name] = c.get_vector(which, case.m if name == "z" else case.n)
    out["padding"] = [name for name in ("xhat", "xprox", "x1", "g1") if not padding_is_zero(c, VECTORS[name], case.n)]
    return out


def assert_equals_model(got, case):
    mdl = FP.model(case)
    bad = [f"{name}: {g!r} != {w!r}" for name, g, w in zip(RP.SUMS, got["sums"], mdl.sums) if g != w]
    assert not bad, bad
    assert got["tail"][0] == 0.0 and got["tail"][1] == 0.0                      # no clipping level; no hand-off timeout
    for name in VECTORS:
        msg = first_bad(name, got[name], mdl.vectors[name])
        assert msg is None, msg
    assert got["padding"] == [], got["padding"]


# ---- the step kernel, exact ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", EXACT, ids=ids(EXACT))
def test_a_launch_is_exact_on_every_path_and_so_is_its_repetition(case):
    """fh_fused_launch_shape == the case's geometry; the entering state; fh_step / fh_step_accel; all fourteen scalars, XHAT, XPROX, X1, G1, Z and
    the padding of the n-side buffers; then the same launch again from the same state on the same context (the other slot parity, the counters the
    first launch re-armed)."""
    st = FP.operands(case)
    with context(case, st.A, st.b) as c:
        check_geometry(c, case)
        enter(c, case, st)
        assert_equals_model(launch(c, case), case)
        assert_equals_model(launch(c, case), case)
        assert_equals_model(launch(c, case), case)


def one_per_form(cases, want):
    out, seen = [], set()
    for c in cases:
        form = FP.form_of(FP.expected_shape(c))
        if want(c) and form not in seen:
            seen.add(form)
            out.append(c)
    assert seen == set(FP.FORMS), set(FP.FORMS) - seen
    return out


AFTER = one_per_form(EXACT, lambda c: c.mode != "plain" and c.cus and c.cus <= 64)


@pytest.mark.parametrize("case", AFTER, ids=ids(AFTER))
def test_an_accelerated_launch_after_a_plain_one_and_a_launch_after_a_change_of_team_shape(case):
    """One context: a plain launch, then the case's accelerated one (the restart-dot line was re-armed by a launch that did not use it); then the
    launch on the whole device -- other teams, other slots, a refill -- and back on the pinned CUs.  Exact sums do not depend on the geometry: all
    three equal the model."""
    st = FP.operands(case)
    with context(case, st.A, st.b) as c:
        check_geometry(c, case)
        enter(c, case, st)
        c.step(FP.TAU)
        assert_equals_model(launch(c, case), case)
        c.set_tuning(hip.TUNE_FUSED_CUS, 0)
        whole = c.fused_launch_shape()
        assert whole.grid != FP.expected_shape(case).grid
        assert_equals_model(launch(c, case), case)
        c.set_tuning(hip.TUNE_FUSED_CUS, case.cus)
        check_geometry(c, case)
        c.step(FP.TAU)
        assert_equals_model(launch(c, case), case)


# ---- the set-up kernel, exact ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SETUP, ids=ids(SETUP))
def test_the_one_read_set_up_is_exact_on_every_path(case):
    """fh_setup through the one-read kernel (one one-pass launch, not the three passes): f's sum, the two norms of L, sum |x0|, g0, A^T A (T0 - T1),
    z (the next step's z_accel0, addressable after a commit) and the padding of the two n-side outputs; twice on one context."""
    o, mdl = FP.setup_operands(case), FP.setup_model(case)
    with context(case, o.A, o.b) as c:
        check_geometry(c, case)
        for rep in range(2):
            for which, v in ((hip.VEC_T0, o.t0), (hip.VEC_T1, o.t1), (hip.VEC_X0, o.x0), (hip.VEC_T2, np.ones(case.n)), (hip.VEC_G0, np.ones(case.n))):
                c.set_vector(which, v)
            c.timing_reset()
            c.timing_enable(True)
            s = c.setup()
            c.timing_enable(False)
            assert c.timing_get(hip.K_FUSED)[1] == 1                          # the one-read kernel ran, not fh_gradient_at x 2 + fh_init
            assert s[15] == 0.0
            for name, slot in (("FSQ", hip.S_FSQ), ("DX2", hip.S_DX2), ("DG2", hip.S_DG2), ("GSUM", hip.S_GSUM)):
                assert s[slot] == mdl[name], (rep, name, s[slot], mdl[name])
            for name, which in (("g0", hip.VEC_G0), ("t2", hip.VEC_T2)):
                msg = first_bad(name, c.get_vector(which, case.n), mdl[name])
                assert msg is None, (rep, msg)
            assert padding_is_zero(c, hip.VEC_G0, case.n, scratch=hip.VEC_T0) and padding_is_zero(c, hip.VEC_T2, case.n, scratch=hip.VEC_T0)
        c.commit()                                                             # z1 := the z the set-up left
        msg = first_bad("z", c.get_vector(hip.VEC_Z, case.m), mdl["z"])
        assert msg is None, msg


def test_the_shape_queries_refuse_what_has_no_one_pass_kernel():
    with hip.HipContext(0) as c:
        c.set_matrix(np.ones((4, 262160)))
        c.set_loss_lsq(np.ones(4))
        for query in (c.fused_launch_shape, c.setup_shape):
            with pytest.raises(hip.HipError, match=rf"^\[{hip.E_STATE}\]"):
                query()
        c.set_matrix(np.ones((40, 600)))
        c.set_loss_lsq(np.ones(40))
        dev, used = c.cu_count()
        assert c.fused_launch_shape() == hip.fused_launch_shape_for(40, 600, cus=used)      # the context form and the pure form: one rule
        with pytest.raises(hip.HipError, match=rf"^\[{hip.E_STATE}\]"):
            c.setup_shape()                                                    # too small to pay: fh_setup takes the three passes
        c.set_loss_logistic(np.ones(40))
        with pytest.raises(hip.HipError, match=rf"^\[{hip.E_STATE}\]"):
            c.setup_shape()


# ---- the logistic loss: not exact --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", LOGISTIC, ids=ids(LOGISTIC))
def test_a_logistic_launch_against_longdouble(case):
    """Labels +-1, a dyadic entering state, ONE launch.  Z, XHAT, XPROX and X1 are exact.  Tolerances: those of the device-loop suite's logistic test
    (the gradient rtol 1e-11, scalars rtol 1e-11, the Barzilai-Borwein pair 1e-10) with 64 * 2^-52 of the sum of the terms' magnitudes added wherever
    a sum is signed: g1 (A^T r), <dx, g0>, <dx, dg>.  The loss terms are summed in the pass after the row loop, under both dealings, past padding rows."""
    st = FP.operands(case)
    mag = {}
    sums, want = FP._attempt(case, st, dtype=np.longdouble, magnitudes=mag)
    with context(case, st.A, st.labels) as c:
        check_geometry(c, case)
        enter(c, case, st)
        got = launch(c, case)
        again = launch(c, case)
    for name in ("xhat", "xprox", "z", "x1"):
        msg = first_bad(name, got[name], np.asarray(want[name], dtype=np.float64))
        assert msg is None, msg
    assert got["padding"] == [] and got["tail"][1] == 0.0
    eps = 64 * 2.0 ** -52
    g1 = np.asarray(want["g1"], dtype=np.float64)
    dev = np.max(np.abs(got["g1"] - g1) / (1e-11 * np.abs(g1) + eps * np.asarray(mag["G1"], dtype=np.float64) + 1e-13))
    assert dev <= 1.0, ("g1", dev)
    slack = {"DXG0": eps * float(mag["DXG0"]), "DXDG": eps * float(mag["DXDG"])}
    worst = {}
    for k, name in enumerate(RP.SUMS):
        w = float(sums[k])
        rtol = 1e-10 if name in ("DXDG", "DG2") else 1e-11
        worst[name] = abs(got["sums"][k] - w) / (abs(w) + 1e-300)
        assert abs(got["sums"][k] - w) <= rtol * abs(w) + slack.get(name, 0.0), (name, got["sums"][k], w)
    print(f"\n{FP.case_id(case)}: worst relative deviations {worst}", end="")
    assert np.array_equal(got["sums"], again["sums"]) and all(np.array_equal(got[k], again[k]) for k in VECTORS)     # bitwise repeatable

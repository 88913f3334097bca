"""GPU tests of EVERY path of the device-side loop kernel (csrc/fh_run.h: k_run_dense<PPT>, what fh_run launches), each against exact arithmetic.

tests/run_paths.py pins the geometry of every case (FH_TUNE_FUSED_CUS, the rows-per-team floor) so that the instantiation, the row blocks and
phase B's split do not depend on the device beyond "at least 64 CUs", and every test here first asks the library what it is about to launch
(fh_run_shape).  The operands are such that every product and every sum of the compared iterations is exactly representable in float64
whatever the order of summation (tests/test_run_paths_cpu.py proves it in integer arithmetic, without a device), so the history records, the
state the launch writes back and the vectors it leaves are compared with == / np.array_equal: a last column pair masked wrongly, a padding row
counted in f, a wrong slice boundary in phase B, a stale block of partial sums after a retry, a prefetch that wraps onto the wrong row or a
wrong entry of f_window cannot hide inside a tolerance.  Only the logistic loss (exp, log, a division per row) is not exact: its first
iteration is compared with an np.longdouble model at the tolerances of DESIGN.md section 13 with 64 * 2^-52 of the sum of their terms'
magnitudes added to the signed sums."""
import ctypes as C

import numpy as np
import pytest

from fasta_python_amd import hip
from tests import run_paths as RP

pytestmark = pytest.mark.gpu
CASES = RP.cases()


def context(case, tuning=None, loss="lsq"):
    A, x0, b, _ = RP.operands(case)
    c = hip.HipContext(0)
    for key, value in (RP.tuning_of(case) if tuning is None else tuning).items():
        c.set_tuning(key, value)
    c.set_matrix(A)
    if loss == "lsq":
        c.set_loss_lsq(b)
    else:
        c.set_loss_logistic(np.where(b > 0, 1.0, -1.0))
    kind, mu, lo, hi = RP.PROX[case.kind]
    c.set_prox(kind, mu, lo, hi)
    c.set_vector(hip.VEC_X0, x0)
    return c


def start(c, case, lsq=True):
    """fh_init and the caller's state before the first iteration"""
    scal = c.init()
    f0 = RP.fc_f(lsq, scal[hip.S_FSQ])
    return RP.entering_state(case, float(f0), RP.operands(case)[3])


def collect(c, case, st, hist):
    out = {"history": np.array(hist), "state": [getattr(st, k) for k in RP.STATE_FIELDS], "f_window": np.array(st.f_window[:])}
    for name, which in RP.VECTORS.items():
        out[name] = c.get_vector(which, case.m if name == "Z" else case.n)
    return out


def launch(case, cut=None, entry="run", tuning=None):
    """The case's launch (or the same iterations cut into launches of `cut`) on a fresh context: everything a test compares."""
    with context(case, tuning) as c:
        if entry == "run":
            sh = c.run_shape()
            assert sh == RP.expected_shape(case), (sh, RP.expected_shape(case))
            assert c.cu_count()[0] >= 64 and c.run_supported()
        o, st = RP.run_opts(case), start(c, case)
        if entry != "run":
            o.launch_mode = hip.LAUNCH_ONEPASS_ALWAYS if c.fused_supported() in (1, 3) else hip.LAUNCH_SEPARATE
            st.spec_cooldown, st.onepass_backoff, st.onepass_off_until = 0, 64, -1
        total, hist = RP.launches_of(case), []
        while len(hist) < total and not st.stopped:
            h = (c.run if entry == "run" else c.iterate)(min(cut or total, total - len(hist)), o, st)
            assert st.stopped in (0, 1) and len(h) > 0
            hist += [list(r) for r in h]
        out = collect(c, case, st, hist)
        out["padding"] = all(padding_is_zero(c, RP.VECTORS[name], case.n) for name in ("X0", "G0", "XHAT", "G1", "BEST"))
        if entry == "run":
            assert c.recovered_count(hip.RECOVERED_RUN_TIMEOUT) == 0
    return out


def padding_is_zero(c, which, n, scratch=hip.VEC_T0):
    """fh_diff_norm adds up the WHOLE device buffers, so against a buffer that holds the same logical entries and untouched (zero) padding the
    norm is exactly zero only if the padding of `which` is (the idiom of tests/test_gpu_factor.py)."""
    c.set_vector(scratch, c.get_vector(which, n))
    return c.diff_norm(which, scratch) == 0.0


def first_bad(name, got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.shape != want.shape:
        return f"{name}: shape {got.shape} != {want.shape}"
    bad = np.argwhere(got != want)
    if bad.size:
        i = tuple(bad[0])
        return f"{name}: {len(bad)} wrong entries, first at {bad[0]}: {got[i]!r} != {want[i]!r}"
    return None


def assert_equals_model(got, case):
    mdl = RP.model(case)
    want = {"history": np.array(mdl.history), "state": [mdl.st[k] for k in RP.STATE_FIELDS], "f_window": np.array(mdl.fwin)}
    want.update({k: v for k, v in mdl.vectors().items() if v is not None})
    assert len(got["history"]) == mdl.steps_done
    for name, w in want.items():
        msg = first_bad(name, got[name], w)
        assert msg is None, msg
    assert got["padding"]


@pytest.mark.parametrize("case", CASES, ids=RP.case_id)
def test_one_launch_is_exact_on_every_path(case):
    """fh_run_shape == the case's geometry; fh_init; ONE fh_run of the compared iterations; history, state on exit, f_window, the vectors the
    launch leaves (X0 = the new iterate, G0, XHAT, G1, BEST, Z and the prox / x1 buffers that hold a defined value) and the n-side padding."""
    assert_equals_model(launch(case), case)


@pytest.mark.parametrize("case", [c for c in CASES if RP.launches_of(c) > 1], ids=RP.case_id)
def test_launches_of_one_iteration_give_the_same_bits(case):
    """The same solve cut into launches of one iteration each: the state that travels between launches makes it independent of the cut."""
    assert_equals_model(launch(case, cut=1), case)


@pytest.mark.parametrize("case", [c for i, c in enumerate(CASES) if i % 3 == 0], ids=RP.case_id)
def test_a_second_run_gives_the_same_bits(case):
    a, b = launch(case), launch(case)
    assert set(a) == set(b)
    for key in a:
        assert np.array_equal(a[key], b[key]), key


@pytest.mark.parametrize("case", CASES, ids=RP.case_id)
def test_the_library_loop_gives_the_same_bits_on_the_exact_operands(case):
    """fh_iterate (the host-side loop; the one-pass kernel where it has a shape) under the automatic launch rules: other kernels, another order
    of summation, the host's square -- and, both being exact, the same history, state and iterate.  (The host squares with pow, the device
    multiplies: equal on these sums, tests/test_run_paths_cpu.py compares the restated controller with both.)"""
    got = launch(case, entry="iterate", tuning={hip.TUNE_NT_LOADS: case.nt})
    mdl = RP.model(case)
    assert first_bad("history", got["history"], np.array(mdl.history)) is None, first_bad("history", got["history"], np.array(mdl.history))
    assert got["state"] == [mdl.st[k] for k in RP.STATE_FIELDS]
    for name in ("X0", "G0", "BEST"):
        msg = first_bad(name, got[name], mdl.vectors()[name])
        assert msg is None, msg


def test_the_window_is_refused_where_the_persistent_launch_has_no_kernel():
    with hip.HipContext(0) as c:
        for prepare in (lambda: c.set_stencil(8, 8), lambda: (c.set_matrix(np.eye(40)), c.set_rhs(3)),
                        lambda: (c.set_rhs(0), c.set_matrix(np.ones((4, 7200))))):
            prepare()
            with pytest.raises(hip.HipError, match=rf"^\[{hip.E_STATE}\]"):
                c.run_shape()
        c.set_matrix(np.eye(40))
        c.set_prox(hip.PROX_LINF, 1.0)
        with pytest.raises(hip.HipError, match=rf"^\[{hip.E_STATE}\]"):
            c.run_shape()
        c.set_prox(hip.PROX_SHRINK, 1.0)
        dev, used = c.cu_count()
        assert c.run_shape() == hip.run_shape_for(40, 40, cus=used)                 # the context form and the pure form: one rule


# ---- the logistic loss: not exact ---------------------------------------------------------------------------------------------------------------
LOGISTIC = [next(c for c in CASES if c.name.startswith(tag)) for tag in ("clamped4", "full10")]      # not BIG / BIG


@pytest.mark.parametrize("case", LOGISTIC, ids=RP.case_id)
def test_the_first_logistic_iteration_against_longdouble(case):
    """Labels sign(b), the case's geometry, ONE iteration (its retries included).  Tolerances: DESIGN.md section 13's (vectors rtol 1e-12 / 1e-11
    for the gradient, scalars rtol 1e-11, the Barzilai-Borwein pair 1e-10) with 64 * 2^-52 of the sum of the terms' magnitudes added wherever a
    sum is signed: g (A^T r), z (A xprox), <Dx, g0>.  The history record's entries are quotients and roots of those sums: rtol 1e-10."""
    mdl = RP.Model(case, loss="logistic", dtype=np.longdouble)
    mdl.run(1)
    with context(case, loss="logistic") as c:
        assert c.run_shape() == RP.expected_shape(case)
        o, st = RP.run_opts(case), start(c, case, lsq=False)
        np.testing.assert_allclose(st.f_window[0], float(mdl.f0), rtol=1e-12)
        h = c.run(1, o, st)
        got = collect(c, case, st, h)
    eps = 64 * 2.0 ** -52
    mag = mdl.magnitudes
    want = mdl.vectors()
    worst = {}

    def close(name, g, w, rtol, slack):
        w = np.asarray(w, dtype=np.float64)
        dev = np.max(np.abs(g - w) / (rtol * np.abs(w) + slack + 1e-300))
        worst[name] = float(np.max(np.abs(g - w) / (np.abs(w) + 1e-300)))
        assert dev <= 1.0, (name, dev)

    assert got["state"][4:] == [1, mdl.st["backtracks"], 0]
    tau = float(mdl.history[0][2])
    close("G0", got["G0"], want["G0"], 1e-11, eps * np.asarray(mag["G1"], dtype=np.float64) + 1e-13)
    close("Z", got["Z"], want["Z"], 1e-12, 1e-13) if want["Z"] is not None else None
    slack_x = tau * (eps * np.abs(np.asarray(mdl.A, dtype=np.float64)).T @ np.ones(case.m) + 1e-13) + 1e-14       # x - tau g0: |r0| <= 1 per row
    close("XHAT", got["XHAT"], want["XHAT"], 1e-12, slack_x)
    close("X0", got["X0"], want["X0"], 1e-12, slack_x)
    close("history", got["history"][0], np.array(mdl.history[0], dtype=np.float64), 1e-10, 0.0)
    print(f"\n{RP.case_id(case)} logistic: worst relative deviations {worst}", end="")

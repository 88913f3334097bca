"""CPU tier of the tests of every path of the device-side loop kernel (csrc/fh_run.h: k_run_dense<PPT>): everything tests/run_paths.py claims,
proven without a device -- the geometry each case pins (against the library's own rule, fh_run_shape_for), the paths that geometry runs and
their union, the exactness of every compared iteration (redone in integer arithmetic: every product exact, every sum below 2^53 of its terms'
common lsb, so any order of summation and any fusing of multiply-adds gives the model's bits), the sensitivity of the compared outputs to the
inputs, and the equality of the restated controller with the shipped one (csrc/fh_controller.h instantiated with the device's square)."""
import collections
import re

import numpy as np
import pytest

from fasta_python_amd import hip
from tests import controller_shim as CS
from tests import run_paths as RP

CASES = RP.cases()
ROW_CLAIMS = {
    "short_last": ("padding rows in a live block", "short last block"),
    "one_row_last": ("r_end == 1", "short last block", "r_end % NB != 0", "padding rows in a live block"),
    "empty_wgs": ("workgroups with no rows", "padding rows in a live block"),
    "one_wg": ("G == 1", "block of >= 2 NB rows", "padding rows in a live block"),
    "floor16": ("block of >= 2 NB rows", "r_end % NB != 0", "short last block", "padding rows in a live block"),
}
NAME_CLAIMS = {"maxbt": ("slices == 1, ragged trips",), "one_trip": ("slices == 1, one trip",)}
CTL_CLAIMS = {"maxbt": "accepted at bt == max_backtracks", "stop": "ended by the stop rule", "stale": "accepted but not better"}


@pytest.fixture(scope="module")
def shipped_controller(tmp_path_factory):
    return CS.build(tmp_path_factory.mktemp("controller_shim"))


# ---- geometry --------------------------------------------------------------------------------------------------------------------------------
def test_the_query_refuses_what_the_launch_has_no_kernel_for():
    for args in ((0, 10), (10, 0), (10, 7169), (4095, 5000)):               # empty; wider than the table; a wide row outside the measured window
        with pytest.raises(hip.HipError):
            hip.run_shape_for(*args)
    with pytest.raises(hip.HipError):
        hip.run_shape_for(10, 10, cus=0)
    assert hip.run_shape_for(4096, 5000).PPT == 10 and hip.run_shape_for(10, 7168, run_max_n=7168).PPT == 14
    # the default floor of 16 rows per workgroup, in steps of 8 workgroups; no floor: every CU
    assert hip.run_shape_for(200, 1000, cus=256).G == 16 and hip.run_shape_for(200, 1000, cus=256, min_rows=0).G == 256
    assert hip.run_shape_for(200, 1000, cus=4).G == 4
    # auto load policy: non-temporal beyond 256 MiB of matrix
    assert hip.run_shape_for(8192, 4096, run_max_n=4096).NT == 0 and hip.run_shape_for(8193, 4096, run_max_n=4096).NT == 1
    assert hip.run_shape_for(8193, 4096, run_max_n=4096, nt_loads=0).NT == 0


@pytest.mark.parametrize("case", CASES, ids=RP.case_id)
def test_the_library_launches_what_the_case_expects(case):
    assert RP.shape_query(case) == RP.expected_shape(case)


@pytest.mark.parametrize("case", CASES, ids=RP.case_id)
def test_a_case_runs_the_paths_its_name_claims(case):
    sh = RP.shape_query(case)
    paths = RP.paths_of(sh, case.m, case.n)
    tag, _, rows = case.name.partition("-")
    claims = list(ROW_CLAIMS.get(rows, ())) + list(NAME_CLAIMS.get(case.name, ()))
    if tag.startswith("full"):
        claims.append("all lanes live")
        assert sh.PPT == int(tag[4:]) and case.n == sh.PPT * 512
    if tag.startswith(("clamped", "extra")):
        claims.append("clamped lanes")
        assert sh.PPT == sh.need == int(re.sub(r"\D", "", tag))
    if tag.startswith("idle"):
        claims += ["idle piece", "clamped lanes"]
        assert sh.need == int(tag[4:]) and sh.PPT == sh.need + 1
    for path in claims:
        assert paths[path], (path, sh)
    if case.ctl:
        assert RP.controller_paths(case, RP.model(case))[CTL_CLAIMS[case.ctl]]
    assert 20 <= case.m <= 320 and sh.G <= 64


def test_the_cases_cover_every_row_of_the_table():
    lanes, blocks, phase_b, controller, options = set(), set(), set(), set(), set()
    for c in CASES:
        sh = RP.shape_query(c)
        for path, yes in RP.paths_of(sh, c.m, c.n).items():
            if yes:
                (lanes if path in RP.LANE_PATHS else blocks).add((path, sh.PPT if path in RP.LANE_PATHS else sh.NB))
                phase_b.add(path)
        mdl = RP.model(c)
        controller |= {p for p, yes in RP.controller_paths(c, mdl).items() if yes}
        options |= {("mode", c.mode, c.restart), ("kind", c.kind, sh.BIG), ("nt", sh.NT), ("objective", c.evalobj), ("geometry", c.geom, sh.PPT),
                    ("exact iterations", c.geom, sh.PPT, c.mode == "plain" and len(mdl.history))}
    for ppt in RP.RUN_TABLE:
        assert ("all lanes live", ppt) in lanes and ("clamped lanes", ppt) in lanes, ppt
        assert ("geometry", "A", ppt) in options and ("exact iterations", "B", ppt, 4) in options, ppt       # one exact iteration in A, four in B
    for ppt in (4, 10, 12, 14):
        assert ("idle piece", ppt) in lanes, ppt
    for nb in (3, 4, 5, 6):
        for path in RP.ROW_PATHS:
            assert (path, nb) in blocks, (path, nb)
    assert set(RP.PHASE_B_PATHS) <= phase_b, set(RP.PHASE_B_PATHS) - phase_b
    assert set(RP.CONTROLLER_PATHS) <= controller, set(RP.CONTROLLER_PATHS) - controller
    assert {("mode", "plain", 0), ("mode", "adaptive", 0), ("mode", "accel", 0), ("mode", "accel", 1), ("nt", 0), ("nt", 1), ("objective", 0),
            ("objective", 1)} <= options
    assert {("kind", k, big) for k in RP.KINDS for big in (0, 1)} <= options


# ---- exactness -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=RP.case_id)
def test_every_compared_iteration_is_exact_in_any_order_of_summation(case):
    """Every attempt of the launch redone over the integers (tests/run_paths.py: prove_attempt): all products exact, sum|terms| / lsb < 2^53 for
    every sum, and the float64 model's sums and vectors equal to the integers'.  A condition, not a measurement."""
    proven, bits, where, failed = RP.prove(case)
    print(f"\n{RP.case_id(case)}: {proven} iterations, worst sum {where}: {bits} bits", end="")
    assert failed is None, failed
    assert proven == case.steps == len(RP.model(case).history[:case.steps]) and bits <= 53


def test_the_proof_refuses_what_is_not_exact():
    """Geometry A past its first iteration, and one more backtrack than 53 bits hold: the proof must say no."""
    case = next(c for c in CASES if c.geom == "A" and c.mode == "plain")
    proven, _, _, failed = RP.prove(case, steps=6)
    assert failed is not None and 1 <= proven < 6
    A, x0, b, _ = RP.operands(case)
    g0 = A.T @ (A @ x0 - b)
    with pytest.raises(RP.NotExact):
        RP.prove_attempt(A.astype(np.int64), b, x0 + 2.0 ** -30, g0, x0, A @ x0, 2.0 ** -30, 0.0, False, "identity", RP.Bits())


# ---- sensitivity -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=RP.case_id)
def test_the_model_is_not_trivial(case):
    A, x0, b, _ = RP.operands(case)
    if case.geom == "A":
        assert A.any(axis=0).all() and A.any(axis=1).all()                   # every column and every row holds a non-zero
        assert 0.2 < np.count_nonzero(A) / A.size < 0.3
    else:
        assert (np.count_nonzero(A, axis=1) >= case.per_row).all() and set(np.unique(A)) == {-1.0, 0.0, 1.0}
    mdl = RP.model(case)
    assert mdl.retries[0] >= 1 and len(mdl.history) == mdl.steps_done == (1 if case.ctl == "stop" else case.steps)
    first = RP.Model(case)
    first.run(1)
    # The prox output differs from x0 in more than half the entries.  In geometry B a column without an entry has g0 = 0 there -- with 8 or 16
    # entries per row most columns of a wide matrix are such, and xhat = x0 in them whatever the data: there the condition is held over the
    # columns that hold an entry (the others check that an entry passes through the forward step unchanged, and through the prox).
    live = np.ones(case.n, dtype=bool) if case.geom == "A" else A.any(axis=0)
    moved = np.count_nonzero((first.last["xprox"] != x0) & live)
    assert moved > np.count_nonzero(live) / 2 and np.count_nonzero(live) >= min(case.n, case.m * case.per_row) / 2, (moved, np.count_nonzero(live))
    if case.mode == "accel":                                                 # alpha1 = 0 on entry: coef = -1, then 0
        assert [r[6] for r in mdl.history] == [0.0, 1.0][:len(mdl.history)]


def probe_entries(case):
    n = case.n
    if n <= 600:
        return range(n)
    rng = np.random.RandomState(n)
    edges = [j for k in range(0, n, 512) for j in (k - 1, k, k + 1) if 0 <= j < n]
    return sorted(set([0, 1, n - 2, n - 1] + edges + list(rng.choice(n, size=8, replace=False))))


@pytest.mark.parametrize("case", CASES, ids=RP.case_id)
def test_every_entry_of_x0_reaches_a_compared_output(case):
    """One entry of x0 moved by 1/2: some compared output of the model moves (every entry for n <= 600; beyond, the first and the last entries,
    the entries either side of every 512-column piece boundary and eight random ones)."""
    _, x0, _, _ = RP.operands(case)
    want = RP.compared_outputs(RP.model(case))
    for j in probe_entries(case):
        x = x0.copy()
        x[j] += 0.5
        mdl = RP.Model(case, x0=x)
        mdl.steps_done = mdl.run(RP.launches_of(case))
        got = RP.compared_outputs(mdl)
        assert len(got) != len(want) or any(not np.array_equal(a, b) for a, b in zip(got, want)), j


# ---- the controller --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=RP.case_id)
def test_the_restated_controller_equals_the_shipped_one(case, shipped_controller):
    """fc_backtrack / fc_alpha / fc_decide / fc_advance / fc_rotate of tests/run_paths.py against csrc/fh_controller.h compiled for the host with
    the DEVICE's square (FcSqMul), on the sums of every attempt of the case: the GPU tier then needs no compiler."""
    mdl = RP.model(case)
    o = RP.run_opts(case, CS.Opts)
    g_kind = 1 if case.kind == "shrink" else 0
    roles, perm = [0, 1, 0, 0, 0, 0, 0], [0, 1, 2, 3, 4]
    accepted = 0
    for sums, tau, bt, st, fwin in mdl.all_sums:
        cst = CS.State(tau_next=st["tau_next"], alpha1=st["alpha1"], max_residual=st["max_residual"], best_quality=st["best_quality"],
                       iteration=st["iteration"], backtracks=st["backtracks"])
        for k, v in enumerate(fwin):
            cst.f_window[k] = v
        reject = CS.backtrack(o, cst, True, sums, tau, bt, mul=True)
        assert reject == RP.fc_backtrack(mdl.o, fwin, st["iteration"], RP.fc_f(True, sums[0]), sums[1], sums[2], tau, bt)
        a = RP.fc_alpha(mdl.o, st["alpha1"], sums[7])
        assert tuple(float(v) for v in a[:3]) == CS.alpha_mul(o, st["alpha1"], sums[7])
        if reject:
            continue
        d, rec = CS.decide(o, cst, True, g_kind, 1.0, sums, tau, bt, mul=True)
        mine = RP.fc_decide(mdl.o, True, g_kind, 1.0, sums, tau, bt, st["alpha1"], st["max_residual"], st["best_quality"])
        assert rec == mine["record"] == mdl.history[accepted]
        for field in ("better", "stop", "restarted"):
            assert bool(getattr(d, field)) == mine[field], field
        for field in ("tau_next", "alpha0", "alpha1", "coef", "f1", "max_residual", "best_quality"):
            assert getattr(d, field) == float(mine[field]), field
        assert (cst.iteration, cst.backtracks, cst.stopped) == (st["iteration"] + 1, st["backtracks"] + bt, int(mine["stop"]))
        assert cst.f_window[(st["iteration"] + 1) % RP.WINDOW_MAX] == float(mine["f1"])
        want_roles, want_perm = CS.rotate(mdl.o.accelerate, mine["better"], roles, perm)
        roles, perm = RP.fc_rotate(bool(mdl.o.accelerate), mine["better"], roles, perm)
        assert (roles, perm) == (want_roles, want_perm)
        accepted += 1
    assert accepted == len(mdl.history) and (roles, perm) == (mdl.roles, mdl.perm)


def test_the_rotation_of_the_buffer_roles_equals_the_shipped_one_from_every_state(shipped_controller):
    seen = collections.Counter()
    for xi in range(3):
        for bi in range(3):
            for ti in range(3):
                if ti in (xi, bi):
                    continue
                for pc in (0, 1):
                    for accel in (0, 1):
                        for better in (0, 1):
                            roles, perm = [xi, ti, bi, pc, pc ^ 1, pc, 0], [2, 0, 1, 4, 3]
                            assert RP.fc_rotate(bool(accel), bool(better), roles, perm) == tuple(CS.rotate(accel, better, roles, perm))
                            seen[(accel, better)] += 1
    assert len(seen) == 4

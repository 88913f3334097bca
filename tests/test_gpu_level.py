"""GPU tier of the clipping-level search's tests (csrc/fh_prox.h; cases, model and inputs: tests/level_cases.py, held to the exact sort-based level
by tests/test_level_cpu.py).  Every kernel the dispatch rule names, at both edges of its range, through the C ABI on the dense operator over a
1 x n zero matrix -- x0, g0 and tau set directly -- in both prox kinds.  On the grid data the level and every output are exact: every assertion
is `==` or np.array_equal.  No case sets the test hooks (the timed-out hand-off and its fall-back: tests/test_gpu_faults.py)."""
import numpy as np
import pytest

import fasta_python_amd as fa
from fasta_python_amd import hip
from tests import level_cases as LC

pytestmark = pytest.mark.gpu

PROX = {"linf": hip.PROX_LINF, "l1ball": hip.PROX_L1BALL}
FWD_SLOTS = (hip.S_FSQ, hip.S_DXG0, hip.S_DX2, hip.S_XH2, hip.S_G02, hip.S_GSUM, hip.S_GMAX, hip.S_RDOT)


def _operator(n):
    op = fa.DenseMatrixMap(np.zeros((1, n)))
    op.ctx.set_loss_lsq(np.zeros(1))
    op.ctx.timing_enable(True)
    return op


@pytest.fixture(scope="module")
def operators():
    """one scratch operator per length, shared by the cases of the module: whatever level a case leaves behind is the next one's guess, and no
    result may depend on it"""
    cache = {}

    def get(n):
        if n not in cache:
            if len(cache) >= 24:
                cache.pop(next(iter(cache))).close()
            cache[n] = _operator(n)
        return cache[n]
    yield get
    for op in cache.values():
        op.close()


def _launch(c, inp, prox):
    """one forward launch of a case: (scalars, xhat, xprox, launches booked under FH_K_LEVEL)"""
    n = inp.x0.size
    c.set_prox(PROX[prox], LC.mu_of(inp, prox))
    c.set_vector(hip.VEC_X0, inp.x0)
    c.set_vector(hip.VEC_G0, inp.g0)
    c.timing_reset()
    s = c.fwd(inp.tau)
    return s, c.get_vector(hip.VEC_XHAT, n), c.get_vector(hip.VEC_XPROX, n), c.timing_get(hip.K_LEVEL)[1]


def _same_bits(a, b):
    return np.array_equal(a, b) and np.array_equal(np.signbit(a), np.signbit(b))


def _check(inp, prox, s, xhat, xprox):
    want_hat = LC.xhat_of(inp)
    level = LC.model(np.abs(want_hat), inp.radius)[0]
    if level > 0.0:
        assert s[hip.S_ALPHA] == level
    else:
        assert not s[hip.S_ALPHA] > 0.0
    assert _same_bits(xhat, want_hat)
    want = LC.prox_of(prox, want_hat, level)
    assert _same_bits(xprox, want)
    assert s[hip.S_GMAX] == np.abs(want).max()
    return level, want


@pytest.mark.parametrize("prox", LC.PROX_KINDS)
@pytest.mark.parametrize("case", LC.cases(), ids=LC.case_id)
def test_level_and_outputs_are_exact(case, prox, operators):
    assert hip.level_shape_for(case.n) == hip.LevelShape(*LC.shape_of(case.n))          # the kernel the id names
    inp = LC.build(case)
    c = operators(case.n).ctx
    s, xhat, xprox, booked = _launch(c, inp, prox)
    assert booked == 1
    level, want = _check(inp, prox, s, xhat, xprox)
    if case.kind in ("radius_is_l1", "radius_above_l1"):
        assert _same_bits(xprox, np.zeros(case.n) if prox == "linf" else LC.xhat_of(inp))
    if case.kind == "radius_zero":
        assert _same_bits(xprox, LC.xhat_of(inp)) if prox == "linf" else not xprox.any()
    if case.kind == "all_equal":
        x0, g0, xh = inp.x0, inp.g0, LC.xhat_of(inp)
        dx = want - x0
        sums = {hip.S_FSQ: 0.0, hip.S_DXG0: np.sum(dx * g0), hip.S_DX2: np.sum(dx * dx), hip.S_XH2: np.sum((want - xh) ** 2), hip.S_G02: np.sum(g0 * g0),
                hip.S_GSUM: np.sum(np.abs(want)), hip.S_GMAX: np.abs(want).max(), hip.S_RDOT: np.sum((x0 - want) * want)}      # (x_accel0 is zero)
        for k in FWD_SLOTS:
            assert s[k] == sums[k], k
    s2, xhat2, xprox2, _ = _launch(c, inp, prox)                                        # again, now from its own level as the guess
    assert np.array_equal(s2, s) and _same_bits(xprox2, xprox) and _same_bits(xhat2, xhat)


@pytest.mark.parametrize("n", LC.EVERY_KIND_AT)
def test_warm_starts_from_any_left_over_level(n):
    assert hip.level_shape_for(n) == hip.LevelShape(*LC.shape_of(n))
    base = LC.build(LC.Case("distinct", n))
    l1 = float(np.abs(LC.xhat_of(base)).sum())
    with_radius = lambda f: base._replace(radius=LC._grid_radius(f * l1))
    other_n = 4097 if n != 4097 else 1025
    # (input, what the level left by the launch BEFORE it is to this launch)
    sequence = [(with_radius(0.9), "none: a fresh context"),
                (with_radius(0.01), "far below the root"),
                (with_radius(0.3), "between the root and the largest entry"),
                (LC.build(LC.Case("dominant", n)), "a level of other data"),
                (LC.build(LC.Case("all_equal", n)), "above every entry: the cold restart inside the warm pass"),
                (LC.build(LC.Case("radius_above_l1", n)), "a level of other data"),
                (with_radius(0.3), "at or below zero"),
                (LC.build(LC.Case("ties", other_n)), "another operator length"),
                (with_radius(0.5), "left by a launch on another operator length")]
    op = _operator(n)
    try:
        c = op.ctx
        left = 0.0
        for k, (inp, what) in enumerate(sequence):
            prox = LC.PROX_KINDS[k % 2]
            if inp.x0.size != c.shape()[1]:                                           # the slot behind the scalar block survives fh_set_matrix
                c.set_matrix(np.zeros((1, inp.x0.size)))
                c.set_loss_lsq(np.zeros(1))
            ax = np.abs(LC.xhat_of(inp))
            if "above every entry" in what:
                assert left > ax.max()
            if "between" in what:
                assert LC.model(ax, inp.radius)[0] < left < ax.max()
            if "far below" in what:
                assert 0.0 < left < LC.model(ax, inp.radius)[0] / 4.0
            if "below zero" in what:
                assert left <= 0.0
            s, xhat, xprox, booked = _launch(c, inp, prox)
            assert booked == 1, what
            _check(inp, prox, s, xhat, xprox)
            left = s[hip.S_ALPHA]
            fresh = _operator(inp.x0.size)
            try:
                s0, xhat0, xprox0, _ = _launch(fresh.ctx, inp, prox)
            finally:
                fresh.close()
            assert np.array_equal(s0, s) and _same_bits(xprox0, xprox) and _same_bits(xhat0, xhat), what
    finally:
        op.close()


@pytest.mark.parametrize("prox", LC.PROX_KINDS)
@pytest.mark.parametrize("n", [4097, 40000])
def test_every_rows_per_pass_form_of_the_forward_kernel_reads_the_same_level(n, prox, operators):
    """k_fwd_dense<R, ., PX_LINF / PX_L1BALL> for R = 4, 8, 16 (FH_TUNE_FWD_ROWS)"""
    inp = LC.build(LC.Case("distinct", n))
    c = operators(n).ctx
    got = []
    try:
        for rows in (4, 8, 16):
            c.set_tuning(hip.TUNE_FWD_ROWS, rows)
            s, xhat, xprox, booked = _launch(c, inp, prox)
            assert booked == 1
            _check(inp, prox, s, xhat, xprox)
            got.append((s, xhat, xprox, c.get_vector(hip.VEC_Z, 1)))
    finally:
        c.set_tuning(hip.TUNE_FWD_ROWS, 0)
    for other in got[1:]:
        assert all(_same_bits(a, b) for a, b in zip(other, got[0]))
    assert not got[0][3].any()                                                        # z = 0 * xprox


STEP_SKIPPED = []


@pytest.mark.parametrize("prox", LC.PROX_KINDS)
@pytest.mark.parametrize("m,n", LC.STEP_SHAPES)
def test_one_pass_step_reads_the_level_the_two_launch_step_reads(m, n, prox):
    """fh_step (fh_fused_body.inc: `*p.px.level`, S_ALPHA) against fh_fwd + fh_adj on exact data.  By design the one-pass launch without acceleration
    leaves FH_S_RDOT zero and reports f in FH_S_FSQ_ADJ: those two slots are not shared with the pair."""
    p = LC.step_problem(m, n)
    mdl = LC.step_model(p, prox)
    op = fa.DenseMatrixMap(p.A)
    try:
        c = op.ctx
        if c.fused_supported() == 0:
            STEP_SKIPPED.append((m, n))
            assert len(set(STEP_SKIPPED)) < len(LC.STEP_SHAPES)
            pytest.skip("no one-pass kernel for this shape on this device")
        mu = p.radius / p.tau if prox == "linf" else p.radius

        def fresh():
            c.set_loss_lsq(p.b)
            c.set_prox(PROX[prox], mu)
            c.set_vector(hip.VEC_X0, p.x0)
            c.init()
        vectors = lambda: [c.get_vector(hip.VEC_XHAT, n), c.get_vector(hip.VEC_XPROX, n), c.get_vector(hip.VEC_Z, m), c.get_vector(hip.VEC_G1, n)]
        fresh()
        assert np.array_equal(c.get_vector(hip.VEC_G0, n), p.g0)
        c.timing_enable(True)
        c.timing_reset()
        s = c.fwd(p.tau)
        a = c.adj(p.tau)
        assert c.timing_get(hip.K_LEVEL)[1] == 1
        two = vectors()
        fresh()
        c.timing_reset()
        f = c.step(p.tau)
        assert c.timing_get(hip.K_LEVEL)[1] == 1
        one = vectors()
        assert f[hip.S_ALPHA] == s[hip.S_ALPHA] == mdl["level"] == 2.0
        for k in (hip.S_FSQ, hip.S_DXG0, hip.S_DX2, hip.S_XH2, hip.S_G02, hip.S_GSUM, hip.S_GMAX):
            assert f[k] == s[k], k
        for k in (hip.S_DXDG, hip.S_DG2, hip.S_XH2_ADJ, hip.S_GSUM_ADJ, hip.S_GMAX_ADJ):
            assert f[k] == a[k], k
        for got, pair, name in zip(one, two, ("xhat", "xprox", "z", "g1")):
            assert _same_bits(got, pair), name
            assert np.array_equal(got, mdl[name]), name
        t = mdl["terms"]
        for k, name in ((hip.S_FSQ, "fsq"), (hip.S_DXG0, "dxg0"), (hip.S_DX2, "dx2"), (hip.S_XH2, "xh2"), (hip.S_G02, "g02"), (hip.S_GSUM, "gsum"),
                        (hip.S_DXDG, "dxdg"), (hip.S_DG2, "dg2")):
            assert f[k] == np.sum(t[name]), name
    finally:
        op.close()

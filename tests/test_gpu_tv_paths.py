"""GPU tests of EVERY instantiation of the 2-D stencil kernels (csrc/fh_tv.h), each against an independent model, all through the C ABI.

The one-pass sweep k_tv_onepass<IDENT, ACCEL, U, NT, NB> has 30 instantiations the host can dispatch; the automatic rules reach three of them
in the earlier tests (a fourth, <1, 0, 2, 0, 1>, only where a solve with no prox happens to run).
tests/tv_paths.py forces each with FH_TUNE_TV_U / _PIPE / _NT (and the chunk height with FH_TUNE_TV_ROWS, the workgroup dealing with
FH_TUNE_TV_XCD) on images of at most 300 x 257 whose geometry hits the seams: wave strips, strip groups, chunks shorter than a trip, every
shape of the NB = 3 rotation, a finaliser that makes a second pass, rows that wrap twice.  The two-launch family (k_fwd_tv_step /
k_adj_tv_step<U, NT>, k_fwd_tv / k_adj_tv<4, NT>) runs over its own tuning grid and its own strip seams.

The reference is tests/tv_paths.py:fbs_step -- one iteration of the reference's loop in NumPy, not another kernel.  With no prox the operands
make every product and every sum of a launch exactly representable whatever the order of summation (tests/test_tv_paths_cpu.py proves it
without a device), so vectors compare with np.array_equal and EVERY scalar of the block with ==: a term dropped at a strip or chunk seam, a
halo lane that owns, the wrong candidate of the finaliser's `plain` selection cannot hide inside a tolerance.  With the TV-ball prox the
vectors still compare with np.array_equal (the model rounds in NumPy's own order, which the kernels reproduce), the maxima with ==, and the
sums within (terms + 4) * 2^-53 * sum|term| of the same terms added in np.longdouble -- the worst case of a float64 sum in any order, below
2e-11 of sum|term| here, where one dropped pixel moves a sum by about 7e-6 of it.

Wall time of the file on an MI355X: 3.6 s (with the mutation runs)."""
import numpy as np
import pytest

import fasta_python_amd as fa
from fasta_python_amd import hip
from oracle import problems as pr
from tests import tv_paths as T

pytestmark = pytest.mark.gpu

SLOT = {name: getattr(hip, name) for name in T.SCALARS}


def tune(c, rows=0, U=0, pipe=0, nt=0, xcd=0):
    for key, value in ((hip.TUNE_TV_ROWS, rows), (hip.TUNE_TV_U, U), (hip.TUNE_TV_PIPE, pipe), (hip.TUNE_TV_NT, nt), (hip.TUNE_TV_XCD, xcd)):
        c.set_tuning(key, value)


def start(c, H, W, prox):
    """fh_init on the case's operands; returns its scalars."""
    x0, b = T.operands(H, W, prox)
    c.set_loss_lsq(b)
    c.set_prox(T.PROX_KIND[prox])
    c.set_vector(hip.VEC_X0, x0)
    return c.init()


def first_bad(name, got, want):
    bad = np.argwhere(got != want)
    if bad.size:
        i = tuple(bad[0])
        return f"{name}: {len(bad)} wrong entries, first at {bad[0]}: {got[i]!r} != {want[i]!r}"
    return None


def assert_vector(c, which, want, tag):
    msg = first_bad(tag, c.get_vector(which, want.size).reshape(want.shape), want)
    assert msg is None, msg


def assert_scalars(scal, m, prox, names, tag):
    """Every named scalar against the model: == with no prox and for the maxima, the summation bound with the TV-ball prox."""
    for name in names:
        got, want = scal[SLOT[name]], T.scalar(m[name])
        print(f"{tag} {name}: got {got!r} model {want!r}" + ("" if prox == T.IDENTITY or name in T.MAXIMA else f" bound {T.sum_bound(m[name]):.3e}"))
        if prox == T.IDENTITY or name in T.MAXIMA:
            assert got == want, f"{tag} {name}: {got!r} != {want!r}"
        else:
            assert abs(np.longdouble(got) - m[name].value) <= T.sum_bound(m[name]), f"{tag} {name}: {got!r} vs {want!r}, bound {T.sum_bound(m[name])!r}"


def assert_launch(c, scal, m, prox, state, tag, names=T.SCALARS):
    """The vectors and the scalar block a launch left, then (after fh_commit) the iterate the next launch starts from."""
    assert_vector(c, hip.VEC_XPROX, m["xprox"], tag + " xprox")
    assert_vector(c, hip.VEC_Z, m["z"], tag + " z")
    assert_scalars(scal, m, prox, [n for n in names if n != "S_RDOT"], tag)
    if state.accel:
        assert_scalars(scal, m, prox, ["S_RDOT"], tag)
        assert (scal[hip.S_RDOT] > T.RESTART_EPS) == (T.scalar(m["S_RDOT"]) > T.RESTART_EPS), f"{tag}: the restart decision differs from the model's"
    c.commit()
    assert_vector(c, hip.VEC_X0, m["x1"], tag + " x1")


def one_pass(c, H, W, prox, state, tag):
    """Bring the context to the state (fh_init, plus one committed accelerated step for a lagged one) and launch."""
    start(c, H, W, prox)
    if state.lagged:
        c.step_accel(T.FIRST_TAU, T.FIRST_COEF, True)
        c.commit()
    tau = T.tau_of(state, prox)
    scal = c.step_accel(tau, state.coef, bool(state.restart)) if state.accel else c.step(tau)
    if not state.accel:
        assert scal[hip.S_RDOT] == 0.0, tag
    assert scal[hip.S_ALPHA] == 0.0 and scal[15] == 0.0, tag
    return scal


# ---- the one-pass sweep ------------------------------------------------------------------------------------------------------------------------
ONEPASS_GROUPS = [(g, prox) for g in T.GEOMETRIES if g.rows for prox in (T.IDENTITY, T.TVBALL)]      # (the automatic rule: its own test below)


@pytest.mark.parametrize("g,prox", ONEPASS_GROUPS, ids=lambda v: T.geometry_id(v) if isinstance(v, T.Geometry) else v)
def test_one_pass_launch_equals_the_model_on_every_instantiation(g, prox):
    """Every state x every (U, PIPE, NT) of this prox [x FH_TUNE_TV_XCD on / off] on one geometry: tests/tv_paths.py:onepass_cases."""
    cases = [c for c in T.onepass_cases() if c.geometry is g and c.prox == prox]
    assert len(cases) == len(T.STATES)
    op = fa.GradDivMap((g.H, g.W))
    try:
        ctx = op.ctx
        assert ctx.fused_supported() == 2
        for case in cases:
            m = T.model(g.H, g.W, prox, case.state.name)
            for U, pipe, nt, xcd in T.onepass_launches(case):
                tune(ctx, g.rows, U, pipe, nt, xcd)
                tag = f"{T.onepass_id(case)} U{U} pipe{pipe} nt{nt} xcd{xcd} {T.onepass_instantiation(prox, case.state.accel, U, pipe, nt)}"
                scal = one_pass(ctx, g.H, g.W, prox, case.state, tag)
                assert_launch(ctx, scal, m, prox, case.state, tag)
    finally:
        op.close()


@pytest.mark.parametrize("prox", [T.IDENTITY, T.TVBALL])
def test_every_tuning_gives_the_same_bits(prox):
    """Several chunks (the last of 2 rows) and two strip groups; all 12 (U, PIPE, NT) under both settings of FH_TUNE_TV_XCD, from the plain state
    and from a lagged one with either restart decision: the same vectors AND the same scalar block, bit for bit.  The partials are slotted by
    logical workgroup id, so the finaliser's order does not depend on the dealing; a lane adds its rows in the same order whatever the trip
    length and the number of trip buffers, and no instantiation may contract a product into a sum that another leaves alone."""
    g = T.GEOMETRY[T.BITS_GEOMETRY]
    op = fa.GradDivMap((g.H, g.W))
    try:
        ctx = op.ctx
        for state in (T.STATE["plain"], T.STATE["keeps"], T.STATE["restarts"]):
            runs = {}
            for U in T.ALL_U:
                for pipe in T.ALL_PIPE:
                    for nt in T.ALL_NT:
                        for xcd in (0, 1, 2):
                            tune(ctx, g.rows, U, pipe, nt, xcd)
                            scal = one_pass(ctx, g.H, g.W, prox, state, "")
                            xp, z = ctx.get_vector(hip.VEC_XPROX, g.H * g.W * 2), ctx.get_vector(hip.VEC_Z, g.H * g.W)
                            ctx.commit()
                            runs[(U, pipe, nt, xcd)] = (scal, xp, z, ctx.get_vector(hip.VEC_X0, g.H * g.W * 2))
            ref = runs[(2, 1, 0, 0)]
            for key, run in runs.items():
                for name, a, b in zip(("scalars", "xprox", "z", "x1"), run, ref):
                    assert np.array_equal(a, b), f"{prox} {state.name} {key} {name}: {first_bad(name, a, b)}"
    finally:
        op.close()


@pytest.mark.parametrize("g", [T.GEOMETRY["auto 40x257"], T.GEOMETRY["auto 130x121"]], ids=T.geometry_id)
def test_the_automatic_rule_with_no_tuning_at_all(g):
    """A context whose tuning was never touched: values only (the instantiation is the automatic rule's business)."""
    for prox in (T.IDENTITY, T.TVBALL):
        op = fa.GradDivMap((g.H, g.W))
        try:
            for state in T.STATES:
                tag = f"{T.geometry_id(g)} {prox} {state.name} untuned"
                scal = one_pass(op.ctx, g.H, g.W, prox, state, tag)
                assert_launch(op.ctx, scal, T.model(g.H, g.W, prox, state.name), prox, state, tag)
        finally:
            op.close()


@pytest.mark.parametrize("prox", [T.IDENTITY, T.TVBALL])
def test_two_launches_back_to_back_leave_the_counters_and_the_workspace_clean(prox):
    """step, commit, step on ONE context with no fh_init in between, 300 workgroups (the finaliser's second pass): the second launch equals the
    model as the first did -- arrival counters back at zero, no stale partial in the workspace.  (The lagged states of the test above are the
    accelerated form of the same: step_accel, commit, step_accel.)"""
    g = T.GEOMETRY[T.BACK_TO_BACK]
    one, two = T.plain_twice(T.reference_number(prox), g.H, g.W, prox)
    plain = T.STATE["plain"]
    op = fa.GradDivMap((g.H, g.W))
    try:
        ctx = op.ctx
        for U, pipe, nt in ((2, 1, 0), (8, 3, 3)):
            tune(ctx, g.rows, U, pipe, nt)
            start(ctx, g.H, g.W, prox)
            for k, m in enumerate((one, two)):
                tag = f"back to back {prox} U{U} launch {k}"
                scal = ctx.step(0.125)
                m = dict(m, **{name: T.as_image(m[name]) for name in ("xprox", "z", "x1")})
                assert_launch(ctx, scal, m, prox, plain, tag)
    finally:
        op.close()


# ---- the two-launch family ---------------------------------------------------------------------------------------------------------------------
TWO_GROUPS = sorted({(c.geometry.name, c.prox) for c in T.two_launch_cases()})


@pytest.mark.parametrize("name,prox", TWO_GROUPS, ids=lambda v: v.replace(" ", "_"))
def test_two_launch_step_equals_the_model_on_every_instantiation(name, prox):
    """fh_fwd + fh_adj, plain and accelerated (the caller applies the restart rule to fh_fwd's dot, as the solver does), over
    FH_TUNE_TV_U x FH_TUNE_TV_NT: k_fwd_tv_step<IDENT, U, NT> and k_adj_tv_step<U, NT> in both `accel` modes."""
    g = T.GEOMETRY[name]
    op = fa.GradDivMap((g.H, g.W))
    try:
        ctx = op.ctx
        for case in (c for c in T.two_launch_cases() if c.geometry is g and c.prox == prox):
            state, tag = case.state, T.two_launch_id(case)
            m = T.model(g.H, g.W, prox, state.name)
            tune(ctx, g.rows, case.U, 0, case.nt)
            start(ctx, g.H, g.W, prox)
            if state.lagged:
                f = ctx.fwd(T.FIRST_TAU)
                assert not f[hip.S_RDOT] > T.RESTART_EPS, tag
                ctx.adj(T.FIRST_TAU, True, T.FIRST_COEF)
                ctx.commit()
            tau = T.tau_of(state, prox)
            f = ctx.fwd(tau)
            assert_scalars(f, m, prox, ("S_FSQ", "S_DXG0", "S_DX2", "S_XH2", "S_G02", "S_RDOT"), tag + " fwd")
            assert_vector(ctx, hip.VEC_XPROX, m["xprox"], tag + " xprox")
            assert_vector(ctx, hip.VEC_Z, m["z"], tag + " z")
            positive = f[hip.S_RDOT] > T.RESTART_EPS
            assert positive == (T.scalar(m["S_RDOT"]) > T.RESTART_EPS), tag
            if state.accel:
                a = ctx.adj(tau, True, 0.0 if (state.restart and positive) else state.coef)
            else:
                a = ctx.adj(tau)
            assert_scalars(a, m, prox, T.ADJ_SCALARS, tag + " adj")
            assert np.array_equal(a[:hip.S_DXDG], f[:hip.S_DXDG]), tag                  # K-adj leaves the forward half of the block alone
            if state.accel:
                assert_vector(ctx, hip.VEC_X1, m["x1"], tag + " x1 before the commit")
            ctx.commit()
            assert_vector(ctx, hip.VEC_X0, m["x1"], tag + " x1")
    finally:
        op.close()


@pytest.mark.parametrize("g,nt", T.plain_pair_cases(), ids=lambda v: T.geometry_id(v) if isinstance(v, T.Geometry) else f"nt{v}")
def test_plain_pair_equals_numpy_rolls_under_both_load_policies(g, nt):
    """k_fwd_tv<4, NT> / k_adj_tv<4, NT> through GradDivMap.__call__ / .H (fh_apply) and fh_init, chunked by FH_TUNE_TV_ROWS."""
    rng = np.random.RandomState(g.H * 1000 + g.W)
    Y, X = rng.randn(g.H, g.W, 2), rng.randn(g.H, g.W)
    x0, b = T.operands(g.H, g.W, T.IDENTITY)
    op = fa.GradDivMap((g.H, g.W))
    try:
        tune(op.ctx, g.rows, 0, 0, nt)
        for k in range(2):                                                              # twice: the counters come back to zero
            assert first_bad("div", op(Y), pr.div(Y)) is None
            assert first_bad("grad", op.H(X), pr.grad(X)) is None
            assert first_bad("div, integers", op(x0), pr.div(x0)) is None
        s = start(op.ctx, g.H, g.W, T.IDENTITY)
        assert s[hip.S_FSQ] == float(((pr.div(x0) - b) ** 2).sum())                     # integers: exact in any order
    finally:
        op.close()


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------
def test_the_tuning_keys_refuse_values_out_of_range():
    op = fa.GradDivMap((8, 8))
    try:
        for key, value, sentence in ((hip.TUNE_TV_U, 3, "TV_U must be"), (hip.TUNE_TV_ROWS, 4097, "TV_ROWS must be"), (hip.TUNE_TV_NT, 4, "TV_NT must be"),
                                     (hip.TUNE_TV_PIPE, 4, "TV_PIPE must be"), (hip.TUNE_TV_XCD, 3, "TV_XCD must be"), (hip.TUNE_TV_U, -2, "TV_U must be"),
                                     (hip.TUNE_TV_ROWS, -1, "TV_ROWS must be"), (hip.TUNE_TV_NT, -1, "TV_NT must be")):
            with pytest.raises(hip.HipError, match=rf"^\[{hip.E_ARG}\].*{sentence}"):
                op.ctx.set_tuning(key, value)
        tune(op.ctx, 4096, 8, 3, 3, 2)                                                  # the ends of every range are accepted
        tune(op.ctx)
    finally:
        op.close()

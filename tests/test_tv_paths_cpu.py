"""CPU tier of the 2-D stencil path tests: the conditions on the INPUTS of tests/test_gpu_tv_paths.py, checked without a device.

* the model: tests/tv_paths.py:fbs_step equals oracle.problems.div / grad, fo.tv_dual_ball and iterations of fo.fasta on the same data (one
  plain iteration, and three accelerated ones, whose third starts from a lagged state (P1, P0, c_prev) as the launches of the GPU tier do);
* exactness: with no prox every vector and every scalar of every case, computed in float64, equals the same quantity in np.longdouble AND in
  scaled integers, bit for bit, and the sum of the MAGNITUDES of the terms of every sum stays at or below 2^52 units of its grid: no
  summation order, chunk split, strip split or fused multiply-add can round;
* the restart rule: both signs of the restart dot occur for every trip length, with either prox; all three arms of the finaliser's `plain`
  predicate occur;
* TV-ball activity: between 20 % and 80 % of the pixels of every TV-ball launch (and of the committed step before it) lie outside the unit ball;
* geometry: every case has the chunks, last-chunk rows, trips, NB = 3 loop passes, strips and grid its name claims, recomputed from
  (H, W, TV_ROWS, U) and the strip widths restated in tests/tv_paths.py -- which csrc/fh_tv.h must still #define;
* coverage: the case lists reach all 30 instantiations of k_tv_onepass the host can dispatch and every two-launch instantiation."""
import os
import re

import numpy as np
import pytest

from oracle import fasta_np as fo
from oracle import problems as pr
from tests import tv_paths as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fasta_python_amd", "csrc")
SHAPES = sorted({(g.H, g.W) for g in T.GEOMETRIES})
SHAPE_IDS = [f"{h}x{w}" for h, w in SHAPES]


# ---- the constants are the kernels' own ----------------------------------------------------------------------------------------------------
def test_the_strip_widths_are_the_kernels_own():
    tv = open(os.path.join(CSRC, "fh_tv.h")).read()
    dev = open(os.path.join(CSRC, "fh_device.h")).read()
    for name in ("TVZ_OWN", "TVS_FWD_OWN", "TVS_ADJ_OWN", "TV_SW"):
        found = re.findall(rf"^#define\s+{name}\s+(\d+)", tv, flags=re.M)
        assert found == [str(getattr(T, name))], (name, found)
    found = re.findall(r"^#define\s+FH_WG\s+(\d+)", dev + tv, flags=re.M)
    assert found == [str(T.FH_WG)], found
    # the owning lanes of the one-pass sweep and its strip stride agree with TVZ_OWN
    assert "lane >= 2u && lane <= 61u" in tv and "(sg * 4u + wave) * TVZ_OWN" in tv and 61 - 2 + 1 == T.TVZ_OWN


def test_the_host_dispatches_what_the_restated_rule_says():
    """launch_tv_onepass names exactly the template arguments tests/tv_paths.py:onepass_instantiation can return."""
    text = open(os.path.join(CSRC, "fh_host_launch.h")).read()
    body = text[text.index("static int launch_tv_onepass"):]
    body = body[:body.index("t_end(c, FH_K_FUSED)")]
    ident = {tuple(int(k) for k in m) for m in re.findall(r"TVZ\((1), ([01]), (\d), (\d), (\d)\)", body)}
    assert ident == {i for i in T.ONEPASS_ALL if i[0] == 1} and len(ident) == 6
    assert "TVZ(0, AC, U, NT, 3); else TVZ(0, AC, U, NT, 1)" in body and "TVZ_NB(AC, 2, NT); else if (tvu == 8) TVZ_NB(AC, 8, NT); else TVZ_NB(AC, 4, NT)" in body
    assert "if (nts) TVZ_U(AC, 2); else TVZ_U(AC, 0)" in body
    assert len(T.ONEPASS_ALL) == 30 and len({i for i in T.ONEPASS_ALL if i[0] == 0}) == 24


# ---- the model against the reference's loop ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(1, 1), (2, 3), (5, 64), (33, 61)])
def test_the_operators_of_the_model_are_the_references(H, W):
    rng = np.random.RandomState(H * 100 + W)
    Y, X = rng.randn(H, W, 2) * 1.5, rng.randn(H, W)
    assert np.array_equal(T.div((Y[..., 0], Y[..., 1])), pr.div(Y))
    assert np.array_equal(T.as_image(T.grad(X)), pr.grad(X))
    assert np.array_equal(T.as_image(T.tv_dual_ball((Y[..., 0], Y[..., 1]))), fo.tv_dual_ball(Y))


def reference_problem(H, W, prox):
    x0, b = T.operands(H, W, prox)
    f = lambda Z: .5 * np.linalg.norm((Z - b).ravel()) ** 2
    gradf = lambda Z: Z - b
    if prox == T.IDENTITY:
        return (pr.div, pr.grad, f, gradf, None, None, x0), x0, b
    return (pr.div, pr.grad, f, gradf, (lambda Y: 0), fo.tv_dual_ball, x0), x0, b


@pytest.mark.parametrize("prox", [T.IDENTITY, T.TVBALL])
@pytest.mark.parametrize("H,W", [(2, 3), (5, 64), (33, 61)])
def test_a_plain_step_of_the_model_is_one_iteration_of_the_reference(H, W, prox):
    """fo.fasta with max_iters = 1; L and tau0 are given, so no RNG is drawn."""
    args, x0, b = reference_problem(H, W, prox)
    tau = 0.125
    want = fo.fasta(*args, max_iters=1, tolerance=0.0, L=8.0, tau0=tau, adaptive=False, accelerate=False, backtrack=False, evaluate_objective=True)
    m = T.fbs_step(T.F64, x0, x0, 0.0, b, tau, 0.0, 0, prox, accel=False)
    assert np.array_equal(T.as_image(m["xprox"]), want.solution)
    np.testing.assert_allclose(np.sqrt(T.scalar(m["S_DX2"])) / tau, want.residuals[0], rtol=1e-14)
    np.testing.assert_allclose(0.5 * T.scalar(m["S_FSQ"]), want.objectives[1], rtol=1e-14)
    np.testing.assert_allclose(0.5 * T.scalar(m["S_FSQ_ADJ"]), want.objectives[1], rtol=1e-14)
    scale = max(np.sqrt(T.scalar(m["S_G02"])), np.sqrt(T.scalar(m["S_XH2_ADJ"])) / tau) + fo.EPS
    np.testing.assert_allclose(np.sqrt(T.scalar(m["S_DX2"])) / tau / scale, want.norm_residuals[0], rtol=1e-13)
    assert T.scalar(m["S_XH2"]) == T.scalar(m["S_XH2_ADJ"]) and T.scalar(m["S_GSUM"]) == T.scalar(m["S_GSUM_ADJ"])
    # the Barzilai-Borwein sums: the reference's own expressions (:253-258) on its own vectors
    x_hat = x0 - tau * pr.grad(pr.div(x0) - b)
    dgrad = pr.grad(pr.div(want.solution) - b) + (x_hat - x0) / tau
    step = want.solution - x0
    np.testing.assert_allclose(T.scalar(m["S_DXDG"]), step.ravel() @ dgrad.ravel(), rtol=1e-13, atol=1e-13 * np.abs(step * dgrad).sum())
    np.testing.assert_allclose(T.scalar(m["S_DG2"]), np.linalg.norm(dgrad.ravel()) ** 2, rtol=1e-13)
    np.testing.assert_allclose(T.scalar(m["S_DXG0"]), step.ravel() @ pr.grad(pr.div(x0) - b).ravel(), rtol=1e-13,
                               atol=1e-13 * float(m["S_DXG0"].mag))
    assert T.scalar(m["S_GMAX"]) == np.abs(want.solution).max()


@pytest.mark.parametrize("restart", [True, False])
@pytest.mark.parametrize("prox", [T.IDENTITY, T.TVBALL])
@pytest.mark.parametrize("H,W", [(2, 3), (5, 64), (33, 61)])
def test_lagged_steps_of_the_model_are_the_references_accelerated_iterations(H, W, prox, restart):
    """Three accelerated iterations of fo.fasta: the second extrapolates, so the third starts from the lagged state (P1, P0, c_prev)."""
    args, x0, b = reference_problem(H, W, prox)
    tau, iters = 0.125, 3
    want = fo.fasta(*args, max_iters=iters, tolerance=0.0, L=8.0, tau0=tau, adaptive=False, accelerate=True, restart=restart, backtrack=False,
                    evaluate_objective=True, record_iterates=True)
    P1, P0, cprev, alpha = x0, x0, 0.0, 1.0
    applied_any = 0
    for k in range(iters):
        coef_of = lambda a0: (a0 - 1) / ((1 + np.sqrt(1 + 4 * a0 ** 2)) / 2)
        m = T.fbs_step(T.F64, P1, P0, cprev, b, tau, coef_of(alpha), int(restart), prox)
        alpha0 = 1.0 if m["restarted"] else alpha
        assert m["applied"] == coef_of(alpha0)
        assert np.array_equal(T.as_image(m["x1"]), want.iterates[k + 1]), k
        np.testing.assert_allclose(np.sqrt(T.scalar(m["S_DX2"])) / tau, want.residuals[k], rtol=1e-13)
        np.testing.assert_allclose(0.5 * T.scalar(m["S_FSQ_ADJ"]), want.objectives[k + 1], rtol=1e-13)
        scale = max(np.sqrt(T.scalar(m["S_G02"])), np.sqrt(T.scalar(m["S_XH2_ADJ"])) / tau) + fo.EPS
        np.testing.assert_allclose(np.sqrt(T.scalar(m["S_DX2"])) / tau / scale, want.norm_residuals[k], rtol=1e-12)
        applied_any += m["applied"] != 0.0
        P0, P1, cprev = P1, T.as_image(m["xprox"]), m["applied"]
        alpha = (1 + np.sqrt(1 + 4 * alpha0 ** 2)) / 2
    assert cprev != 0.0 or restart          # without the restart rule the third iteration did start from a lagged state
    assert applied_any >= (1 if restart else 2)


# ---- exactness -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", SHAPES, ids=SHAPE_IDS)
def test_every_identity_case_is_exact(H, W):
    widest = 0
    for state in T.STATES:
        f64, ld, fx = (T.chain(ns, H, W, T.IDENTITY, state) for ns in (T.F64, T.LONGDOUBLE, T.INTEGER))
        for a, b, c in (zip(f64, ld, fx) if state.lagged else [(f64[1], ld[1], fx[1])]):
            for name in ("xprox", "z", "x1", "x_hat"):
                assert np.array_equal(T.as_image(a[name]), T.as_image(c[name])), (state.name, name)
                assert np.array_equal(np.stack(b[name], -1) if isinstance(b[name], tuple) else b[name], T.as_image(c[name])), (state.name, name)
            for name in T.SCALARS:
                assert T.scalar(a[name]) == T.scalar(c[name]) and b[name].value == T.scalar(c[name]), (state.name, name)
                if name not in T.MAXIMA:
                    assert float(a[name].mag) == float(b[name].mag) == T.scalar(T.Sum(c[name].mag, 0, None)), (state.name, name)
                    widest = max(widest, int(c[name].mag.m))                       # in units of the sum's own grid
            assert a["restarted"] == b["restarted"] == c["restarted"] and a["applied"] == c["applied"]
        if state.lagged:                                                            # the launch starts where the committed step ended
            x0 = T.operands(H, W, T.IDENTITY)[0]
            P1 = T.as_image(f64[0]["xprox"])
            assert np.array_equal(T.as_image(f64[0]["x1"]), P1 + T.FIRST_COEF * (P1 - x0))
    assert widest <= 2 ** 52


@pytest.mark.parametrize("name", [T.BACK_TO_BACK, "xcd 13"])
def test_two_plain_steps_back_to_back_are_exact(name):
    g = T.GEOMETRY[name]
    f64, fx = (T.plain_twice(ns, g.H, g.W, T.IDENTITY) for ns in (T.F64, T.INTEGER))
    for a, c in zip(f64, fx):
        assert all(np.array_equal(T.as_image(a[k]), T.as_image(c[k])) for k in ("xprox", "z", "x1"))
        assert all(T.scalar(a[k]) == T.scalar(c[k]) for k in T.SCALARS)
        assert max(int(c[k].mag.m) for k in T.SCALARS if k not in T.MAXIMA) <= 2 ** 52
    tv = T.plain_twice(T.F64, g.H, g.W, T.TVBALL)
    assert all(0.2 <= T.outside_ball(m["x_hat"]) <= 0.8 for m in tv)


def test_the_model_in_integers_is_not_the_model_in_floats_by_construction():
    """Fx really is integer arithmetic: a sum that float64 cannot hold differs."""
    a = T.Fx.of(np.array([2.0 ** 53, 1.0, -2.0 ** 53]))
    assert a.sum().m == 1 and float(np.array([2.0 ** 53, 1.0]).sum() - 2.0 ** 53) != 1.0
    assert (T.Fx.of(0.375) * T.Fx.of(np.array([3.0]))).to_float()[0] == 1.125 and (T.Fx.of(np.array([3.0])) / T.Fx.of(-0.125)).to_float()[0] == -24.0


# ---- the restart rule ------------------------------------------------------------------------------------------------------------------------
def test_both_restart_branches_and_all_arms_of_the_predicate_occur_for_every_trip_length():
    signs = {(prox, U): set() for prox in (T.IDENTITY, T.TVBALL) for U in T.ALL_U}
    arms = {prox: set() for prox in (T.IDENTITY, T.TVBALL)}
    for c in T.onepass_cases():
        if not c.state.accel or c.geometry.rows == 0:
            continue
        m = T.model(c.geometry.H, c.geometry.W, c.prox, c.state.name)
        positive = T.scalar(m["S_RDOT"]) > T.RESTART_EPS
        arm = "restart" if (c.state.restart and positive) else ("coef == 0" if c.state.coef == 0.0 else "extrapolated")
        assert (arm == "extrapolated") == (m["applied"] != 0.0) and m["restarted"] == (arm == "restart")
        arms[c.prox].add(arm)
        if c.state.restart:
            for U, _, _, _ in T.onepass_launches(c):
                signs[(c.prox, U)].add(positive)
        pixels = c.geometry.H * c.geometry.W
        if c.state.lagged and (pixels >= 3 if c.prox == T.IDENTITY else pixels >= 64):
            assert positive == (c.state.name in ("restarts", "no-restart")), T.onepass_id(c)
    assert all(s == {True, False} for s in signs.values()), signs
    assert all(a == {"restart", "coef == 0", "extrapolated"} for a in arms.values()), arms
    names = {s.name: s for s in T.STATES}
    assert names["no-restart"].restart == 0 and names["no-restart"].coef != 0.0 and names["coef-zero"].coef == 0.0
    assert names["first"].lagged == 0 and names["first"].accel == 1                # c_prev = 0 under ACCEL: the sweep's `lag` is false


# ---- TV-ball activity ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", SHAPES, ids=SHAPE_IDS)
def test_every_tv_ball_launch_has_pixels_on_both_sides_of_the_ball(H, W):
    for state in T.STATES:
        m = T.model(H, W, T.TVBALL, state.name)
        fractions = [T.outside_ball(m["x_hat"])] + ([T.outside_ball(m["first"]["x_hat"])] if m["first"] else [])
        if H * W == 1:
            continue                                     # one pixel: no fraction between 0 and 1 (tests/tv_paths.py)
        assert all(0.2 <= f <= 0.8 for f in fractions), (state.name, fractions)
        # ... and the projection did something: the prox output differs from the forward point exactly on those pixels
        moved = np.any(m["xprox"] != m["x_hat"], axis=-1)
        assert abs(moved.mean() - fractions[0]) < 1e-12


def test_the_tv_ball_operands_are_dyadic_and_the_bound_is_tight():
    x0, b = T.operands(300, 250, T.TVBALL)
    assert np.array_equal(x0 * 4, np.rint(x0 * 4)) and np.array_equal(b * 2, np.rint(b * 2))
    worst = 0.0
    for state in T.STATES:
        m = T.model(300, 250, T.TVBALL, state.name)
        for name in T.SCALARS:
            if name not in T.MAXIMA:
                assert m[name].terms <= 150000
                worst = max(worst, T.sum_bound(m[name]) / float(m[name].mag))
    assert worst < 2e-11 < 1.0 / 150000 / 1000          # a dropped pixel moves a sum by ~1 / terms of sum|term|: far above the bound


# ---- geometry --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", T.GEOMETRIES, ids=T.geometry_id)
def test_every_geometry_is_what_its_name_claims(g):
    got = T.claims_of(g)
    assert g.claim and all(got[k] == v for k, v in g.claim.items()), (g.claim, got)
    assert g.H <= 300 and g.W <= 250 + 7
    rows = g.rows or got["auto_rows"]
    sh = T.sweep_shape(g.H, g.W, rows)
    assert 1 <= sh.last_rows <= rows and (sh.chunks - 1) * rows + sh.last_rows == g.H and sh.grid == sh.strip_groups * sh.chunks
    assert (sh.strips - 1) * T.TVZ_OWN < g.W <= sh.strips * T.TVZ_OWN
    if g.name.startswith("wrap"):
        assert g.H <= 3 and g.W <= 5 and (g.H <= 2 or g.W < 4)          # rows i0 - 2 and i0 + rows + 1 wrap (twice when H = 1); % W with W < 4
    if g.name.startswith("rotation"):
        total, U = got["total"], g.U
        kind = g.name.split(" ", 2)[2]
        assert {"one pass": total < 3 * U, "exact": total == 3 * U, "two passes": 3 * U < total < 6 * U and total % U != 0}[kind]
        assert sh.last_rows == rows                                       # every chunk of the image has that total
    if g.name == "short chunk":
        assert got["last_total"] < g.U and sh.last_rows == 1
    if g.name == "ragged trips":
        assert got["total"] % g.U != 0
    if g.name == "rows above H":
        assert g.rows > g.H
    if g.name.startswith("xcd"):
        on = [T.xcd_order(b, sh.grid, 1) for b in range(sh.grid)]
        assert sorted(on) == list(range(sh.grid))                         # a bijection: every partial slot is written once
        assert [T.xcd_order(b, sh.grid, 0) for b in range(sh.grid)] == list(range(sh.grid))
        assert (on == list(range(sh.grid))) == (got["per"] <= 1)          # the dealing moves something only from 16 workgroups on ...
        assert on[sh.grid - got["kept"]:] == list(range(sh.grid - got["kept"], sh.grid))
    if g.name == "xcd 600":
        assert on != list(range(sh.grid)) and on[1] == 75 and on[8] == 1
    if g.name in ("finaliser second pass", "xcd 600"):
        assert sh.grid > T.FH_WG


def test_the_two_launch_seams_are_the_two_launch_kernels_own():
    """Widths 62 / 63 / 64 (+ 1) are one strip exactly, then one column into the next wave, of k_fwd_tv_step / k_adj_tv_step / the plain pair; four
    times that, the same for a strip group."""
    widths = {g.W for g in T.GEOMETRIES if g.name.startswith("two-launch")}
    for own in (T.TVS_FWD_OWN, T.TVS_ADJ_OWN, T.TV_SW):
        assert {own, own + 1, 4 * own, 4 * own + 1} <= widths
        assert T.sweep_shape(5, own, 3, own).strips == 1 and T.sweep_shape(5, own + 1, 3, own).strips == 2
        assert T.sweep_shape(5, 4 * own, 3, own).strip_groups == 1 and T.sweep_shape(5, 4 * own + 1, 3, own).strip_groups == 2
    two = {c.geometry.name for c in T.two_launch_cases()}
    assert {g.name for g in T.GEOMETRIES if g.name.startswith("two-launch")} <= two
    # their row chunks: fh_fwd walks FH_TUNE_TV_ROWS rows per workgroup too, trips of U rows, a clamped last trip
    assert {"short chunk", "ragged trips", "rows above H", "finaliser second pass"} <= two


# ---- coverage --------------------------------------------------------------------------------------------------------------------------------
def test_the_cases_reach_every_instantiation():
    assert T.reached_onepass() == T.ONEPASS_ALL and len(T.ONEPASS_ALL) == 30
    assert T.reached_two_launch() == T.TWO_LAUNCH_ALL and len(T.TWO_LAUNCH_ALL) == 6 * 2 + 3 * 2 + 2 + 2
    # every one-pass instantiation meets every geometry that forces its tuning, in every state of its ACCEL
    forced = [g for g in T.GEOMETRIES if g.rows]
    for g in forced:
        cases = [c for c in T.onepass_cases() if c.geometry is g]
        assert T.reached_onepass(cases) == T.ONEPASS_ALL, g.name
    # the two-launch step kernels: every (U, NT, prox) under the plain and an accelerated fh_adj
    seen = {(c.U, c.nt, c.prox, bool(c.state.accel)) for c in T.two_launch_cases()}
    assert len(seen) == 3 * 2 * 2 * 2
    for c in T.two_launch_cases():
        assert c.geometry.rows > 0

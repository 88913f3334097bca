"""CPU tier of the bilinear smooth term (fh_set_factorization, csrc/fh_bilinear.h; losses.Factorization, proximal.RowSplit): the fixtures
tests/golden/factor/*.npz were captured from the reference core (scripts/make_factor_golden.py) with the tags' closures and the identity
operator; the NumPy oracle and `fasta(None, None, ..., backend="numpy")` must reproduce them bit for bit, the closures must be the reference
example's own, operand recognition must name what the device does not serve, the exported launch geometry must hold what every GPU-tier case
claims of it, the exact inputs must be exact, and nothing may fall back when there is no GPU.  No GPU."""
import os
import warnings

import numpy as np
import pytest
from numpy import linalg as la

import fasta_python_amd as fa
from fasta_python_amd import hip, solver
from fasta_python_amd import stopping as fstop
from oracle import fasta_np as fo
from tests import factor_cases as FC


def assert_same_run(c, z):
    assert c.iteration_count == int(z["iteration_count"]) and c.backtracks == int(z["backtracks"])
    for field in FC.HISTORIES:
        assert np.array_equal(getattr(c, field), z[field], equal_nan=True), field
    assert np.array_equal(c.solution, z["solution"])


# ---- the fixture set ---------------------------------------------------------------------------------------------------------------------------
def test_the_fixture_set_is_the_one_the_script_describes():
    names = [row[0] for row in FC.capture_script().case_table()]
    assert sorted(names) == FC.FIXTURES == FC.EXPECTED
    assert all(os.path.getsize(os.path.join(FC.FACTOR, n + ".npz")) < 100 << 10 for n in FC.FIXTURES)


def test_the_fixtures_cover_the_modes_the_column_layouts_the_prox_forms_and_the_prefix_condition():
    kinds, lbs, modes = set(), set(), {}
    for name in FC.FIXTURES:
        meta, z, d = FC.load(name)
        kinds.add(meta["kind"])
        lbs.add(FC.lb_of(d["x0"].shape[1]))
        m, (ms, n) = int(d["m"]), d["S"].shape
        assert ms == m and d["x0"].shape[0] == m + n and d["S"].dtype == np.float64, name
        assert z["solution"].shape == d["x0"].shape and meta["options"]["L"] > 0 and meta["options"]["tau0"] > 0, name
        k, whole = FC.compared_prefix(meta, z)
        o = meta["options"]
        mode = "adaptive" if o["adaptive"] else ("accelerated" if o["accelerate"] else "plain")
        modes[mode] = max(modes.get(mode, 0), 10 ** 9 if whole else k)
        assert whole or k >= FC.MIN_PREFIX, name                       # every fixture is compared whole, or on at least 30 iterations
    assert kinds == {"nnf", "nonneg", "gnone"} and lbs == {2, 4, 8, 16}
    assert set(modes) == {"adaptive", "accelerated", "plain"} and min(modes.values()) >= FC.MIN_PREFIX
    meta, z, d = FC.load("nnf_60x40x5_backtracks")
    kept = int(z["backtracks"]) if FC.compared_prefix(meta, z)[1] else meta["backtracks_at_divergence"]
    assert kept >= FC.MIN_BACKTRACKS
    meta, z, d = FC.load("nnf_60x40x5_plain")
    assert int(z["iteration_count"]) == 300                              # plain, capped at 300


@pytest.mark.parametrize("name", FC.EXPECTED)
def test_twin_parting_iteration_is_recomputed(name):
    """The basis for what the device is held to: the oracle and a twin of itself -- rows of X and of S, rows of Y and columns of S, and the K
    columns permuted; same L, same tau0 -- agree on every step size up to the stored iteration."""
    meta, z, d = FC.load(name)
    ms = FC.capture_script()
    assert ms.twin_divergence(meta["kind"], d, meta["options"]) == meta["twin_divergence"]
    k, whole = FC.compared_prefix(meta, z)
    if not whole:
        cut = ms.run_oracle(meta["kind"], d, meta["options"], max_iters=k, tolerance=0.0)
        assert cut.iteration_count == k and cut.backtracks == meta["backtracks_at_divergence"]
        assert np.array_equal(cut.stepsizes[:k], z["stepsizes"][:k])


@pytest.mark.parametrize("name", FC.EXPECTED)
def test_oracle_and_the_numpy_backend_reproduce_the_fixture_bit_for_bit(name):
    meta, z, d = FC.load(name)
    ms = FC.capture_script()
    assert_same_run(ms.run_oracle(meta["kind"], d, meta["options"]), z)
    f, gradf, g, proxg, x0 = ms.operands(fa, meta["kind"], d)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        c = fa.fasta(None, None, f, gradf, g, proxg, x0, verbose=False, backend="numpy", **ms.resolve(meta["options"], fstop))
    assert_same_run(c, z)


# ---- the closures -------------------------------------------------------------------------------------------------------------------------------
def test_closures_are_the_examples_forms():
    rng = np.random.RandomState(4)
    N, n, K, mu = 23, 17, 5, 0.7
    S, Z = rng.randn(N, n), rng.randn(N + n, K)
    fz, reg = fa.Factorization(S), fa.RowSplit(N, fa.Shrink(mu), fa.Box(0, 1))
    # examples/nn_factorization.py:48-61, restated
    f = lambda Z: .5 * la.norm((S - Z[:N, ...] @ Z[N:, ...].T).ravel())**2

    def gradf(Z):
        X = Z[:N, ...]
        Y = Z[N:, ...]
        d = X @ Y.T - S
        return np.concatenate((d @ Y, d.T @ X))

    g = lambda Z: mu * la.norm(Z[:N, ...].ravel(), 1)
    proxg = lambda Z, t: np.concatenate((fa.proximal.shrink(Z[:N, ...], t * mu), np.minimum(np.maximum(Z[N:, ...], 0), 1)))
    assert abs(fz.f(Z) - f(Z)) <= 1e-12 * abs(f(Z)) and fz(Z) == fz.f(Z)
    np.testing.assert_allclose(fz.gradf(Z), gradf(Z), rtol=1e-12, atol=1e-12)
    assert abs(reg.g(Z) - g(Z)) <= 1e-12 * g(Z)
    assert np.array_equal(reg.prox(Z, 0.3), proxg(Z, 0.3)) and np.array_equal(reg(Z, 0.3), proxg(Z, 0.3))       # bit for bit
    # the gradient is the derivative of f
    E = rng.randn(*Z.shape)
    h = 1e-6
    assert abs((fz.f(Z + h * E) - fz.f(Z - h * E)) / (2 * h) - np.sum(fz.gradf(Z) * E)) <= 1e-6 * abs(np.sum(fz.gradf(Z) * E))
    # each half of RowSplit is the tag of that half; g_from_sums is the top tag's
    for top in (fa.NoProx(), fa.Shrink(0.4), fa.NonNeg(), fa.Box(-0.2, 0.5)):
        for bottom in (fa.NoProx(), fa.NonNeg(), fa.Box(0.1, 0.9)):
            rs = fa.RowSplit(N, top, bottom)
            out = rs.prox(Z, 0.3)
            assert np.array_equal(out[:N], top.prox(Z[:N], 0.3)) and np.array_equal(out[N:], bottom.prox(Z[N:], 0.3))
            assert rs.g(Z) == top.g(Z[:N]) and rs.g_from_sums(3.0, 2.0) == top.g_from_sums(3.0, 2.0)
    assert reg.kind == hip.PROX_ROWSPLIT == 9 and fz.f_from_device(2.5) == 2.5


def test_tags_refuse_what_they_cannot_hold():
    with pytest.raises(ValueError, match="2-D matrix S"):
        fa.Factorization(np.zeros(5))
    with pytest.raises(ValueError, match="float64 matrix S"):
        fa.Factorization(np.zeros((3, 4), dtype=np.float32))
    with pytest.raises(ValueError, match="bottom rows take NoProx, NonNeg or Box"):
        fa.RowSplit(3, fa.Shrink(1.0), fa.Shrink(1.0))                    # a bottom tag with a nonzero g
    with pytest.raises(ValueError, match="top rows take NoProx, Shrink, NonNeg or Box"):
        fa.RowSplit(3, fa.L1Ball(1.0), fa.Box(0, 1))
    with pytest.raises(ValueError, match="two proximal"):
        fa.RowSplit(3, None, fa.Box(0, 1))
    with pytest.raises(ValueError, match=r"takes an unknown of shape \(7, K\), K <= 16"):
        fa.BilinearMap(fa.Factorization(np.zeros((3, 4))), (7, 17))
    with pytest.raises(ValueError, match="losses.Factorization only"):
        fa.proximal.device_prox(fa.RowSplit(3, fa.Shrink(1.0), fa.Box(0, 1)), np.zeros((7, 2)), 0.1)
    B = fa.BilinearMap(fa.Factorization(np.zeros((3, 4))), (7, 2))        # lazy: no device needed; the identity on host arrays
    V = np.arange(14.0).reshape(7, 2)
    assert np.array_equal(B(V), V) and np.array_equal(B.H(V), V) and B.shape == (7, 7) and B.rhs == 2


# ---- recognition --------------------------------------------------------------------------------------------------------------------------------
def test_unrecognised_names_what_is_refused():
    S = np.zeros((5, 4))
    fz, reg, Z0 = fa.Factorization(S), fa.RowSplit(5, fa.Shrink(1.0), fa.Box(0, 1)), np.zeros((9, 3))
    why = lambda *a: solver._unrecognised(*a)
    assert why(None, None, fz.f, fz.gradf, reg.g, reg.prox, Z0) is None
    assert why(None, None, fz.f, fz.gradf, None, None, Z0) is None
    for tag in (fa.Shrink(1.0), fa.NonNeg(), fa.Box(0, 1), fa.NoProx()):
        assert why(None, None, fz.f, fz.gradf, tag.g, tag.prox, Z0) is None
    assert "A must be None" in why(np.eye(9), None, fz.f, fz.gradf, reg.g, reg.prox, Z0)
    assert "of one losses.Factorization" in why(None, None, fz.f, fa.Factorization(S).gradf, reg.g, reg.prox, Z0)
    assert "Z0 has shape (9,)" in why(None, None, fz.f, fz.gradf, reg.g, reg.prox, np.zeros(9))
    assert "shape (8, 3)" in why(None, None, fz.f, fz.gradf, reg.g, reg.prox, np.zeros((8, 3)))
    assert "at most 16 columns" in why(None, None, fz.f, fz.gradf, reg.g, reg.prox, np.zeros((9, 17)))
    other = fa.RowSplit(4, fa.Shrink(1.0), fa.Box(0, 1))
    assert "splits at row 4, the factorization at m = 5" in why(None, None, fz.f, fz.gradf, other.g, other.prox, Z0)
    for tag, word in ((fa.LinfProx(1.0), "level-search"), (fa.L1Ball(1.0), "level-search"), (fa.TVDualBall(), "level-search"),
                      (fa.GroupShrink(1.0), "row-norm"), (fa.RowBall(1.0), "row-norm")):
        assert word in why(None, None, fz.f, fz.gradf, tag.g, tag.prox, Z0) and type(tag).__name__ in why(None, None, fz.f, fz.gradf, tag.g, tag.prox, Z0)
    assert "one proximal.* tag" in why(None, None, fz.f, fz.gradf, lambda Z: 0, reg.prox, Z0)
    # RowSplit with another loss
    ls, q = fa.LeastSquares(np.zeros(9)), fa.Quadratic(np.eye(9))
    assert "factorization loss only" in why(np.eye(9), None, ls.f, ls.gradf, reg.g, reg.prox, np.zeros(9))
    assert "factorization loss only" in why(None, None, q.f, q.gradf, reg.g, reg.prox, np.zeros((9, 3)))
    with pytest.raises(TypeError, match=r"fasta\(backend='hip'\): .*at most 16 columns"):
        fa.fasta(None, None, fz.f, fz.gradf, reg.g, reg.prox, np.zeros((9, 17)), backend="hip")


def test_no_gpu_is_an_error_not_a_fallback():
    try:
        ndev = hip.device_count()
    except hip.HipError:
        ndev = 0
    S = np.ones((5, 4))
    fz, reg, Z0 = fa.Factorization(S), fa.RowSplit(5, fa.Shrink(1.0), fa.Box(0, 1)), np.full((9, 3), 0.5)
    from fasta_python_amd.examples.nn_factorization import NNFactorizationProblem
    p, inits = NNFactorizationProblem.construct(M=12, N=9, K=2, seed=1, backend="hip")
    if ndev == 0:
        for form in ((None, None), (None,)):
            with pytest.raises(hip.HipError):
                fa.fasta(*form, fz.f, fz.gradf, reg.g, reg.prox, Z0, verbose=False)
        with pytest.raises(hip.HipError):
            p.solve(inits)
    else:
        c = fa.fasta(None, None, fz.f, fz.gradf, reg.g, reg.prox, Z0, verbose=False, L=10.0, tau0=0.02, max_iters=20)
        assert c.solution.shape == (9, 3) and np.isfinite(c.solution).all()


def test_example_constructs_in_the_reference_order_and_solves_on_the_host():
    from fasta_python_amd.examples.nn_factorization import NNFactorizationProblem
    p, (X0, Y0) = NNFactorizationProblem.construct(M=30, N=20, K=4, seed=5, backend="numpy")
    np.random.seed(5)                                                    # examples/nn_factorization.py:80-94, restated
    X = np.random.rand(30, 4)
    Y = np.random.rand(20, 4)
    X *= np.random.rand(30, 4) > 0.75
    S = X @ Y.T + 0.1 * np.random.randn(30, 20)
    assert np.array_equal(p.S, S) and not X0.any() and np.array_equal(Y0, np.random.rand(20, 4)) and p.mu == 1.0
    L = float(la.norm(S, 2))
    opts = dict(L=L, tau0=(2 / L) / 10, evaluate_objective=True, max_iters=60)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        (Xs, Ys), c = p.solve((X0, Y0), opts)
        fz, reg = fa.Factorization(S), fa.RowSplit(30, fa.Shrink(1.0), fa.Box(0, 1))
        t = fa.fasta(None, None, fz.f, fz.gradf, reg.g, reg.prox, np.concatenate((X0, Y0)), backend="numpy", verbose=False, **opts)
    assert Xs.shape == (30, 4) and Ys.shape == (20, 4) and Ys.min() >= 0 and Ys.max() <= 1
    assert np.array_equal(t.solution, c.solution) and np.array_equal(t.objectives, c.objectives)       # the tags ARE the closures
    assert c.objectives[c.iteration_count] < c.objectives[0]
    construct_default = NNFactorizationProblem.construct.__defaults__
    assert construct_default[:6] == (800, 200, 10, 0.75, 0.1, 1.0)


# ---- geometry ---------------------------------------------------------------------------------------------------------------------------------------
def needs_library():
    if not os.path.exists(hip.LIB_PATH):
        pytest.fail("libfasta_hip.so is not built: python __graft_entry__.py")


@pytest.mark.parametrize("case", FC.cases(), ids=FC.case_id)
def test_exported_geometry_holds_what_the_gpu_cases_claim(case):
    needs_library()
    sh = hip.bilinear_shape(case.m, case.n, case.K, grid_cap=case.cap, nt_loads=case.nt)
    assert sh == FC.expected_shape(case), (sh, FC.expected_shape(case))
    panels, last_rows, tiles, live, uneven = FC.claimed_path(case)
    assert (sh.row_panels, sh.last_rows, sh.col_tiles, sh.last_live_lanes) == (panels, last_rows, tiles, live)
    assert (sh.tiles_max != sh.tiles_min) == uneven and sh.LB == case.LB and sh.RB * sh.LB == FC.ns_of(case.LB)


def test_the_case_set_covers_what_the_issue_asks_of_it():
    needs_library()
    shapes = {c: hip.bilinear_shape(c.m, c.n, c.K, grid_cap=c.cap, nt_loads=c.nt) for c in FC.cases()}
    wide = [s for c, s in shapes.items() if (c.m, c.n) == FC.WIDE]
    # more than one row panel and column tile, each with a ragged last one; a grid cap that does not divide the tiles; nearly every lane idle
    assert all(s.row_panels > 1 and s.col_tiles > 1 and s.last_rows < s.tile_rows and s.last_live_lanes <= 3 for s in wide)
    assert all(s.last_live_rows < s.RB for s in wide if s.RB > 1)         # the last trip down the last panel is ragged wherever a trip has several rows
    assert all((s.row_panels * s.col_tiles) % s.grid != 0 and s.tiles_max == s.tiles_min + 1 for s in wide)
    assert {c.m for c in FC.cases()} >= {1} and {c.n for c in FC.cases()} >= {1} and {c.K for c in FC.cases()} >= {1}
    for LB in FC.ALL_LB:
        assert {c.K for c in FC.cases() if c.LB == LB and (c.m, c.n) == FC.WIDE} == set(FC.columns_of(LB))
        assert {c.nt for c in FC.cases() if c.LB == LB and (c.m, c.n) == FC.WIDE} == {0, 1}
        assert {c.kind for c in FC.cases() if c.LB == LB} == set(FC.TOP_KINDS)
    assert any(c.cap == 0 and c.nt == -1 and (c.m, c.n) == FC.CONTROL for c in FC.cases())


def test_geometry_rule_fills_the_device_and_bounds_the_partials():
    needs_library()
    for m, n in ((16384, 16384), (32768, 32768), (65536, 4096)):
        for K in (1, 2, 4, 8, 10, 16):
            s = hip.bilinear_shape(m, n, K)
            assert s.row_panels * s.col_tiles >= 512 and s.grid == 512 and s.NT == 1
            frac = (s.gx_bytes + s.gy_bytes) / (m * n * 8)
            assert abs(frac - s.LB * (1 / 512 + 1 / s.tile_rows)) < 1e-12 and frac <= 16 * (1 / 512 + 1 / 1024)
    s = hip.bilinear_shape(800, 200, 10)                                  # the example: 50 panels of 16 rows, not a handful
    assert (s.row_panels, s.col_tiles, s.grid) == (50, 1, 50)
    with pytest.raises(hip.HipError, match="1 to 16 columns"):
        hip.bilinear_shape(10, 10, 17)
    with pytest.raises(hip.HipError, match="non-empty"):
        hip.bilinear_shape(0, 10, 1)
    with pytest.raises(hip.HipError, match="below 2\\^27"):
        hip.bilinear_shape(1 << 27, 10, 1)
    with pytest.raises(hip.HipError, match="would reach 4 GiB"):
        hip.bilinear_shape(1 << 26, 600, 16)


# ---- exactness --------------------------------------------------------------------------------------------------------------------------------------
UNIT = {"init": 2.0 ** -6, "fwd": 2.0 ** -10, "adj": 2.0 ** -12, "adja": 2.0 ** -24}


@pytest.mark.parametrize("m,n,K,kind", sorted({(c.m, c.n, c.K, c.kind) for c in FC.cases()}))
def test_the_exact_step_is_exact(m, n, K, kind):
    """float64 == longdouble == integer arithmetic for every matrix product and every sum of the model, and every sum of magnitudes stays
    below 2^53 units: neither the order of summation nor a fused multiply-add can matter, so the kernels are compared with ==."""
    S, Z0, G0 = FC.exact_inputs(m, n, K)
    assert set(np.unique(S)) <= {-1.0, 0.0, 1.0} and (m * n < 5000 or 0.7 < np.mean(S == 0) < 0.8)
    assert np.array_equal(2 * Z0, np.round(2 * Z0)) and np.array_equal(2 * G0, np.round(2 * G0))
    terms = {}
    a = FC.model_step(S, Z0, G0, m, FC.top_tag(kind), FC.BOTTOM, terms=terms)
    b = FC.model_step(S, Z0, G0, m, FC.top_tag(kind), FC.BOTTOM, dtype=np.longdouble)
    for name in FC.MATRICES:
        assert np.array_equal(a[name], b[name].astype(np.float64)) and np.array_equal(a[name].astype(np.longdouble), b[name]), name
    Si = S.astype(np.int64)
    # d = X Y^T - S and both halves of the gradient once more in integers: the three points are multiples of 1/2, 1/4 and 1/16
    for Z, scale, d, G in ((Z0, 2, a["D"][0], a["GINIT"]), (a["XPROX"], 4, a["D"][1], a["G1"]), (a["X1"], 16, a["D"][2], a["G1A"])):
        Zi = Z * scale
        assert np.array_equal(Zi, np.round(Zi))
        Xi, Yi = Zi[:m].astype(np.int64), Zi[m:].astype(np.int64)
        di = Xi @ Yi.T - Si * scale * scale
        assert np.array_equal(di / (scale * scale), d)
        assert np.array_equal(np.concatenate((di @ Yi, di.T @ Xi)) / scale ** 3, G)
        bound = np.concatenate((np.abs(di) @ np.abs(Yi), np.abs(di).T @ np.abs(Xi)))
        assert float(np.max(bound)) < 2.0 ** 53 and float(np.max(np.abs(Xi) @ np.abs(Yi).T)) < 2.0 ** 53
    for blk in FC.BLOCKS:
        for slot, value in a[blk].items():
            assert value == float(b[blk][slot]), (blk, slot)
            t = terms[(blk, slot)] / UNIT[blk]
            assert np.array_equal(t, np.round(t)) and float(np.sum(np.abs(t))) < 2.0 ** 53, (blk, slot)
            if slot not in (hip.S_GMAX, hip.S_GMAX_ADJ):
                total = int(np.sum(t.astype(np.int64).astype(object)))
                half = 0.5 if slot in (hip.S_FSQ, hip.S_FSQ_ADJ) else 1.0
                assert total * UNIT[blk] * half == value, (blk, slot)
    assert a["fwd"][hip.S_RDOT] == -a["fwd"][hip.S_DX2]                     # x_accel0 = x0 right after fh_init
    if (m, n) == FC.WIDE:
        assert not np.array_equal(a["XPROX"][m:], a["XHAT"][m:])           # BOX(0, 1) clips the bottom rows at this scale
        assert kind == "none" or not np.array_equal(a["XPROX"][:m], a["XHAT"][:m])
        # what the three value-only mutations of DESIGN.md section 14 would change is visible in exact numbers: d without -S, GY over one
        # panel fewer (the last 7 rows of S feed GY), FH_S_GSUM over all rows
        assert np.any(S != 0) and np.any(a["D"][1][-7:].T @ a["XPROX"][m - 7:m] != 0)
        assert a["fwd"][hip.S_GSUM] != np.sum(np.abs(a["XPROX"]))

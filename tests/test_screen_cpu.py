"""Host tests of gap-safe screening: the statement (fasta_python_amd/certificates.py: screen), the kappa rule against the library's export, the
screened path on the host loop, and that header, library and binding name the four entry points.  Cases: tests/screen_cases.py.

Bounds.  Safety is a property, not a tolerance: a discarded feature is exactly zero in a solution solved to a relative gap of 1e-12.  Exactness: on
dyadic data norms2 equals its rational evaluation with `==` and the mask a 50-digit evaluation of the same inequality, no feature standing within
2^-30 relative of the threshold (asserted).  The path: two points whose gap is at most e = gap_tolerance * f0 both lie within sqrt(2 e) of the
optimum in A x, f being 1-strongly convex there, hence within 2 sqrt(2 e) of each other."""
import ctypes
import math
import os
import warnings
from fractions import Fraction

import numpy as np
import pytest

import fasta_python_amd as fa
from fasta_python_amd import certificates as ce
from fasta_python_amd import hip
from tests import screen_cases as S


def solve(A, loss, reg, x0, **opts):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fa.fasta(A, A.T, loss.f, loss.gradf, reg.g, reg.prox, x0, backend="numpy", verbose=False, **opts)


def safety_problem(seed, group):
    rng = np.random.RandomState(1000 * group + seed)
    m, n, L = rng.randint(20, 61), rng.randint(80, 301), (1, 3)[seed % 2]
    A = rng.randn(m, n) / math.sqrt(m)
    shape = (n, L) if (group or L > 1) else (n,)
    xt = np.zeros(shape)
    xt[rng.permutation(n)[:6]] = rng.randn(*((6,) + shape[1:]))
    b = A @ xt + 0.05 * rng.randn(*((m,) + shape[1:]))
    loss = fa.LeastSquares(b)
    prox_class = fa.GroupShrink if group else fa.Shrink
    mu = rng.uniform(0.2, 0.7) * ce.critical_mu(A, loss, prox_class, shape)
    return A, loss, prox_class(mu), shape


@pytest.mark.parametrize("group", [0, 1], ids=["shrink", "group"])
def test_no_discarded_feature_is_nonzero_in_the_solution(group):
    discarded = 0
    for seed in range(40):
        A, loss, reg, shape = safety_problem(seed, group)
        np.random.seed(seed)
        conv = solve(A, loss, reg, np.zeros(shape), stop_rule=fa.DualityGap(1e-12, 10), max_iters=100000)
        assert conv.certificate.relative <= 1e-12, (seed, conv.certificate.relative)
        support = np.any(conv.solution.reshape(shape[0], -1) != 0, axis=1)
        for iters in (1, 3, 10, 30, 100):
            np.random.seed(seed)
            x = solve(A, loss, reg, np.zeros(shape), tolerance=0.0, max_iters=iters).solution
            sc = ce.screen(A, loss, reg, x)
            assert sc.radius > 0 and sc.keep.shape == (shape[0],)
            assert not np.any(support & ~sc.keep), (seed, iters, np.flatnonzero(support & ~sc.keep))
            discarded += int(np.count_nonzero(~sc.keep))
    assert discarded > 0                                  # the rule does discard on these problems: the property above is not vacuous


@pytest.mark.parametrize("group", [0, 1], ids=["shrink", "group"])
def test_at_zero_from_the_critical_mu_on_the_radius_is_zero_and_every_feature_inside_the_ball_goes(group):
    for seed in range(8):
        A, loss, reg, shape = safety_problem(seed, group)
        mu_c = ce.critical_mu(A, loss, type(reg), shape)
        g = (A.T @ loss.gradf(np.zeros_like(loss.b))).reshape(shape[0], -1)
        size = np.sqrt(np.sum(g * g, axis=1)) if group else np.max(np.abs(g), axis=1)
        for mu in (mu_c, 2.0 * mu_c):
            sc = ce.screen(A, loss, type(reg)(mu), np.zeros(shape))
            assert sc.radius == 0.0 and sc.certificate.gap == 0.0
            np.testing.assert_array_equal(~sc.keep, size < mu)
            assert np.count_nonzero(sc.keep) == (1 if mu == mu_c else 0)


def quarter_problem(m, n, L, seed, group):
    """entries k/4, small integers"""
    rng = np.random.RandomState(seed)
    A = rng.randint(-4, 5, size=(m, n)) / 4.0
    cols = () if L == 1 and not group else (L,)
    b = rng.randint(-8, 9, size=(m,) + cols) / 4.0
    x = np.zeros((n,) + cols)
    x[rng.permutation(n)[:3]] = rng.randint(-2, 3, size=(3,) + cols) / 4.0
    return A, b, x


EXACT = [(7, 40, 1, False), (20, 33, 3, False), (16, 64, 2, True), (33, 17, 3, True), (257, 300, 1, False)]


@pytest.mark.parametrize("m,n,L,group", EXACT)
def test_on_dyadic_data_the_norms_are_exact_and_the_mask_is_the_exact_inequalitys(m, n, L, group):
    A, b, x = quarter_problem(m, n, L, seed=m + n + L, group=group)
    loss = fa.LeastSquares(b)
    prox_class = fa.GroupShrink if group else fa.Shrink
    dn = ce.duality_gap(A, loss, prox_class(1.0), x).dual_norm
    exact = S.exact_norms2(A)
    seen = set()
    # away from a solution the gap is large and nothing goes; at x = 0 just below the critical mu the radius is sqrt(2 f0) (1 - s) and most features go
    for xs, mus in ((x, (dn / 2.0, dn / 8.0, 2.0 * dn)), (np.zeros_like(x), None)):
        if mus is None:
            dz = ce.duality_gap(A, loss, prox_class(1.0), xs).dual_norm
            mus = (dz * 63 / 64, dz * 15 / 16, dz * 3 / 4, dz, 2.0 * dz)
        for mu in mus:
            reg = prox_class(mu)
            sc = ce.screen(A, loss, reg, xs)
            assert [Fraction(float(v)) for v in sc.norms2] == exact
            g = A.T @ (A @ xs - b)
            want, margin = S.decimal_mask(sc.certificate, g, sc.norms2, mu, ce.screen_kappa(m, n, L), group)
            if not (mu == mus[-2] and not xs.any()):      # (at the critical mu itself the feature that attains it stands ON the threshold, and is kept)
                assert margin > 2.0 ** -30, (mu, margin)
            np.testing.assert_array_equal(sc.keep, want)
            seen.add((bool(sc.keep.all()), 0 < np.count_nonzero(sc.keep) < n))
    assert seen == {(True, False), (False, True)} or seen == {(True, False), (False, True), (False, False)}


def test_norms_of_a_sparse_matrix_and_of_a_map_and_what_is_refused():
    from scipy import sparse as sp
    A, b, x = quarter_problem(30, 50, 1, seed=3, group=False)
    A = A * (np.random.RandomState(0).rand(30, 50) < 0.3)
    Sm = sp.csr_matrix(A)
    loss, reg = fa.LeastSquares(b), fa.Shrink(0.5)
    want = ce.screen(A, loss, reg, x)
    for form in (Sm, Sm.tocsc(), fa.DenseMatrixMap(A), fa.SparseMatrixMap(Sm)):
        got = ce.screen(form, loss, reg, x)
        np.testing.assert_array_equal(got.norms2, want.norms2)
        np.testing.assert_array_equal(got.keep, want.keep)
        assert got.radius == want.radius and tuple(got.certificate) == tuple(want.certificate)
    general = fa.LinearMap(lambda v: A @ v, lambda w: A.T @ w, (50,), (30,))
    with pytest.raises(TypeError, match="a general map cannot give its columns"):
        ce.screen(general, loss, reg, x)
    with pytest.raises(TypeError, match="stated for losses.LeastSquares"):
        ce.screen(A, fa.LogisticLoss(np.where(b > 0, 1.0, -1.0)), reg, x)
    with pytest.raises(TypeError, match="proximal.Shrink and proximal.GroupShrink"):
        ce.screen(A, loss, fa.NonNeg(), x)


def test_the_guard_keeps_a_cancelling_gap_from_shrinking_the_radius():
    """Near the optimum P - D cancels: the computed gap may even be <= 0; gap_safe stays above what rounding can have taken."""
    A, loss, reg, shape = safety_problem(3, 0)
    np.random.seed(0)
    conv = solve(A, loss, reg, np.zeros(shape), stop_rule=fa.DualityGap(0.0, 50), max_iters=20000)
    cert = conv.certificate
    kappa = ce.screen_kappa(A.shape[0], A.shape[1], 3 if len(shape) == 2 else 1)
    gs = ce.gap_safe(cert, kappa)
    assert cert.relative < 1e-13 and gs >= kappa * 2.0 ** -52 * cert.primal and gs > 10 * abs(cert.gap)      # the guard, not the cancelled difference, sets the radius
    sc = ce.screen(A, loss, reg, conv.solution)
    support = np.any(conv.solution.reshape(shape[0], -1) != 0, axis=1)
    assert sc.radius > 0 and not np.any(support & ~sc.keep)


SIDES = (1, 255, 256, 257, 65536, 65537, 2 ** 20)


def test_the_kappa_rule_is_the_librarys():
    for m in SIDES:
        for n in SIDES:
            for L in (1, 16):
                shape = hip.screen_shape_for(m, n, L)
                assert shape.kappa == ce.screen_kappa(m, n, L), (m, n, L)
                assert shape.slab % 16 == 0 and shape.slab * shape.nslab >= m and shape.tiles * shape.tile_cols >= n
                assert shape.grid == shape.tiles * shape.nslab and shape.slab * (shape.nslab - 1) < (m + 15) // 16 * 16
    assert ce.screen_kappa(1, 1, 1) == 1 + 10 + 1 + 8 and ce.screen_kappa(65537, 1, 16) == 2 * 16 + 10 + 2 + 8
    assert hip.screen_shape_for(4096, 65536, storage="f32").tile_cols == 1024
    for bad in ((0, 4, 1), (4, 0, 1), (2 ** 31, 4, 1), (4, 4, 17)):
        with pytest.raises(hip.HipError, match=r"\[10001\] fh_screen_shape_for: "):
            hip.screen_shape_for(*bad)


@pytest.mark.parametrize("name", S.PATH_NAMES)
def test_the_screened_path_on_the_host_loop(name):
    A, b = S.path_problems()[name]
    loss = fa.LeastSquares(b)
    runs = {}
    for screen in (False, True):
        np.random.seed(2)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            runs[screen] = fa.path(A, loss, fa.Shrink, backend="numpy", screen=screen, **S.PATH_OPTS)
    plain, got = runs[False], runs[True]
    tol = S.PATH_OPTS["gap_tolerance"]
    f0 = 0.5 * float(b @ b)
    n = A.shape[1]
    assert len(got) == len(plain) == S.PATH_OPTS["n_mus"]
    np.testing.assert_array_equal([p.mu for p in got], [p.mu for p in plain])
    for p, q in zip(got, plain):
        full = ce.duality_gap(A, loss, fa.Shrink(p.mu), p.solution)
        assert p.solution.shape == (n,) and tuple(p.certificate) == tuple(full)          # the full problem's certificate, always
        assert full.gap <= tol * f0 and q.certificate.gap <= tol * f0
        assert set(np.flatnonzero(p.solution)) == set(np.flatnonzero(q.solution))
        assert np.linalg.norm(A @ p.solution - A @ q.solution) <= 2.0 * math.sqrt(2.0 * tol * f0)
        assert p.kept >= np.count_nonzero(p.solution) and 0 <= p.rounds <= 8
    assert any(p.kept < n for p in got)
    assert not hasattr(plain[0], "kept")


def test_what_the_screened_path_refuses():
    A, b = S.path_problems()["dense64x128"]
    with pytest.raises(TypeError, match="screen=True is stated for losses.LeastSquares"):
        fa.path(A, fa.LogisticLoss(np.where(b > 0, 1.0, -1.0)), fa.Shrink, backend="numpy", screen=True)
    for bad in (dict(screen_shrink=0.0), dict(screen_shrink=1.0), dict(screen_max_rounds=-1)):
        with pytest.raises(ValueError, match="screen_shrink"):
            fa.path(A, fa.LeastSquares(b), fa.Shrink, backend="numpy", screen=True, **bad)


def test_header_library_and_binding_name_the_four_entry_points():
    names = ("fh_column_norms", "fh_screen", "fh_gather_columns", "fh_screen_shape_for")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "fasta_hip.h")).read()
    lib = hip.load_library()
    for name in names:
        assert name in hip.SIGNATURES and ("int %s(" % name) in header
        assert getattr(lib, name).restype is ctypes.c_int
    assert "#define FH_SCREEN_NOUT 4" in header and hip.SCREEN_NOUT == 4
    assert "#define FH_SCREEN_SHAPE_LEN 6" in header and hip.SCREEN_SHAPE_LEN == 6
    assert hip.SIGNATURES["fh_screen"][1][2] == ctypes.POINTER(ctypes.c_uint8)
    assert hip.SIGNATURES["fh_gather_columns"][1] == [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32), ctypes.c_uint64]
    for method in ("column_norms", "screen", "gather_columns"):
        assert callable(getattr(hip.HipContext, method))
    assert not [k for k in vars(hip) if k.startswith("SCREEN_") and k not in ("SCREEN_NOUT", "SCREEN_SHAPE_LEN")]

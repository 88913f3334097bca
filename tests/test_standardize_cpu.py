"""CPU tests of standardised features: the host statement (fasta_python_amd/preprocess.py), the way back to the caller's units, the path with
standardize / intercept on the host loop, the geometry tests/standardize_cases.py claims, and the entry point's declaration.

Bounds.  Balanced dyadic data (tests/standardize_cases.py): sums, means and sums of squares are exact, so the statement equals NumPy's mean / std
chain with `==` wherever both spell single rounded operations on exact operands.  Seeded data: 1e-13 relative against A.mean(0) / A.std(0) (pairwise
against recursive summation of at most 40 terms: a few eps)."""
import os
import re
import warnings

import numpy as np
import pytest

import fasta_python_amd as fa
from fasta_python_amd import hip, preprocess
from tests import standardize_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("case", SC.SHAPES, ids=SC.IDS)
def test_the_shapes_are_the_geometry_the_cases_claim(case):
    storage, m, n = case
    sh = hip.screen_shape_for(m, n, 0, storage, 256)
    assert (sh.slab, sh.nslab, sh.tile_cols, sh.tiles, sh.grid) == SC.GEOMETRY[case]
    mp = (m + 15) // 16 * 16
    if (m, n) == (33, 530):
        assert mp == 48 and sh.nslab * sh.slab == mp and m - 2 * sh.slab == 1          # a ragged last slab: one live row, fifteen padding rows
    assert n % (32 if storage == "f32" else 16) != 0                                    # padding columns behind the last one


@pytest.mark.parametrize("case", SC.SHAPES, ids=SC.IDS)
def test_the_statement_on_dyadic_data_is_numpys_bit_for_bit(case):
    _, m, n = case
    A = SC.balanced_dyadic(m, n, seed=m + n)
    kept = A.copy()
    Z, st = preprocess.standardize(A)
    np.testing.assert_array_equal(A, kept)                                              # the caller's matrix is not written
    means, scales, rows = st
    assert rows == m
    np.testing.assert_array_equal(means, A.mean(axis=0))                                # exact sums: any order
    d = A - means
    ss = (d * d).sum(axis=0)
    want = np.sqrt(ss / m)
    assert want[SC.CONSTANT] == 0.0 and want[SC.ZERO] == 0.0
    want[want == 0.0] = 1.0
    np.testing.assert_array_equal(scales, want)
    np.testing.assert_array_equal(Z, d / want)
    assert np.all(Z[:, SC.CONSTANT] == 0.0) and np.all(Z[:, SC.ZERO] == 0.0)
    assert len(set(scales.tolist())) > 3                                                # not trivially all equal
    assert scales[SC.LARGE] > 1e4 * np.median(scales)
    # each half alone
    Zc, (mc, sc, _) = preprocess.standardize(A, scale=False)
    np.testing.assert_array_equal(mc, means)
    np.testing.assert_array_equal(sc, np.ones(n))
    np.testing.assert_array_equal(Zc, d)
    Zs, (ms, ss_, _) = preprocess.standardize(A, center=False)
    np.testing.assert_array_equal(ms, np.zeros(n))
    rms = np.sqrt((A * A).sum(axis=0) / m)
    rms[rms == 0.0] = 1.0
    np.testing.assert_array_equal(ss_, rms)
    np.testing.assert_array_equal(Zs, A / rms)


def test_the_statement_on_seeded_data_is_mean_and_std():
    A = SC.seeded(40, 1030, seed=3)
    Z, st = preprocess.standardize(A)
    std = A.std(axis=0)
    live = std > 0
    np.testing.assert_allclose(st.means, A.mean(axis=0), rtol=1e-13, atol=0)
    np.testing.assert_allclose(st.scales[live], std[live], rtol=1e-13, atol=0)
    assert st.scales[SC.CONSTANT] == 1.0 and st.scales[SC.ZERO] == 1.0                  # (the constant is dyadic: d = 0 exactly)
    np.testing.assert_array_equal(Z, (A - st.means) / st.scales)
    assert np.all(np.abs(Z[:, live].mean(axis=0)) < 1e-13)
    np.testing.assert_allclose(np.sqrt((Z[:, live] ** 2).mean(axis=0)), 1.0, rtol=1e-13)


def test_a_sparse_matrix_is_scaled_only():
    from scipy import sparse as sp
    S = SC.long_sparse()
    before = S.copy()
    Z, st = preprocess.standardize(S, center=False)
    assert (S != before).nnz == 0
    D = S.toarray()
    norms2 = (D * D).sum(axis=0)                                                        # integers: exact
    want = np.sqrt(norms2 / S.shape[0])
    assert want[5] == 0.0
    want[want == 0.0] = 1.0
    np.testing.assert_array_equal(st.scales, want)
    np.testing.assert_array_equal(st.means, np.zeros(S.shape[1]))
    np.testing.assert_array_equal(Z.toarray(), D / want)
    assert sp.issparse(Z) and Z.nnz == S.nnz
    with pytest.raises(TypeError) as err:
        preprocess.standardize(S)
    assert str(err.value) == "standardize: centring would fill the sparse matrix: a sparse matrix is served with scale alone (center=False)"
    with pytest.raises(ValueError, match="nothing to do"):
        preprocess.standardize(D, center=False, scale=False)


def test_the_way_back_to_the_callers_units():
    rng = np.random.RandomState(2)
    A = SC.seeded(33, 60, seed=2)
    Z, st = preprocess.standardize(A)
    for shape, b_mean in (((60,), 1.25), ((60, 3), np.array([1.25, -2.0, 0.0]))):
        x = rng.randn(*shape) * (rng.rand(*shape) < 0.3)
        beta, beta0 = st.coefficients(x), st.intercept(x, b_mean)
        np.testing.assert_array_equal(beta, x / (st.scales if x.ndim == 1 else st.scales[:, None]))
        assert isinstance(beta0, float) if x.ndim == 1 else beta0.shape == (3,)
        lhs, rhs = A @ beta + beta0, Z @ x + b_mean
        assert np.max(np.abs(lhs - rhs)) <= 1e-12 * np.max(np.abs(rhs))
    assert st.intercept(np.zeros(60), 1.25) == 1.25
    assert fa.standardize is preprocess.standardize and fa.Standardization is preprocess.Standardization
    import fasta
    assert fasta.preprocess is preprocess


def run_path(A, loss, prox_class, **kw):
    np.random.seed(2)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fa.path(A, loss, prox_class, backend="numpy", **SC.PATH_OPTS, **kw)


@pytest.mark.parametrize("screen", [False, True], ids=["plain", "screen"])
def test_the_host_path_is_the_path_on_the_standardised_matrix(screen):
    A, b = SC.path_problem()
    kept = A.copy()
    got = run_path(A, fa.LeastSquares(b), fa.Shrink, standardize=True, intercept=True, screen=screen)
    np.testing.assert_array_equal(A, kept)
    Z, st = preprocess.standardize(A)
    want = run_path(Z, fa.LeastSquares(b - b.mean()), fa.Shrink, screen=screen)
    assert len(got) == len(want) == SC.PATH_OPTS["n_mus"]
    for p, q in zip(got, want):
        assert p.mu == q.mu and p.iteration_count == q.iteration_count and tuple(p.certificate) == tuple(q.certificate) and p.gaps == q.gaps
        np.testing.assert_array_equal(p.solution, q.solution)
        np.testing.assert_array_equal(p.coefficients, st.coefficients(q.solution))
        lhs, rhs = A @ p.coefficients + p.intercept, Z @ q.solution + b.mean()
        assert np.max(np.abs(lhs - rhs)) <= 1e-12 * np.max(np.abs(rhs))
        assert not hasattr(q, "coefficients")
    assert not np.any(got[0].solution) and not np.any(got[0].coefficients) and got[0].intercept == b.mean()
    assert np.count_nonzero(got[-1].coefficients) >= 5
    np.testing.assert_array_equal(got[0].standardization.scales, st.scales)
    np.testing.assert_array_equal(got[0].standardization.means, st.means)


def test_each_flag_alone_and_a_matrix_unknown_on_the_host():
    A, b = SC.path_problem()
    only_scale = run_path(A, fa.LeastSquares(b), fa.Shrink, standardize=True)
    Z, st = preprocess.standardize(A, center=False)
    want = run_path(Z, fa.LeastSquares(b), fa.Shrink)
    for p, q in zip(only_scale, want):
        np.testing.assert_array_equal(p.solution, q.solution)
        assert p.intercept == 0.0
    only_center = run_path(A, fa.LeastSquares(b), fa.Shrink, intercept=True)
    Z, st = preprocess.standardize(A, scale=False)
    want = run_path(Z, fa.LeastSquares(b - b.mean()), fa.Shrink)
    for p, q in zip(only_center, want):
        np.testing.assert_array_equal(p.solution, q.solution)
        np.testing.assert_array_equal(p.coefficients, q.solution)
    B = np.stack([b, 2.0 * b - 1.0], axis=1)
    mmv = run_path(A, fa.LeastSquares(B), fa.GroupShrink, standardize=True, intercept=True, x0=np.zeros((200, 2)))
    np.testing.assert_array_equal(mmv[0].intercept, B.mean(axis=0))
    assert mmv[-1].coefficients.shape == (200, 2) and mmv[-1].intercept.shape == (2,)
    S, bs = SC.sparse_path_problem()
    sparse = run_path(S, fa.LeastSquares(bs), fa.Shrink, standardize=True)
    Zs, _ = preprocess.standardize(S, center=False)
    want = run_path(Zs, fa.LeastSquares(bs), fa.Shrink)
    for p, q in zip(sparse, want):
        np.testing.assert_array_equal(p.solution, q.solution)


def test_what_the_standardised_path_refuses():
    for kw, words in SC.path_refusals(fa):
        for backend in ("numpy", "hip"):
            with pytest.raises(TypeError) as err:
                fa.path(kw["A"], kw["loss"], fa.Shrink, n_mus=3, backend=backend, **{k: v for k, v in kw.items() if k not in ("A", "loss")})
            for w in words:
                assert w in str(err.value), (w, str(err.value))
    A = np.ones((4, 5))
    with pytest.raises(TypeError, match="without weights"):
        fa.path(A, fa.LeastSquares(np.ones(4), weights=np.ones(4)), fa.Shrink, intercept=True, backend="numpy")


def test_the_entry_point_is_declared_and_is_no_setter():
    assert "fh_standardize" in hip.SIGNATURES
    header = open(os.path.join(ROOT, "include", "fasta_hip.h")).read()
    assert re.search(r"^int fh_standardize\(fh_ctx\* ctx, int center, int scale, double\* means, double\* scales\);$", header, re.M)
    assert not any(name.startswith("fh_set_") and "standard" in name for name in hip.SIGNATURES)
    lib = hip.load_library()
    assert lib.fh_standardize(None, 1, 1, None, None) == hip.E_ARG
    assert lib.fh_last_error().decode() == "fh_standardize: null context"
    assert callable(hip.HipContext.standardize)

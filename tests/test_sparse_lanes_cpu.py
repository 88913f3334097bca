"""CPU tier of the sparse-lane tests: the conditions on the INPUTS of tests/test_gpu_sparse_lanes.py, checked without a device.

* coverage: the matrices of tests/sparse_lanes.py land on every (G, LB) instantiation of csrc/fh_spmulti.h and every G of csrc/fh_sparse.h,
  on both copies of the operator, by the host's rule as lanes_of restates it (the GPU tier asks the library what it chose: fh_sparse_lanes);
* exactness: every quantity of a step and every apply, computed in float64, equals the same quantity in np.longdouble AND in exact integer
  arithmetic (everything scaled by 16, the sums of squares by 256), bit for bit -- and the sum of the MAGNITUDES of the terms of every sum
  stays below 2^53 units, so no summation order, lane split or fused multiply-add can round."""
import numpy as np
import pytest

from fasta_python_amd import hip
from tests import sparse_lanes as SL

EXACT = 2 ** 53


def test_the_binding_knows_the_read_only_window():
    assert "fh_sparse_lanes" in hip.SIGNATURES and len(hip.SIGNATURES["fh_sparse_lanes"][1]) == 5 and hasattr(hip.HipContext, "sparse_lanes")


# ---- coverage ------------------------------------------------------------------------------------------------------------------------------
def test_the_recipe_reaches_every_instantiation_on_both_copies():
    assert len(SL.PAIRS) == 19 and len(set(SL.PAIRS)) == 19
    for G, LB in SL.PAIRS + [(G, 0) for G in SL.VECTOR_G]:
        S = SL.exact_matrix(G, LB)
        a, at = SL.both_lanes(S, LB)
        assert (a.G, at.G) == (G, G), (G, LB, a.G, at.G)
        assert a.E == at.E == G // SL.column_lanes(LB)
        assert a.long_rows.size == 0 and at.long_rows.size == 0
        lens = np.diff(S.indptr)
        assert set(lens) == {0, 2 if a.E == 1 else 2 * a.E - 1}            # the last lane of a group walks one entry fewer (E = 1: two trips)


def test_every_exact_matrix_has_empty_rows_and_empty_columns():
    for G, LB in SL.PAIRS + [(G, 0) for G in SL.VECTOR_G]:
        S = SL.exact_matrix(G, LB)
        assert S.shape == (230, 251)
        assert list(np.flatnonzero(np.diff(S.indptr) == 0)) == list(range(5, 230, 37))
        cols = np.diff(S.T.tocsr().indptr)
        assert not cols[-3:].any() and np.count_nonzero(cols == 0) >= 3
        assert set(np.unique(S.data)) <= {-3.0, -2.0, -1.0, 1.0, 2.0, 3.0}


def test_every_long_matrix_puts_one_row_on_the_whole_workgroup_path_on_both_copies():
    for LB in (0,) + SL.ALL_LB:
        S = SL.long_matrix(LB)
        a, at = SL.both_lanes(S, LB)
        assert list(a.long_rows) == [311] and list(at.long_rows) == [407], (LB, a, at)
        # more entries than one trip of the whole workgroup serves, so every lane of it walks
        assert S.shape[1] > SL.FH_WG and S.shape[0] > SL.FH_WG


@pytest.mark.parametrize("LB", [0, 2, 16])
def test_the_staircase_gives_uneven_row_ranges(LB):
    S = SL.staircase()
    C = SL.column_lanes(LB)
    la = SL.lanes_of(S, C)
    assert la.long_rows.size == 0
    part = SL.row_ranges(S, C)
    owned = np.diff(part)
    groups = SL.FH_WG // la.G
    assert part[0] == 0 and part[-1] == 400 and np.all(owned >= 0) and len(part) == (400 + groups - 1) // groups + 1
    assert owned.max() > groups and 0 < owned.min() < groups, (la.G, groups, owned.min(), owned.max())


def test_the_cases_rotate_every_prox_kind_over_every_column_width():
    cases = SL.step_cases()
    assert sorted((G, LB) for G, LB, L, kind in cases if LB) == sorted(SL.PAIRS)
    assert [G for G, LB, L, kind in cases if not LB] == SL.VECTOR_G
    for LB in (0,) + SL.ALL_LB:
        assert {kind for G, lb, L, kind in cases if lb == LB} == set(SL.PROX_KINDS), LB
    assert all(SL.lb_of(L) == LB for G, LB, L, kind in cases)
    assert all(SL.lb_of(L) == LB for G, LB, L in SL.apply_cases() + SL.group_cases())
    assert sorted((G, LB) for G, LB, L in SL.group_cases()) == sorted(SL.PAIRS)


# ---- exactness -----------------------------------------------------------------------------------------------------------------------------
def ints(V, scale):
    W = np.asarray(V, dtype=np.float64) * scale
    assert np.array_equal(W, np.rint(W)) and np.all(np.abs(W) < 2 ** 62)
    return W.astype(np.int64).astype(object)


def isum(a, b=None):
    """(sum of the products a * b, sum of their magnitudes) in Python integers."""
    b = a if b is None else b
    p = np.ravel(a * b)
    return int(sum(p)), int(sum(abs(v) for v in p))


def imat(A, X):
    """A @ X in Python integers, with the largest sum of magnitudes of a dot product."""
    A64, X64 = A.astype(np.int64), X.astype(np.int64)
    assert int(np.max(np.abs(A64) @ np.abs(X64), initial=0)) < EXACT
    return (A64 @ X64).astype(object)


def integer_step(S, X0, B, tag):
    """exact_step restated in integers: matrices in units of 1/16, scalar sums of squares in units of 1/256, sums of magnitudes in 1/16.
    tau = 1/2 and coef = 1/4 are divisions by 2 and 4 that must come out even.  Returns (values, worst sum of magnitudes in units)."""
    A = ints(SL.dense_of(S), 1)
    x0, b = ints(X0, 16), ints(B, 16)
    worst = [0]

    def dot(a, c=None):
        s, mag = isum(a, c)
        worst[0] = max(worst[0], mag)
        return s

    def half(v, k):
        assert not np.any(v % k), "a quotient leaves the grid"
        return v // k

    def prox(x):
        if tag.kind == hip.PROX_SHRINK:
            thr = int(tag.mu * 8)                                   # tau * mu in units of 1/16
            return np.array([(1 if v > 0 else -1) * max(abs(v) - thr, 0) for v in np.ravel(x)], dtype=object).reshape(x.shape)
        if tag.kind == hip.PROX_NONNEG:
            return np.maximum(x, 0)
        if tag.kind == hip.PROX_BOX:
            return np.minimum(np.maximum(x, int(tag.lo * 16)), int(tag.hi * 16))
        return x.copy()

    amax = lambda v: max(abs(int(k)) for k in np.ravel(v))
    asum = lambda v: sum(abs(int(k)) for k in np.ravel(v))
    z0 = imat(A, x0)
    g0 = imat(A.T, z0 - b)
    out = {"G0": g0, "init": {hip.S_FSQ: dot(z0 - b), hip.S_GSUM: asum(x0)}}
    xh = x0 - half(g0, 2)
    xp = prox(xh)
    dx, z = xp - x0, imat(A, xp)
    out.update(XHAT=xh, XPROX=xp, Z=z)
    out["fwd"] = {hip.S_FSQ: dot(z - b), hip.S_DXG0: dot(dx, g0), hip.S_DX2: dot(dx), hip.S_XH2: dot(xp - xh), hip.S_G02: dot(g0),
                  hip.S_GSUM: asum(xp), hip.S_GMAX: amax(xp), hip.S_RDOT: dot(x0 - xp, xp - x0)}

    def adjoint(x1, z1):
        g1 = imat(A.T, z1 - b)
        dg = g1 + 2 * (xh - x0)
        return g1, {hip.S_DXDG: dot(dx, dg), hip.S_DG2: dot(dg), hip.S_FSQ_ADJ: dot(z1 - b), hip.S_XH2_ADJ: dot(x1 - xh),
                    hip.S_GSUM_ADJ: asum(x1), hip.S_GMAX_ADJ: amax(x1)}

    out["G1"], out["adj"] = adjoint(xp, z)
    x1, z1 = xp + half(xp - x0, 4), z + half(z - z0, 4)
    out["X1"] = x1
    out["G1A"], out["adja"] = adjoint(x1, z1)
    worst[0] = max(worst[0], 16 * asum(x1), 16 * asum(xp), 16 * asum(x0))
    return out, worst[0]


LINEAR = (hip.S_GSUM, hip.S_GMAX, hip.S_GSUM_ADJ, hip.S_GMAX_ADJ)          # slots in units of 1/16; every other slot in 1/256


def assert_step_is_exact(S, L, kind):
    tag = SL.prox_tag(kind)
    X0, B = SL.step_operands(S, L)
    f64 = SL.exact_step(S, X0, B, tag)
    ext = SL.exact_step(S, X0, B, tag, dtype=np.longdouble)
    want, worst = integer_step(S, X0, B, tag)
    assert worst < EXACT, f"a sum of magnitudes reaches 2^{np.log2(float(worst)):.1f} units: the inputs are too large"
    for name in SL.MATRICES:
        w = want[name].astype(np.float64) / 16.0
        assert f64[name].dtype == np.float64 and ext[name].dtype == np.longdouble
        assert np.array_equal(f64[name], w), name
        assert np.array_equal(ext[name], want[name].astype(np.longdouble) / 16), name
    for block in SL.BLOCKS:
        assert set(f64[block]) == set(want[block]) == set(ext[block])
        for slot, v in want[block].items():
            unit = 16 if slot in LINEAR else 256
            assert abs(v) < EXACT
            assert float(f64[block][slot]) == float(v) / unit, (block, slot)
            assert ext[block][slot] == np.longdouble(v) / unit, (block, slot)
    return f64


@pytest.mark.parametrize("G,LB,L,kind", SL.step_cases())
def test_one_step_on_the_exact_matrices_is_exact_in_float64(G, LB, L, kind):
    f = assert_step_is_exact(SL.exact_matrix(G, LB), L, kind)
    # the prox is at work, and the rows of the three empty columns carry something for the epilogue to extrapolate
    if kind != "none":
        assert np.any(f["XPROX"] != f["XHAT"])
    assert np.any(f["X1"][-3:] != 0) and not f["G1"][-3:].any() and not f["G1A"][-3:].any()


@pytest.mark.parametrize("LB", (0,) + SL.ALL_LB)
def test_one_step_on_the_long_matrices_is_exact_in_float64(LB):
    assert_step_is_exact(SL.long_matrix(LB), LB or None, "shrink")


@pytest.mark.parametrize("LB", [0, 2, 16])
def test_one_step_on_the_staircase_is_exact_in_float64(LB):
    assert_step_is_exact(SL.staircase(), LB or None, "box")


def test_every_apply_is_exact_in_float64():
    sets = [(SL.exact_matrix(G, LB), L) for G, LB, L in SL.apply_cases()]
    sets += [(SL.long_matrix(LB), LB or None) for LB in (0,) + SL.ALL_LB] + [(SL.staircase(), LB or None) for LB in (0, 2, 16)]
    for S, L in sets:
        V, W = SL.apply_operands(S, L)
        assert np.abs(V).max() == 4 and np.abs(W).max() == 4
        A = ints(SL.dense_of(S), 1)
        for M, I, X in ((S, A, V), (S.T.tocsr(), A.T, W)):
            want = imat(I, ints(X, 1))
            assert np.array_equal(M @ X, want.astype(np.float64))
            assert np.array_equal(M.astype(np.longdouble).toarray() @ X.astype(np.longdouble), want.astype(np.longdouble))


# ---- the GroupShrink step: not exact, so the tolerances of the GPU tier are checked against float64's own error ----------------------------
def group_sets():
    return [(SL.exact_matrix, (G, LB), G, L) for G, LB, L in SL.group_cases()] + [(SL.long_matrix, (LB,), None, LB) for LB in SL.ALL_LB]


@pytest.mark.parametrize("make,args,G,L", group_sets(), ids=lambda v: getattr(v, "__name__", str(v)))
def test_float64_meets_the_group_tolerances_with_room(make, args, G, L):
    """The float64 model against the longdouble model at a TENTH of the tolerances the device is held to (tests/test_gpu_sparse_mmv.py:
    test_single_step_scalars_match_numpy): the data leaves the kernels' different summation order room inside them."""
    from fasta_python_amd import proximal
    S0 = make(*args)
    S, X0, B, tau, mu = SL.group_problem(S0, L)
    assert [(la.G, list(la.long_rows)) for la in SL.both_lanes(S, SL.lb_of(L))] == [(la.G, list(la.long_rows)) for la in SL.both_lanes(S0, SL.lb_of(L))]
    assert G is None or SL.both_lanes(S, SL.lb_of(L))[0].G == G
    tag = proximal.GroupShrink(mu)
    a = SL.exact_step(S, X0, B, tag, tau=tau, coef=0.37)
    b = SL.exact_step(S, X0, B, tag, tau=tau, coef=0.37, dtype=np.longdouble)
    zeroed = np.count_nonzero(~b["XPROX"][:-3].any(axis=1))
    assert 0 < zeroed < S.shape[1] // 2, zeroed                                   # some rows vanish, at least half of them survive
    for name, (rtol, atol) in SL.GROUP_TOL.items():
        np.testing.assert_allclose(a[name], b[name].astype(np.float64), rtol=rtol / 10, atol=atol / 10, err_msg=name)
    for block in SL.BLOCKS:
        for slot, v in b[block].items():
            rtol, atol = SL.scalar_tol(block, slot)
            np.testing.assert_allclose(a[block][slot], float(v), rtol=rtol / 10, atol=atol / 10, err_msg=f"{block} {slot}")

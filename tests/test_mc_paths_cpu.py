"""CPU tier of the multi-column path tests: the conditions on the INPUTS of tests/test_gpu_mc_paths.py, checked without a device.

* geometry: through the pure form of the library's own launch rule (fh_multi_shape_for, the function both launchers call) every case of
  tests/mc_paths.py has the geometry its name claims -- stages per slab, rows of the last stage and of the last slab, column chunks and
  their live lanes, trips, passes per workgroup and their unevenness -- and every (LB, NT) instantiation of MC_FOR_EACH occurs;
* exactness: every quantity of a step and every apply, computed in float64, equals the same quantity in np.longdouble AND in integer
  arithmetic (everything scaled by 16, the sums of squares by 256), bit for bit, the sum of the MAGNITUDES of the terms of every sum stays
  below 2^53 units (the widest, sum dG^2 of the accelerated adjoint, at or below 2^52), and products over permuted rows and columns equal
  the unpermuted ones: no summation order, slab split, stage split or fused multiply-add can round."""
import os
import re

import numpy as np
import pytest

from fasta_python_amd import hip, proximal
from tests import mc_paths as MC
from tests import sparse_lanes as SL
from tests.test_sparse_lanes_cpu import EXACT, LINEAR, imat, integer_step, ints

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = MC.cases()


def test_the_binding_knows_the_read_only_window():
    assert "fh_multi_shape" in hip.SIGNATURES and len(hip.SIGNATURES["fh_multi_shape"][1]) == 2 and hasattr(hip.HipContext, "multi_shape")
    assert "fh_multi_shape_for" in hip.SIGNATURES and len(hip.SIGNATURES["fh_multi_shape_for"][1]) == 7 and callable(hip.multi_shape)
    assert len(hip.MultiShape._fields) == hip.MULTI_SHAPE_LEN == 14
    text = open(os.path.join(ROOT, "include", "fasta_hip.h")).read()
    assert int(re.search(r"#define\s+FH_MULTI_SHAPE_LEN\s+(\d+)", text).group(1)) == hip.MULTI_SHAPE_LEN


def test_the_pure_window_refuses_what_fh_set_tuning_and_fh_set_rhs_refuse():
    for args in ((0, 10, 2), (10, 0, 2), (10, 10, 0), (10, 10, 17), (10, 10, 2, 12), (10, 10, 2, 2056), (10, 10, 2, 0, -1), (10, 10, 2, 0, 0, 2)):
        with pytest.raises(hip.HipError, match=rf"^\[{hip.E_ARG}\]"):
            hip.multi_shape(*args)


def test_the_table_of_instantiations_is_the_kernels_own():
    text = open(os.path.join(ROOT, "fasta_python_amd", "csrc", "fh_multi.h")).read()
    line = re.search(r"#define MC_FOR_EACH\(X\)(.*)", text).group(1)
    rows = {int(lb): (int(ch), int(r)) for lb, ch, r in re.findall(r"X\((\d+),\s*(\d+),\s*(\d+)\)", line)}
    assert rows == MC.MC_FOR_EACH
    assert int(re.search(r"#define MC_LDS_DOUBLES\s+(\d+)", text).group(1)) == MC.MC_LDS_DOUBLES
    assert int(re.search(r"#define MC_ADJ_CPT\s+(\d+)", text).group(1)) == MC.MC_ADJ_CPT


def launch_rule(m, n, L, slab=0, cap=0, nt=-1):
    """The arithmetic launch_fwd_multi / launch_adj_multi did inline before they shared mc_shape_for, restated: the window must report it."""
    LB = SL.lb_of(L)
    CH, R = MC.MC_FOR_EACH[LB]
    mp, ld = MC.round_up(m, 16), MC.round_up(n, 16)
    ld2, nrg = ld // 2, mp // R
    ncc = -(-ld2 // (MC.FH_WG * MC.MC_ADJ_CPT))
    if not slab:
        target = max(32, -(-128 // ncc))
        slab = min(max(MC.round_up(-(-mp // target), 8), 128 if ncc >= 8 else 32), MC.ADJ_MAX_SLAB)
    nslab = -(-mp // slab)
    NT = nt if nt >= 0 else int(mp * ld * 8 > 256 << 20)
    return hip.MultiShape(LB, CH, R, NT, min(nrg, cap if cap > 0 else 512), nrg, -(-ld2 // (MC.FH_WG * CH // LB)), -(-ld // MC.FH_WG), slab, nslab,
                          mp - (nslab - 1) * slab, 2048 // LB, -(-slab // (2048 // LB)), ncc)


def test_the_window_reports_the_launchers_rule_at_every_size():
    rng = np.random.RandomState(5)
    shapes = [(1, 1), (17, 33), (200, 1000), (1030, 2049), (4096, 4096), (4097, 8190), (8192, 8192), (8193, 5000), (16384, 16384), (16400, 16390),
              (32768, 1024), (32769, 1000), (65536, 16384), (70000, 20000), (3000, 8193), (5000, 40000)]
    shapes += [(int(rng.randint(1, 70000)), int(rng.randint(1, 20000))) for _ in range(300)]
    seen = set()
    for m, n in shapes:
        for L in (1, 2, 3, 4, 5, 8, 9, 16):
            for slab, cap, nt in ((0, 0, -1), (0, 0, 0), (0, 7, 1), (264, 0, -1), (2048, 3, 1)):
                got = hip.multi_shape(m, n, L, slab, cap, nt)
                assert got == launch_rule(m, n, L, slab, cap, nt), (m, n, L, slab, cap, nt)
                seen.add((got.NT, got.stages > 1, got.nrg > got.fwd_grid, got.ncc >= 8))
    assert len(seen) == 16                                               # both sides of every threshold of the rule


# ---- geometry ------------------------------------------------------------------------------------------------------------------------------
def passes(sh):
    """Passes of k_mc_fwd's grid-stride loop, per workgroup."""
    return [len(range(b, sh.nrg, sh.fwd_grid)) for b in range(sh.fwd_grid)]


@pytest.mark.parametrize("nt", [0, 1])
@pytest.mark.parametrize("case", CASES, ids=MC.case_id)
def test_every_case_has_the_geometry_its_name_claims(case, nt):
    sh = hip.multi_shape(case.m, case.n, case.L, case.slab, case.cap, nt)
    assert sh == MC.expected_shape(case, nt)
    assert SL.lb_of(case.L) == case.LB == sh.LB and (sh.CH, sh.R) == MC.MC_FOR_EACH[case.LB] and sh.NT == nt
    mp, ld2 = MC.round_up(case.m, 16), MC.round_up(case.n, 16) // 2
    assert case.m % 16 and case.n % 16                                    # padding rows on both sides
    assert sh.SB == 2048 // case.LB and sh.slab_rows % 8 == 0 and sh.slab_rows <= MC.ADJ_MAX_SLAB
    assert (sh.nslab - 1) * sh.slab_rows + sh.last_slab_rows == mp and sh.nrg * sh.R == mp
    last_stage = sh.slab_rows - (sh.stages - 1) * sh.SB
    lanes = MC.FH_WG * sh.CH // sh.LB
    live_last_trip = ld2 - (sh.ntrip - 1) * lanes
    live_last_chunk = ld2 - (sh.ncc - 1) * MC.FH_WG * MC.MC_ADJ_CPT
    p = passes(sh)
    assert sum(p) == sh.nrg
    paths = MC.paths_of(sh, case.m, case.n)
    if case.name in ("staged", "narrow"):
        assert (sh.stages, last_stage) == (2, 8) and (sh.nslab, sh.last_slab_rows) == (3, 16)
        assert sh.fwd_grid == case.cap and min(p) >= 2 and max(p) == min(p) + 1          # every workgroup comes round again, some once more
        assert all(paths[k] for k in ("several stages", "short last stage", "ragged last slab", "clamped chunk", "K-fwd second pass", "uneven passes"))
    if case.name in ("staged", "many stages"):
        assert ld2 == 520 and sh.ncc == 2 and live_last_chunk == 8                       # the second column chunk: 8 live lanes of 512
        assert sh.ntrip == (5 if case.LB == 16 else 3) and live_last_trip == 8           # ... and the last trip 8 of `lanes`
        assert paths["ncc > 1"] and paths["masked last trip"]
    if case.name == "narrow":
        assert ld2 == 16 and sh.ncc == 1 and sh.ntrip == 1 and live_last_chunk == live_last_trip == 16
    if case.name == "many stages":
        assert case.LB == 16 and sh.slab_rows == 2048 and sh.stages == 16 and last_stage == sh.SB
        assert (sh.nslab, sh.last_slab_rows) == (2, 64) and sh.last_slab_rows < sh.SB     # the last slab: half a stage
        assert min(p) >= 2 and max(p) == min(p) + 1
    if case.name == "default":
        assert (case.slab, case.cap) == (0, 0) and sh.stages == 1 and sh.ncc == 1 and p == [1] * sh.nrg
        assert sh.slab_rows == 32 and paths["ragged last slab"] and not paths["several stages"] and not paths["K-fwd second pass"]


def test_the_table_holds_every_case_the_paths_need():
    names = {LB: {c.name for c in CASES if c.LB == LB} for LB in MC.ALL_LB}
    assert all({"staged", "narrow", "default"} <= names[LB] for LB in MC.ALL_LB) and "many stages" in names[16]
    pairs = {(hip.multi_shape(c.m, c.n, c.L, c.slab, c.cap, nt).LB, nt) for c in CASES for nt in (0, 1)}
    assert pairs == {(LB, nt) for LB in MC.MC_FOR_EACH for nt in (0, 1)}                 # every k_mc_fwd / k_mc_adj<LB, .., NT>
    for LB in MC.ALL_LB:
        mine = [c for c in CASES if c.LB == LB]
        assert {c.kind for c in mine} == set(SL.PROX_KINDS), LB                          # each elementwise prox kind meets each LB
        for name in names[LB]:
            assert {LB, max(1, LB - 1)} <= {c.L for c in mine if c.name == name}, (LB, name)      # without and with a padding column
        assert min(c.L for c in mine if c.name == "staged") == (1 if LB == 2 else LB // 2 + 1)    # ... and the most padding columns
    assert len(set(CASES)) == len(CASES)
    assert [(c.name, c.LB) for c, nt in MC.group_cases()] == [(g[0], g[1]) for g in MC._geometries()]
    assert all(SL.lb_of(c.L) == c.LB for c, nt in MC.group_cases()) and {nt for c, nt in MC.group_cases()} == {0, 1}


def test_the_vector_cases_cover_the_tuning_grid():
    cases = MC.vector_cases()
    fwd = {(t[hip.TUNE_FWD_ROWS], t[hip.TUNE_NT_LOADS]) for t, kind in cases if hip.TUNE_FWD_ROWS in t}
    adj = {(t[hip.TUNE_ADJ_CPT], t[hip.TUNE_NT_LOADS], t[hip.TUNE_ADJ_CYCLIC]) for t, kind in cases if hip.TUNE_ADJ_CPT in t}
    assert fwd == {(R, nt) for R in (4, 8, 16) for nt in (0, 1)}
    assert adj == {(cpt, nt, cy) for cpt in (1, 2, 4) for nt in (0, 1) for cy in (0, 1)}
    assert len(cases) == 18 and {kind for t, kind in cases} == set(SL.PROX_KINDS)
    assert {kind for t, kind in cases if hip.TUNE_FWD_ROWS in t} == set(SL.PROX_KINDS)
    mp = MC.round_up(MC.VECTOR_M, 16)
    assert all(t[hip.TUNE_ADJ_SLAB_ROWS] == MC.VECTOR_SLAB and t[hip.TUNE_FWD_GRID_CAP] == MC.VECTOR_CAP for t, kind in cases)
    assert MC.VECTOR_SLAB % 8 == 0 and 0 < mp % MC.VECTOR_SLAB < MC.VECTOR_SLAB                 # a ragged last slab
    assert all((mp // R) % MC.VECTOR_CAP for R in (4, 8, 16))                                    # uneven passes at every R


# ---- exactness -----------------------------------------------------------------------------------------------------------------------------
def step_sets():
    """Every distinct (m, n, L, prox kind) a step test of the GPU tier runs."""
    sets = {(c.m, c.n, c.L, c.kind): MC.case_id(c) for c in CASES}
    for t, kind in MC.vector_cases():
        sets.setdefault((MC.VECTOR_M, MC.VECTOR_N, None, kind), f"vector-{kind}")
    return sets


@pytest.mark.parametrize("m,n,L,kind", list(step_sets()), ids=list(step_sets().values()))
def test_one_step_is_exact_in_float64(m, n, L, kind):
    A, X0, B = MC.step_inputs(m, n, L)
    assert set(np.unique(A)) == {-1.0, 0.0, 1.0} and 0.70 < np.mean(A == 0) < 0.80
    tag = SL.prox_tag(kind)
    f64 = MC.step_model(m, n, L, kind)
    ext = SL.exact_step(A, X0, B, tag, dtype=np.longdouble)
    want, worst = integer_step(A, X0, B, tag)
    assert worst < EXACT, f"a sum of magnitudes reaches 2^{np.log2(float(worst)):.1f} units: the inputs are too large"
    for name in SL.MATRICES:
        assert f64[name].dtype == np.float64 and ext[name].dtype == np.longdouble
        assert np.array_equal(f64[name], want[name].astype(np.float64) / 16.0), name
        assert np.array_equal(ext[name], want[name].astype(np.longdouble) / 16), name
    for block in SL.BLOCKS:
        assert set(f64[block]) == set(want[block]) == set(ext[block])
        for slot, v in want[block].items():
            unit = 16 if slot in LINEAR else 256
            assert abs(v) < EXACT
            assert float(f64[block][slot]) == float(v) / unit, (block, slot)
            assert ext[block][slot] == np.longdouble(v) / unit, (block, slot)
    # the widest sum of a step: sum dG^2 of the accelerated adjoint, all terms positive, in units of 1/256
    widest = want["adja"][hip.S_DG2]
    assert widest == max(abs(v) for block in SL.BLOCKS for slot, v in want[block].items() if slot not in LINEAR)
    assert 0 < widest <= 2 ** 52, f"sum dG^2 = 2^{np.log2(float(widest)):.1f} units"
    if kind != "none":
        assert np.any(f64["XPROX"] != f64["XHAT"])                       # the prox is at work
    # products over permuted rows / columns equal the unpermuted ones: the order of a slab's, a stage's or a trip's terms cannot matter
    rng = np.random.RandomState(m + n)
    p, q = rng.permutation(m), rng.permutation(n)
    R0 = A @ X0 - B
    assert np.array_equal(A[p].T @ R0[p], f64["G0"]) and np.array_equal(A[:, q] @ f64["XPROX"][q], f64["Z"])
    R1 = f64["Z"] + MC.COEF * (f64["Z"] - A @ X0) - B
    assert np.array_equal(A[p].T @ R1[p], f64["G1A"])


def test_every_apply_is_exact_in_float64():
    for m, n, L in sorted({(c.m, c.n, c.L) for c in CASES}):
        A = MC.matrix(m, n)
        V, W = SL.apply_operands(A, L)
        assert np.abs(V).max() == 4 and np.abs(W).max() == 4
        I = ints(A, 1)
        for M, Im, X in ((A, I, V), (A.T, I.T, W)):
            want = imat(Im, ints(X, 1))
            assert np.array_equal(M @ X, want.astype(np.float64))
            assert np.array_equal(M.astype(np.longdouble) @ X.astype(np.longdouble), want.astype(np.longdouble))


# ---- the GroupShrink step: not exact, so the tolerances of the GPU tier are checked against float64's own error ----------------------------
@pytest.mark.parametrize("case,nt", MC.group_cases(), ids=lambda v: MC.case_id(v) if isinstance(v, MC.Case) else f"nt{v}")
def test_float64_meets_the_group_tolerances_with_room(case, nt):
    """The float64 model against the longdouble model at a TENTH of the tolerances the device is held to (GROUP_TOL, scalar_tol of
    tests/sparse_lanes.py): the data leaves the kernels' different summation order room inside them."""
    A, X0, B, tau, mu = SL.group_problem(MC.matrix(case.m, case.n), case.L)
    tag = proximal.GroupShrink(mu)
    a = SL.exact_step(A, X0, B, tag, tau=tau, coef=0.37)
    b = SL.exact_step(A, X0, B, tag, tau=tau, coef=0.37, dtype=np.longdouble)
    zeroed = np.count_nonzero(~b["XPROX"].any(axis=1))
    assert 0 < zeroed < case.n, zeroed                                    # some rows vanish, some survive
    for name, (rtol, atol) in SL.GROUP_TOL.items():
        np.testing.assert_allclose(a[name], b[name].astype(np.float64), rtol=rtol / 10, atol=atol / 10, err_msg=name)
    for block in SL.BLOCKS:
        for slot, v in b[block].items():
            rtol, atol = SL.scalar_tol(block, slot)
            np.testing.assert_allclose(a[block][slot], float(v), rtol=rtol / 10, atol=atol / 10, err_msg=f"{block} {slot}")

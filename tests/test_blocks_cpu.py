"""CPU tier of the row-block tests: every claim tests/block_cases.py makes about the INPUTS of tests/test_gpu_blocks.py, checked without a device.

* the split and the geometry: the restated split rule, each block's padding, the slab / chunk rule of launch_adj_dense as restated there and --
  through the library's device-free exports fh_fused_launch_shape_for / fh_setup_shape_for -- the one-pass shape of every block;
* coverage: the tables hold every CPT x NT x cyclic x storage combination, every loop form, every mode twice, a block without rows for some team
  in every one-pass case, a single-row block, the mixed set-up verdict -- remove one and a test here fails;
* exactness: the integer-arithmetic proofs of tests/test_sparse_lanes_cpu.py, tests/run_paths.py and tests/fused_paths.py hold for every new case;
* the block model: partials formed block by block and added in shard order equal the whole-matrix model bit for bit, and each of the six defects
  a shell could have changes a compared field on the operands of some case."""
import collections
import os
import re

import numpy as np
import pytest

from fasta_python_amd import hip
from tests import block_cases as BC
from tests import fused_paths as FP
from tests import level_cases as LC
from tests import mc_paths as MC
from tests import run_paths as RP
from tests import sparse_lanes as SL
from tests.test_sparse_lanes_cpu import EXACT, assert_step_is_exact, imat, ints

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fasta_python_amd", "csrc")
STEP_CASES, SETUP_CASES, LOGISTIC_CASES = BC.step_shell_cases(), BC.setup_shell_cases(), BC.logistic_shell_cases()


def test_the_binding_knows_the_read_only_window():
    assert "fh_last_scalars" in hip.SIGNATURES and len(hip.SIGNATURES["fh_last_scalars"][1]) == 2 and hasattr(hip.HipContext, "last_scalars")


# ---- the split --------------------------------------------------------------------------------------------------------------------------------
def test_the_split_rule_is_the_librarys():
    text = open(os.path.join(CSRC, "fasta_hip.hip")).read()
    assert "c->shard_row0[k + 1] = c->shard_row0[k] + m / p + (k < m % p ? 1 : 0);" in text           # the line BC.split restates
    assert int(re.search(r"#define FH_MAX_SHARDS (\d+)", open(os.path.join(CSRC, "fh_host_ctx.h")).read()).group(1)) == BC.FH_MAX_SHARDS
    for m, p in [(7, 3), (2070, 7), (67, 64), (3, 3), (4, 3), (96, 8), (100, 8)]:
        cuts = BC.split(m, p)
        rows = [r for _, r in cuts]
        assert cuts[0][0] == 0 and all(a[0] + a[1] == b[0] for a, b in zip(cuts, cuts[1:])) and sum(rows) == m
        assert rows == sorted(rows, reverse=True) and max(rows) - min(rows) <= 1 and min(rows) >= 1 and rows.count(max(rows)) == (m % p or p)
    assert BC.split(7, 3) == [(0, 3), (3, 2), (5, 2)] and BC.split_remainder_last(7, 3) == [(0, 2), (2, 2), (4, 3)]
    assert BC.split(100, 8) == [(13 * k, 13) for k in range(4)] + [(52 + 12 * k, 12) for k in range(4)]


def test_the_restated_launch_rule_of_the_two_launch_adjoint():
    """adj_launch against the text of launch_adj_dense (the vector kernels have no shape window) and against the numbers the existing cases rely on"""
    text = open(os.path.join(CSRC, "fh_host_launch.h")).read()
    for line in ("if (CPT == 0) CPT = p.ld2 <= 512 ? 1 : (p.ld2 < 16384 ? 2 : 4);", "p.ncc = (p.ld2 + FH_WG * CPT - 1) / (FH_WG * CPT);",
                 "std::max<uint64_t>(32, ((c->f32 ? 1024 : 128) + p.ncc - 1) / p.ncc);", "const uint64_t slab_min = p.ncc >= 8 ? 128 : 32;",
                 "p.ld2 = (uint32_t)(c->ld / (c->f32 ? 4 : 2)); p.nv2 = (uint32_t)(c->nv / 2);"):
        assert line in text, line
    assert "const uint32_t nchunks = (p.ld2 + FH_WG - 1) / FH_WG;" in text and "p.ld2 = (uint32_t)(c->nv / 2)" in text          # bb_epilogue_only
    assert BC.adj_launch(MC.VECTOR_M, MC.N_WIDE, "f64", 0, MC.VECTOR_SLAB) == BC.AdjLaunch(2, 2, 1032, 3, 16)
    assert BC.adj_launch(MC.VECTOR_M, MC.N_WIDE, "f32", 0, MC.VECTOR_SLAB) == BC.AdjLaunch(1, 2, 1032, 3, 16)                   # 264 pieces: CPT keyed on ld / 4
    assert BC.adj_launch(96, 160, "f64") == BC.AdjLaunch(1, 1, 32, 3, 32) and BC.adj_launch(65536, 65536, "f64")[:4] == (4, 32, 2048, 32)
    assert BC.epilogue_chunks(1030, "f64") == BC.epilogue_chunks(1029, "f64") == (3, 8) and BC.epilogue_chunks(160, "f64") == (1, 80)
    assert BC.epilogue_chunks(1029, "f32") == (3, 16) and BC.row_length(1029, "f32") == 1056 and BC.row_length(1030, "f32", 32) == 1088


# ---- A: the float32 axis of the vector tuning grid ------------------------------------------------------------------------------------------------
def test_the_float32_vector_cases_cover_what_float32_storage_changes():
    cases = MC.vector_cases("f32")
    assert MC.vector_cases() == MC.vector_cases("f64") and len(MC.vector_cases()) == 18
    fwd = collections.Counter((t[hip.TUNE_FWD_ROWS], kind) for t, kind, n in cases if n == MC.N_WIDE and hip.TUNE_LD_PAD not in t and hip.TUNE_FWD_ROWS in t)
    assert set(fwd) == {(R, kind) for R in (4, 8, 16) for kind in SL.PROX_KINDS}                       # k_fwd_dense<4|8, 1, KIND, 1>, and 16 -> 8
    adj = {(t[hip.TUNE_ADJ_CPT], t[hip.TUNE_ADJ_CYCLIC]) for t, kind, n in cases if n == MC.N_WIDE and hip.TUNE_LD_PAD not in t and hip.TUNE_ADJ_CPT in t}
    assert adj == {(cpt, cy) for cpt in (1, 2, 4) for cy in (0, 1)}                                    # k_adj_dense<1|2|4, 1, 1>
    assert all(hip.TUNE_NT_LOADS not in t for t, kind, n in cases)                                     # (float32 storage always loads non-temporally)
    ragged = [(t, n) for t, kind, n in cases if n != MC.N_WIDE]
    assert ragged and all(n % 4 and n % 32 for t, n in ragged) and any(hip.TUNE_ADJ_CPT not in t for t, n in ragged)      # ... once under the automatic CPT
    assert sum(t.get(hip.TUNE_LD_PAD, 0) == 32 for t, kind, n in cases) == 1
    mp = MC.round_up(MC.VECTOR_M, 16)
    assert all(t[hip.TUNE_ADJ_SLAB_ROWS] == MC.VECTOR_SLAB and t[hip.TUNE_FWD_GRID_CAP] == MC.VECTOR_CAP for t, kind, n in cases)
    assert all((mp // R) % MC.VECTOR_CAP for R in (4, 8))
    for t, kind, n in cases:
        la = BC.adj_launch(MC.VECTOR_M, n, "f32", t.get(hip.TUNE_ADJ_CPT, 0), MC.VECTOR_SLAB, t.get(hip.TUNE_LD_PAD, 0))
        assert (la.nslab, la.last_slab_rows) == (3, 16) and la.CPT == (t.get(hip.TUNE_ADJ_CPT) or 1)
        assert la.ncc == (2 if la.CPT == 1 else 1)                                                    # 264 (272 padded) pieces: a clamped second chunk, or lanes past the row
    level = MC.vector_level_cases()
    assert {(t[hip.TUNE_FWD_ROWS], prox) for t, prox in level} == {(R, prox) for R in (4, 8) for prox in LC.PROX_KINDS}


# ---- B: the table of shells -----------------------------------------------------------------------------------------------------------------------
def test_the_shell_table_covers_the_tuning_grid_on_both_storages():
    grid = [c for c in BC.shell_cases() if c.name == "grid"]
    combos = {(dict(c.tuning)[hip.TUNE_ADJ_CPT], dict(c.tuning)[hip.TUNE_NT_LOADS], dict(c.tuning)[hip.TUNE_ADJ_CYCLIC], c.storage) for c in grid}
    assert combos == {(cpt, nt, cy, st) for cpt in (1, 2, 4) for nt in (0, 1) for cy in (0, 1) for st in ("f64", "f32")} and len(grid) == 24
    assert len(BC.adj_tunings()) == 12
    for storage in ("f64", "f32"):
        mine = [c for c in grid if c.storage == storage]
        assert {c.p for c in mine} == set(BC.SHELL_BLOCKS) and {c.n for c in mine} == set(BC.SHELL_WIDTHS) and {c.kind for c in mine} == set(SL.PROX_KINDS)
    assert {(c.p, c.n) for c in grid} == {(p, n) for p in BC.SHELL_BLOCKS for n in BC.SHELL_WIDTHS}
    assert {(c.kind, c.storage) for c in BC.level_shell_cases()} == {("linf", "f64"), ("l1ball", "f32")}
    small = {c.name: c for c in BC.shell_cases() if c.n == BC.N_SMALL}
    assert {(c.m - c.p) for c in BC.shell_cases() if c.name == "one_row_each"} == {0} and {(c.m - c.p) for c in BC.shell_cases() if c.name == "one_more"} == {1}
    assert (small["max_shards"].p, small["max_shards"].m) == (BC.FH_MAX_SHARDS, 67)
    assert len(set(BC.shell_cases())) == len(BC.shell_cases()) == 31


@pytest.mark.parametrize("case", BC.shell_cases(), ids=BC.shell_id)
def test_every_block_of_a_shell_has_the_geometry_the_table_claims(case):
    t = dict(case.tuning)
    cuts = BC.split(case.m, case.p)
    pads = BC.padding_rows(case.m, case.p)
    launches = [BC.adj_launch(rows, case.n, case.storage, t.get(hip.TUNE_ADJ_CPT, 0), t.get(hip.TUNE_ADJ_SLAB_ROWS, 0)) for _, rows in cuts]
    if case.name in ("grid", "level"):
        assert all(rows % 16 for _, rows in cuts) and len({rows for _, rows in cuts}) == (1 if case.m % case.p == 0 else 2)      # uneven, none a multiple of 16 rows
        assert all(0 < pad < 16 for pad in pads)
        for la in launches:                                                                    # at least two slabs and a ragged last one in EVERY block
            assert la.nslab == 3 and la.last_slab_rows == 16 < la.slab_rows and la.slab_rows == t[hip.TUNE_ADJ_SLAB_ROWS] <= BC.ADJ_MAX_SLAB
        nchunks, live = BC.epilogue_chunks(case.n, case.storage)
        assert (nchunks, live) == ((3, 8) if case.storage == "f64" else (3, 16))              # k_bb_epilogue: three chunks, a ragged last one
        if case.name == "grid":
            pieces = BC.row_length(case.n, case.storage) // (4 if case.storage == "f32" else 2)
            assert all(la.CPT == t[hip.TUNE_ADJ_CPT] and la.ncc == BC.cdiv(pieces, 256 * la.CPT) for la in launches)
            assert launches[0].ncc == {1: 3 if case.storage == "f64" else 2, 2: 2 if case.storage == "f64" else 1, 4: 1}[launches[0].CPT]
    else:
        assert all(rows in (1, 2) for _, rows in cuts) and all(pad in (14, 15) for pad in pads)
        assert sum(pads) >= 14 * case.p and all(la.nslab == 1 for la in launches)
        if case.name == "one_row_each":
            assert all(rows == 1 for _, rows in cuts)
        else:
            assert [rows for _, rows in cuts].count(2) == case.m - case.p


# ---- C, D, F: the one-pass tables --------------------------------------------------------------------------------------------------------------------
def test_the_one_pass_shell_table_holds_every_form_and_every_mode_twice():
    forms = collections.Counter(FP.form_of(FP.expected_shape(c)) for c in STEP_CASES)
    assert set(forms) == set(FP.FORMS) and len(STEP_CASES) == len(FP.FORMS) + 1
    modes = collections.Counter(c.mode for c in STEP_CASES)
    assert set(modes) == set(FP.MODES) and min(modes.values()) >= 2
    assert all(c.cus == BC.STEP_CUS <= 64 and c.variant is not None and c.loss == "lsq" and c.what == "step" for c in STEP_CASES)
    assert all(FP.tuning_of(c)[hip.TUNE_FUSED_CUS] == c.cus for c in STEP_CASES)
    last_chunks = [BC.epilogue_chunks(c.n, c.storage) for c in STEP_CASES]
    assert any(nch > 1 and live < BC.FH_WG for nch, live in last_chunks) and any(live == BC.FH_WG for nch, live in last_chunks)      # k_bb_epilogue: ragged and full
    assert any(c.n % 2 for c in STEP_CASES)
    singles = [(c, p) for c in STEP_CASES for p in BC.STEP_BLOCKS if 1 in [rows for _, rows in BC.split(c.m, p)]]
    assert singles, "no block of a single row"
    by_base = {(b.n, b.storage, b.variant, b.kind, b.dens) for b in FP.exact_step_cases()}
    assert all((c.n, c.storage, c.variant, c.kind, c.dens) in by_base for c in STEP_CASES)               # cases of tests/fused_paths.py, other rows


@pytest.mark.parametrize("case", STEP_CASES + tuple(c for c, p, route in LOGISTIC_CASES), ids=FP.case_id)
def test_every_block_of_a_one_pass_case_launches_what_the_table_claims(case):
    whole = FP.expected_shape(case)
    assert FP.shape_query(case) == whole
    some_team_idle = False
    for p in BC.STEP_BLOCKS:
        for (r0, rows), sh in zip(BC.split(case.m, p), BC.block_shapes(case, p)):
            mine = BC.block_case(case, rows)
            assert sh is not None and sh == FP.expected_shape(mine), (p, r0, rows)                      # the library's pure rule == the restated one
            assert FP.row_of(sh) == FP.row_of(whole)                                                    # the same instantiation as the whole matrix
            ends = FP.r_ends(sh, FP.round_up(rows, 16))
            live = [len([r for r in FP.team_rows(sh, FP.round_up(rows, 16), t) if r < rows]) for t in range(sh.nteams)]
            assert sum(ends) == FP.round_up(rows, 16) and sum(live) == rows
            some_team_idle |= rows < sh.nteams and 0 in live
    if case.loss == "lsq":
        assert some_team_idle, "no block with fewer rows than its launch has teams"


def test_the_set_up_table_holds_both_storages_and_the_mixed_verdict():
    verdicts = collections.Counter((c.storage, one_read) for c, p, one_read in SETUP_CASES)
    assert verdicts == {("f64", True): 2, ("f32", True): 2, ("f64", False): 1}
    assert {p for c, p, one_read in SETUP_CASES if one_read} == {2, 3}
    assert any(FP.expected_shape(c).threads == 512 for c, p, one_read in SETUP_CASES if one_read)          # a 512-thread shape among them
    named = {c for c in FP.setup_cases()}
    for case, p, one_read in SETUP_CASES:
        shapes = BC.block_shapes(case, p)
        if one_read:
            assert case in named and all(sh is not None for sh in shapes)
            for (r0, rows), sh in zip(BC.split(case.m, p), shapes):
                assert sh == FP.expected_shape(BC.block_case(case, rows)) and FP.row_of(sh) == FP.row_of(FP.expected_shape(case))
        else:
            assert [sh is None for sh in shapes] == [False, True]                                       # one block keeps its kernel, the other has none
            assert FP.setup_key(2048, case.n, 0, FP.word_of(case), case.cus) and FP.setup_key(2047, case.n, 0, FP.word_of(case), case.cus) is None
            assert hip.setup_shape_for(case.m, case.n, cus=case.cus) is not None                          # (the whole matrix would take it)


def test_the_logistic_blocks_all_carry_padding_rows():
    rows = sorted({r for c, p, route in LOGISTIC_CASES for _, r in BC.split(c.m, p)})
    assert rows == [5, 6, 9] and {route for c, p, route in LOGISTIC_CASES} == {"two-launch", "one-pass"}
    assert all(pad > 0 for c, p, route in LOGISTIC_CASES for pad in BC.padding_rows(c.m, p))
    assert all(c.loss == "logistic" and np.all(np.abs(FP.operands(c).labels) == 1) for c, p, route in LOGISTIC_CASES)


# ---- exactness ------------------------------------------------------------------------------------------------------------------------------------
def step_sets():
    """every distinct (m, n, prox kind) of the exact two-launch cases that tests/test_mc_paths_cpu.py does not prove already"""
    sets = {(c.m, c.n, c.kind): f"{c.m}x{c.n}-{c.kind}" for c in BC.exact_shell_cases()}
    sets.update({(MC.VECTOR_M, n, kind): f"{MC.VECTOR_M}x{n}-{kind}" for t, kind, n in MC.vector_cases("f32")})
    return {k: v for k, v in sets.items() if k[1] != MC.N_WIDE or k[0] != MC.VECTOR_M}


@pytest.mark.parametrize("m,n,kind", list(step_sets()), ids=list(step_sets().values()))
def test_the_two_launch_step_is_exact_in_float64(m, n, kind):
    """float64 == longdouble == integers (units of 1/16 and 1/256), every sum of magnitudes below 2^53 units; the float32 cases run the same
    model: -1, 0 and 1 are float32 numbers"""
    A = MC.matrix(m, n)
    assert np.array_equal(A.astype(np.float32).astype(np.float64), A)
    f64 = assert_step_is_exact(A, None, kind)
    want = MC.step_model(m, n, None, kind)
    assert all(np.array_equal(f64[name], want[name]) for name in SL.MATRICES)


@pytest.mark.parametrize("m,n", sorted({(c.m, c.n) for c in BC.exact_shell_cases()}))
def test_the_rest_of_the_sequence_is_exact_in_float64(m, n):
    """fh_apply both ways and fh_gradient_at at V: float64 == integers (units of 1/2), sums of magnitudes below 2^53"""
    A, X0, B = MC.step_inputs(m, n, None)
    ex = BC.sequence_extras(m, n)
    I, V, W, Bi = ints(A, 1), ints(ex["V"], 2), ints(ex["W"], 2), ints(B, 2)
    AV = imat(I, V)
    assert np.array_equal(ex["AV"], AV.astype(np.float64) / 2) and np.array_equal(ex["ATW"], imat(I.T, W).astype(np.float64) / 2)
    assert np.array_equal(ex["GRAD"], imat(I.T, AV - Bi).astype(np.float64) / 2)
    assert int(np.max(np.abs(A) @ np.abs(ex["V"]))) + int(np.max(np.abs(B))) < EXACT


def test_the_level_problem_of_the_shells_is_exact():
    p = LC.step_problem(BC.SHELL_M, MC.N_WIDE)
    assert np.array_equal(p.A.astype(np.float32).astype(np.float64), p.A)
    for prox in LC.PROX_KINDS:
        mdl = LC.step_model(p, prox)
        assert mdl["level"] == 2.0 == LC.exact_level(np.abs(mdl["xhat"]), p.radius)
        assert LC.sums_are_exact(mdl["terms"], 2.0 ** -8)
        assert np.any(mdl["xprox"] != mdl["xhat"]) and np.any(mdl["xprox"])
    I = ints(p.A, 1)
    z0 = imat(I, ints(p.x0, 16))
    assert np.array_equal(imat(I.T, z0 - ints(p.b, 16)).astype(np.float64) / 16, p.g0)                   # fh_init's g0, in any order


@pytest.mark.parametrize("case", STEP_CASES, ids=FP.case_id)
def test_the_one_pass_cases_are_exact(case):
    bits, where = FP.prove(case)
    assert bits <= 51, (bits, where)
    st, sh = FP.operands(case), FP.expected_shape(case)
    assert np.array_equal(st.A.astype(np.float32).astype(np.float64), st.A)
    assert FP._sensitive(case, sh, st)
    if case.mode == "restart_hi":
        assert FP.model(case).vectors["coef"] == 0.0 and FP.model(case).sums[7] > 1e-30
    if case.mode in ("accel", "restart_lo"):
        assert FP.model(case).vectors["coef"] == FP.COEF


@pytest.mark.parametrize("case,p,one_read", SETUP_CASES, ids=[f"{FP.case_id(c)}-p{p}" for c, p, one_read in SETUP_CASES])
def test_the_set_up_cases_are_exact(case, p, one_read):
    bits, where = FP.prove_setup(case)
    assert bits <= 51, (bits, where)
    if not one_read:                                                                                    # the three passes form the two gradients themselves
        o, mdl = FP.setup_operands(case), FP.setup_model(case)
        I = ints(o.A, 1)
        grads = [imat(I.T, imat(I, ints(t, 2)) - ints(o.b, 2)) for t in (o.t0, o.t1)]
        assert np.array_equal((grads[0] - grads[1]).astype(np.float64) / 2, mdl["t2"])
        assert all(np.array_equal(o.A.T @ (o.A @ t - o.b), g.astype(np.float64) / 2) for t, g in zip((o.t0, o.t1), grads))


# ---- the block model ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", STEP_CASES, ids=FP.case_id)
def test_partials_added_in_shard_order_equal_the_whole_matrix_model(case):
    whole = FP.compared(FP.model(case))
    for p in BC.STEP_BLOCKS + (case.m,):
        blocks = BC.block_model(case, p)
        assert not FP.differs(BC.compared(blocks)[:-1], whole), p
        assert blocks.cuts == tuple(BC.split(case.m, p)) and blocks.pack[1] == 0.0
        assert blocks.pack[0] == FP.model(case).sums[0] and blocks.pack[2] == FP.model(case).sums[10]


@pytest.mark.parametrize("m,n,kind", sorted({(c.m, c.n, c.kind) for c in BC.exact_shell_cases()}))
def test_the_two_launch_partials_added_in_shard_order_equal_the_model(m, n, kind):
    A, X0, B = MC.step_inputs(m, n, None)
    want = MC.step_model(m, n, None, kind)
    Z0, Z = A @ X0, want["Z"]
    Z1 = Z + SL.COEF * (Z - Z0)
    for p in sorted({c.p for c in BC.exact_shell_cases() if (c.m, c.n, c.kind) == (m, n, kind)}):
        for name, R, slot, block in (("G0", Z0 - B, hip.S_FSQ, "init"), ("G1", Z - B, hip.S_FSQ_ADJ, "adj"), ("G1A", Z1 - B, hip.S_FSQ_ADJ, "adja")):
            g, f = None, None
            for r0, rows in BC.split(m, p):
                part, fk = A[r0:r0 + rows].T @ R[r0:r0 + rows], np.sum(R[r0:r0 + rows] ** 2)
                g, f = (part, fk) if g is None else (g + part, f + fk)
            assert np.array_equal(g, want[name]) and f == want[block][slot], (p, name)


@pytest.mark.parametrize("defect", BC.DEFECTS)
def test_every_defect_of_a_shell_changes_a_compared_field(defect):
    """If a defect shows on no case the operands are too tame: change the operands, not the list."""
    shown = []
    for case, p in BC.sensitivity_cases():
        right, wrong = BC.block_model(case, p), BC.block_model(case, p, defect)
        if FP.differs(BC.compared(right), BC.compared(wrong)):
            shown.append((FP.case_id(case), p))
    print(f"\n{defect}: shown by {len(shown)} of {len(BC.sensitivity_cases())}: {shown}", end="")
    assert shown, defect
    if defect == "padding row of a middle block in f":
        assert all("logistic" in name for name, p in shown)                                              # least squares: (0 - 0)^2, whatever the data

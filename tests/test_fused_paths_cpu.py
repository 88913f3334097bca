"""CPU tier of the tests of every instantiation and path of the one-pass dense kernels (csrc/fh_fused.h: k_fused_dense; csrc/fh_setup.h:
k_setup_dense): everything tests/fused_paths.py claims, proven without a device -- that the cases launch every row of both instance tables (parsed,
not restated), the geometry each case pins (against the library's own rule, fh_fused_launch_shape_for / fh_setup_shape_for), the paths that geometry
runs and the matrix of loop forms x paths up to the cells listed as unreachable, the exactness of every compared launch (redone in integer
arithmetic), the sensitivity of the inputs, and that the defects a kernel could have change a compared output of the model."""
import collections
import itertools

import numpy as np
import pytest

from fasta_python_amd import hip
from tests import fused_paths as FP
from tests import run_paths as RP

CASES = FP.cases()
EXACT = FP.exact_step_cases()

# what a row geometry is for, by dealing (blocked, cyclic); asserted of every case that carries the name and the geometry's team count
ROW_CLAIMS = {
    "one_row_last": (("r_end == 1", "uneven last team", "r_end % NB != 0", "r_end < NB - 1"), ("uneven last team", "r_end % NB != 0")),
    "one_each": (("r_end == 1", "team of padding rows only", "r_end < NB - 1"),) * 2,
    "some_empty": (("team with no rows", "r_end == 1"),) * 2,
    "empty_last": (("team with no rows",), ("uneven last team",)),
    "pairs": (("padding rows in a live team", "team of padding rows only", "r_end % NB != 0"), ("padding rows in a live team", "r_end % NB != 0")),
    "uneven": (("several trips", "uneven last team", "padding rows in a live team", "team of padding rows only"),
               ("several trips", "uneven last team", "padding rows in a live team")),
    "long": (("several trips", "uneven last team"),) * 2,
    "single": (("several trips", "padding rows in a live team"),) * 2,
    "tall": (("several trips", "padding rows in a live team"),) * 2,
    "halves": (("several trips", "padding rows in a live team"),) * 2,
    "three": (("several trips", "uneven last team", "padding rows in a live team", "team of padding rows only"), ("several trips", "uneven last team")),
}
TAG_CLAIMS = {"full": ("all lanes live",), "ragged": ("clamped lanes",), "cut": ("slices > 1, last slice cut",), "beyond": ("share beyond nv2",),
              "trips": ("slices == 1, several trips",), "onetrip": ("slices == 1, one trip",), "idlemem": ("idle members", "clamped lanes", "odd n")}
NAME_CLAIMS = {"plain-empty12": ("team with no rows",), "full-long4": ("several trips",),
               "whole-TEAM1": ("team with no rows", "r_end == 1"), "whole-inline8": ("team with no rows", "r_end == 1"),
               "whole-inline16": ("r_end == 1", "team of padding rows only", "share beyond nv2", "slices == 1, one trip"),
               "whole-one_ahead": ("team with no rows", "r_end == 1", "r_end <= PIPE"), "whole-two_ahead": ("r_end == 1", "r_end <= PIPE", "team of padding rows only"),
               "whole-lds16": ("r_end == 1", "r_end <= PIPE", "slices == 1, one trip"), "whole-lds32": ("r_end < NB - 1",),
               "whole-f32": ("team with no rows", "r_end == 1"), "whole-two_per_cu": ("grid > 256", "team with no rows", "r_end == 1"),
               "whole-two_per_cu_blocked": ("grid > 256", "team with no rows", "team of padding rows only")}


def ids(cases):
    return [FP.case_id(c) for c in cases]


# ---- table coverage --------------------------------------------------------------------------------------------------------------------------
def test_the_tables_are_parsed_whole():
    assert len(FP.fused_table()) == 69 and len(set(FP.fused_table())) == 69 and sum(1 for r in FP.fused_table() if r[5]) == 25
    assert len(FP.setup_table()) == 32 and len(set(FP.setup_table())) == 32 and sum(1 for r in FP.setup_table() if r[5]) == 7
    assert sum(1 for r in FP.setup_table() if r[3] == 512) == 2


def test_every_row_of_both_instance_tables_is_claimed_by_a_case():
    """a new table row with no case fails here; so does a case that launches something the tables do not hold"""
    step = {FP.row_of(FP.shape_query(c)) for c in FP.step_cases()}
    setup = {FP.row_of(FP.shape_query(c)) for c in FP.setup_cases()}
    assert step == set(FP.fused_table()), (set(FP.fused_table()) - step, step - set(FP.fused_table()))
    assert setup == set(FP.setup_table()), (set(FP.setup_table()) - setup, setup - set(FP.setup_table()))
    named = "\n".join(ids(CASES))
    for row in FP.fused_table():
        assert "step-" + "x".join(str(v) for v in row) + "-" in named, row
    for row in FP.setup_table():
        assert "setup-" + "x".join(str(v) for v in row) + "-" in named, row
    assert len(set(ids(CASES))) == len(CASES)


# ---- geometry --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=ids(CASES))
def test_the_library_launches_what_the_case_expects(case):
    want = FP.expected_shape(case)
    assert FP.shape_query(case) == want
    assert FP.row_of(want) in (FP.fused_table() if case.what == "step" else FP.setup_table())
    if not case.cus:                                                           # a whole-device case: the rule restated holds for other devices too
        for cus in (64, 128, 320):
            assert FP.shape_query(case, cus) == FP.expected_shape(case, cus)
    assert case.m * case.n * (4 if case.storage == "f32" else 8) <= 100 << 20      # no matrix above 100 MiB on the device
    if case.what == "setup":
        assert case.n >= 16384 or case.m * case.n >= 1 << 23                       # fh_setup takes the one-read kernel


def test_the_restated_rule_equals_the_librarys_over_the_widths():
    """expected_shape's restatement against the library across widths, storages, A/B bits, CU counts and floors (not only at the cases)"""
    rng = np.random.RandomState(3)
    for _ in range(3000):
        n = int(rng.choice([rng.randint(1, 4097), rng.randint(1, 262145), 4096 * rng.randint(1, 65)]))
        storage, word = ("f64", "f32")[rng.randint(2)], int(rng.choice([34, 2, 0, 38, 34 | 8, 2 | 16]))
        auto = bool(rng.randint(2))
        case = FP.Case("probe", "step", int(rng.randint(1, 3000)), n, storage, int(rng.choice([8, 16, 40, 48, 64, 96, 256])), int(rng.choice([0, 16])),
                       None if auto else word, "plain", "box", "lsq", 4)
        try:
            got = FP.shape_query(case)
        except hip.HipError:
            f32 = int(storage == "f32")
            assert FP.step_key(n, f32, FP.word_of(case), case.cus) is None
            continue
        assert got == FP.expected_shape(case), case


# ---- paths -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=ids(CASES))
def test_a_case_runs_the_paths_its_name_claims(case):
    sh = FP.shape_query(case)
    paths = FP.paths_of(sh, case.m, case.n)
    tag, _, rows = case.name.partition("-")
    claims = list(TAG_CLAIMS.get(tag, ())) + list(NAME_CLAIMS.get(case.name, ()))
    if rows in FP.ROWS:
        assert (case.m, sh.nteams) == FP.ROWS[rows], (rows, sh)
        claims += ROW_CLAIMS[rows][1 if sh.variant & 32 else 0]
    if rows.startswith("many"):
        assert sh.nteams == int(rows[4:])
        claims += ["several trips", "padding rows in a live team"]
    if tag == "ragged":
        claims.append("f32: n % 4 != 0 and n % 32 != 0" if sh.F32 else "odd n")
    if tag == "auto":
        assert case.variant is None and bool(sh.variant & 32) == (rows == "cyclic") == (sh.rows_per_team >= 128)
    for path in claims:
        assert paths[path], (path, sh)
    assert case.cus <= 256 and (case.what == "setup" or case.m <= 64 or tag == "auto")


def coverage():
    rows_fin, columns = collections.defaultdict(list), collections.defaultdict(list)
    for c in CASES:
        sh = FP.shape_query(c)
        for path, yes in FP.paths_of(sh, c.m, c.n).items():
            if yes and path in FP.COLUMN_PATHS:
                columns[(c.what, FP.row_of(sh), path)].append(c)
            elif yes and c.what == "step":
                rows_fin[(FP.form_of(sh), path)].append(c)
    return rows_fin, columns


def test_every_row_side_and_finaliser_path_is_reached_in_every_loop_form():
    rows_fin, _ = coverage()
    for form, path in itertools.product(FP.FORMS, FP.ROW_PATHS + FP.FIN_PATHS):
        if (form, path) in FP.UNREACHABLE:
            assert not rows_fin[(form, path)], ("listed as unreachable, yet reached", form, path)
        else:
            assert rows_fin[(form, path)], ("no case", form, path)
    assert set(FP.UNREACHABLE) <= set(itertools.product(FP.FORMS, FP.ROW_PATHS + FP.FIN_PATHS))
    # the exact cases alone reach them too, except where only a logistic case could (none)
    exact = collections.defaultdict(int)
    for (form, path), cs in rows_fin.items():
        exact[(form, path)] = sum(1 for c in cs if c.loss == "lsq")
    assert all(exact[k] for k in rows_fin if rows_fin[k])


def _probe_shapes():
    """(loop form, launch geometry) over the table rows, widths, CU counts up to 256, row counts, floors and both dealings"""
    for row in FP.fused_table():
        ppt, pipe, team, xlds, nbo, f32 = row
        for tag, n in FP.widths_of(row) + [("mid", max(1, FP.widths_of(row)[0][1] - 2 * 77))]:
            for bits in (0, 8, 16):
                for cus in range(team, 257, team):
                    if FP.step_key(n, int(f32), 2 | bits, cus) != row[:5]:
                        continue
                    case = FP.Case("probe", "step", 16, n, "f32" if f32 else "f64", cus, 0, 2 | bits, "plain", "box", "lsq", 4)
                    for m, floor, word in itertools.product((16, 64, 1024, 16384), (0, 16), (2 | bits, 34 | bits)):
                        sh = FP.expected_shape(case._replace(m=m, floor=floor, variant=word))
                        yield FP.form_of(sh), sh


def test_the_cells_listed_as_unreachable_are_not_reached_by_any_geometry_on_256_cus():
    """every listed cell is a finaliser path or `r_end <= PIPE`: searched over the launch geometries of its loop form"""
    by_form, count = collections.defaultdict(list), collections.Counter()
    for (form, path), why in FP.UNREACHABLE.items():
        assert why and (path in FP.FIN_PATHS or path == "r_end <= PIPE")
        by_form[form].append(path)
    for form, sh in _probe_shapes():
        count[form] += 1
        share, slices, tps, trips = FP.finaliser_of(sh)
        reached = {"slices > 1, last slice cut": slices > 1 and slices * tps > sh.nteams, "grid > 256": sh.grid > 256, "r_end <= PIPE": FP.distance_of(sh) > 0}
        for path in by_form[form]:
            assert not reached[path], (form, path, sh)
    assert all(count[form] > 100 for form in FP.FORMS), count


def _reachable_column_paths():
    """(what, table row, column path) that SOME width reaches: widths k * 64 + {0, 1, 3, 37}, both storages, the A/B bits"""
    out = set()
    for storage, f32 in (("f64", 0), ("f32", 1)):
        for word in (34, 34 | 8, 34 | 16):
            for n in (k * 64 + d for k in range(0, 4097) for d in (0, 1, 3, 37)):
                if n < 1 or n > 262144:
                    continue
                for what, m in (("step", 16), ("setup", 1 << 23)):
                    key = FP.step_key(n, f32, word, 256) if what == "step" else FP.setup_key(m, n, f32, word, 256)
                    if key is None:
                        continue
                    e = 4 if f32 else 2
                    ld2 = FP.round_up(n, 32) // 4 if f32 else FP.round_up(n, 16) // 2
                    per, team = FP.FH_WG * key[0], key[2]
                    row = tuple(key) + ((f32,) if what == "step" else ())
                    flags = {"all lanes live": n == e * per * team, "clamped lanes": ld2 < per * team, "odd n": n % 2 == 1 and not f32,
                             "f32: n % 4 != 0 and n % 32 != 0": bool(f32) and n % 4 != 0 and n % 32 != 0, "idle piece": FP.cdiv(ld2, FP.FH_WG * team) < key[0],
                             "idle members": (team - 1) * per >= ld2}
                    out |= {(what, row, path) for path, yes in flags.items() if yes}
    return out


def test_every_column_side_path_is_reached_for_every_table_row_that_can_reach_it():
    _, columns = coverage()
    reachable = _reachable_column_paths()
    assert {(w, r) for w, r, _ in reachable} == {("step", r) for r in FP.fused_table()} | {("setup", r) for r in FP.setup_table()}
    missing = sorted(k for k in reachable if not columns[k])
    assert not missing, missing
    for what, table in (("step", FP.fused_table()), ("setup", FP.setup_table())):
        for row in table:
            assert columns[(what, row, "all lanes live")], row
    # what the issue names: members 13-15 of 16 x 5 pieces own no column at n = 32 784
    sh = hip.fused_launch_shape_for(50, 32785, cus=48, variant_auto=False, min_rows=0)
    assert FP.row_of(sh) == (5, 2, 16, 0, 0, 0) and [FP.member_columns(sh, 32785, k)[0] == 32785 for k in range(16)] == [False] * 13 + [True] * 3


def test_the_geometry_recipes():
    """mp = 16 on 6 teams, blocked: 3, 3, 3, 3, 3 and one row; on 16 teams and more: one row each and the rest empty under both dealings.  (Two
    teams get 8 rows each -- rows_per_team = ceil(mp / teams) -- so a one-row team needs six.)"""
    for word in (2, 34):
        sh = hip.fused_launch_shape_for(16, 3000, cus=6, variant_word=word, variant_auto=False, min_rows=0)
        assert FP.r_ends(sh, 16) == ([3, 3, 3, 3, 3, 1] if word == 2 else [3, 3, 3, 3, 2, 2])
        assert FP.r_ends(hip.fused_launch_shape_for(16, 3000, cus=2, variant_word=word, variant_auto=False, min_rows=0), 16) == [8, 8]
        for teams in (16, 20, 64):
            sh = hip.fused_launch_shape_for(16, 3000, cus=teams, variant_word=word, variant_auto=False, min_rows=0)
            assert FP.r_ends(sh, 16) == [1] * 16 + [0] * (teams - 16)
            assert sorted(r for t in range(teams) for r in FP.team_rows(sh, 16, t)) == list(range(16))
    # every dealing deals every row exactly once
    for c in CASES[::7]:
        sh, mp = FP.shape_query(c), FP.round_up(c.m, 16)
        assert sorted(r for t in range(sh.nteams) for r in FP.team_rows(sh, mp, t)) == list(range(mp))
        assert [len(FP.team_rows(sh, mp, t)) for t in range(sh.nteams)] == FP.r_ends(sh, mp)


def test_the_options_are_spread_over_the_loop_forms():
    seen = set()
    for c in FP.step_cases():
        sh = FP.shape_query(c)
        seen |= {("mode", FP.form_of(sh), c.mode), ("kind", FP.form_of(sh), c.kind), ("word", c.variant if c.variant is None else c.variant & 38),
                 ("preload", FP.preload_of(sh)), ("NB", FP.nb_of(sh)), ("loss", FP.form_of(sh), c.loss)}
    for form in FP.FORMS:
        for mode in FP.MODES:
            assert ("mode", form, mode) in seen, (form, mode)
        assert ("kind", form, "box") in seen and ("kind", form, "shrink") in seen and ("loss", form, "logistic") in seen, form
    assert {("word", w) for w in (34, 2, 0, 38, None)} <= seen and {("NB", k) for k in (3, 4, 5, 6)} <= seen and {("preload", True), ("preload", False)} <= seen


# ---- exactness -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", EXACT, ids=ids(EXACT))
def test_every_compared_launch_is_exact_in_any_order_of_summation(case):
    """The launch redone over the integers (run_paths.prove_attempt with the dyadic coefficient): all products exact, sum|terms| / lsb < 2^53 for
    every sum -- two bits of headroom asked for -- and the float64 model's sums and vectors equal to the integers'.  A condition, not a measurement."""
    bits, where = FP.prove(case)
    assert bits <= 51, (bits, where)
    mdl = FP.model(case)
    applied = mdl.vectors["coef"]
    assert applied == {"plain": 0.0, "accel": FP.COEF, "restart_hi": 0.0, "restart_lo": FP.COEF}[case.mode]
    if case.mode == "restart_hi":
        assert mdl.sums[7] > 1e-30
    if case.mode == "restart_lo":
        assert mdl.sums[7] <= 1e-30


@pytest.mark.parametrize("case", FP.setup_cases(), ids=ids(FP.setup_cases()))
def test_every_set_up_is_exact_in_any_order_of_summation(case):
    bits, where = FP.prove_setup(case)
    assert bits <= 51, (bits, where)


def test_the_generalised_proof_keeps_the_loop_suites_results_and_refuses_what_is_not_exact():
    """prove_attempt with coefficient 0 and -1 is what the device-loop suite relies on (tests/test_run_paths_cpu.py runs it for every case); here: a
    dyadic coefficient moves x1 and g1 to a finer scale and still equals float64, and a coefficient that is not dyadic is refused."""
    case = next(c for c in EXACT if c.mode == "accel" and c.n < 3000)
    st = FP.operands(case)
    Ai = st.A.astype(np.int64)
    for coef in (0.0, -1.0, 0.5, -0.75, 3.0):
        sums, v = RP.attempt(st.A, st.b, st.x0, st.g0, st.xacc0, st.zacc0, FP.TAU, coef, True, case.kind)
        isums, iv = RP.prove_attempt(Ai, st.b, st.x0, st.g0, st.xacc0, st.zacc0, FP.TAU, coef, True, case.kind, RP.Bits())
        assert [float(s) for s in sums] == isums and all(np.array_equal(iv[k], v[k]) for k in iv), coef
    with pytest.raises(RP.NotExact):
        RP.prove_attempt(Ai, st.b, st.x0, st.g0, st.xacc0, st.zacc0, FP.TAU, 0.3, True, case.kind, RP.Bits())
    with pytest.raises(RP.NotExact):
        RP.prove_attempt(Ai, st.b, st.x0 + 2.0 ** -30, st.g0, st.xacc0, st.zacc0, 2.0 ** -30, 0.5, True, "identity", RP.Bits())


# ---- sensitivity of the inputs ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", EXACT, ids=ids(EXACT))
def test_the_inputs_leave_no_row_column_or_piece_without_effect(case):
    st, sh = FP.operands(case), FP.shape_query(case)
    assert set(np.unique(st.A)) == {-1.0, 0.0, 1.0} and st.A.any(axis=0).all() and st.A.any(axis=1).all()
    assert np.array_equal(st.g0, st.A.T @ (st.A @ st.x0 - st.b))
    rv = FP.gradient_factors(case, st)
    nz = rv != 0
    assert np.count_nonzero(nz) >= 0.9 * case.m
    assert nz[FP.required_rows(case, sh)].all()                    # row m - 1, the first and the last live row of every team (so every row of a one-row team)
    assert case.m - 1 in FP.required_rows(case, sh)
    assert st.A[nz].any(axis=0).all()                              # every column has an entry in a row whose factor is not zero
    xp = FP.model(case).vectors["xprox"]
    for lo, hi in FP.required_pieces(case, sh):
        assert xp[lo:hi].any(), (lo, hi)
    moved = st.g0 != 0                                             # (a sparse matrix of few rows leaves many entries of g0 zero: xhat = x0 there)
    assert np.count_nonzero((xp != st.x0) & moved) > np.count_nonzero(moved) / 4 and np.count_nonzero(moved) > case.n / 16
    if case.mode != "plain":                                       # the entering history differs from (x0, z0)
        assert np.count_nonzero(st.xacc0 != st.x0) > case.n / 16 and not np.array_equal(st.zacc0, st.A @ st.x0)
        assert np.array_equal(st.zacc0, st.A @ st.xacc0) and np.array_equal((st.xacc0 - st.x0) * 2, np.rint((st.xacc0 - st.x0) * 2))


@pytest.mark.parametrize("case", FP.setup_cases(), ids=ids(FP.setup_cases()))
def test_the_set_ups_inputs_leave_no_row_or_column_without_effect(case):
    o, mdl = FP.setup_operands(case), FP.setup_model(case)
    zd, r = mdl["factors"]
    assert (r != 0).all() and np.count_nonzero(zd) >= 0.9 * case.m
    assert o.A.any(axis=0).all() and o.A[zd != 0].any(axis=0).all()
    assert np.count_nonzero(o.t0 - o.t1) > case.n / 2 and o.x0[case.n - 1] != 0 and o.t0[case.n - 1] != o.t1[case.n - 1]
    assert mdl["DG2"] > 0 and mdl["DX2"] > 0 and mdl["FSQ"] > 0


# ---- mutants of the model --------------------------------------------------------------------------------------------------------------------
def test_every_defect_changes_a_compared_output_of_a_case_that_claims_its_path():
    shown, unmasked = collections.Counter(), collections.Counter()
    for case in EXACT:
        true = FP.compared(FP.model(case))
        sh = FP.shape_query(case)
        for which in ("last pair unmasked", "last row skipped", "member slice dropped from z", "team partial dropped from g1", "x0 for x_accel0"):
            got = FP.mutant(case, which)
            if got is None:
                continue
            if which == "last pair unmasked":
                # only the box maps the zero padding to something else: every other kind hides the defect, which is why the ragged widths rotate through it
                assert FP.differs(got[:1], true[:1]) == (case.kind == "box"), (which, FP.case_id(case))
                unmasked[FP.row_of(sh)] += case.kind == "box"
                continue
            assert FP.differs(got, true), (which, FP.case_id(case))
            shown[which] += 1
    assert shown["last row skipped"] == len(EXACT)
    assert shown["member slice dropped from z"] == sum(1 for c in EXACT if FP.shape_query(c).TEAM > 1)
    assert shown["team partial dropped from g1"] == sum(1 for c in EXACT if FP.shape_query(c).nteams > 1)
    assert shown["x0 for x_accel0"] == sum(1 for c in EXACT if c.mode != "plain")
    assert sum(1 for k in unmasked.values() if k) >= len(FP.fused_table()) - 2, unmasked                                  # table rows whose odd widths meet the box
    # a padding row counted in f: invisible for least squares ((0 - 0)^2), log 2 per row for the logistic loss -- far beyond that test's tolerance
    for case in FP.logistic_cases():
        f, bad = FP.padding_rows_in_f(case)
        assert FP.paths_of(FP.shape_query(case), case.m, case.n)["padding rows in a live team"]
        assert abs(bad - f) > 1e5 * (1e-11 * abs(f))                   # (the logistic test holds f to rtol 1e-11)

"""CPU tier of the clipping-level search's tests (tests/level_cases.py; the GPU tier is tests/test_gpu_level.py): the restated rule finds the exact
sort-based level on every case, from every left-over guess; every input meets the precondition of the exactness argument; the restated dispatch
rule is the library's own."""
import numpy as np
import pytest

from fasta_python_amd import hip
from tests import level_cases as LC

CASES = LC.cases()


@pytest.mark.parametrize("case", CASES, ids=LC.case_id)
def test_the_model_finds_the_exact_sort_based_level_from_any_guess(case):
    inp = LC.build(case)
    ax = np.abs(LC.xhat_of(inp))
    want = LC.exact_level(ax, inp.radius)
    level, passes, count = LC.model(ax, inp.radius)
    assert LC.same_level(level, want), (level, want)
    assert (level > 0.0) == (want > 0.0)
    if level > 0.0:
        assert level == want
    for guess in LC.guesses(ax, level):
        warm = LC.model(ax, inp.radius, guess)[0]
        if level > 0.0:
            assert warm == level, (guess, warm, level)
        else:
            assert not warm > 0.0, (guess, warm)
    if case.kind == "one_per_pass":
        assert passes >= 16 and count == 1
    if case.kind == "ties":
        assert level == 2.0 and (case.n == 1 or (ax == level).any())      # the level lands on an entry (n = 1 holds the one 4 alone)
    if case.kind == "all_equal":
        assert level == 2.75
    if case.kind == "radius_zero":
        assert level == ax.max()
    if case.kind == "radius_is_l1":
        assert level == 0.0
    if case.kind == "radius_above_l1":
        assert level < 0.0


@pytest.mark.parametrize("case", CASES, ids=LC.case_id)
def test_every_input_is_on_the_grid_and_its_sums_are_exact(case):
    inp = LC.build(case)
    assert inp.tau in (1.0, 0.25)
    for v in (inp.x0, inp.g0):
        assert np.array_equal(np.rint(v * 16.0), v * 16.0)
        if case.kind != "one_per_pass":
            assert np.abs(v).max() <= 64.0
    units = LC._units(np.abs(LC.xhat_of(inp)))             # asserts the grid
    assert int(units.sum()) < 2 ** 53
    assert np.rint(inp.radius / LC.GRID) == inp.radius / LC.GRID and inp.radius / LC.GRID < 2.0 ** 53
    if case.kind != "one_per_pass":
        assert int(units.max()) <= 80 * 64 and int(units.sum()) < 2 ** 40
    if case.kind == "mostly_zero":
        z = LC.xhat_of(inp)
        zero = z == 0.0
        assert (zero & np.signbit(z)).any() and (zero & ~np.signbit(z)).any()


def test_every_dispatch_class_is_reached_at_both_edges_by_distinct_and_ties():
    seen = {}
    for c in CASES:
        if c.kind in ("distinct", "ties"):
            seen.setdefault((LC.class_name(c.n), c.kind), set()).add(c.n)
    edges = {"one-4x256": (1, 1024), "one-16x256": (1025, 4096), "one-32x256": (4097, 8192), "one-16x1024": (8193, 16384), "multi-G3": (16385, 24576),
             "multi-G4": (24577,), "multi-G32": (262143, 262144), "one-0x1024": (262145, 300000)}
    for name, ns in edges.items():
        for kind in ("distinct", "ties"):
            assert set(ns) <= seen[(name, kind)], (name, kind)


def test_the_restated_dispatch_rule_is_the_librarys():
    assert "fh_level_shape_for" in hip.SIGNATURES and len(hip.SIGNATURES["fh_level_shape_for"][1]) == 2
    ns = set(range(1, 300001, 97)) | set(LC.LENGTHS) | set(LC.CLASS_EDGES)
    for e in LC.CLASS_EDGES:
        ns |= {max(1, e - 1), e + 1}
    ns |= {k * 8192 + d for k in range(2, 33) for d in (0, 1)}
    for n in sorted(ns):
        got = hip.level_shape_for(n)
        assert tuple(got) == tuple(LC.shape_of(n)), n
    assert hip.level_shape_for(2 ** 31 - 1) == hip.LevelShape(0, 1024, 0, 1)
    for bad in (0, 2 ** 31):
        with pytest.raises(hip.HipError):
            hip.level_shape_for(bad)


def test_exact_level_agrees_with_the_host_projection_on_the_distinct_inputs():
    """fasta_python_amd.proximal.project_Linf_ball is the reference's sort-based form in float64: within 1 ulp of the rationals' value, seen through
    the clipped entries."""
    from fasta_python_amd import proximal
    for case in CASES:
        if case.kind != "distinct":
            continue
        inp = LC.build(case)
        xhat = LC.xhat_of(inp)
        want = LC.exact_level(np.abs(xhat), inp.radius)
        out = np.abs(proximal.project_Linf_ball(xhat, inp.radius))
        clipped = out[np.abs(xhat) > out]
        if clipped.size:
            assert abs(clipped.max() - want) <= np.spacing(want) and clipped.max() == clipped.min(), case


@pytest.mark.parametrize("m,n", LC.STEP_SHAPES)
@pytest.mark.parametrize("prox", LC.PROX_KINDS)
def test_the_one_pass_step_problem_is_exact_in_any_order(m, n, prox):
    p = LC.step_problem(m, n)
    for v in (p.x0, p.g0, p.b):
        assert np.array_equal(np.rint(v * 8.0), v * 8.0)
    assert np.array_equal(p.A.T @ (p.A @ p.x0 - p.b), p.g0)
    mdl = LC.step_model(p, prox)
    assert mdl["level"] == 2.0
    assert LC.sums_are_exact(mdl["terms"], 2.0 ** -6)
    # the products behind z and g1: |A| |xprox| and |A^T| |z - b| stay far below 2^53 eighths
    assert float((np.abs(p.A) @ np.abs(mdl["xprox"])).max()) < 2.0 ** 40 and float((np.abs(p.A.T) @ np.abs(mdl["z"] - p.b)).max()) < 2.0 ** 40

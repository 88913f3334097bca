"""The device sees the same calls: every case of tests/path_call_cases.py runs path() with a HipContext that writes down the methods called on
it, and the sequence is the one of tests/golden/path_calls.json with `==`.  The fixture was taken on the commit it names; equal sequences on
equal shapes are equal launches and equal transfers, which is what a change to the drivers of regpath.py has to keep.  No timing is asserted."""
import pytest

from tests import path_call_cases as P

pytestmark = pytest.mark.gpu

GOLDEN = P.load_golden()


def test_the_fixture_holds_exactly_the_cases_of_the_list():
    assert sorted(GOLDEN["cases"]) == sorted(P.CASES)


@pytest.mark.parametrize("cid", list(P.CASES))
def test_path_makes_the_recorded_calls_in_the_recorded_order(cid):
    log, op = P.record(cid)
    try:
        assert log == GOLDEN["cases"][cid]
        if op is not None:                              # the caller's map: path() has not closed its context, it still answers
            assert "0:close" not in log and op.ctx.shape() == (P.M, P.N)
    finally:
        if op is not None:
            op.close()


def test_the_cases_reach_what_they_are_there_for():
    """... as the fixture shows it: a working context that gathers, one that takes a second slice through the CSR setter or not at all, a
    standardised operator, and without screening neither a certificate's mask nor a second context."""
    calls = GOLDEN["cases"]
    assert "1:gather_columns" in calls["dense_screen"] and "1:set_rhs" in calls["dense_group_screen"]
    assert "0:standardize" in calls["dense_screen_standardize_intercept"] and "0:standardize" in calls["csr_standardize"]
    assert any(c.startswith("1:set_matrix_csr") for c in calls["csr_screen"])
    for cid in ("dense", "csr", "csr_standardize", "dense_map_of_the_caller"):
        assert not any(c.startswith("1:") or c == "0:screen" for c in calls[cid]), cid
    assert calls["dense"][-1] == "0:close" and "0:close" not in calls["dense_map_of_the_caller"]

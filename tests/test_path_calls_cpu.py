"""The cases of tests/path_call_cases.py without a device: the fixture holds exactly the list, and on the host path (backend="numpy") the
screened vector cases pass through every branch of a screening round, so that the call sequences on record cover them."""
import pytest

from tests import path_call_cases as P


def test_the_fixture_holds_exactly_the_cases_of_the_list():
    G = P.load_golden()
    assert sorted(G["cases"]) == sorted(P.CASES) and all(calls and all(":" in c for c in calls) for calls in G["cases"].values())


@pytest.mark.parametrize("cid", ["dense_screen", "csr_screen"])
def test_a_screened_case_reaches_the_branches_of_a_round(cid):
    """A point's `kept` starts at n; only a compacting round lowers it, and a point at which every feature is screened sets it to 0 and solves
    nothing.  So a point with rounds and kept = n ran all of them on the full operator."""
    _, out = P.run(cid, "numpy")
    assert any(p.rounds >= 1 and p.kept == 0 and p.iteration_count == 0 for p in out)             # every feature screened
    compacted = [p for p in out if 0 < p.kept < P.N]
    if cid == "dense_screen":
        assert compacted and any(p.rounds >= 1 and p.kept == P.N for p in out)                    # a round that compacts, rounds on the full operator
    else:
        assert len(compacted) >= 2                                                                # a second slice for the same working context


def test_the_group_case_compacts_a_matrix_unknown():
    _, out = P.run("dense_group_screen", "numpy")
    assert all(p.solution.shape == (P.N, 2) for p in out) and any(0 < p.kept < P.N for p in out)

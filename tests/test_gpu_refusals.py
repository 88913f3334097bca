"""What a context accepts, through the C ABI: every case of tests/refusal_cases.py replayed on the device and compared, call by call, with the
pair (status, text of fh_last_error) that tests/golden/refusals/c_abi.json holds -- with `==`: a refusal is behaviour down to its last
character, and so is a call that used to succeed.  The fixture is taken by scripts/make_refusal_golden.py."""
import pytest

from fasta_python_amd import hip
from tests import refusal_cases as RC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return RC.load_golden()["cases"]


@pytest.mark.parametrize("case", RC.CASES, ids=RC.IDS)
def test_every_call_answers_as_the_fixture_says(case, golden):
    want = golden[case[0]]["got"]
    got = RC.replay(hip.load_library(), case)
    names = [name for name, _ in case[2]] + ["fh_step_end"]
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"call {k} ({names[k]}) of {case[0]}"
    assert len(got) == len(want)

"""The fixture of tests/test_gpu_refusals.py against the list it was taken from (tests/refusal_cases.py), without a device: it holds exactly
the cases and the calls of the list, the list covers every prox kind and every operator setter hip.py knows -- one added later fails here until
the fixture is taken again (scripts/make_refusal_golden.py) -- the operators are set at shapes at which they succeed, and every operator form
has at least one refusal on record."""
import os
import re

from fasta_python_amd import hip
from tests import refusal_cases as RC

GOLDEN = RC.load_golden()


def test_the_fixture_holds_exactly_the_cases_of_the_list():
    assert re.fullmatch(r"[0-9a-f]{40}", GOLDEN["commit"])
    assert sorted(GOLDEN["cases"]) == sorted(RC.IDS)
    for cid, state, calls in RC.CASES:
        rec = GOLDEN["cases"][cid]
        assert rec["calls"] == [name for name, _ in calls], cid
        assert len(rec["got"]) == len(calls) + (1 if state.endswith("in_flight") else 0), cid          # (fh_step_end closes a step in flight)
        for status, text in rec["got"]:
            assert isinstance(status, int) and (text == "") == (status == 0) or text.startswith("L = "), cid


def test_the_list_is_built_from_the_constants_of_the_binding():
    kinds = sorted(v for k, v in vars(hip).items() if k.startswith("PROX_"))
    assert kinds == RC.KINDS == list(range(len(kinds)))
    assert set(RC.HOME_OF) <= set(kinds)
    # every way the ABI has to set something is either swept as an operator setter or known not to be one
    setters = {n for n in hip.SIGNATURES if n.startswith("fh_set_") or n == "fh_generate_matrix"}
    assert setters == set(RC.OPERATOR_SETTERS) | RC.NOT_OPERATOR_SETTERS
    assert not set(RC.OPERATOR_SETTERS) & RC.NOT_OPERATOR_SETTERS
    called = {name for _, _, calls in RC.CASES for name, _ in calls}
    assert setters - {"fh_set_tuning", "fh_set_vector"} <= called
    # every kind, one below and one above, on every form; every kind before every form; every setter in every state
    for form in RC.FORMS:
        kinds_set = [args[0] for name, args in dict((c[0], c) for c in RC.CASES)[f"form/{form}/prox"][2] if name == "fh_set_prox"]
        assert kinds_set == [-1] + kinds + [len(kinds)]
        for kind in kinds:
            assert f"survive/{RC.KIND_NAMES[kind]}/{form}" in RC.IDS
    for state in RC.STATES:
        swept = {name for cid, st, calls in RC.CASES if st == state for name, _ in calls}
        assert set(RC.OPERATOR_SETTERS) <= swept, state


def test_every_operator_is_set_successfully_on_a_plain_context():
    for form, (setup, _, _, _) in RC.FORMS.items():
        for cid in (f"form/{form}/prox", f"form/{form}/loss", f"form/{form}/rhs", f"state/plain/{form}"):
            got = GOLDEN["cases"][cid]["got"][:len(setup)]
            assert got == [[0, ""]] * len(setup), cid
    assert GOLDEN["cases"]["state/plain/dense_generated"]["got"] == [[0, ""]]


def test_every_operator_form_has_a_refusal_on_record():
    refused = set()
    for cid, rec in GOLDEN["cases"].items():
        if cid.startswith("form/"):
            form = cid.split("/")[1]
            if any(status for status, _ in rec["got"][len(RC.FORMS[form][0]):]):
                refused.add(RC.OP_OF[form])
    with open(os.path.join(os.path.dirname(hip.__file__), "csrc", "fh_host_ctx.h")) as f:       # the enum itself: a form added there fails here
        forms = set(re.findall(r"\b(OP_[A-Z0-9]+) = \d+", re.search(r"enum \{ OP_NONE = 0,[^}]*\}", f.read()).group(0))) - {"OP_NONE"}
    assert len(forms) >= 9 and refused == set(RC.OP_OF.values()) == forms

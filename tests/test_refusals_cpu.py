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


def _operators_of_the_enum():
    with open(os.path.join(os.path.dirname(hip.__file__), "csrc", "fh_host_ctx.h")) as f:       # the enum itself: a form added there fails here
        return set(re.findall(r"\b(OP_[A-Z0-9]+) = \d+", re.search(r"enum \{ OP_NONE = 0,[^}]*\}", f.read()).group(0))) - {"OP_NONE"}


def test_every_operator_form_has_a_refusal_on_record():
    refused = set()
    for cid, rec in GOLDEN["cases"].items():
        if cid.startswith("form/"):
            form = cid.split("/")[1]
            if any(status for status, _ in rec["got"][len(RC.FORMS[form][0]):]):
                refused.add(RC.OP_OF[form])
    forms = _operators_of_the_enum()
    assert len(forms) >= 9 and refused == set(RC.OP_OF.values()) == forms


# the entry points that answer by operator form (csrc/fh_host_ctx.h: check_can and the rows' no_rows / no_apply; the guards of fh_sparse_lanes and
# of the fh_*_shape exports): fh_apply in both directions, so eighteen names
ENTRY_POINTS = ("fh_step", "fh_step_begin", "fh_step_accel", "fh_run", "fh_comm_init", "fh_get_matrix_rows", "fh_stream_read_ms", "fh_apply_forward",
                "fh_apply_adjoint", "fh_sparse_lanes", "fh_multi_shape", "fh_quad_shape", "fh_bilinear_shape", "fh_tv3d_shape", "fh_conv_shape",
                "fh_dct_shape", "fh_dct2_shape", "fh_nuclear_shape")


def test_the_entry_family_is_every_form_times_every_entry_point():
    family = [cid for cid in RC.IDS if cid.startswith("entry/")]
    assert sorted(family) == sorted(f"entry/{form}/{entry}" for form in RC.FORMS for entry in ENTRY_POINTS) and len(family) == 13 * 18
    cases = {c[0]: c for c in RC.CASES}
    for form, (setup, _, _, _) in RC.FORMS.items():
        for entry in ENTRY_POINTS:
            cid, state, calls = cases[f"entry/{form}/{entry}"]
            assert state == "plain", cid
            # the call the id names comes last (fh_step_begin: before its fh_step_end) and is the only one of the family in the case
            names = [name for name, _ in calls]
            called = "fh_apply" if entry.startswith("fh_apply") else entry
            assert names[-2:] == ["fh_step_begin", "fh_step_end"] if entry == "fh_step_begin" else names[-1] == called, cid
            assert sum(1 for n in names if n in ENTRY_POINTS or n == "fh_apply") == 1, cid
            if entry.startswith("fh_apply"):
                assert calls[-1][1][0] == (1 if entry.endswith("adjoint") else 0), cid
            # everything before it succeeded: the operator, the loss where the form takes one, fh_init
            before = len(calls) - len(RC.ENTRIES[entry])
            assert names[:before][-1] == "fh_init" and GOLDEN["cases"][cid]["got"][:before] == [[0, ""]] * before, cid


def test_every_operator_but_the_dense_one_has_an_entry_point_refusal_on_record():
    """... by an entry point that the form table decides, in a sentence about that operator: not merely the guards that refuse every other form."""
    refused = set()
    for form in RC.FORMS:
        for entry in ("fh_step", "fh_step_accel", "fh_run", "fh_comm_init", "fh_get_matrix_rows", "fh_stream_read_ms"):
            status, _ = GOLDEN["cases"][f"entry/{form}/{entry}"]["got"][-1]
            if status:
                refused.add(RC.OP_OF[form])
    assert refused >= _operators_of_the_enum() - {"OP_DENSE"}
    # the dense form itself is served by every one of them; in multi-column form it is refused the step, the loop and the sharding
    for entry in ("fh_step", "fh_step_begin", "fh_step_accel", "fh_run", "fh_comm_init", "fh_get_matrix_rows", "fh_stream_read_ms", "fh_apply_forward", "fh_apply_adjoint"):
        assert all(status == 0 for status, _ in GOLDEN["cases"][f"entry/dense/{entry}"]["got"]), entry

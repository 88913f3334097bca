"""What the Python front end recognises, against the fixture tests/golden/refusals/front_end.json (tests/front_end_cases.py has the list,
scripts/make_front_end_golden.py takes the fixture): every case's answer -- the whole sentence, or what the operands become -- with `==`; the
fixture holds exactly the list; and every sentence the recognition code of solver.py can say is said -- a sentence put together from parts:
each part -- to at least one case, so that a check that moves in front of another one changes an answer on record.  No device is touched; the
library's host functions are (DCTMap, ConvMap)."""
import ast
import inspect
import re

from fasta_python_amd import solver
from tests import front_end_cases as FC

COMMIT, GOLDEN = FC.load_golden()


def test_the_fixture_holds_exactly_the_cases_of_the_list():
    assert re.fullmatch(r"[0-9a-f]{40}", COMMIT)
    assert list(GOLDEN) == FC.ids() and len(GOLDEN) == len(set(GOLDEN)) >= 50000


def test_every_case_gets_the_answer_on_record():
    wrong = [(cid, got, GOLDEN[cid]) for cid in FC.ids() for got in (FC.answer(cid),) if got != GOLDEN[cid]]
    assert not wrong, (len(wrong), wrong[:3])


def test_the_two_thin_names_give_the_same_answers():
    """solver._unrecognised and solver._recognise, which tests and older callers import, are the two halves of the one walk."""
    trim = lambda a: {"recognised": a["recognised"][:6]} if isinstance(a, dict) and "recognised" in a else a
    wrong = [(cid, got, GOLDEN[cid]) for cid in FC.ids() for got in (FC.answer_of_the_two_names(cid),) if got != trim(GOLDEN[cid])]
    assert not wrong, (len(wrong), wrong[:3])


def test_the_list_reaches_every_kind_of_answer():
    answers = list(GOLDEN.values())
    assert any(isinstance(a, str) for a in answers) and any("raises" in a for a in answers if isinstance(a, dict))
    maps = {a["recognised"][0] for a in answers if isinstance(a, dict) and "recognised" in a}
    assert maps == {"DenseMatrixMap", "ShardedDenseMatrixMap", "SparseMatrixMap", "GradDivMap", "DCTMap", "ConvMap", "QuadraticMap", "BilinearMap", "IdentityMap"}
    owned = {a["recognised"][0] for a in answers if isinstance(a, dict) and "recognised" in a and a["recognised"][6]}
    assert owned == {"DenseMatrixMap", "SparseMatrixMap", "QuadraticMap", "BilinearMap", "IdentityMap"}
    # the library's own sentences pass through (DCTMap.refusal, ConvMap.refusal)
    assert sum(1 for a in set(a for a in answers if isinstance(a, str)) if a.startswith("[")) == 2


# ---- every sentence of the source is on record ------------------------------------------------------------------------------------------------------
def _sentences_of_the_source():
    """One regular expression per sentence the recognition code can say: the string literals (f-strings: their fixed text, a field matches
    anything) of solver.py from _tag_of up to FBSolver that read as a sentence -- a blank in them, twenty characters or more -- docstrings
    apart.  Literals that stand side by side are one literal to the parser, so a sentence written over several lines is one sentence here."""
    tree = ast.parse(inspect.getsource(solver))
    first = next(n.lineno for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "_tag_of")
    last = next(n.lineno for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "FBSolver")
    out = []

    def pattern(node):
        if isinstance(node, ast.Constant):
            return re.sub(r"\\\{[^{}]*\\\}", ".*", re.escape(node.value)) if isinstance(node.value, str) else None
        return "".join(re.escape(v.value) if isinstance(v, ast.Constant) else ".*" for v in node.values)

    def visit(node, docstring_of=None):
        if isinstance(node, (ast.Constant, ast.JoinedStr)):
            text = node.value if isinstance(node, ast.Constant) else "".join(v.value for v in node.values if isinstance(v, ast.Constant))
            if isinstance(text, str) and node is not docstring_of and " " in text and len(text) >= 20:
                out.append(pattern(node))
            return                                      # (what an f-string's fields hold is part of that sentence)
        doc = docstring_of
        if isinstance(node, (ast.FunctionDef, ast.ClassDef)) and node.body and isinstance(node.body[0], ast.Expr):
            doc = node.body[0].value
        for child in ast.iter_child_nodes(node):
            visit(child, doc)

    for node in tree.body:
        if first <= node.lineno < last:
            visit(node)
    return out


def test_every_sentence_of_the_recognition_code_is_said_to_some_case():
    said = {a for a in GOLDEN.values() if isinstance(a, str)} | {a["raises"].split(": ", 1)[1] for a in GOLDEN.values() if isinstance(a, dict) and "raises" in a}
    patterns = _sentences_of_the_source()
    unsaid = [p for p in patterns if not any(re.search(p, s, re.S) for s in said)]
    assert len(patterns) >= 60 and len(said) >= len(set(patterns)) and not unsaid, unsaid

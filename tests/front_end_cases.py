"""What tests/test_front_end_cpu.py and scripts/make_front_end_golden.py share about what the Python front end RECOGNISES: the list of calls whose
answer -- the whole sentence of solver._unrecognised, or what solver._recognise makes of the seven operands -- is pinned in
tests/golden/refusals/front_end.json.  It is the counterpart of tests/refusal_cases.py one layer up: that one pins what a context accepts, this one
what fasta() and path() hand to a context at all, and in which words they decline.  The fixture is taken on the CPU, on the commit whose
answers are to be kept, and compared with `==`; it must be taken again whenever a form, a tag or a sentence is added.

A case is (id, how to build the seven operands from plain values): the id is "<operator>/<loss>/<prox>/<x0>", one name from each of the four
tables below, and the list is their product.  Shapes are a few rows and columns; every map is lazy, so no context is created.  The DCT and the
convolution operator ask the library's host functions for their refusal (DCTMap.refusal, ConvMap.refusal): the library must be built, as for
tests/test_dct_cpu.py.

The answer of a case: the sentence; or, where there is none, {"recognised": [map class, Vshape, Wshape, rhs, loss class, prox class, whether
fasta() would own the map]}; or, where building the map raises, {"raises": "<exception class>: <text>"}.  All of it, the owner included, comes
from one call of solver._front_end, the call fasta() and path() make (answer())."""
import itertools
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refusals", "front_end.json")
M, N = 3, 5                                         # the matrices; the square ones are N x N, the factorised one is 2 x 3 (2 + 3 = N rows)


def _matrix():
    return np.array([((7 * i) % 5 - 2) / 4.0 for i in range(M * N)]).reshape(M, N)


def _csr():
    from scipy import sparse as sp
    return sp.csr_matrix(_matrix() * (np.arange(M * N).reshape(M, N) % 3 != 0))


def _operators():
    """name -> (A, At).  Built once: recognition reads a map, it does not change it."""
    import fasta_python_amd as fa
    from fasta_python_amd import linalg
    A, S = _matrix(), _csr()
    Q = np.eye(N) * 2.0
    out = {
        "ndarray": (A, None), "ndarray_with_At": (A, A.T.copy()), "ndarray_with_a_wrong_At": (A, A), "ndarray_1d": (np.ones(N), None),
        "scipy": (S, None), "scipy_with_a_wrong_At": (S, S),
        "none": (None, None), "closure": (lambda x: x, lambda y: y),
        "LinearMap": (linalg.LinearMap(lambda x: A @ x, lambda y: A.T @ y, (N,), (M,)), None),
        "DenseMatrixMap": (fa.DenseMatrixMap(A), None), "DenseMatrixMap_rhs": (fa.DenseMatrixMap(A, rhs=2), None),
        "DenseMatrixMap_f32": (fa.DenseMatrixMap(A, storage="f32"), None), "ShardedDenseMatrixMap": (fa.ShardedDenseMatrixMap(A, devices=(0, 0)), None),
        "SparseMatrixMap": (fa.SparseMatrixMap(S), None), "SparseMatrixMap_rhs": (fa.SparseMatrixMap(S, rhs=2), None),
        "GradDivMap": (fa.GradDivMap((1, 1, N)), None),
        "DCTMap": (fa.DCTMap(N, lazy=True), None), "DCTMap_2d": (fa.DCTMap((N, 2), lazy=True), None), "DCTMap_refused": (fa.DCTMap(7, lazy=True), None),
        "ConvMap": (fa.ConvMap((N, 2), np.ones((2, 2))), None), "ConvMap_1d": (fa.ConvMap((N,), np.ones(3)), None),
        "ConvMap_refused": (fa.ConvMap((20,), np.ones(17)), None),
        "QuadraticMap": (fa.QuadraticMap(fa.Quadratic(Q), (N,)), None), "BilinearMap": (fa.BilinearMap(fa.Factorization(np.ones((2, 3))), (N, 2)), None),
        "IdentityMap": (fa.IdentityMap((N, 2)), None),
    }
    classes = {c.__name__ for c in vars(linalg).values() if isinstance(c, type) and issubclass(c, linalg.LinearMap)} - {"_DeviceMap"}
    assert classes == {type(a).__name__ for a, _ in out.values()} & classes and len(classes) == 10, classes
    return out


def _data_shape(A, x0):
    """The shape of b: the operator's Wshape, a matrix's rows by x0's columns, or -- the identity, a closure -- x0's own shape."""
    if type(A).__name__ == "IdentityMap" and x0 is not None:
        return tuple(np.shape(x0))
    if getattr(A, "Wshape", None) is not None:
        return tuple(A.Wshape)
    if getattr(A, "shape", None) is not None:
        return (A.shape[0],) + (() if x0 is None or np.ndim(x0) != 2 else (np.shape(x0)[1],))
    return (N, 2) if x0 is None else tuple(np.shape(x0))


LOSSES = ("lsq", "logistic", "softmax", "quadratic", "quadratic_with_c", "factorization", "lsq_weighted", "logistic_weighted",
          "lsq_f_of_one_gradf_of_another", "lsq_f_logistic_gradf", "lsq_f_closure_gradf", "closure_f_lsq_gradf", "closures",
          "softmax_f_closure_gradf", "quadratic_f_closure_gradf", "closure_f_factorization_gradf", "lsq_of_another_shape")


def _loss(name, shape):
    """(f, gradf) of the loss called `name` for data of `shape`."""
    import fasta_python_amd as fa
    b = np.ones(shape)
    f = lambda z: 0.0
    tags = {"lsq": lambda: fa.LeastSquares(b), "logistic": lambda: fa.LogisticLoss(b),
            "softmax": lambda: fa.SoftmaxLoss(np.arange(shape[0] if shape else 1) % 2, classes=2),
            "quadratic": lambda: fa.Quadratic(np.eye(N) * 2.0), "quadratic_with_c": lambda: fa.Quadratic(np.eye(N) * 2.0, c=np.ones(N)),
            "factorization": lambda: fa.Factorization(np.ones((2, 3))),
            "lsq_of_another_shape": lambda: fa.LeastSquares(np.ones(7)),
            "lsq_weighted": lambda: fa.LeastSquares(b, weights=np.ones(shape)), "logistic_weighted": lambda: fa.LogisticLoss(b, weights=np.ones(shape))}
    if name in tags:
        tag = tags[name]()
        return tag.f, tag.gradf
    pairs = {"lsq_f_of_one_gradf_of_another": lambda: (fa.LeastSquares(b).f, fa.LeastSquares(b).gradf),
             "lsq_f_logistic_gradf": lambda: (fa.LeastSquares(b).f, fa.LogisticLoss(b).gradf),
             "lsq_f_closure_gradf": lambda: (fa.LeastSquares(b).f, f), "closure_f_lsq_gradf": lambda: (f, fa.LeastSquares(b).gradf),
             "closures": lambda: (f, f), "softmax_f_closure_gradf": lambda: (tags["softmax"]().f, f),
             "quadratic_f_closure_gradf": lambda: (tags["quadratic"]().f, f), "closure_f_factorization_gradf": lambda: (f, tags["factorization"]().gradf)}
    return pairs[name]()


def _prox():
    """name -> (g, proxg).  Built once."""
    import fasta_python_amd as fa
    from fasta_python_amd import proximal
    tags = {"NoProx": proximal.NoProx(), "Shrink": fa.Shrink(0.5), "NonNeg": fa.NonNeg(), "LinfProx": fa.LinfProx(0.5), "L1Ball": fa.L1Ball(0.5),
            "Box": fa.Box(-1.0, 1.0), "TVDualBall": fa.TVDualBall(), "GroupShrink": fa.GroupShrink(0.5), "RowBall": fa.RowBall(0.5),
            "RowSplit": fa.RowSplit(2, fa.Shrink(0.5), fa.NonNeg()), "RowSplit_elsewhere": fa.RowSplit(1, fa.Shrink(0.5), fa.NonNeg()),
            "NuclearShrink": fa.NuclearShrink(0.5), "NuclearBall": fa.NuclearBall(0.5)}
    every = {c.__name__ for c in vars(proximal).values() if isinstance(c, type) and issubclass(c, proximal.ProxTag) and c is not proximal.ProxTag}
    assert every == {type(t).__name__ for t in tags.values()}, every
    out = {name: (tag.g, tag.prox) for name, tag in tags.items()}
    h = lambda x, t=None: x
    out.update({"none": (None, None), "closures": (h, h), "g_of_one_prox_of_another": (fa.Shrink(0.5).g, fa.Shrink(0.5).prox),
                "no_g_prox_of_a_tag": (None, fa.Shrink(0.5).prox), "closure_g_prox_of_a_tag": (h, fa.Shrink(0.5).prox),
                "g_of_a_tag_closure_prox": (fa.Shrink(0.5).g, h), "g_of_a_tag_no_prox": (fa.Shrink(0.5).g, None)})
    return out


X0S = ("vector", "matrix", "matrix_of_16", "matrix_of_17", "matrix_of_0", "wrong", "none", "the_operators_own")


def _x0(name, A):
    if name == "the_operators_own":
        V = getattr(A, "Vshape", None)
        return np.zeros((N, N)) if V is None else np.zeros(V)
    return {"vector": np.zeros(N), "matrix": np.zeros((N, 2)), "matrix_of_16": np.zeros((N, 16)), "matrix_of_17": np.zeros((N, 17)),
            "matrix_of_0": np.zeros((N, 0)), "wrong": np.zeros(N + 1), "none": None}[name]


_TABLES = {}


def tables():
    if not _TABLES:
        _TABLES.update(operators=_operators(), prox=_prox())
    return _TABLES["operators"], _TABLES["prox"]


def axes():
    """The four lists of names the ids are the product of, in the order of the fixture."""
    operators, prox = tables()
    return [list(operators), list(LOSSES), list(prox), list(X0S)]


def _beyond_the_nuclear_rank(tag):
    """A 1025 x 1025 unknown on the identity operator: beyond the rank the nuclear-norm prox serves (too large a B to build once per case of the product)."""
    import fasta_python_amd as fa
    X0 = np.zeros((1025, 1025))
    ls = fa.LeastSquares(X0)
    return (None, None, ls.f, ls.gradf, tag.g, tag.prox, X0)


def _extras():
    import fasta_python_amd as fa
    return {"extra/beyond_the_nuclear_rank/NuclearShrink": lambda: _beyond_the_nuclear_rank(fa.NuclearShrink(0.5)),
            "extra/beyond_the_nuclear_rank/NuclearBall": lambda: _beyond_the_nuclear_rank(fa.NuclearBall(0.5)),
            "extra/beyond_the_nuclear_rank/Shrink": lambda: _beyond_the_nuclear_rank(fa.Shrink(0.5))}


def ids():
    """The product of the four tables, then the few cases that are not of it."""
    return ["/".join(names) for names in itertools.product(*axes())] + list(_extras())


def operands(cid):
    """The seven operands of the case, built from plain values."""
    if cid.startswith("extra/"):
        return _extras()[cid]()
    operators, prox = tables()
    op, loss, px, x0 = cid.split("/")
    A, At = operators[op]
    x0 = _x0(x0, A)
    f, gradf = _loss(loss, _data_shape(A, x0))
    g, proxg = prox[px]
    return A, At, f, gradf, g, proxg, x0


def answer(cid):
    """What the front end says to the case (the module text): from the one call fasta() and path() make, solver._front_end, with x0 as the caller
    gave it.  On a commit from before that function -- to take the fixture there -- from the two calls fasta() made, with its own rule for who
    closes the map."""
    from fasta_python_amd import solver
    A, At, f, gradf, g, proxg, x0 = operands(cid)
    try:
        if hasattr(solver, "_front_end"):
            found = solver._front_end(A, At, f, gradf, g, proxg, x0)
            if isinstance(found, str):
                return found
            op, loss, prox, owns = found
        else:
            from fasta_python_amd.linalg import is_sparse_matrix
            why_not = solver._unrecognised(A, At, f, gradf, g, proxg, x0)
            if why_not is not None:
                return why_not
            owns = A is None or isinstance(A, np.ndarray) or is_sparse_matrix(A)
            op, loss, prox = solver._recognise(A, At, f, gradf, g, proxg, np.asarray(x0, dtype=np.float64))
    except Exception as exc:
        return {"raises": "%s: %s" % (type(exc).__name__, exc)}
    return {"recognised": [type(op).__name__, list(op.Vshape), list(op.Wshape), getattr(op, "rhs", None), type(loss).__name__, type(prox).__name__, bool(owns)]}


def answer_of_the_two_names(cid):
    """The same answer from the two names tests and older callers import: solver._unrecognised, then solver._recognise (without the owner)."""
    from fasta_python_amd import solver
    A, At, f, gradf, g, proxg, x0 = operands(cid)
    why_not = solver._unrecognised(A, At, f, gradf, g, proxg, x0)
    if why_not is not None:
        return why_not
    try:
        op, loss, prox = solver._recognise(A, At, f, gradf, g, proxg, np.asarray(x0, dtype=np.float64))
    except Exception as exc:
        return {"raises": "%s: %s" % (type(exc).__name__, exc)}
    return {"recognised": [type(op).__name__, list(op.Vshape), list(op.Wshape), getattr(op, "rhs", None), type(loss).__name__, type(prox).__name__]}


# ---- the fixture's file --------------------------------------------------------------------------------------------------------------------------------
# Most cases get one of a few hundred answers, and most operators, losses and prox operands get the same answers as a neighbour.  The file says each
# thing once: "answers" the distinct answers; "by_x0" the distinct rows of answer numbers along the last list of names; "by_prox" the distinct rows
# of by_x0 numbers along the prox operands; "by_loss" the same one level up; "operators" one by_loss number per operator; "extras" name -> answer number.
LEVELS = ("by_x0", "by_prox", "by_loss")


def _fold(values, width, table):
    """`values` cut into rows of `width`; each row's number in `table` (appended to where it is new)."""
    seen = {tuple(row): k for k, row in enumerate(table)}
    out = []
    for at in range(0, len(values), width):
        row = tuple(values[at:at + width])
        if row not in seen:
            seen[row] = len(table)
            table.append(list(row))
        out.append(seen[row])
    return out


def dump_golden(path, commit, answers_of):
    """Write the fixture from {id: answer} over exactly ids()."""
    names = ids()
    assert list(answers_of) == names
    answers, number = [], {}
    for got in answers_of.values():
        key = json.dumps(got, sort_keys=True)
        if key not in number:
            number[key] = len(answers)
            answers.append(got)
    flat = [number[json.dumps(answers_of[cid], sort_keys=True)] for cid in names]
    ax = axes()
    product = len(flat) - len(_extras())
    G = {"commit": commit, "axes": ax, "answers": answers, "extras": dict(zip(names[product:], flat[product:]))}
    values = flat[:product]
    for level, width in zip(LEVELS, (len(ax[3]), len(ax[2]), len(ax[1]))):
        G[level] = []
        values = _fold(values, width, G[level])
    G["operators"] = values
    rows = lambda v: "[\n" + ",\n".join(json.dumps(r) for r in v) + "\n]"
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join('"%s": %s' % (k, rows(G[k]) if k in LEVELS + ("answers", "axes") else json.dumps(G[k])) for k in sorted(G)) + "\n}\n")
    return len(names), len(answers)


def load_golden():
    """(the commit, {id: answer}) of the fixture."""
    with open(GOLDEN) as f:
        G = json.load(f)
    values = G["operators"]
    for level in reversed(LEVELS):
        values = [k for v in values for k in G[level][v]]
    names = ["/".join(t) for t in itertools.product(*G["axes"])]
    assert len(names) == len(values)
    out = {cid: G["answers"][k] for cid, k in zip(names, values)}
    out.update({cid: G["answers"][k] for cid, k in G["extras"].items()})
    return G["commit"], out

"""Capture the fixtures of a MATRIX unknown over a SPARSE operator, tests/golden/sparse_mmv/*.npz, from the REFERENCE core, the way
scripts/make_sparse_golden.py captures the vector ones and scripts/make_mmv_golden.py the dense matrix-unknown ones:

    MPLBACKEND=Agg python scripts/make_sparse_mmv_golden.py <path to the reference checkout>

The operator is the closure pair the reference is given for a scipy.sparse matrix S and an (n, L) unknown:
`LinearMap(lambda X: S @ X, lambda Y: S.T @ Y, (n, L), (m, L))`; f, gradf, g, proxg are the closures the two scripts above restate
(examples/mmv.py:49-61 for the row-wise shrink, sparse_least_squares.py:41-44, nn_least_squares.py:39-42, svm.py:71 for the box), over
matrices.  Stored: the canonical CSR arrays of S, the other inputs, every history and the solution.
Every full-length case is a run that does NOT depend on the order of its sums: its regularisation weight was chosen so that the NumPy
oracle and a copy of itself with permuted ROWS of S (same probes, another summation order in S.T @ Y) agree on every step size of the whole
solve (`row_permuted_divergence`; on the skewed matrix a weight of 1 or 2 lets the twin part after 49 to 79 of 90 to 120 iterations, 4 does
not) -- tests/test_sparse_mmv_cpu.py asserts it, so the device runs are held to the full histories.
The forced-backtracking case stores, in its meta, the iteration at which the oracle parts from a copy of itself whose unknowns are permuted
(columns of S, rows of X) and the reference's backtracks up to there; it is compared only to that point.
Our own code and data only: nothing of the reference is copied."""
import importlib.util
import json
import os
import sys
import warnings

import numpy as np
from numpy import linalg as la
from scipy import sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "sparse_mmv")
TEST_MODES = dict(tolerance=1e-5, evaluate_objective=True)            # examples/__init__.py:63-91
MODES = {"adaptive": dict(adaptive=True, accelerate=False), "accelerated": dict(adaptive=False, accelerate=True),
         "plain": dict(adaptive=False, accelerate=False)}


def _sparse_script():
    """scripts/make_sparse_golden.py: the seeded matrix generators (the skewed one among them) are stated there, once."""
    spec = importlib.util.spec_from_file_location("make_sparse_golden", os.path.join(ROOT, "scripts", "make_sparse_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def construct(kind, m, n, L, density=0.1, K=8, sigma=0.05, mu=1.0, skewed=False):
    """The problem data from the global RNG (seeded by the caller): matrix, row-sparse truth (K live rows), right-hand sides."""
    gen = _sparse_script()
    rs = np.random.RandomState(np.random.randint(1 << 30))
    S = gen.skewed_csr(m, n, rs) if skewed else gen.random_csr(m, n, density, rs)
    X = np.zeros((n, L))
    support = np.random.permutation(n)[:K]
    X[support] = np.abs(np.random.randn(K, L)) + 0.5 if kind == "nnls" else np.random.randn(K, L)
    B = S @ X + sigma * np.random.randn(m, L)
    d = dict(data=S.data.astype(np.float64), indices=S.indices.astype(np.int32), indptr=S.indptr.astype(np.int64),
             shape=np.array(S.shape, dtype=np.int64), B=B, mu=np.float64(mu), X=X)
    if kind == "box":
        d["lo"], d["hi"] = np.float64(-0.25), np.float64(0.5)
    return d


def matrix_of(d):
    return sp.csr_matrix((d["data"], d["indices"], d["indptr"]), shape=tuple(int(k) for k in d["shape"]))


def closures(kind, d, shrink):
    """f, gradf, g, proxg of the reference's examples over the data `d`; `shrink` = the soft-threshold to use inside the prox."""
    B, mu = d["B"], float(d["mu"])
    f = lambda Z: .5 * la.norm((Z - B).ravel()) ** 2
    gradf = lambda Z: Z - B
    if kind == "mmv":                                        # examples/mmv.py:49-61

        def prox_rows(X, t):
            norms = la.norm(X, axis=1)
            scale = shrink(norms, t) / (norms + (norms == 0))
            return X * scale[:, np.newaxis]

        return f, gradf, (lambda X: mu * np.sum(np.sqrt(np.sum(X * X, axis=1)))), (lambda X, t: prox_rows(X, mu * t))
    if kind in ("lasso", "skewed"):
        return f, gradf, (lambda X: mu * la.norm(X.ravel(), 1)), (lambda X, t: shrink(X, t * mu))
    if kind == "nnls":
        return f, gradf, (lambda X: 0), (lambda X, t: np.maximum(X, 0))
    if kind == "box":
        lo, hi = float(d["lo"]), float(d["hi"])
        return f, gradf, (lambda X: 0), (lambda X, t: np.minimum(np.maximum(X, lo), hi))
    raise KeyError(kind)


def case_table():
    """(name, kind, construct kwargs, problem seed, solver seed, options)"""
    cases = [(f"mmv_60x90x5_{mode}", "mmv", dict(m=60, n=90, L=5, density=0.1, K=7, mu=1.0), 71, 701, dict(TEST_MODES, **mo)) for mode, mo in MODES.items()]
    cases.append(("lasso_120x200x3_adaptive", "lasso", dict(m=120, n=200, L=3, density=0.05, K=10, mu=0.5), 72, 702, dict(TEST_MODES, **MODES["adaptive"])))
    cases.append(("nnls_150x80x16_accelerated", "nnls", dict(m=150, n=80, L=16, density=0.08, K=10), 73, 703, dict(TEST_MODES, **MODES["accelerated"])))
    cases.append(("box_100x60x2_plain", "box", dict(m=100, n=60, L=2, density=0.2, K=10), 74, 704, dict(TEST_MODES, **MODES["plain"])))
    cases.append(("skewed_257x515x8_adaptive", "skewed", dict(m=257, n=515, L=8, K=12, mu=4.0, skewed=True), 75, 705, dict(TEST_MODES, **MODES["adaptive"])))
    # a first step far beyond 2 / L: the solve opens with a run of backtracks
    cases.append(("mmv_40x60x10_backtracks", "mmv", dict(m=40, n=60, L=10, density=0.1, K=7, mu=1.0), 76, 706,
                  dict(tolerance=1e-5, L=1.0, tau0=50.0, evaluate_objective=True, max_iters=300)))
    return cases


def resolve(opts, stopping_module):
    o = dict(opts)
    if isinstance(o.get("stop_rule"), str):
        o["stop_rule"] = getattr(stopping_module, o["stop_rule"])
    return o


def run(core, linear_map, shrink, kind, d, opts, sseed, S=None, **extra):
    """One solve with the closure LinearMap over S, by `core.fasta` (the reference's, or the oracle's)."""
    S = matrix_of(d) if S is None else S
    (m, n), L = S.shape, d["B"].shape[1]
    f, gradf, g, proxg = closures(kind, d, shrink)
    A = linear_map(lambda X: S @ X, lambda Y: S.T @ Y, (n, L), (m, L))
    np.random.seed(sseed)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return core.fasta(A, f, gradf, g, proxg, np.zeros((n, L)), **extra, **resolve(opts, core))


def _oracle():
    sys.path.insert(0, ROOT)
    from oracle import fasta_np as fo
    from tests.helpers import first_divergence
    return fo, first_divergence


def permuted_divergence(kind, d, opts, sseed):
    """First iteration at which the oracle's step sizes differ (> 1e-6 relative) between the problem and the same problem with its
    unknowns permuted (columns of S) -- the same mathematics, another summation order in S @ X; the shorter iteration count if they never do."""
    fo, first_divergence = _oracle()
    S = matrix_of(d)
    runs = []
    for perm in (np.arange(S.shape[1]), np.random.RandomState(7).permutation(S.shape[1])):
        Sp = S[:, perm].tocsr()
        Sp.sort_indices()
        runs.append(run(fo, fo.LinearMap, fo.shrink, kind, d, opts, sseed, S=Sp))
    k = min(runs[0].iteration_count, runs[1].iteration_count)
    return first_divergence(runs[1].stepsizes, runs[0].stepsizes, k)


def row_permuted_divergence(kind, d, opts, sseed):
    """The same for permuted ROWS of S (and of B): the Lipschitz probes keep their order, only the sums of S.T @ Y change theirs."""
    fo, first_divergence = _oracle()
    S = matrix_of(d)
    perm = np.random.RandomState(7).permutation(S.shape[0])
    Sp = S[perm].tocsr()
    Sp.sort_indices()
    runs = [run(fo, fo.LinearMap, fo.shrink, kind, d, opts, sseed), run(fo, fo.LinearMap, fo.shrink, kind, dict(d, B=d["B"][perm]), opts, sseed, S=Sp)]
    if runs[0].iteration_count != runs[1].iteration_count:
        return min(first_divergence(runs[1].stepsizes, runs[0].stepsizes, min(r.iteration_count for r in runs)), min(r.iteration_count for r in runs) - 1)
    return first_divergence(runs[1].stepsizes, runs[0].stepsizes, runs[0].iteration_count)


def main(reference):
    sys.path.insert(0, reference)
    os.environ.setdefault("MPLBACKEND", "Agg")
    import fasta as ref
    assert os.path.abspath(ref.__file__).startswith(os.path.abspath(reference)), ref.__file__

    class RefCore:                                   # the reference's fasta() and stop rules under one name
        fasta = staticmethod(ref.fasta)
    for rule in ("residual", "norm_residual", "ratio_residual", "hybrid_residual"):
        setattr(RefCore, rule, staticmethod(getattr(ref.stopping, rule)))
    os.makedirs(OUT, exist_ok=True)
    for name, kind, ckw, pseed, sseed, opts in case_table():
        np.random.seed(pseed)
        d = construct(kind, **ckw)
        c = run(RefCore, ref.linalg.LinearMap, ref.proximal.shrink, kind, d, opts, sseed, verbose=False)
        out = dict(residuals=c.residuals, norm_residuals=c.norm_residuals, stepsizes=c.stepsizes, backtracks=np.int64(c.backtracks),
                   iteration_count=np.int64(c.iteration_count), solution=c.solution)
        if c.objectives is not None:
            out["objectives"] = c.objectives
        meta = dict(name=name, kind=kind, construct=ckw, problem_seed=pseed, solver_seed=sseed, options=opts, numpy=np.__version__)
        note = ""
        if "backtracks" in name:
            meta["permuted_divergence"] = permuted_divergence(kind, d, opts, sseed)
            # ... and the reference's backtracks within that prefix (the same run cut there: the trajectory does not depend on max_iters)
            cut = run(RefCore, ref.linalg.LinearMap, ref.proximal.shrink, kind, d, dict(opts, max_iters=meta["permuted_divergence"], tolerance=0.0), sseed, verbose=False)
            assert np.array_equal(cut.stepsizes[:meta["permuted_divergence"]], c.stepsizes[:meta["permuted_divergence"]])
            meta["backtracks_at_divergence"] = int(cut.backtracks)
            note = f" permuted copy parts at {meta['permuted_divergence']} ({meta['backtracks_at_divergence']} backtracks up to there)"
        else:
            twin = row_permuted_divergence(kind, d, opts, sseed)
            note = f" row-permuted twin agrees for {twin} of {int(c.iteration_count)}"
            assert twin == int(c.iteration_count), f"{name}: the row-permuted twin parts at {twin}: choose another weight"
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, meta=json.dumps(meta), **{"in_" + k: np.asarray(v) for k, v in d.items()}, **out)
        print(f"{name:32s} nnz={d['data'].size:6d} iters={int(c.iteration_count):4d} backtracks={int(c.backtracks):3d} {os.path.getsize(path):7d} B" + note)


if __name__ == "__main__":
    main(sys.argv[1])

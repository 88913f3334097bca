"""Capture the sparse-operator fixtures tests/golden/sparse/*.npz from the REFERENCE core, the way scripts/make_mmv_golden.py captures the
matrix-unknown ones:

    MPLBACKEND=Agg python scripts/make_sparse_golden.py <path to the reference checkout>

The operator is what the reference is given for a scipy.sparse design matrix S: `LinearMap(lambda x: S @ x, lambda y: S.T @ y, (n,), (m,))`;
f, gradf, g, proxg are the closures of its examples (sparse_least_squares.py:41-44, nn_least_squares.py:39-42, sparse_logistic.py:47-50,
svm.py:71 for the box), restated here.  Stored: the canonical CSR arrays of S, the other inputs, every history and the solution.  The
forced-backtracking case also stores, in its meta, the iteration at which the NumPy oracle parts from a copy of itself whose unknowns are
permuted (columns of S): how far summation order alone lets two correct solvers agree on that run -- tests/test_sparse_cpu.py recomputes
it, tests/test_gpu_sparse.py pins the device run up to there.
Every other case is a run that does NOT depend on the order of its sums: its regularisation weight and shape were chosen so that the oracle
and a copy of itself with permuted ROWS (same probes, another summation order in S.T @ y) agree on every step size of the whole solve
(`row_permuted_divergence` below; with a weight of 0.1 on these matrices the adaptive runs collect 30-360 backtracks and the twin already
differs in its iteration count) -- tests/test_sparse_cpu.py asserts it, so the device runs can be held to the full histories.
The skewed 257 x 515 matrix has the shape the cases were specified with: its dense row (505 entries, G = 4 on A) is walked by a workgroup
of its own, its dense column (247 entries) stays below the 256-entry threshold of the A^T copy; the whole-workgroup path of the adjoint is
covered by the larger matrices of tests/test_gpu_sparse.py (a dense column of 9000 / 5000 entries), not by this fixture.
Our own code and data only: nothing of the reference is copied."""
import json
import os
import sys
import warnings

import numpy as np
from numpy import linalg as la
from scipy import sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "sparse")
TEST_MODES = dict(tolerance=1e-5, evaluate_objective=True)            # examples/__init__.py:63-91
MODES = {"adaptive": dict(adaptive=True, accelerate=False), "accelerated": dict(adaptive=False, accelerate=True),
         "plain": dict(adaptive=False, accelerate=False)}


def random_csr(m, n, density, rs):
    """A seeded random sparse matrix with standard-normal entries, canonical CSR."""
    S = sp.random(m, n, density=density, format="csr", random_state=rs, data_rvs=rs.standard_normal)
    S.sum_duplicates()
    S.sort_indices()
    return S


def skewed_csr(m, n, rs):
    """One fully dense row, one column with an entry in every non-empty row, ten empty rows, ten empty columns, every other row 1-3 entries."""
    empty_rows, empty_cols = set(range(5, 15)), set(range(20, 30))
    dense_row, dense_col = 100, 200
    live_cols = np.array([j for j in range(n) if j not in empty_cols])
    rows, cols = [], []
    for i in range(m):
        if i in empty_rows:
            continue
        if i == dense_row:
            js = live_cols
        else:                                    # 1-3 entries, one of them in the dense column
            others = live_cols[live_cols != dense_col]
            js = np.sort(np.append(rs.choice(others, size=rs.randint(0, 3), replace=False), dense_col))
        rows += [i] * len(js)
        cols += list(js)
    S = sp.csr_matrix((rs.standard_normal(len(rows)), (rows, cols)), shape=(m, n))
    S.sum_duplicates()
    S.sort_indices()
    return S


def construct(kind, m, n, density=0.05, K=10, sigma=0.05, mu=0.1, skewed=False):
    """The problem data from the global RNG (seeded by the caller): matrix, sparse truth, right-hand side."""
    rs = np.random.RandomState(np.random.randint(1 << 30))
    S = skewed_csr(m, n, rs) if skewed else random_csr(m, n, density, rs)
    x = np.zeros(n)
    support = np.random.permutation(n)[:K]
    if kind == "logistic":                                   # sparse_logistic.py: a 0/1 signal, labels from the logistic model
        x[support] = 1.0
        prob = 1.0 / (1.0 + np.exp(-(S @ x)))
        b = 2.0 * (np.random.rand(m) < prob) - 1.0
    elif kind == "nnls":                                     # nn_least_squares.py: a non-negative signal
        x[support] = np.abs(np.random.randn(K)) + 0.5
        b = S @ x + sigma * np.random.randn(m)
    else:
        x[support] = np.random.randn(K)
        b = S @ x + sigma * np.random.randn(m)
    d = dict(data=S.data.astype(np.float64), indices=S.indices.astype(np.int32), indptr=S.indptr.astype(np.int64),
             shape=np.array(S.shape, dtype=np.int64), b=b, mu=np.float64(mu), x=x)
    if kind == "box":
        d["lo"], d["hi"] = np.float64(-0.25), np.float64(0.5)
    return d


def matrix_of(d):
    return sp.csr_matrix((d["data"], d["indices"], d["indptr"]), shape=tuple(int(k) for k in d["shape"]))


def closures(kind, d, shrink):
    """f, gradf, g, proxg of the reference's examples over the data `d`; `shrink` = the soft-threshold to use inside the prox."""
    b, mu = d["b"], float(d["mu"])
    if kind == "logistic":
        f = lambda z: np.sum(np.log(1 + np.exp(z)) - (b == 1) * z)
        gradf = lambda z: -b / (1 + np.exp(b * z))
    else:
        f = lambda z: .5 * la.norm((z - b).ravel()) ** 2
        gradf = lambda z: z - b
    if kind in ("lasso", "logistic", "skewed"):
        return f, gradf, (lambda x: mu * la.norm(x.ravel(), 1)), (lambda x, t: shrink(x, t * mu))
    if kind == "nnls":
        return f, gradf, (lambda x: 0), (lambda x, t: np.maximum(x, 0))
    if kind == "box":
        lo, hi = float(d["lo"]), float(d["hi"])
        return f, gradf, (lambda x: 0), (lambda x, t: np.minimum(np.maximum(x, lo), hi))
    if kind == "gnone":
        return f, gradf, None, None
    raise KeyError(kind)


def case_table():
    """(name, kind, construct kwargs, problem seed, solver seed, options)"""
    cases = []
    for mode, mo in MODES.items():
        cases.append((f"lasso_200x400_{mode}", "lasso", dict(m=200, n=400, density=0.05, K=10, mu=0.5), 41, 401, dict(TEST_MODES, **mo)))
        cases.append((f"logistic_150x240_{mode}", "logistic", dict(m=150, n=240, density=0.08, K=8, mu=1.0), 43, 403, dict(TEST_MODES, **mo)))
    cases.append(("nnls_300x150", "nnls", dict(m=300, n=150, density=0.05, K=10), 42, 402, dict(TEST_MODES)))
    cases.append(("box_300x150", "box", dict(m=300, n=150, density=0.05, K=10), 44, 404, dict(TEST_MODES)))
    cases.append(("gnone_160x80", "gnone", dict(m=160, n=80, density=0.1, K=10), 45, 405, dict(tolerance=1e-5)))
    for rule in ("residual", "norm_residual", "ratio_residual", "hybrid_residual"):
        cases.append((f"stop_{rule}", "lasso", dict(m=100, n=200, density=0.05, K=8, mu=0.5), 46, 406, dict(tolerance=1e-4, stop_rule=rule)))
    # a first step far beyond 2 / L: the solve opens with a run of backtracks
    cases.append(("lasso_100x200_backtracks", "lasso", dict(m=100, n=200, density=0.05, K=8, mu=0.5), 47, 407,
                  dict(tolerance=1e-5, L=1.0, tau0=50.0, evaluate_objective=True, max_iters=300)))
    cases.append(("skewed_257x515", "skewed", dict(m=257, n=515, K=12, mu=1.0, skewed=True), 48, 408, dict(TEST_MODES)))
    return cases


def resolve(opts, stopping_module):
    o = dict(opts)
    if isinstance(o.get("stop_rule"), str):
        o["stop_rule"] = getattr(stopping_module, o["stop_rule"])
    return o


def run(core, linear_map, shrink, kind, d, opts, sseed, S=None, **extra):
    """One solve with the closure LinearMap over S, by `core.fasta` (the reference's, or the oracle's)."""
    S = matrix_of(d) if S is None else S
    m, n = S.shape
    f, gradf, g, proxg = closures(kind, d, shrink)
    A = linear_map(lambda x: S @ x, lambda y: S.T @ y, (n,), (m,))
    np.random.seed(sseed)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return core.fasta(A, f, gradf, g, proxg, np.zeros(n), **extra, **resolve(opts, core))


def permuted_divergence(kind, d, opts, sseed):
    """First iteration at which the oracle's step sizes differ (> 1e-6 relative) between the problem and the same problem with its
    unknowns permuted -- the same mathematics, another summation order in S @ x; the shorter iteration count if they never do."""
    sys.path.insert(0, ROOT)
    from oracle import fasta_np as fo
    from tests.helpers import first_divergence
    S = matrix_of(d)
    runs = []
    for perm in (np.arange(S.shape[1]), np.random.RandomState(7).permutation(S.shape[1])):
        Sp = S[:, perm].tocsr()
        Sp.sort_indices()
        runs.append(run(fo, fo.LinearMap, fo.shrink, kind, d, opts, sseed, S=Sp))
    k = min(runs[0].iteration_count, runs[1].iteration_count)
    return first_divergence(runs[1].stepsizes, runs[0].stepsizes, k)


def row_permuted_divergence(kind, d, opts, sseed):
    """The same for permuted ROWS of S (and of b): the Lipschitz probes keep their order, only the sums of S.T @ y change theirs."""
    sys.path.insert(0, ROOT)
    from oracle import fasta_np as fo
    from tests.helpers import first_divergence
    S = matrix_of(d)
    perm = np.random.RandomState(7).permutation(S.shape[0])
    Sp = S[perm].tocsr()
    Sp.sort_indices()
    runs = [run(fo, fo.LinearMap, fo.shrink, kind, d, opts, sseed), run(fo, fo.LinearMap, fo.shrink, kind, dict(d, b=d["b"][perm]), opts, sseed, S=Sp)]
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
        if "backtracks" in name:
            meta["permuted_divergence"] = permuted_divergence(kind, d, opts, sseed)
            # ... and the reference's backtracks within that prefix (the same run cut there: the trajectory does not depend on max_iters)
            cut = run(RefCore, ref.linalg.LinearMap, ref.proximal.shrink, kind, d, dict(opts, max_iters=meta["permuted_divergence"], tolerance=0.0), sseed, verbose=False)
            assert np.array_equal(cut.stepsizes[:meta["permuted_divergence"]], c.stepsizes[:meta["permuted_divergence"]])
            meta["backtracks_at_divergence"] = int(cut.backtracks)
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, meta=json.dumps(meta), **{"in_" + k: np.asarray(v) for k, v in d.items()}, **out)
        print(f"{name:32s} nnz={d['data'].size:6d} iters={int(c.iteration_count):4d} backtracks={int(c.backtracks):3d} {os.path.getsize(path):7d} B" +
              (f" permuted copy parts at {meta['permuted_divergence']}" if "permuted_divergence" in meta else ""))


if __name__ == "__main__":
    main(sys.argv[1])

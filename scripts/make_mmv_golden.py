"""Capture the matrix-unknown (MMV) fixtures tests/golden/mmv/*.npz from the REFERENCE core, the way oracle/make_golden.py captures the
vector ones:

    MPLBACKEND=Agg python scripts/make_mmv_golden.py <path to the reference checkout>

The operands are the reference's `LinearMap(lambda X: A @ X, lambda Y: A.T @ Y, (N, L), (M, L))` and the closures of its
examples/mmv.py:49-61, restated here (that file's own 7-argument call does not run against the reference's 6-argument `fasta()`).
Stored: inputs, every history, the solution.  The backtracking case also stores, in its meta, the iteration at which the NumPy oracle
parts from a copy of itself whose unknowns are permuted (columns of A, rows of X): how far summation order alone lets two correct
solvers agree on that run -- tests/test_mmv_cpu.py recomputes it, tests/test_gpu_mmv.py pins the device run up to there.
Our own code and data only: nothing of the reference is copied."""
import json
import os
import sys
import warnings

import numpy as np
from numpy import linalg as la

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "mmv")
TEST_MODES = dict(tolerance=1e-5, evaluate_objective=True)            # examples/__init__.py:63-91
MODES = {"adaptive": dict(adaptive=True, accelerate=False), "accelerated": dict(adaptive=False, accelerate=True),
         "plain": dict(adaptive=False, accelerate=False)}


def construct(M=20, N=30, L=10, K=7, sigma=0.1, mu=1.0):
    """examples/mmv.py:81-91: permutation, randn(K, L), randn(M, N), randn(M, L) from the global RNG, in this order."""
    X = np.zeros((N, L))
    X[np.random.permutation(N)[:K], ] = np.random.randn(K, L)
    A = np.random.randn(M, N)
    B = A @ X + sigma * np.random.randn(M, L)
    return dict(A=A, B=B, mu=np.float64(mu), X=X)


def closures(d, shrink):
    """f, gradf, g, proxg of examples/mmv.py:49-61 over the data `d`; `shrink` = the soft-threshold to use inside the prox."""
    B, mu = d["B"], float(d["mu"])
    f = lambda Z: .5 * la.norm((Z - B).ravel()) ** 2
    gradf = lambda Z: Z - B
    g = lambda X: mu * np.sum(np.sqrt(np.sum(X * X, axis=1)))

    def prox_rows(X, t):
        norms = la.norm(X, axis=1)
        scale = shrink(norms, t) / (norms + (norms == 0))
        return X * scale[:, np.newaxis]

    return f, gradf, g, (lambda X, t: prox_rows(X, mu * t))


def case_table():
    """(name, construct kwargs, problem seed, solver seed, options)"""
    cases = [(f"mmv_20x30x10_{mode}", dict(), 31, 301, dict(TEST_MODES, **mo)) for mode, mo in MODES.items()]
    cases.append(("mmv_64x128x5_objective", dict(M=64, N=128, L=5, K=9), 32, 302, dict(tolerance=1e-5, evaluate_objective=True)))
    # a step far beyond 2 / L (||A||^2 is about 90 here): every early iteration backtracks
    cases.append(("mmv_20x30x10_backtracks", dict(), 33, 303, dict(tolerance=1e-5, L=1.0, tau0=5.0, evaluate_objective=True, max_iters=300)))
    return cases


def permuted_divergence(d, opts, sseed):
    """First iteration at which the oracle's step sizes differ (> 1e-6 relative) between the problem and the same problem with its
    unknowns permuted -- the same mathematics, another summation order in A @ X; the shorter iteration count if they never do."""
    sys.path.insert(0, ROOT)
    from oracle import fasta_np as fo
    from tests.helpers import first_divergence
    runs = []
    for perm in (np.arange(d["A"].shape[1]), np.random.RandomState(7).permutation(d["A"].shape[1])):
        dp = dict(d, A=np.ascontiguousarray(d["A"][:, perm]))
        f, gradf, g, proxg = closures(dp, fo.shrink)
        N, L, M = dp["A"].shape[1], dp["B"].shape[1], dp["A"].shape[0]
        A = fo.LinearMap(lambda X, a=dp["A"]: a @ X, lambda Y, a=dp["A"]: a.T @ Y, (N, L), (M, L))
        np.random.seed(sseed)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            runs.append(fo.fasta(A, f, gradf, g, proxg, np.zeros((N, L)), **opts))
    k = min(runs[0].iteration_count, runs[1].iteration_count)
    return first_divergence(runs[1].stepsizes, runs[0].stepsizes, k)


def main(reference):
    sys.path.insert(0, reference)
    os.environ.setdefault("MPLBACKEND", "Agg")
    import fasta as ref
    assert os.path.abspath(ref.__file__).startswith(os.path.abspath(reference)), ref.__file__
    os.makedirs(OUT, exist_ok=True)
    for name, ckw, pseed, sseed, opts in case_table():
        np.random.seed(pseed)
        d = construct(**ckw)
        f, gradf, g, proxg = closures(d, ref.proximal.shrink)
        (M, N), L = d["A"].shape, d["B"].shape[1]
        A = ref.linalg.LinearMap(lambda X: d["A"] @ X, lambda Y: d["A"].T @ Y, (N, L), (M, L))
        np.random.seed(sseed)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            c = ref.fasta(A, f, gradf, g, proxg, np.zeros((N, L)), verbose=False, **opts)
        out = dict(residuals=c.residuals, norm_residuals=c.norm_residuals, stepsizes=c.stepsizes, backtracks=np.int64(c.backtracks),
                   iteration_count=np.int64(c.iteration_count), solution=c.solution)
        if c.objectives is not None:
            out["objectives"] = c.objectives
        meta = dict(name=name, construct=ckw, problem_seed=pseed, solver_seed=sseed, options=opts, numpy=np.__version__)
        if "backtracks" in name:
            meta["permuted_divergence"] = permuted_divergence(d, opts, sseed)
        np.savez_compressed(os.path.join(OUT, name + ".npz"), meta=json.dumps(meta), **{"in_" + k: np.asarray(v) for k, v in d.items()}, **out)
        print(f"{name:32s} iters={int(c.iteration_count):4d} backtracks={int(c.backtracks):3d}" +
              (f" permuted copy parts at {meta['permuted_divergence']}" if "permuted_divergence" in meta else ""))


if __name__ == "__main__":
    main(sys.argv[1])

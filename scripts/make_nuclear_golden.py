"""Capture the fixtures of the IDENTITY operator with an elementwise loss, tests/golden/nuclear/*.npz, from the REFERENCE core, the way
scripts/make_quad_golden.py captures the quadratic ones:

    MPLBACKEND=Agg python scripts/make_nuclear_golden.py <path to the reference checkout>

The operator is the identity (what `A = None` means, examples/logistic_matrix_completion.py:47); f, gradf, g, proxg are the closures of the
tags losses.LogisticLoss(B) / LeastSquares(B) and proximal.NuclearShrink / Shrink on host arrays -- tests/test_nuclear_cpu.py holds them to
the example's own closure forms.  The problems:
  lmc      examples/logistic_matrix_completion.py:62-78 at a small size: a rank-K matrix, B its logistic +-1 observations, NuclearShrink(mu)
  lsq      least squares against a noisy low-rank B with NuclearShrink(mu): the minimiser is prox(B, mu), known in closed form
  shrink   the lmc data with Shrink(mu) in place of the nuclear norm (an elementwise prox on the identity operator)
Every case GIVES L (1/4 for the logistic loss, 1 for least squares: the Lipschitz constants of the elementwise gradients) and tau0, the
reference's (2 / L) / 10 -- the forced-backtracking case 40 times that: the Lipschitz probes are random draws in the order of the unknowns, so a
run and its permuted twin would otherwise start from different steps.  mu is chosen so that the solution's rank is strictly between 0 and
min(M, N); the script asserts it.
Every fixture stores, in its meta, the iteration at which the NumPy oracle parts from a twin of itself whose rows and columns are permuted
(B[p][:, q], X0[p][:, q]; step sizes compared at 1e-6 relative, tests/helpers.py:first_divergence).  Our own code and data only: nothing of
the reference is copied."""
import json
import os
import sys
import warnings

import numpy as np
from numpy import linalg as la

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "nuclear")
TEST_MODES = dict(tolerance=1e-5, evaluate_objective=True)            # examples/__init__.py:63-91
MODES = {"adaptive": dict(adaptive=True, accelerate=False), "accelerated": dict(adaptive=False, accelerate=True),
         "plain": dict(adaptive=False, accelerate=False, max_iters=300)}


def construct(kind, M, N, K, mu, **_):
    """The problem data from the global RNG (seeded by the caller), in the example's draw order (:62-78)."""
    X = np.random.randn(M, N) * 3.0
    U, s, V = la.svd(X, full_matrices=False)
    X = (U[:, :K] * s[:K]) @ V[:K]
    if kind == "lsq":
        B = X + 0.3 * np.random.randn(M, N)
    else:
        B = 2.0 * (np.random.rand(M, N) < 1 / (1 + np.exp(-X))) - 1
    return dict(B=B, x0=np.zeros((M, N)), mu=np.float64(mu), truth=X)


def tags(fa, kind, d):
    loss = fa.LeastSquares(d["B"]) if kind == "lsq" else fa.LogisticLoss(d["B"])
    reg = fa.Shrink(float(d["mu"])) if kind == "shrink" else fa.NuclearShrink(float(d["mu"]))
    return loss, reg


def given_steps(kind, scale=1.0):
    L = 1.0 if kind == "lsq" else 0.25
    return dict(L=L, tau0=(2 / L) / 10 * scale)


def case_table():
    """(name, kind, construct kwargs, problem seed, mode options, tau0 scale)"""
    cases = [(f"lmc_12x20_{mode}", "lmc", dict(M=12, N=20, K=3, mu=1.5), 91, dict(TEST_MODES, **mo), 1.0) for mode, mo in MODES.items()]
    cases.append(("lmc_20x12_adaptive", "lmc", dict(M=20, N=12, K=3, mu=1.5), 92, dict(TEST_MODES, **MODES["adaptive"]), 1.0))
    # a first step 40 times too long: the backtracking test has to cut it
    cases.append(("lmc_12x20_backtracks", "lmc", dict(M=12, N=20, K=3, mu=1.5), 93, dict(TEST_MODES, **MODES["adaptive"]), 40.0))
    cases.append(("lsq_10x14_plain", "lsq", dict(M=10, N=14, K=3, mu=2.0), 94, dict(TEST_MODES, **MODES["plain"]), 1.0))
    cases.append(("shrink_9x7_adaptive", "shrink", dict(M=9, N=7, K=2, mu=0.4), 95, dict(TEST_MODES, **MODES["adaptive"]), 1.0))
    return cases


def resolve(opts, stopping_module):
    o = dict(opts)
    if isinstance(o.get("stop_rule"), str):
        o["stop_rule"] = getattr(stopping_module, o["stop_rule"])
    return o


def operands(fa, kind, d):
    loss, reg = tags(fa, kind, d)
    return loss.f, loss.gradf, reg.g, reg.prox, d["x0"]


def permuted(d, rows, cols):
    out = dict(d)
    for k in ("B", "x0"):
        out[k] = np.ascontiguousarray(d[k][rows][:, cols])
    return out


def run_oracle(kind, d, opts, **extra):
    sys.path.insert(0, ROOT)
    import fasta_python_amd as fa
    from oracle import fasta_np as fo
    f, gradf, g, proxg, x0 = operands(fa, kind, d)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fo.fasta(None, None, f, gradf, g, proxg, x0, **extra, **resolve(opts, fo))


def twin_divergence(kind, d, opts):
    """First iteration at which the oracle's step sizes differ (> 1e-6 relative) between the problem and its permuted twin; the (shorter)
    iteration count when they never do."""
    sys.path.insert(0, ROOT)
    from tests.helpers import first_divergence
    rs = np.random.RandomState(7)
    rows, cols = rs.permutation(d["B"].shape[0]), rs.permutation(d["B"].shape[1])
    a, b = run_oracle(kind, d, opts), run_oracle(kind, permuted(d, rows, cols), opts)
    k = min(a.iteration_count, b.iteration_count)
    at = first_divergence(b.stepsizes, a.stepsizes, k)
    return at if a.iteration_count == b.iteration_count else min(at, k - 1)


def solution_rank(kind, X):
    """Singular values of the solution above 1e-3 of the largest: the thresholding leaves the others at rounding level, the extrapolation of an
    accelerated run at the level of its last step."""
    s = la.svd(X, compute_uv=False)
    return int(np.sum(s > 1e-3 * max(s[0], 1e-300)))


def main(reference):
    sys.path.insert(0, ROOT)
    import fasta_python_amd as fa
    sys.path.insert(0, reference)
    os.environ.setdefault("MPLBACKEND", "Agg")
    for name in [k for k in sys.modules if k == "fasta" or k.startswith("fasta.")]:
        del sys.modules[name]                          # (this repository has a package of that name too: the reference's is meant)
    import fasta as ref
    assert os.path.abspath(ref.__file__).startswith(os.path.abspath(reference)), ref.__file__
    os.makedirs(OUT, exist_ok=True)
    for name, kind, ckw, pseed, mode_opts, scale in case_table():
        np.random.seed(pseed)
        d = construct(kind, **ckw)
        opts = dict(mode_opts, **given_steps(kind, scale))
        f, gradf, g, proxg, x0 = operands(fa, kind, d)
        o = resolve(opts, ref.stopping)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            c = ref.fasta(ref.linalg.LinearMap.identity(x0.shape), f, gradf, g, proxg, x0, verbose=False, **o)
        out = dict(residuals=c.residuals, norm_residuals=c.norm_residuals, stepsizes=c.stepsizes, backtracks=np.int64(c.backtracks),
                   iteration_count=np.int64(c.iteration_count), solution=c.solution, objectives=c.objectives)
        meta = dict(name=name, kind=kind, construct=ckw, problem_seed=pseed, options=opts, numpy=np.__version__)
        if kind != "shrink":
            meta["solution_rank"] = solution_rank(kind, c.solution)
            assert 0 < meta["solution_rank"] < min(x0.shape), f"{name}: rank {meta['solution_rank']} of {min(x0.shape)}: choose another mu"
        meta["twin_divergence"] = twin_divergence(kind, d, opts)
        whole = meta["twin_divergence"] == int(c.iteration_count)
        if not whole:                                  # the reference's backtracks within the prefix (the same run cut there)
            k = meta["twin_divergence"]
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                cut = ref.fasta(ref.linalg.LinearMap.identity(x0.shape), f, gradf, g, proxg, x0, verbose=False, **dict(o, max_iters=k, tolerance=0.0))
            assert np.array_equal(cut.stepsizes[:k], c.stepsizes[:k])
            meta["backtracks_at_divergence"] = int(cut.backtracks)
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, meta=json.dumps(meta), **{"in_" + k: np.asarray(v) for k, v in d.items()}, **out)
        print(f"{name:24s} iters={int(c.iteration_count):4d} backtracks={int(c.backtracks):3d} twin parts at {meta['twin_divergence']:4d} "
              f"rank={meta.get('solution_rank', -1):2d} f={c.objectives[int(c.iteration_count)]:+.6e} {os.path.getsize(path):7d} B")


if __name__ == "__main__":
    main(sys.argv[1])

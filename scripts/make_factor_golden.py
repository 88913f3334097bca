"""Capture the fixtures of the BILINEAR smooth term, tests/golden/factor/*.npz, from the REFERENCE core, the way scripts/make_quad_golden.py
captures the quadratic ones:

    MPLBACKEND=Agg python scripts/make_factor_golden.py <path to the reference checkout>

The reference's examples/nn_factorization.py cannot be imported as it stands (it imports a module that does not exist and uses a name it never
imports), so the problem is restated here: the operator is the identity (what `A = None` means, :63); f, gradf, g, proxg are the closures of the
tags losses.Factorization(S) and proximal.RowSplit(m, top, bottom) on host arrays -- tests/test_factor_cpu.py holds them to the example's own
closure forms (:48-61).  The problems:
  nnf      the example's construct (:80-94) at a small size: X, Y random, X made sparse, S = X Y^T + noise, X0 = 0, Y0 random;
           RowSplit(m, Shrink(mu), Box(0, 1))
  nonneg   the same data with RowSplit(m, NonNeg(), Box(0, 1));   gnone  the same data with no prox (g = proxg = None)
Every case GIVES L and tau0 (L = ||S||_2, the gradient's Lipschitz constant along one factor at unit scale of the other; tau0 = (2 / L) / 10
times the case's scale): the Lipschitz probes are random draws in the order of the unknowns, so a run and its permuted twin would otherwise
start from different steps.
The problem is NOT convex, so a run can part from a reordered copy of itself.  Every fixture stores, in its meta, the iteration at which the NumPy
oracle parts from a twin of itself whose rows of X (and of S), rows of Y (columns of S) and K columns are permuted (step sizes compared at
1e-6 relative, tests/helpers.py:first_divergence): a run whose twin never parts is compared whole, any other up to that iteration -- which must
then be at least 30, and for the forced-backtracking case must keep at least 5 backtracks.  Our own code and data only: nothing of the reference
is copied."""
import json
import os
import sys
import warnings

import numpy as np
from numpy import linalg as la

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "factor")
TEST_MODES = dict(tolerance=1e-5, evaluate_objective=True)            # examples/__init__.py:63-91
MODES = {"adaptive": dict(adaptive=True, accelerate=False), "accelerated": dict(adaptive=False, accelerate=True),
         "plain": dict(adaptive=False, accelerate=False, max_iters=300)}
MIN_PREFIX, MIN_BACKTRACKS = 30, 5


def construct(M, N, K, b=0.75, sigma=0.1, mu=1.0):
    """examples/nn_factorization.py:80-94, the global RNG in its order."""
    X = np.random.rand(M, K)
    Y = np.random.rand(N, K)
    X *= np.random.rand(M, K) > b
    S = X @ Y.T + sigma * np.random.randn(M, N)
    X0 = np.zeros((M, K))
    Y0 = np.random.rand(N, K)
    return dict(S=S, x0=np.concatenate((X0, Y0)), mu=np.float64(mu), m=np.int64(M))


def tags(fa, kind, d):
    """(loss, prox tag or None) of a case: the tags whose host closures every run here uses."""
    m = int(d["m"])
    loss = fa.Factorization(d["S"])
    reg = {"nnf": lambda: fa.RowSplit(m, fa.Shrink(float(d["mu"])), fa.Box(0.0, 1.0)),
           "nonneg": lambda: fa.RowSplit(m, fa.NonNeg(), fa.Box(0.0, 1.0)),
           "gnone": lambda: None}[kind]()
    return loss, reg


def operands(fa, kind, d):
    """f, gradf, g, proxg, x0: the tags' closures (g = proxg = None for the case without a prox term)."""
    loss, reg = tags(fa, kind, d)
    return (loss.f, loss.gradf) + ((None, None) if reg is None else (reg.g, reg.prox)) + (d["x0"],)


def given_steps(S, scale=1.0):
    L = float(la.norm(S, 2))
    return dict(L=L, tau0=(2 / L) / 10 * scale)


def case_table():
    """(name, kind, construct kwargs, problem seed, mode options, tau0 scale)"""
    cases = [(f"nnf_60x40x5_{mode}", "nnf", dict(M=60, N=40, K=5), 91, dict(TEST_MODES, **mo), 1.0) for mode, mo in MODES.items()]
    cases.append(("nnf_97x33x16_accelerated", "nnf", dict(M=97, N=33, K=16), 92, dict(TEST_MODES, **MODES["accelerated"]), 1.0))
    cases.append(("nnf_50x70x3_adaptive", "nnf", dict(M=50, N=70, K=3), 93, dict(TEST_MODES, **MODES["adaptive"]), 1.0))
    cases.append(("nnf_30x30x1_adaptive", "nnf", dict(M=30, N=30, K=1), 94, dict(TEST_MODES, **MODES["adaptive"]), 1.0))
    # a first step far too long: the line search has to cut it back
    cases.append(("nnf_60x40x5_backtracks", "nnf", dict(M=60, N=40, K=5), 91, dict(TEST_MODES, **MODES["adaptive"]), 200.0))
    cases.append(("nonneg_45x35x6_adaptive", "nonneg", dict(M=45, N=35, K=6), 95, dict(TEST_MODES, **MODES["adaptive"]), 1.0))
    cases.append(("gnone_40x30x2_plain", "gnone", dict(M=40, N=30, K=2), 96, dict(TEST_MODES, **MODES["plain"]), 1.0))
    return cases


def resolve(opts, stopping_module):
    o = dict(opts)
    if isinstance(o.get("stop_rule"), str):
        o["stop_rule"] = getattr(stopping_module, o["stop_rule"])
    return o


def permuted(d, seed=7):
    """The twin: rows of X (and of S), rows of Y (columns of S) and the K columns reordered."""
    m = int(d["m"])
    n, K = d["S"].shape[1], d["x0"].shape[1]
    rng = np.random.RandomState(seed)
    pr, pc, pk = rng.permutation(m), rng.permutation(n), rng.permutation(K)
    out = dict(d)
    out["S"] = np.ascontiguousarray(d["S"][pr][:, pc])
    out["x0"] = np.ascontiguousarray(np.concatenate((d["x0"][:m][pr], d["x0"][m:][pc]))[:, pk])
    return out


def run_oracle(kind, d, opts, **extra):
    sys.path.insert(0, ROOT)
    import fasta_python_amd as fa
    from oracle import fasta_np as fo
    f, gradf, g, proxg, x0 = operands(fa, kind, d)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fo.fasta(None, None, f, gradf, g, proxg, x0, **dict(resolve(opts, fo), **extra))


def twin_divergence(kind, d, opts):
    """First iteration at which the oracle's step sizes differ (> 1e-6 relative) between the problem and its permuted twin; the (shorter)
    iteration count when they never do."""
    sys.path.insert(0, ROOT)
    from tests.helpers import first_divergence
    a, b = run_oracle(kind, d, opts), run_oracle(kind, permuted(d), opts)
    k = min(a.iteration_count, b.iteration_count)
    at = first_divergence(b.stepsizes, a.stepsizes, k)
    return at if a.iteration_count == b.iteration_count else min(at, k - 1)


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
        d = construct(**ckw)
        opts = dict(mode_opts, **given_steps(d["S"], scale))
        f, gradf, g, proxg, x0 = operands(fa, kind, d)
        o = resolve(opts, ref.stopping)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            c = ref.fasta(ref.linalg.LinearMap.identity(x0.shape), f, gradf, g, proxg, x0, verbose=False, **o)
        out = dict(residuals=c.residuals, norm_residuals=c.norm_residuals, stepsizes=c.stepsizes, backtracks=np.int64(c.backtracks),
                   iteration_count=np.int64(c.iteration_count), solution=c.solution, objectives=c.objectives)
        meta = dict(name=name, kind=kind, construct=ckw, problem_seed=pseed, options=opts, numpy=np.__version__)
        meta["twin_divergence"] = twin_divergence(kind, d, opts)
        whole = meta["twin_divergence"] == int(c.iteration_count)
        if not whole:                                  # the reference's backtracks within the prefix (the same run cut there)
            k = meta["twin_divergence"]
            assert k >= MIN_PREFIX, f"{name}: the permuted twin parts at {k} of {int(c.iteration_count)}: choose another seed or size"
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                cut = ref.fasta(ref.linalg.LinearMap.identity(x0.shape), f, gradf, g, proxg, x0, verbose=False, **dict(o, max_iters=k, tolerance=0.0))
            assert np.array_equal(cut.stepsizes[:k], c.stepsizes[:k])
            meta["backtracks_at_divergence"] = int(cut.backtracks)
        kept = int(c.backtracks) if whole else meta["backtracks_at_divergence"]
        assert "backtracks" not in name or kept >= MIN_BACKTRACKS, f"{name}: {kept} backtracks inside the compared prefix"
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, meta=json.dumps(meta), **{"in_" + k: np.asarray(v) for k, v in d.items()}, **out)
        assert os.path.getsize(path) < 100 * 1024, (name, os.path.getsize(path))
        print(f"{name:28s} iters={int(c.iteration_count):4d} backtracks={int(c.backtracks):3d} (kept {kept:3d}) twin parts at {meta['twin_divergence']:4d} "
              f"f={c.objectives[int(c.iteration_count)]:+.6e} {os.path.getsize(path):7d} B")


if __name__ == "__main__":
    main(sys.argv[1])

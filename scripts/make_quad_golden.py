"""Capture the fixtures of a QUADRATIC smooth term, tests/golden/quad/*.npz, from the REFERENCE core, the way scripts/make_sparse_golden.py
captures the sparse ones:

    MPLBACKEND=Agg python scripts/make_quad_golden.py <path to the reference checkout>

The operator is the identity (what `A = None` means, examples/svm.py:74, examples/max_norm.py:61); f, gradf, g, proxg are the closures of the
tags losses.Quadratic(Q, c) and proximal.RowBall / Box / Shrink / NonNeg / GroupShrink on host arrays -- tests/test_quad_cpu.py holds them
to the examples' own closure forms.  The problems:
  maxnorm   examples/max_norm.py:36-40 and :66-95: two moons, S = delta - exp(-d^2 / sigma^2 / 2), Q = S + S.T (negative eigenvalues), RowBall(mu)
  svm       examples/svm.py:26-43 and :81-100 with an RBF kernel in place of D D^T: Q = (l l^T) * K, c = -1, Box(0, C), y0 = 0
  shrink    a positive definite Q, c = -Q x* for a sparse x*, Shrink(mu);  nonneg / group / gnone: the same Q family with the other terms
Every case GIVES L and tau0 (the spectral norm of Q and the reference's (2 / L) / 10): the Lipschitz probes are random draws in the order of
the unknowns, so a run and its permuted twin would otherwise start from different steps.
Every fixture stores, in its meta, the iteration at which the NumPy oracle parts from a twin of itself whose unknowns are permuted
(Q[p][:, p], c[p], x0[p]; step sizes compared at 1e-6 relative, tests/helpers.py:first_divergence): a run whose twin never parts is compared
whole, the forced-backtracking case up to that iteration.  Our own code and data only: nothing of the reference is copied."""
import json
import os
import sys
import warnings

import numpy as np
from numpy import linalg as la

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "quad")
TEST_MODES = dict(tolerance=1e-5, evaluate_objective=True)            # examples/__init__.py:63-91
MODES = {"adaptive": dict(adaptive=True, accelerate=False), "accelerated": dict(adaptive=False, accelerate=True),
         "plain": dict(adaptive=False, accelerate=False, max_iters=300)}


def two_moons_S(N, noise=0.15, dx=(1, 0.5), sigma=0.1, delta=0.01):
    """examples/max_norm.py:78-90 (points, global RNG) and :36-40 (similarity matrix), D = 2."""
    theta = np.arange(0, N) / N * 2 * np.pi
    points = np.zeros((N, 2))
    points[:, 0] = np.cos(theta)
    points[:, 1] = np.sin(theta)
    points[:N // 2, :2] -= dx
    points += noise * np.random.randn(N, 2)
    diff = points[:, None, :] - points[None, :, :]
    distances = np.sqrt(np.sum(diff * diff, axis=2))          # (symmetric bit for bit: (a - b)^2 == (b - a)^2)
    return delta - np.exp(-distances ** 2 / sigma ** 2 / 2)


def svm_data(M, N=15, separation=1.0):
    """examples/svm.py:91-95 and :26-43: the hyperplane, then the labelled points, in the reference's RNG order."""
    w = np.random.randn(N)
    w /= la.norm(w)
    w *= separation
    permutation = np.random.permutation(M)
    negative, positive = permutation[:M // 2], permutation[M // 2:]
    D = 2 * np.random.randn(M, N)
    D[negative] -= w
    D[positive] += w
    l = np.zeros(M)
    l[negative] -= 1.0
    l[positive] += 1.0
    return D, l


def rbf_kernel(D, gamma):
    diff = D[:, None, :] - D[None, :, :]
    return np.exp(-gamma * np.sum(diff * diff, axis=2))


def pd_matrix(n):
    G = np.random.randn(n + n // 2, n)
    Q = G.T @ G / n
    return np.triu(Q) + np.triu(Q, 1).T                       # exactly symmetric, whatever the product routine did


def construct(kind, **kw):
    """The problem data from the global RNG (seeded by the caller)."""
    if kind == "maxnorm":
        N, K, mu = kw["N"], kw["K"], kw.get("mu", 1.0)
        S = two_moons_S(N)
        X0 = np.random.randn(N, K) / np.sqrt(K) / 10          # examples/max_norm.py:93
        return dict(S=S, Q=S + S.T, x0=X0, mu=np.float64(mu))
    if kind == "svm":
        M, C = kw["M"], kw["C"]
        D, l = svm_data(M)
        Q = np.outer(l, l) * rbf_kernel(D, kw.get("gamma", 0.05))
        return dict(D=D, l=l, Q=Q, c=-np.ones(M), x0=np.zeros(M), lo=np.float64(0.0), hi=np.float64(C))
    n, L = kw["n"], kw.get("L")
    shape = (n,) if L is None else (n, L)
    Q = pd_matrix(n)
    xs = np.zeros(shape)
    support = np.random.permutation(n)[:max(n // 10, 3)]
    xs[support] = np.random.randn(*((len(support),) + shape[1:]))
    if kind == "nonneg":
        xs = np.abs(xs)
    d = dict(Q=Q, c=-(Q @ xs), x0=np.zeros(shape), xstar=xs)
    if kind in ("shrink", "group"):
        d["mu"] = np.float64(kw.get("mu", 0.05))
    return d


def tags(fa, kind, d, g_none=False):
    """(loss, prox tag or None) of a case: the tags whose host closures every run here uses."""
    loss = fa.Quadratic(d["Q"], d.get("c"))
    reg = {"maxnorm": lambda: fa.RowBall(float(d["mu"])), "svm": lambda: fa.Box(float(d["lo"]), float(d["hi"])),
           "shrink": lambda: fa.Shrink(float(d["mu"])), "nonneg": lambda: fa.NonNeg(), "group": lambda: fa.GroupShrink(float(d["mu"])),
           "gnone": lambda: None}[kind]()
    return loss, reg


def given_steps(Q, scale=1.0):
    L = float(la.norm(Q, 2))
    return dict(L=L, tau0=(2 / L) / 10 * scale)


def case_table():
    """(name, kind, construct kwargs, problem seed, mode options, tau0 scale)"""
    cases = [(f"maxnorm_60x5_{mode}", "maxnorm", dict(N=60, K=5), 81, dict(TEST_MODES, **mo), 1.0) for mode, mo in MODES.items()]
    cases.append(("maxnorm_130x10_adaptive", "maxnorm", dict(N=130, K=10), 82, dict(TEST_MODES, **MODES["adaptive"]), 1.0))
    cases.append(("maxnorm_97x16_accelerated", "maxnorm", dict(N=97, K=16), 83, dict(TEST_MODES, **MODES["accelerated"]), 1.0))
    cases.append(("maxnorm_75x3_plain", "maxnorm", dict(N=75, K=3), 84, dict(TEST_MODES, **MODES["plain"]), 1.0))
    cases += [(f"svm_rbf_80_{mode}", "svm", dict(M=80, C=0.5, gamma=0.004), 85, dict(TEST_MODES, **mo), 1.0) for mode, mo in MODES.items()]
    # a wide box lets the adaptive steps overshoot: 3 backtracks, and the twin still agrees over the whole solve
    cases.append(("svm_rbf_80_c10_adaptive", "svm", dict(M=80, C=10.0, gamma=0.02), 85, dict(TEST_MODES, **MODES["adaptive"]), 1.0))
    # a first step 50 times too long on a box of 2 (with these seeded points C = 0.5 never backtracks): 12 backtracks, and the twin parts
    # before the end -- compared on the prefix
    cases.append(("svm_rbf_80_backtracks", "svm", dict(M=80, C=2.0, gamma=0.005), 85, dict(TEST_MODES, **MODES["adaptive"]), 50.0))
    cases.append(("shrink_90_adaptive", "shrink", dict(n=90, mu=0.05), 86, dict(TEST_MODES, **MODES["adaptive"]), 1.0))
    cases.append(("nonneg_70x2_accelerated", "nonneg", dict(n=70, L=2), 87, dict(TEST_MODES, **MODES["accelerated"]), 1.0))
    cases.append(("group_64x6_adaptive", "group", dict(n=64, L=6, mu=0.1), 88, dict(TEST_MODES, **MODES["adaptive"]), 1.0))
    cases.append(("gnone_50_plain", "gnone", dict(n=50), 89, dict(TEST_MODES, **MODES["plain"]), 1.0))
    return cases


def resolve(opts, stopping_module):
    o = dict(opts)
    if isinstance(o.get("stop_rule"), str):
        o["stop_rule"] = getattr(stopping_module, o["stop_rule"])
    return o


def operands(fa, kind, d):
    """f, gradf, g, proxg, x0: the tags' closures (g = proxg = None for the case without a prox term)."""
    loss, reg = tags(fa, kind, d)
    return (loss.f, loss.gradf) + ((None, None) if reg is None else (reg.g, reg.prox)) + (d["x0"],)


def permuted(d, perm):
    out = dict(d)
    out["Q"] = np.ascontiguousarray(d["Q"][perm][:, perm])
    for k in ("c", "x0"):
        if k in d:
            out[k] = d[k][perm]
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
    perm = np.random.RandomState(7).permutation(d["Q"].shape[0])
    a, b = run_oracle(kind, d, opts), run_oracle(kind, permuted(d, perm), opts)
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
        d = construct(kind, **ckw)
        opts = dict(mode_opts, **given_steps(d["Q"], scale))
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
        assert whole or "backtracks" in name, f"{name}: the permuted twin parts at {meta['twin_divergence']} of {int(c.iteration_count)}: choose another seed"
        if not whole:                                  # the reference's backtracks within the prefix (the same run cut there)
            k = meta["twin_divergence"]
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                cut = ref.fasta(ref.linalg.LinearMap.identity(x0.shape), f, gradf, g, proxg, x0, verbose=False, **dict(o, max_iters=k, tolerance=0.0))
            assert np.array_equal(cut.stepsizes[:k], c.stepsizes[:k])
            meta["backtracks_at_divergence"] = int(cut.backtracks)
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, meta=json.dumps(meta), **{"in_" + k: np.asarray(v) for k, v in d.items()}, **out)
        print(f"{name:28s} iters={int(c.iteration_count):4d} backtracks={int(c.backtracks):3d} twin parts at {meta['twin_divergence']:4d} "
              f"f={c.objectives[int(c.iteration_count)]:+.6e} {os.path.getsize(path):7d} B")


if __name__ == "__main__":
    main(sys.argv[1])

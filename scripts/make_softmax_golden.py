"""Capture the fixtures of the softmax loss over a matrix unknown, tests/golden/softmax/*.npz, from the REFERENCE core, in the manner of
scripts/make_nuclear_golden.py and scripts/make_sparse_mmv_golden.py:

    MPLBACKEND=Agg python scripts/make_softmax_golden.py <path to the reference checkout>

The reference has no multinomial example; its core is run with the host closures of losses.SoftmaxLoss (f, gradf) and of the prox tags
(proximal.GroupShrink / proximal.Shrink: g, proxg) over the closure pair the reference is given for a matrix A and an (n, L) unknown,
`LinearMap(lambda X: A @ X, lambda Y: A.T @ Y, (n, L), (m, L))`, A a dense array or a scipy.sparse matrix.  Labels are drawn from the softmax of
A X_true for a row-sparse X_true.  Unless a case says otherwise, L = .5 * ||A||_2^2 and tau0 = (2 / L) / 10 are given.
Stored: the inputs, every history, the solution and -- in the meta -- the iteration at which the NumPy oracle parts from a copy of itself with
permuted ROWS of A (and of y): the same mathematics, another summation order in A.T @ R (tests/helpers.py: first_divergence; the iteration count
when they never part).  A device run is held to the histories up to there.
Asserted for every case: the run ends before max_iters (except in plain mode), the backtracking case backtracks, and each penalised solution
has at least one zero and one non-zero row (GroupShrink) or entry (Shrink).  If a seed fails an assertion, change the seed, not the assertion.
Our own code and data only: nothing of the reference is copied."""
import json
import os
import sys
import warnings

import numpy as np
from numpy import linalg as la
from scipy import sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "softmax")
TEST_MODES = dict(tolerance=1e-5, evaluate_objective=True)            # examples/__init__.py:63-91
MODES = {"adaptive": dict(adaptive=True, accelerate=False), "accelerated": dict(adaptive=False, accelerate=True),
         "plain": dict(adaptive=False, accelerate=False, max_iters=400)}


def construct(m, n, L, K, mu, density=None):
    """The problem data from the global RNG (seeded by the caller): A (dense, or CSR arrays), row-sparse truth (K live rows), labels drawn
    from the softmax of A X_true."""
    if density is None:
        A = np.random.randn(m, n)
        d = dict(A=A)
        op = A
    else:
        rs = np.random.RandomState(np.random.randint(1 << 30))
        S = sp.random(m, n, density=density, format="csr", random_state=rs, data_rvs=rs.standard_normal)
        S.sort_indices()
        d = dict(data=S.data.astype(np.float64), indices=S.indices.astype(np.int32), indptr=S.indptr.astype(np.int64),
                 shape=np.array(S.shape, dtype=np.int64))
        op = S
    X = np.zeros((n, L))
    X[np.random.permutation(n)[:K]] = 2.0 * np.random.randn(K, L)
    Z = op @ X
    P = np.exp(Z - Z.max(axis=1)[:, np.newaxis])
    P /= P.sum(axis=1)[:, np.newaxis]
    u = np.random.rand(m)
    y = np.minimum((np.cumsum(P, axis=1) < u[:, np.newaxis]).sum(axis=1), L - 1).astype(np.int64)
    d.update(y=y, classes=np.int64(L), mu=np.float64(mu), X=X)
    return d


def matrix_of(d):
    if "A" in d:
        return d["A"]
    return sp.csr_matrix((d["data"], d["indices"], d["indptr"]), shape=tuple(int(k) for k in d["shape"]))


def lipschitz(d):
    A = matrix_of(d)
    return .5 * la.norm(A.toarray() if sp.issparse(A) else A, 2) ** 2


def tags(prox, d):
    """The tagged loss and prox of the package: their `.f` / `.gradf` / `.g` / `.prox` on host arrays are the closures every core here runs."""
    sys.path.insert(0, ROOT)
    from fasta_python_amd import losses, proximal
    loss = losses.SoftmaxLoss(d["y"], classes=int(d["classes"]))
    reg = {"group": lambda: proximal.GroupShrink(float(d["mu"])), "l1": lambda: proximal.Shrink(float(d["mu"])), "none": lambda: None}[prox]()
    return loss, reg


def case_table():
    """(name, prox, construct kwargs, problem seed, solver seed, options, set-up: "given" | "long" (first step 40 x too long) | "estimated")"""
    g3 = dict(m=60, n=40, L=3, K=6, mu=3.0)
    cases = [(f"group_60x40x3_{mode}", "group", g3, 81, 801, dict(TEST_MODES, **mo), "given") for mode, mo in MODES.items()]
    cases.append(("group_60x40x3_backtracks", "group", g3, 81, 802, dict(TEST_MODES, **MODES["adaptive"]), "long"))
    cases.append(("group_50x70x5_adaptive", "group", dict(m=50, n=70, L=5, K=8, mu=2.5), 83, 803, dict(TEST_MODES, **MODES["adaptive"]), "given"))
    cases.append(("l1_80x30x2_accelerated", "l1", dict(m=80, n=30, L=2, K=6, mu=1.5), 84, 804, dict(TEST_MODES, **MODES["accelerated"]), "given"))
    cases.append(("l1_97x33x16_adaptive", "l1", dict(m=97, n=33, L=16, K=8, mu=1.0), 85, 805, dict(TEST_MODES, **MODES["adaptive"]), "given"))
    sparse7 = dict(m=120, n=90, L=7, K=10, mu=0.8, density=0.1)
    cases.append(("sparse_120x90x7_adaptive", "group", sparse7, 86, 806, dict(TEST_MODES, **MODES["adaptive"]), "given"))
    cases.append(("sparse_120x90x7_accelerated", "group", sparse7, 86, 807, dict(TEST_MODES, **MODES["accelerated"]), "given"))
    cases.append(("noprox_40x20x4_plain", "none", dict(m=40, n=20, L=4, K=5, mu=0.0), 88, 808, dict(TEST_MODES, **MODES["plain"]), "given"))
    cases.append(("estimated_60x40x3_adaptive", "group", g3, 81, 809, dict(TEST_MODES, **MODES["adaptive"]), "estimated"))
    return cases


def solver_options(d, opts, setup):
    """The options of a case with its step-size set-up resolved (plain floats, as the fixture's meta stores them)."""
    o = dict(opts)
    if setup != "estimated":
        Lc = lipschitz(d)
        o["L"] = float(Lc)
        o["tau0"] = float((2 / Lc) / 10) * (40.0 if setup == "long" else 1.0)
    return o


def resolve(opts, stopping_module):
    o = dict(opts)
    if isinstance(o.get("stop_rule"), str):
        o["stop_rule"] = getattr(stopping_module, o["stop_rule"])
    return o


def run(core, linear_map, prox, d, opts, sseed, perm=None, **extra):
    """One solve by `core.fasta` (the reference's, or the oracle's) over the closure LinearMap; perm: the rows of A and y in that order."""
    A = matrix_of(d)
    if perm is not None:
        A = A[perm].tocsr() if sp.issparse(A) else np.ascontiguousarray(A[perm])
        d = dict(d, y=d["y"][perm])
    (m, n), L = A.shape, int(d["classes"])
    At = A.T.tocsr() if sp.issparse(A) else A.T
    loss, reg = tags(prox, d)
    g, proxg = (None, None) if reg is None else (reg.g, reg.prox)
    op = linear_map(lambda X: A @ X, lambda Y: At @ Y, (n, L), (m, L))
    np.random.seed(sseed)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return core.fasta(op, loss.f, loss.gradf, g, proxg, np.zeros((n, L)), **extra, **resolve(opts, core))


def twin_divergence(prox, d, opts, sseed):
    """First iteration at which the oracle's step sizes differ (> 1e-6 relative) between the problem and its row-permuted twin; the
    (shorter) iteration count if they never do."""
    sys.path.insert(0, ROOT)
    from oracle import fasta_np as fo
    from tests.helpers import first_divergence
    perm = np.random.RandomState(7).permutation(int(d["y"].size))
    runs = [run(fo, fo.LinearMap, prox, d, opts, sseed), run(fo, fo.LinearMap, prox, d, opts, sseed, perm=perm)]
    k = min(r.iteration_count for r in runs)
    at = first_divergence(runs[1].stepsizes, runs[0].stepsizes, k)
    if runs[0].iteration_count != runs[1].iteration_count:
        at = min(at, k - 1)
    return int(at)


def check(name, prox, c, opts, setup):
    if "plain" not in name:
        assert int(c.iteration_count) < int(opts.get("max_iters", 1000)), f"{name}: ran into max_iters"
    if setup == "long":
        assert int(c.backtracks) >= 1, f"{name}: no backtrack"
    if prox == "group":
        live = np.abs(c.solution).sum(axis=1) != 0
        assert live.any() and not live.all(), f"{name}: {int(live.sum())} of {live.size} rows non-zero"
    if prox == "l1":
        live = c.solution != 0
        assert live.any() and not live.all(), f"{name}: {int(live.sum())} of {live.size} entries non-zero"


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
    for name, prox, ckw, pseed, sseed, opts, setup in case_table():
        np.random.seed(pseed)
        d = construct(**ckw)
        o = solver_options(d, opts, setup)
        c = run(RefCore, ref.linalg.LinearMap, prox, d, o, sseed, verbose=False)
        check(name, prox, c, o, setup)
        out = dict(residuals=c.residuals, norm_residuals=c.norm_residuals, stepsizes=c.stepsizes, backtracks=np.int64(c.backtracks),
                   iteration_count=np.int64(c.iteration_count), solution=c.solution)
        if c.objectives is not None:
            out["objectives"] = c.objectives
        twin = twin_divergence(prox, d, o, sseed)
        meta = dict(name=name, prox=prox, construct=ckw, problem_seed=pseed, solver_seed=sseed, options=o, setup=setup,
                    twin_divergence=twin, numpy=np.__version__)
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, meta=json.dumps(meta), **{"in_" + k: np.asarray(v) for k, v in d.items()}, **out)
        print(f"{name:30s} iters={int(c.iteration_count):4d} backtracks={int(c.backtracks):3d} twin agrees for {twin:4d} {os.path.getsize(path):7d} B")


if __name__ == "__main__":
    main(sys.argv[1])

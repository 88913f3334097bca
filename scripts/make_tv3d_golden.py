"""Capture the volumetric total-variation fixtures tests/golden/tv3d/*.npz from the REFERENCE core, the way scripts/make_mmv_golden.py captures
the matrix-unknown ones:

    MPLBACKEND=Agg python scripts/make_tv3d_golden.py <path to the reference checkout>

The operator is the reference's own N-dimensional `grad` / `div` (fasta/examples/tv_denoising.py:26-63) wrapped in its `LinearMap`, the closures
are those of tv_denoising.py:85-96 restated here (that file's own 7-argument call does not run against the reference's 6-argument `fasta()`).
The volume is synthetic: {0, 1} blocks of side 4 plus Gaussian noise from a seeded generator.  Stored: inputs, every history, the solution.

Adaptive runs of TV amplify summation order, so every adaptive fixture also stores, in its meta, the iteration at which the
NumPy oracle parts from a TWIN of itself -- the same volume with its axes rotated (2, 0, 1), both runs given the same L and tau0 so that they
start from the same step: how far summation order alone lets two correct solvers agree on that run.  tests/test_tv3d_cpu.py recomputes it,
tests/test_gpu_tv3d.py pins the device run up to there.  The prefix must be at least 40 iterations (or the whole run); a seed that gives a
shorter one is replaced by another seed, the bound is not shortened.
Our own code and data only: nothing of the reference is copied."""
import json
import os
import sys
import warnings

import numpy as np
from numpy import linalg as la

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "tv3d")
TEST_MODES = dict(tolerance=1e-5, evaluate_objective=True)            # examples/__init__.py:63-91
MODES = {"adaptive": dict(adaptive=True, accelerate=False), "accelerated": dict(adaptive=False, accelerate=True),
         "plain": dict(adaptive=False, accelerate=False)}
MIN_PREFIX = 40
TWIN_AXES = (2, 0, 1)


def blocks(shape, side):
    """{0, 1} blocks of `side` voxels: the 3-D checkerboard."""
    idx = np.indices(shape)
    return (sum(i // side for i in idx) % 2).astype(float)


def construct(shape=(8, 8, 8), side=4, sigma=0.1, mu=0.1):
    """tv_denoising.py:105-125 on a synthetic volume: normalise, add sigma * randn from the global RNG."""
    M = blocks(shape, side)
    M /= max(np.max(M), 1.0)
    M += sigma * np.random.randn(*M.shape)
    return dict(M=M, mu=np.float64(mu))


def closures(d, prox):
    """f, gradf, g, proxg of tv_denoising.py:85-96 over the data `d`; prox = "ball" (the reference's) or "box" (clip to [-1, 1]: anisotropic TV)."""
    M, mu = d["M"], float(d["mu"])
    f = lambda Z: .5 * la.norm((Z - M / mu).ravel()) ** 2
    gradf = lambda Z: Z - M / mu
    g = lambda Y: 0

    def ball(Y, t):
        norms = la.norm(Y, axis=Y.ndim - 1)
        norms = np.maximum(norms, 1)
        return Y / norms[..., np.newaxis]

    box = lambda Y, t: np.minimum(np.maximum(Y, -1.0), 1.0)
    return f, gradf, g, (ball if prox == "ball" else box)


def case_table():
    """(name, construct kwargs, prox, problem seed, solver seed, options)"""
    cases = []
    for mode, mo in MODES.items():
        o = dict(TEST_MODES, **mo)
        if mode == "plain":
            o["max_iters"] = 300
        cases.append((f"tv3d_8x8x8_{mode}", dict(), "ball", 41, 411, o))
    cases.append(("tv3d_6x10x12_accelerated", dict(shape=(6, 10, 12)), "ball", 42, 421, dict(TEST_MODES, **MODES["accelerated"])))
    cases.append(("tv3d_5x9x16_box_accelerated", dict(shape=(5, 9, 16)), "box", 43, 431, dict(TEST_MODES, **MODES["accelerated"])))
    cases.append(("tv3d_2x3x1_adaptive", dict(shape=(2, 3, 1)), "ball", 44, 441, dict(TEST_MODES, **MODES["adaptive"])))
    return cases


def oracle_run(d, prox, opts, sseed=None, **given):
    """The NumPy oracle on the data `d` (solver seed set when no L / tau0 is given)."""
    sys.path.insert(0, ROOT)
    from oracle import fasta_np as fo
    from oracle import problems as pr
    f, gradf, g, proxg = closures(d, prox)
    shape = d["M"].shape
    A = fo.LinearMap(pr.div, pr.grad, shape + (len(shape),), shape)
    if sseed is not None:
        np.random.seed(sseed)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fo.fasta(A, f, gradf, g, proxg, np.zeros(shape + (len(shape),)), **dict(opts, **given))


def step_estimate(d, prox, sseed):
    """L and tau0 as the solver estimates them from its two probes (fasta/__init__.py:100-113) under the solver seed."""
    sys.path.insert(0, ROOT)
    from oracle import fasta_np as fo
    from oracle import problems as pr
    shape = d["M"].shape
    A = fo.LinearMap(pr.div, pr.grad, shape + (len(shape),), shape)
    np.random.seed(sseed)
    L, tau0 = fo.estimate_lipschitz(A, closures(d, prox)[1], shape + (len(shape),))
    return float(L), float(tau0)


def twin_divergence(d, prox, opts, sseed):
    """(first iteration at which the oracle's step sizes differ, > 1e-6 relative, between the volume and its twin with the axes rotated
    TWIN_AXES, both started from the same L and tau0 -- the shorter iteration count if they never do; backtracks of the run up to there)."""
    sys.path.insert(0, ROOT)
    from tests.helpers import first_divergence
    L, tau0 = step_estimate(d, prox, sseed)
    a = oracle_run(d, prox, opts, L=L, tau0=tau0)
    b = oracle_run(dict(d, M=np.ascontiguousarray(np.transpose(d["M"], TWIN_AXES))), prox, opts, L=L, tau0=tau0)
    k = first_divergence(b.stepsizes, a.stepsizes, min(a.iteration_count, b.iteration_count))
    head = oracle_run(d, prox, dict(opts, max_iters=k, tolerance=0.0), L=L, tau0=tau0) if k else None
    return int(k), int(head.backtracks) if head is not None else 0


def reference_grad_div(reference):
    """The reference's own `grad` and `div`, compiled from its examples/tv_denoising.py.  The module itself no longer imports (it asks SciPy
    for a test image SciPy has dropped and `fasta.linalg` for a name it has dropped), so the two function definitions are taken out of its
    syntax tree and compiled alone; they need nothing but NumPy."""
    import ast
    import types
    path = os.path.join(reference, "fasta", "examples", "tv_denoising.py")
    tree = ast.parse(open(path).read(), path)
    tree.body = [node for node in tree.body if isinstance(node, ast.FunctionDef) and node.name in ("grad", "div")]
    assert [node.name for node in tree.body] == ["grad", "div"], path
    for node in tree.body:                         # (the annotations name types of the module that does not import)
        node.returns = None
        for arg in node.args.args:
            arg.annotation = None
    mod = types.ModuleType("reference_tv_denoising")
    mod.np = np
    exec(compile(tree, path, "exec"), mod.__dict__)
    return mod


def main(reference):
    sys.path.insert(0, reference)
    os.environ.setdefault("MPLBACKEND", "Agg")
    import fasta as ref
    ref_tv = reference_grad_div(reference)
    assert os.path.abspath(ref.__file__).startswith(os.path.abspath(reference)), ref.__file__
    os.makedirs(OUT, exist_ok=True)
    for name, ckw, prox, pseed, sseed, opts in case_table():
        np.random.seed(pseed)
        d = construct(**ckw)
        f, gradf, g, proxg = closures(d, prox)
        shape = d["M"].shape
        A = ref.linalg.LinearMap(ref_tv.div, ref_tv.grad, shape + (3,), shape)
        np.random.seed(sseed)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            c = ref.fasta(A, f, gradf, g, proxg, np.zeros(shape + (3,)), verbose=False, **opts)
        out = dict(residuals=c.residuals, norm_residuals=c.norm_residuals, stepsizes=c.stepsizes, backtracks=np.int64(c.backtracks),
                   iteration_count=np.int64(c.iteration_count), solution=c.solution, primal=d["M"] - float(d["mu"]) * ref_tv.div(c.solution))
        if c.objectives is not None:
            out["objectives"] = c.objectives
        meta = dict(name=name, construct={k: list(v) if isinstance(v, tuple) else v for k, v in ckw.items()}, prox=prox, problem_seed=pseed,
                    solver_seed=sseed, options=opts, numpy=np.__version__)
        if opts.get("adaptive"):
            k, bt = twin_divergence(d, prox, opts, sseed)
            assert k >= MIN_PREFIX or k == int(c.iteration_count), f"{name}: the twin parts at iteration {k} < {MIN_PREFIX}: choose another seed"
            meta["twin_divergence"], meta["backtracks_at_divergence"] = k, bt
        np.savez_compressed(os.path.join(OUT, name + ".npz"), meta=json.dumps(meta), **{"in_" + k: np.asarray(v) for k, v in d.items()}, **out)
        print(f"{name:32s} iters={int(c.iteration_count):4d} backtracks={int(c.backtracks):3d}" +
              (f" twin parts at {meta['twin_divergence']} ({meta['backtracks_at_divergence']} backtracks)" if "twin_divergence" in meta else ""))


if __name__ == "__main__":
    main(sys.argv[1])

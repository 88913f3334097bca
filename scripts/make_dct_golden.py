"""Capture the democratic-representation fixtures tests/golden/dct/*.npz from the REFERENCE core, the way scripts/make_tv3d_golden.py captures
the volumetric ones:

    MPLBACKEND=Agg python scripts/make_dct_golden.py <path to the reference checkout>

The operator is the reference's subsampled DCT -- `mask * dct(x, norm='ortho')` and `idct(mask * x, norm='ortho')` of
fasta/examples/democratic_representation.py:80-82 -- wrapped in its `LinearMap`; the data are those of its `construct` (:61-82: the same draws
from the global RNG in the same order) and the closures those of its `solve` (:42-45), restated here (the example module itself asks for
matplotlib and for names `fasta.linalg` has dropped).  One case swaps the l-infinity term for `mu * |x|_1` with the reference's `shrink`.
Stored: inputs, every history, the solution.

Adaptive runs amplify rounding, so every adaptive fixture also stores, in its meta, the iteration at which the NumPy
oracle parts from a TWIN of itself -- the same run with the operator computed by one complex FFT of length N (Makhoul's permutation, numpy.fft,
the route the device takes) instead of scipy.fftpack, both given the same L and tau0: how far rounding alone lets two correct solvers agree
on that run.  tests/test_dct_cpu.py recomputes it, tests/test_gpu_dct.py pins the device run up to there.
`construct` and the closures are the reference's recipe restated, so that the draws and the arithmetic match; the data are our own."""
import json
import os
import sys
import warnings

import numpy as np
from numpy import linalg as la
from scipy.fftpack import dct, idct

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "dct")
TEST_MODES = dict(tolerance=1e-5, evaluate_objective=True)            # examples/__init__.py:63-91
MODES = {"adaptive": dict(adaptive=True, accelerate=False), "accelerated": dict(adaptive=False, accelerate=True),
         "plain": dict(adaptive=False, accelerate=False)}
PROBLEM_SEED, SOLVER_SEED = 7, 107


def construct(M=500, N=1000, mu=300.0):
    """democratic_representation.py:61-82: M random DCT modes out of 1 .. N - 1 (the last one replaced by mode 1), a 0/1 mask, Gaussian data on
    the sampled modes, x0 = 0."""
    samples = np.random.permutation(N - 1)[:M] + 1
    samples[M - 1] = 1
    samples.sort()
    mask = np.zeros(N)
    mask[samples] = 1
    b = np.zeros(N)
    b[samples] = np.random.randn(M)
    return dict(mask=mask, b=b, mu=np.float64(mu))


def fftpack_pair(mask):
    """The reference's closures (:80-82)."""
    return (lambda x: mask * dct(x, norm='ortho')), (lambda x: idct(mask * x, norm='ortho'))


def makhoul_pair(mask):
    """The same operator by one complex FFT of length N: v[j] = x[2j], v[N-1-j] = x[2j+1], y[k] = s_k Re(e^{-i pi k / 2N} FFT(v)[k]) and the
    transposed chain -- the twin's route, and the device's."""
    N = len(mask)
    j = np.arange(N)
    src = np.where(j < (N + 1) // 2, 2 * j, 2 * (N - 1 - j) + 1)
    pw = np.exp(-1j * np.pi * j / (2 * N))
    s = np.full(N, np.sqrt(2.0 / N))
    s[0] = np.sqrt(1.0 / N)

    def fwd(x):
        return mask * ((pw * np.fft.fft(x[src])).real * s)

    def adj(w):
        u = mask * w * np.where(j == 0, np.sqrt(N), np.sqrt(N / 2.0))
        um = np.zeros(N)
        um[1:] = u[1:][::-1]
        v = np.fft.ifft(pw.conj() * (u - 1j * um)).real
        x = np.empty(N)
        x[src] = v
        return x

    return fwd, adj


def closures(d, prox, shrink=None, project_linf=None):
    """f, gradf, g, proxg of democratic_representation.py:42-45 over the data `d`; prox = "linf" (the reference's) or "shrink" (mu * |x|_1)."""
    sys.path.insert(0, ROOT)
    from oracle import fasta_np as fo
    b, mu = d["b"], float(d["mu"])
    f = lambda z: .5 * la.norm((z - b).ravel()) ** 2
    gradf = lambda z: z - b
    if prox == "linf":
        project = project_linf or fo.prox_linf
        return f, gradf, (lambda x: mu * la.norm(x, np.inf)), (lambda x, t: project(x, t * mu))
    soft = shrink or fo.shrink
    return f, gradf, (lambda x: mu * la.norm(x.ravel(), 1)), (lambda x, t: soft(x, t * mu))


def case_table():
    """(name, construct kwargs, prox, options)"""
    cases = [(f"dct_60_{mode}", dict(N=60, M=30, mu=20.0), "linf", dict(TEST_MODES, **mo)) for mode, mo in MODES.items()]
    cases.append(("dct_250_accelerated", dict(N=250, M=120, mu=80.0), "linf", dict(TEST_MODES, **MODES["accelerated"])))
    cases.append(("dct_1000_adaptive", dict(N=1000, M=500, mu=300.0), "linf", dict(TEST_MODES, **MODES["adaptive"])))
    cases.append(("dct_96_adaptive", dict(N=96, M=48, mu=5.0), "linf", dict(TEST_MODES, **MODES["adaptive"])))          # the one that backtracks
    cases.append(("dct_45_adaptive", dict(N=45, M=20, mu=10.0), "linf", dict(TEST_MODES, **MODES["adaptive"])))         # odd N, radices 3 and 5
    cases.append(("dct_1000_shrink_accelerated", dict(N=1000, M=300, mu=0.05), "shrink", dict(TEST_MODES, **MODES["accelerated"])))
    return cases


def oracle_run(d, prox, opts, sseed=None, pair=fftpack_pair, **given):
    """The NumPy oracle on the data `d` (solver seed set when no L / tau0 is given)."""
    sys.path.insert(0, ROOT)
    from oracle import fasta_np as fo
    f, gradf, g, proxg = closures(d, prox)
    N = len(d["mask"])
    fwd, adj = pair(d["mask"])
    A = fo.LinearMap(fwd, adj, (N,), (N,))
    if sseed is not None:
        np.random.seed(sseed)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fo.fasta(A, f, gradf, g, proxg, np.zeros(N), **dict(opts, **given))


def step_estimate(d, prox, sseed):
    """L and tau0 as the solver estimates them from its two probes (fasta/__init__.py:100-113) under the solver seed."""
    sys.path.insert(0, ROOT)
    from oracle import fasta_np as fo
    N = len(d["mask"])
    fwd, adj = fftpack_pair(d["mask"])
    np.random.seed(sseed)
    L, tau0 = fo.estimate_lipschitz(fo.LinearMap(fwd, adj, (N,), (N,)), closures(d, prox)[1], (N,))
    return float(L), float(tau0)


def twin_divergence(d, prox, opts, sseed):
    """(first iteration at which the oracle's step sizes differ, > 1e-6 relative, between the scipy.fftpack operator and its Makhoul twin, both
    started from the same L and tau0 -- the shorter iteration count if they never do; backtracks of the run up to there)."""
    sys.path.insert(0, ROOT)
    from tests.helpers import first_divergence
    L, tau0 = step_estimate(d, prox, sseed)
    a = oracle_run(d, prox, opts, L=L, tau0=tau0)
    b = oracle_run(d, prox, opts, pair=makhoul_pair, L=L, tau0=tau0)
    k = first_divergence(b.stepsizes, a.stepsizes, min(a.iteration_count, b.iteration_count))
    head = oracle_run(d, prox, dict(opts, max_iters=k, tolerance=0.0), L=L, tau0=tau0) if k else None
    return int(k), int(head.backtracks) if head is not None else 0


def main(reference):
    sys.path.insert(0, reference)
    os.environ.setdefault("MPLBACKEND", "Agg")
    import fasta as ref
    assert os.path.abspath(ref.__file__).startswith(os.path.abspath(reference)), ref.__file__
    os.makedirs(OUT, exist_ok=True)
    for name, ckw, prox, opts in case_table():
        np.random.seed(PROBLEM_SEED)
        d = construct(**ckw)
        f, gradf, g, proxg = closures(d, prox, shrink=ref.proximal.shrink, project_linf=ref.proximal.project_Linf_ball)
        N = ckw["N"]
        fwd, adj = fftpack_pair(d["mask"])
        A = ref.linalg.LinearMap(fwd, adj, (N,), (N,))
        np.random.seed(SOLVER_SEED)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            c = ref.fasta(A, f, gradf, g, proxg, np.zeros(N), verbose=False, **opts)
        out = dict(residuals=c.residuals, norm_residuals=c.norm_residuals, stepsizes=c.stepsizes, backtracks=np.int64(c.backtracks),
                   iteration_count=np.int64(c.iteration_count), solution=c.solution)
        if c.objectives is not None:
            out["objectives"] = c.objectives
        meta = dict(name=name, construct=ckw, prox=prox, problem_seed=PROBLEM_SEED, solver_seed=SOLVER_SEED, options=opts, numpy=np.__version__)
        if opts.get("adaptive"):
            k, bt = twin_divergence(d, prox, opts, SOLVER_SEED)
            meta["twin_divergence"], meta["backtracks_at_divergence"] = k, bt
        np.savez_compressed(os.path.join(OUT, name + ".npz"), meta=json.dumps(meta), **{"in_" + k: np.asarray(v) for k, v in d.items()}, **out)
        print(f"{name:32s} iters={int(c.iteration_count):4d} backtracks={int(c.backtracks):3d}" +
              (f" twin parts at {meta['twin_divergence']} ({meta['backtracks_at_divergence']} backtracks)" if "twin_divergence" in meta else ""))


if __name__ == "__main__":
    main(sys.argv[1])

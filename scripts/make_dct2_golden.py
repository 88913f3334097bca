"""Capture the compressive-imaging fixtures tests/golden/dct2/*.npz from the REFERENCE core, the way scripts/make_dct_golden.py captures the 1-D
ones:

    MPLBACKEND=Agg python scripts/make_dct2_golden.py <path to the reference checkout>

The operator is the subsampled 2-D DCT of an (H, W) image as a caller of the reference writes it -- `mask * dctn(x, norm='ortho')` and
`idctn(mask * w, norm='ortho')` from scipy.fftpack -- wrapped in the reference's `LinearMap`; the data are a 0/1 mask of M random coefficients
and Gaussian data on them, x0 = 0; the closures are those of the reference's democratic-representation example (l-infinity) or `mu * |x|_1`
with the reference's `shrink`, the image taken as the vector of its entries.  Stored: inputs, every history, the solution.

Adaptive runs amplify rounding, so every adaptive fixture also stores, in its meta, the iteration at which the NumPy
oracle parts from a TWIN of itself -- the same run with the operator computed by one complex FFT per row along each axis (Makhoul's
permutation, numpy.fft, the route the device takes) instead of scipy.fftpack, both given the same L and tau0 -- computed the way
scripts/make_dct_golden.py computes it.  tests/test_dct2_cpu.py recomputes it, tests/test_gpu_dct2.py pins the device run up to there."""
import json
import os
import sys
import warnings

import numpy as np
from numpy import linalg as la
from scipy.fftpack import dctn, idctn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "dct2")
TEST_MODES = dict(tolerance=1e-5, evaluate_objective=True)
MODES = {"adaptive": dict(adaptive=True, accelerate=False), "accelerated": dict(adaptive=False, accelerate=True),
         "plain": dict(adaptive=False, accelerate=False)}
PROBLEM_SEED, SOLVER_SEED = 11, 111


def construct(H=36, W=50, M=600, mu=0.05):
    """M random 2-D DCT coefficients out of the H * W (the constant one always among them), a 0/1 mask, Gaussian data on them."""
    samples = np.random.permutation(H * W - 1)[:M] + 1
    samples[M - 1] = 0
    samples.sort()
    mask = np.zeros(H * W)
    mask[samples] = 1
    b = np.zeros(H * W)
    b[samples] = np.random.randn(M)
    return dict(mask=mask.reshape(H, W), b=b.reshape(H, W), mu=np.float64(mu))


def fftpack_pair(mask):
    """The closures a caller writes."""
    return (lambda x: mask * dctn(x, norm='ortho')), (lambda w: idctn(mask * w, norm='ortho'))


def _makhoul_rows(X, adjoint):
    """The orthonormal DCT-II (adjoint: DCT-III) of every row of X by one complex FFT of the row's length."""
    N = X.shape[1]
    j = np.arange(N)
    src = np.where(j < (N + 1) // 2, 2 * j, 2 * (N - 1 - j) + 1)
    pw = np.exp(-1j * np.pi * j / (2 * N))
    s = np.full(N, np.sqrt(2.0 / N))
    s[0] = np.sqrt(1.0 / N)
    if not adjoint:
        return (pw * np.fft.fft(X[:, src], axis=1)).real * s
    u = X * np.where(j == 0, np.sqrt(N), np.sqrt(N / 2.0))
    um = np.zeros(X.shape)
    um[:, 1:] = u[:, 1:][:, ::-1]
    v = np.fft.ifft(pw.conj() * (u - 1j * um), axis=1).real
    out = np.empty(X.shape)
    out[:, src] = v
    return out


def makhoul_pair(mask):
    """The same operator by row FFTs along W, a transpose, row FFTs along H -- the twin's route, and the device's."""
    def fwd(x):
        return mask * _makhoul_rows(_makhoul_rows(x, False).T, False).T

    def adj(w):
        return _makhoul_rows(_makhoul_rows((mask * w).T, True).T, True)

    return fwd, adj


def closures(d, prox, shrink=None, project_linf=None):
    """f, gradf, g, proxg over the data `d`; prox = "linf" or "shrink" (mu * |x|_1); the image is the vector of its entries."""
    sys.path.insert(0, ROOT)
    from oracle import fasta_np as fo
    b, mu = d["b"], float(d["mu"])
    f = lambda z: .5 * la.norm((z - b).ravel()) ** 2
    gradf = lambda z: z - b
    if prox == "linf":
        project = project_linf or fo.prox_linf
        return f, gradf, (lambda x: mu * la.norm(x.ravel(), np.inf)), (lambda x, t: project(x.ravel(), t * mu).reshape(x.shape))
    soft = shrink or fo.shrink
    return f, gradf, (lambda x: mu * la.norm(x.ravel(), 1)), (lambda x, t: soft(x, t * mu))


def case_table():
    """(name, construct kwargs, prox, options)"""
    cases = [(f"dct2_8x12_{mode}", dict(H=8, W=12, M=48, mu=20.0), "linf", dict(TEST_MODES, **mo)) for mode, mo in MODES.items()]
    cases.append(("dct2_15x9_adaptive", dict(H=15, W=9, M=60, mu=20.0), "linf", dict(TEST_MODES, **MODES["adaptive"])))          # odd radices
    cases.append(("dct2_36x50_shrink_accelerated", dict(H=36, W=50, M=600, mu=0.05), "shrink", dict(TEST_MODES, **MODES["accelerated"])))
    cases.append(("dct2_12x8_adaptive", dict(H=12, W=8, M=48, mu=5.0), "linf", dict(TEST_MODES, **MODES["adaptive"])))          # the one that backtracks
    return cases


def oracle_run(d, prox, opts, sseed=None, pair=fftpack_pair, **given):
    """The NumPy oracle on the data `d` (solver seed set when no L / tau0 is given)."""
    sys.path.insert(0, ROOT)
    from oracle import fasta_np as fo
    f, gradf, g, proxg = closures(d, prox)
    shape = d["mask"].shape
    fwd, adj = pair(d["mask"])
    A = fo.LinearMap(fwd, adj, shape, shape)
    if sseed is not None:
        np.random.seed(sseed)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fo.fasta(A, f, gradf, g, proxg, np.zeros(shape), **dict(opts, **given))


def step_estimate(d, prox, sseed):
    """L and tau0 as the solver estimates them from its two probes under the solver seed."""
    sys.path.insert(0, ROOT)
    from oracle import fasta_np as fo
    shape = d["mask"].shape
    fwd, adj = fftpack_pair(d["mask"])
    np.random.seed(sseed)
    L, tau0 = fo.estimate_lipschitz(fo.LinearMap(fwd, adj, shape, shape), closures(d, prox)[1], shape)
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
        shape = d["mask"].shape
        fwd, adj = fftpack_pair(d["mask"])
        A = ref.linalg.LinearMap(fwd, adj, shape, shape)
        np.random.seed(SOLVER_SEED)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            c = ref.fasta(A, f, gradf, g, proxg, np.zeros(shape), verbose=False, **opts)
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

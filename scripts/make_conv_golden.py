"""Capture the deconvolution fixtures tests/golden/conv/*.npz from the REFERENCE core, the way scripts/make_tv3d_golden.py and
scripts/make_dct_golden.py capture theirs:

    MPLBACKEND=Agg python scripts/make_conv_golden.py <path to the reference checkout>

The solver is the reference's `fasta()` over its `LinearMap`; the operator is our own roll-based convolution (the closures of
`linalg.ConvMap`: `out += K[a,b] * np.roll(x, (a-oh, b-ow))`, the mask last, and the negated shifts of mask * w), the data our own seeded
star field (fasta_python_amd/examples/deconvolution.py: sparse non-negative spikes blurred by a Gaussian point-spread function plus noise), the
closures f = .5 |z - b|^2 and one of: mu |x|_1 with the reference's `shrink`, x >= 0, a box, the l-infinity term with its
`project_Linf_ball`, the l1 ball with its `project_L1_ball`, or no term at all.  Stored: inputs, every history, the solution.

Adaptive runs amplify summation order, so every adaptive fixture also stores, in its meta, the iteration at which the
NumPy oracle parts from a TWIN of itself -- the same problem with image, kernel, mask and data transposed: the same element arithmetic, every dot
product summed in another order -- both given the same L and tau0 so that they start from the same step: how far summation order alone lets two
correct solvers agree on that run.  "Parts" means: the first iteration at which ANY of the four histories the tests compare differs by more
than TWIN_RTOL = 1e-7 relative, a tenth of the tolerance the comparisons use (1e-6).  The twin is ONE other summation order and the device a
third; where rounding is being amplified the deviation grows about tenfold every two to three iterations (the nonneg case: 4e-8, 4e-7, 3e-6 at
iterations 76, 78, 80), so a run that is within 1e-7 of its twin leaves another order that much room before it reaches 1e-6.  tests/test_conv_cpu.py recomputes it, tests/test_gpu_conv.py pins the device run up to there.  The prefix
must be at least 20 iterations (or the whole run): asserted here; a case that gives a shorter one is replaced, the bound is not shortened.
Our own code and data only: nothing of the reference is copied."""
import json
import os
import sys
import warnings

import numpy as np
from numpy import linalg as la

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "conv")
TEST_MODES = dict(tolerance=1e-5, evaluate_objective=True)            # examples/__init__.py:63-91
MODES = {"adaptive": dict(adaptive=True, accelerate=False), "accelerated": dict(adaptive=False, accelerate=True),
         "plain": dict(adaptive=False, accelerate=False)}
MIN_PREFIX = 20
TWIN_RTOL = 1e-7
HISTORIES = ("residuals", "norm_residuals", "stepsizes", "objectives")
PROBLEM_SEED, SOLVER_SEED = 11, 111


def construct(shape, psf, sigma=1.2, noise=0.01, mu=0.02, missing=0.0, origin=None, seed=PROBLEM_SEED):
    """The example's star field (its draws, in its order) -- a (1, N) field for a signal; `psf`: a size, or (kh, kw) for a Gaussian cut to an
    even, off-centre window."""
    sys.path.insert(0, ROOT)
    from fasta_python_amd.examples.deconvolution import conv_closures, gaussian_psf, star_field
    rng = np.random.RandomState(seed)
    shape = tuple(shape)
    two = shape if len(shape) == 2 else (1, shape[0])
    truth = star_field(two, max(1, int(np.prod(two)) // 25), rng)
    if np.ndim(psf) == 0:
        k = gaussian_psf(psf, sigma) if len(shape) == 2 else gaussian_psf(psf, sigma)[psf // 2:psf // 2 + 1]
    else:
        full = gaussian_psf(2 * max(psf) + 1, sigma)
        k = full[:psf[0], :psf[1]]
    k = k / k.sum()
    o = (k.shape[0] // 2, k.shape[1] // 2) if origin is None else tuple(origin)
    b = conv_closures(k, o, None)[0](truth) + noise * rng.randn(*two)
    d = dict(kernel=k.reshape(k.shape if len(shape) == 2 else (-1,)), b=b.reshape(shape), truth=truth.reshape(shape), mu=np.float64(mu))
    if missing > 0.0:
        d["mask"] = (rng.rand(*two) >= missing).astype(np.float64).reshape(shape)
        d["b"] = d["mask"] * d["b"]
    return d, o


def operator_pair(d, origin, transpose=False):
    """(A, A^T, shape) as closures on arrays of the image's shape: ConvMap's host closures; transpose=True: the twin's."""
    sys.path.insert(0, ROOT)
    from fasta_python_amd.examples.deconvolution import conv_closures
    shape = d["b"].shape
    two = shape if len(shape) == 2 else (1, shape[0])
    k = d["kernel"].reshape(d["kernel"].shape if len(shape) == 2 else (1, -1))
    mask = d.get("mask")
    mask = None if mask is None else mask.reshape(two)
    if transpose:
        k, origin, mask, two = k.T.copy(), origin[::-1], (None if mask is None else mask.T.copy()), two[::-1]
        fwd, adj = conv_closures(k, origin, mask)
        return fwd, adj, two
    fwd, adj = conv_closures(k, origin, mask)
    return (lambda x: fwd(x.reshape(two)).reshape(shape)), (lambda w: adj(w.reshape(two)).reshape(shape)), shape


def closures(d, prox, box=None, b=None, shrink=None, project_linf=None, project_l1=None):
    sys.path.insert(0, ROOT)
    from oracle import fasta_np as fo
    b = d["b"] if b is None else b
    mu = float(d["mu"])
    f = lambda z: .5 * la.norm((z - b).ravel()) ** 2
    gradf = lambda z: z - b
    zero = lambda x: 0
    if prox == "shrink":
        soft = shrink or fo.shrink
        return f, gradf, (lambda x: mu * la.norm(x.ravel(), 1)), (lambda x, t: soft(x, t * mu))
    if prox == "nonneg":
        return f, gradf, zero, (lambda x, t: np.maximum(x, 0))
    if prox == "box":
        return f, gradf, zero, (lambda x, t: np.minimum(np.maximum(x, box[0]), box[1]))
    if prox == "linf":
        project = project_linf or fo.prox_linf
        return f, gradf, (lambda x: mu * la.norm(x.ravel(), np.inf)), (lambda x, t: project(x.ravel(), t * mu).reshape(x.shape))
    if prox == "l1ball":
        project = project_l1 or fo.project_l1
        return f, gradf, zero, (lambda x, t: project(x.ravel(), mu).reshape(x.shape))
    return f, gradf, zero, (lambda x, t: x)


def case_table():
    """(name, construct kwargs, prox, box, options)"""
    T = lambda mode, **kw: dict(TEST_MODES, **MODES[mode], **kw)
    return [
        ("conv_24x20_shrink_adaptive", dict(shape=(24, 20), psf=3, sigma=0.8), "shrink", None, T("adaptive")),
        ("conv_24x20_shrink_accelerated", dict(shape=(24, 20), psf=3, sigma=0.8), "shrink", None, T("accelerated")),
        ("conv_24x20_shrink_plain", dict(shape=(24, 20), psf=3, sigma=0.8), "shrink", None, T("plain")),
        ("conv_24x20_shrink_backtracking", dict(shape=(24, 20), psf=3, sigma=0.8), "shrink", None, T("plain", L=1.0, tau0=20.0)),   # forced: L = 1, a large first step
        ("conv_32x40_nonneg_adaptive", dict(shape=(32, 40), psf=5, sigma=1.0), "nonneg", None, T("adaptive")),
        ("conv_20x24_box_accelerated", dict(shape=(20, 24), psf=5, sigma=1.0), "box", (0.0, 3.0), T("accelerated")),
        ("conv_30x30_linf_accelerated", dict(shape=(30, 30), psf=3, sigma=0.8, mu=20.0), "linf", None, T("accelerated")),
        ("conv_30x30_l1ball_adaptive", dict(shape=(30, 30), psf=3, sigma=0.8, mu=60.0), "l1ball", None, T("adaptive")),
        ("conv_16x18_noprox_plain", dict(shape=(16, 18), psf=3, sigma=0.6), "none", None, T("plain")),
        ("conv_25x25_masked_shrink_adaptive", dict(shape=(25, 25), psf=5, sigma=1.0, missing=0.3), "shrink", None, T("adaptive")),
        ("conv_200_signal_shrink_accelerated", dict(shape=(200,), psf=9, sigma=1.5), "shrink", None, T("accelerated")),
        ("conv_20x22_even_offcentre_adaptive", dict(shape=(20, 22), psf=(4, 6), sigma=2.0, mu=0.005, origin=(0, 1)), "shrink", None, T("adaptive")),
    ]


def oracle_run(d, origin, prox, box, opts, sseed=None, transpose=False, **given):
    """The NumPy oracle on the data `d`, or on its transposed twin (solver seed set when no L / tau0 is given)."""
    sys.path.insert(0, ROOT)
    from oracle import fasta_np as fo
    fwd, adj, shape = operator_pair(d, origin, transpose)
    two = d["b"].shape if len(d["b"].shape) == 2 else (1, d["b"].shape[0])
    b = d["b"].reshape(two).T.copy() if transpose else d["b"]
    f, gradf, g, proxg = closures(d, prox, box, b=b)
    A = fo.LinearMap(fwd, adj, shape, shape)
    if sseed is not None:
        np.random.seed(sseed)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fo.fasta(A, f, gradf, g, proxg, np.zeros(shape), **dict(opts, **given))


def step_estimate(d, origin, prox, box, sseed):
    """L and tau0 as the solver estimates them from its two probes (fasta/__init__.py:100-113) under the solver seed."""
    sys.path.insert(0, ROOT)
    from oracle import fasta_np as fo
    fwd, adj, shape = operator_pair(d, origin)
    np.random.seed(sseed)
    L, tau0 = fo.estimate_lipschitz(fo.LinearMap(fwd, adj, shape, shape), closures(d, prox, box)[1], shape)
    return float(L), float(tau0)


def twin_divergence(d, origin, prox, box, opts, sseed):
    """(first iteration at which one of the oracle's histories differs, > TWIN_RTOL relative, between the problem and its transposed twin, both
    started from the same L and tau0 -- the shorter iteration count if none does; backtracks of the run up to there; that shorter count)."""
    sys.path.insert(0, ROOT)
    from tests.helpers import first_divergence
    L, tau0 = step_estimate(d, origin, prox, box, sseed)
    a = oracle_run(d, origin, prox, box, opts, L=L, tau0=tau0)
    b = oracle_run(d, origin, prox, box, opts, transpose=True, L=L, tau0=tau0)
    shorter = min(a.iteration_count, b.iteration_count)
    k = min(first_divergence(getattr(b, h), getattr(a, h), shorter, rtol=TWIN_RTOL) for h in HISTORIES)
    head = oracle_run(d, origin, prox, box, dict(opts, max_iters=k, tolerance=0.0), L=L, tau0=tau0) if k else None
    return int(k), int(head.backtracks) if head is not None else 0, int(shorter)


def main(reference):
    sys.path.insert(0, reference)
    os.environ.setdefault("MPLBACKEND", "Agg")
    import fasta as ref
    assert os.path.abspath(ref.__file__).startswith(os.path.abspath(reference)), ref.__file__
    os.makedirs(OUT, exist_ok=True)
    for name, ckw, prox, box, opts in case_table():
        d, origin = construct(**ckw)
        shape = d["b"].shape
        f, gradf, g, proxg = closures(d, prox, box, shrink=ref.proximal.shrink, project_linf=ref.proximal.project_Linf_ball,
                                      project_l1=ref.proximal.project_L1_ball)
        fwd, adj, _ = operator_pair(d, origin)
        A = ref.linalg.LinearMap(fwd, adj, shape, shape)
        np.random.seed(SOLVER_SEED)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            c = ref.fasta(A, f, gradf, g, proxg, np.zeros(shape), verbose=False, **opts)
        out = dict(residuals=c.residuals, norm_residuals=c.norm_residuals, stepsizes=c.stepsizes, backtracks=np.int64(c.backtracks),
                   iteration_count=np.int64(c.iteration_count), solution=c.solution)
        if c.objectives is not None:
            out["objectives"] = c.objectives
        meta = dict(name=name, construct={k: v for k, v in ckw.items()}, prox=prox, origin=list(origin) if len(shape) == 2 else [origin[1]],
                    problem_seed=PROBLEM_SEED, solver_seed=SOLVER_SEED, options=opts, numpy=np.__version__)
        if box is not None:
            meta["box"] = list(box)
        if opts.get("adaptive"):
            k, bt, shorter = twin_divergence(d, origin, prox, box, opts, SOLVER_SEED)
            assert k >= min(MIN_PREFIX, shorter), (name, k, shorter)
            meta["twin_divergence"], meta["backtracks_at_divergence"] = k, bt
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, meta=json.dumps(meta), **{"in_" + k: np.asarray(v) for k, v in d.items()}, **out)
        print(f"{name:40s} iters={int(c.iteration_count):4d} backtracks={int(c.backtracks):3d} {os.path.getsize(path) // 1024:3d} KiB" +
              (f" twin parts at {meta['twin_divergence']} ({meta['backtracks_at_divergence']} backtracks)" if "twin_divergence" in meta else ""))


if __name__ == "__main__":
    main(sys.argv[1])

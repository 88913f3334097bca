"""A regularisation path with duality-gap certificates: min_x f(A x) + mu * Omega(x) from the critical mu (above which the solution is zero) down
a geometric grid, every solve warm-started from the one before and stopped at gap <= 1e-6 * f(0) (fasta.path, fasta.stopping.DualityGap).
LASSO by default; --logistic: sparse logistic regression; --columns L: L right-hand sides and the row-wise l2 penalty (MMV); --sparse DENSITY: a
scipy.sparse design matrix.  On the device the matrix is uploaded once and the certificate is one call (fh_dual_gap, csrc/fh_gap.h).
--screen (least squares): gap-safe screening, every round solved over the columns the certificate could not prove zero (fasta.path(screen=True);
fh_screen and fh_gather_columns, csrc/fh_screen.h); the table then also lists the columns kept and the rounds of each point.
--standardize / --intercept (fasta.path(standardize=True, intercept=True); fh_standardize, csrc/fh_standardize.h): the generated columns then get
scales spread over six decades (and, with --intercept, offsets and an offset of the observations), the path runs on standardised columns, and the
table lists the support of the coefficients in the caller's units and the intercept.  Run it once with and once without --standardize: on the raw
columns one mu penalises a feature a million times more lightly than its neighbour, and the support follows the units instead of the signal.

    python -m fasta.examples.lasso_path [--backend hip|numpy] [--rows M] [--features N] [--sparse DENSITY] [--logistic] [--columns L] [--screen]
                                        [--standardize] [--intercept]

Three modes as in the other examples (adaptive, accelerated, plain); per point: mu, iterations, support size, relative gap.  The device does not
certify an accelerated iterate (the image of the extrapolated point is never stored): that mode reports the library's sentence on backend hip.
"""

import sys

import numpy as np

from .. import GroupShrink, LeastSquares, LogisticLoss, Shrink, path
from . import cli_backend

__all__ = ["construct", "run_modes", "main"]

MODES = (("adaptive", True, False), ("accelerated", False, True), ("plain", False, False))


def construct(M=200, N=1000, K=10, density=None, logistic=False, columns=1, sigma=0.01, seed=0, spread=False, offset=False):
    """(A, loss, prox_class): a seeded design matrix (dense, or scipy.sparse at `density`), K active features, its observations.  spread: column
    scales over six decades, the active coefficients sized to match; offset (dense): column offsets and observations shifted by 5."""
    rng = np.random.RandomState(seed)
    if density is None:
        A = rng.randn(M, N) / np.sqrt(M)
    else:
        from scipy import sparse as sp
        A = sp.random(M, N, density=density, format="csr", random_state=rng, data_rvs=rng.standard_normal)
    shape = (N,) if columns == 1 else (N, columns)
    x = np.zeros(shape)
    x[rng.permutation(N)[:K]] = rng.randn(*((K,) + shape[1:]))
    if spread:
        units = 10.0 ** rng.uniform(-3, 3, size=N)
        A = A @ sp.diags(units) if density is not None else A * units
        if offset and density is None:
            A = A + rng.randn(N) * units / np.sqrt(M)
        x = x / (units if columns == 1 else units[:, None])
    z = A @ x + (5.0 if offset else 0.0)
    if logistic:
        if columns != 1:
            raise SystemExit("--logistic goes with one column (the logistic loss has no multi-column form)")
        return A, LogisticLoss(2.0 * (rng.rand(M) < 1 / (1 + np.exp(-4.0 * z))) - 1), Shrink
    return A, LeastSquares(z + sigma * rng.randn(*z.shape)), (Shrink if columns == 1 else GroupShrink)


def run_modes(A, loss, prox_class, backend, n_mus=10, ratio=1e-2, gap_tolerance=1e-6, max_iters=5000, modes=MODES, screen=False,
              standardize=False, intercept=False):
    """The path in each mode; prints one line per point and returns {mode: list of Convergence, or the refusal's sentence}."""
    out = {}
    units = standardize or intercept                    # the path then uploads and rewrites a copy of its own, once per mode
    flags = dict(screen=True) if screen else {}
    if units:
        flags.update(standardize=standardize, intercept=intercept)
    if backend == "hip" and not hasattr(A, "ctx") and not units:      # one upload for all three modes
        from .. import DenseMatrixMap, SparseMatrixMap
        L = loss.b.shape[1] if loss.b.ndim == 2 else None
        A = SparseMatrixMap(A, rhs=L) if hasattr(A, "tocsr") else DenseMatrixMap(A, rhs=L)
    try:
        for label, adaptive, accelerate in modes:
            print()
            print("Computing the path with {} FBS.".format(label))
            np.random.seed(1)                           # the Lipschitz probes: the same draws for both backends
            try:
                pts = path(A, loss, prox_class, n_mus=n_mus, ratio=ratio, gap_tolerance=gap_tolerance, backend=backend, adaptive=adaptive,
                           accelerate=accelerate, max_iters=max_iters, **flags)
            except ValueError as refusal:
                if backend != "hip" or not accelerate:
                    raise
                print("not served on the device: {}".format(refusal))
                out[label] = str(refusal)
                continue
            print("{:>14}  {:>10}  {:>8}  {:>12}".format("mu", "iterations", "support", "relative gap") + ("  {:>8}  {:>6}".format("kept", "rounds") if screen else "")
                  + ("  {:>12}".format("intercept") if units else ""))
            for p in pts:
                rows = np.abs(np.reshape(p.coefficients if units else p.solution, (p.solution.shape[0], -1))).sum(axis=1)
                print("{:14.6e}  {:10d}  {:8d}  {:12.3e}".format(p.mu, p.iteration_count, int(np.count_nonzero(rows)), p.certificate.relative)
                      + ("  {:8d}  {:6d}".format(p.kept, p.rounds) if screen else "")
                      + ("  {:12.5e}".format(float(np.mean(p.intercept))) if units else ""))
            out[label] = pts
    finally:
        if hasattr(A, "close") and backend == "hip":
            A.close()
    return out


def _option(argv, name, cast, default):
    return cast(argv[argv.index(name) + 1]) if name in argv else default


def main(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    backend = cli_backend(argv)
    M, N = _option(argv, "--rows", int, 200), _option(argv, "--features", int, 1000)
    density, columns = _option(argv, "--sparse", float, None), _option(argv, "--columns", int, 1)
    standardize, intercept = "--standardize" in argv, "--intercept" in argv
    if intercept and ("--logistic" in argv or density is not None):
        raise SystemExit("--intercept goes with least squares on a dense matrix (the logistic intercept has no closed form; centring would fill a sparse matrix)")
    A, loss, prox_class = construct(M, N, density=density, logistic="--logistic" in argv, columns=columns, spread=standardize or intercept, offset=intercept)
    print("Constructed a {} path problem on a {} x {} {} design matrix, {} column(s).".format(
        "sparse logistic" if "--logistic" in argv else ("LASSO" if columns == 1 else "MMV"), M, N, "dense" if density is None else "sparse", columns))
    if "--screen" in argv and "--logistic" in argv:
        raise SystemExit("--screen goes with least squares (the screening radius of the logistic loss has another constant)")
    return run_modes(A, loss, prox_class, backend, screen="--screen" in argv, standardize=standardize, intercept=intercept)


if __name__ == "__main__":
    main()

"""Compressive imaging: min_x mu*||x||_1 + .5*||mask * dctn(x) - b||^2 -- recover a sparse image from a random subset of its 2-D DCT
coefficients, the textbook partial-transform sensing problem.  The image is a seeded star field (examples/deconvolution.py: sparse spikes on a
zero background); it is observed through M of its H * W orthonormal 2-D DCT coefficients, chosen at random (the constant one always among
them), plus Gaussian noise.  Nothing is downloaded.

    python -m fasta.examples.compressive_imaging [--backend hip|numpy] [--shape H W] [--samples M] [--mu MU]

backend "hip" runs the transform on the device through `DCTMap((H, W), mask)` (csrc/fh_dct2.h: no matrix is stored); "numpy" runs the closures
`mask * scipy.fftpack.dctn(x, norm='ortho')` and `scipy.fftpack.idctn(mask * w, norm='ortho')` on the generic host loop -- what the map is on
host arrays, bit for bit."""

import sys

import numpy as np
from numpy import linalg as la
from scipy.fftpack import dctn, idctn

from .. import DCTMap, LeastSquares, LinearMap, Shrink, fasta, proximal
from . import ExampleProblem, cli_backend, test_modes
from .deconvolution import _cli_value, star_field

__all__ = ["CompressiveImagingProblem"]


class CompressiveImagingProblem(ExampleProblem):
    def __init__(self, mask, b, mu, truth=None, backend="hip", solver_seed=None):
        """solver_seed: the global RNG is seeded with it before every solve (the solver's two step-size probes draw from it)."""
        self.mask, self.b, self.mu, self.truth = mask, b, mu, truth
        self.backend, self.solver_seed = backend, solver_seed
        self.A = LinearMap(lambda x: mask * dctn(x, norm='ortho'), lambda w: idctn(mask * w, norm='ortho'), b.shape, b.shape)

    def objective(self, x):
        r = self.A(x) - self.b
        return .5 * float(np.sum(r * r)) + self.mu * float(np.abs(x).sum())

    def relative_error(self, x):
        return float(la.norm(x - self.truth) / la.norm(self.truth))

    def solve(self, x0, fasta_options=None):
        opts = dict(verbose=False)
        opts.update(fasta_options or {})
        if self.solver_seed is not None:
            np.random.seed(self.solver_seed)
        if self.backend == "hip":
            op = self.device_operator(lambda: DCTMap(self.b.shape, self.mask, lazy=True))
            loss, reg = LeastSquares(self.b), Shrink(self.mu)
            c = fasta(op, loss.f, loss.gradf, reg.g, reg.prox, x0, backend="hip", **opts)
        else:
            f = lambda z: .5 * la.norm((z - self.b).ravel()) ** 2
            gradf = lambda z: z - self.b
            g = lambda x: self.mu * la.norm(x.ravel(), 1)
            proxg = lambda x, t: proximal.shrink(x, t * self.mu)
            c = fasta(self.A, f, gradf, g, proxg, x0, **opts)
        return c.solution, c

    @staticmethod
    def construct(shape=(64, 64), samples=None, noise=0.01, mu=0.02, stars=None, seed=None, backend="hip"):
        """samples=None: a third of the coefficients; stars=None: one pixel in fifty.  Draws, in this order, from RandomState(seed): the star
        positions and magnitudes, the sampled coefficients, the noise."""
        rng = np.random.RandomState(seed)
        shape = tuple(int(k) for k in shape)
        n = int(np.prod(shape))
        truth = star_field(shape, max(1, n // 50) if stars is None else int(stars), rng)
        M = max(1, n // 3) if samples is None else int(samples)
        if not 1 <= M <= n:
            raise ValueError(f"--samples must lie in [1, {n}] for an image of shape {shape} (got {M})")
        at = rng.permutation(n - 1)[:M] + 1
        at[M - 1] = 0                                       # the constant coefficient is always observed
        mask = np.zeros(n)
        mask[at] = 1.0
        mask = mask.reshape(shape)
        b = mask * (dctn(truth, norm='ortho') + noise * rng.randn(*shape))
        return CompressiveImagingProblem(mask, b, mu, truth=truth, backend=backend), np.zeros(shape)


def main(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    shape = _cli_value(argv, "--shape", 2, int, (64, 64))
    samples = _cli_value(argv, "--samples", 1, int, None)
    mu = _cli_value(argv, "--mu", 1, float, 0.02)
    backend = cli_backend(argv)
    problem, x0 = CompressiveImagingProblem.construct(shape=shape, samples=samples, mu=mu, seed=0, backend=backend)
    problem.solver_seed = 1
    print("Constructed compressive imaging problem: {} x {}, {} of {} DCT coefficients, mu = {}.".format(
        *shape, int(problem.mask.sum()), problem.mask.size, mu))
    results = test_modes(problem, x0, {"max_iters": 500})
    for label, (x, c) in zip(("adaptive", "accelerated", "plain"), results):
        print("{:12s} {:4d} iterations, {:3d} backtracks, objective {:.9e}, relative error {:.4f}".format(
            label, c.iteration_count, c.backtracks, problem.objective(x), problem.relative_error(x)))
    problem.close()
    return results


if __name__ == "__main__":
    main()

"""Sparse deconvolution: min_x mu*||x||_1 + .5*||d*(k conv x) - b||^2 -- the image-deblurring problem forward-backward splitting is best known
for (Beck & Teboulle's FISTA paper), here on a seeded synthetic star field: sparse non-negative spikes, blurred periodically by a Gaussian
point-spread function k, plus Gaussian noise; optionally a random share of the pixels is never observed (the 0/1 mask d: deconvolution and
inpainting at once).  `--nonneg` swaps the l1 term for the constraint x >= 0 (non-negative least squares, as in astronomy and microscopy).
Nothing is downloaded.

    python -m fasta.examples.deconvolution [--backend hip|numpy] [--shape H W] [--psf K] [--sigma S] [--mu MU] [--nonneg] [--missing FRACTION]
                                           [--closures]

backend "hip" runs the convolution on the device through `ConvMap(shape, psf, mask=d)` (csrc/fh_conv.h: no matrix is stored -- at 1024 x 1024
the explicit one would have 2^40 entries); "numpy" runs the same tagged operands on the generic host loop, where the map is its roll-based
closures -- the arithmetic the device keeps term by term; `--closures` (with "numpy") passes plain closures instead of tagged operands, the
reference's calling convention.  The three report the same iteration and backtrack counts on the default problem (a narrow point-spread function,
sigma = 0.8: the adaptive run is short and does not backtrack).  A wider one makes the problem ill-conditioned; an adaptive run of hundreds of
iterations with backtracking then amplifies the order of the device's sums and may count differently, as it does between
the problem and its own transpose on the host."""

import sys

import numpy as np
from numpy import linalg as la

from .. import ConvMap, LeastSquares, LinearMap, NonNeg, Shrink, fasta, proximal
from . import ExampleProblem, cli_backend, test_modes

__all__ = ["DeconvolutionProblem", "gaussian_psf", "star_field"]


def gaussian_psf(size, sigma):
    """A size x size Gaussian of standard deviation `sigma` pixels centred on the middle tap, normalised to sum 1."""
    r = np.arange(size) - size // 2
    k = np.exp(-0.5 * (r[:, None] ** 2 + r[None, :] ** 2) / float(sigma) ** 2)
    return k / k.sum()


def star_field(shape, count, rng):
    """`count` spikes at seeded pixels with magnitudes uniform in [1, 5) on a zero background."""
    x = np.zeros(shape)
    at = rng.permutation(int(np.prod(shape)))[:count]
    x.flat[at] = rng.uniform(1.0, 5.0, size=len(at))
    return x


def conv_closures(kernel, origin, mask):
    """The operator as two plain closures: `out += K[a,b] * np.roll(x, (a-oh, b-ow))` and the negated shifts of mask * w."""
    oh, ow = origin

    def rolls(x, sign):
        out = np.zeros(x.shape)
        for a in range(kernel.shape[0]):
            for b in range(kernel.shape[1]):
                out += kernel[a, b] * np.roll(x, (sign * (a - oh), sign * (b - ow)), axis=(0, 1))
        return out

    if mask is None:
        return (lambda x: rolls(x, 1)), (lambda w: rolls(w, -1))
    return (lambda x: mask * rolls(x, 1)), (lambda w: rolls(mask * w, -1))


class DeconvolutionProblem(ExampleProblem):
    def __init__(self, psf, mask, b, mu, truth=None, nonneg=False, backend="hip", solver_seed=None):
        """backend: "hip", "numpy" (tagged operands on the host loop) or "closures" (plain closures on the host loop).  solver_seed: the global
        RNG is seeded with it before every solve (the solver's two step-size probes draw from it)."""
        self.psf, self.mask, self.b, self.mu, self.truth, self.nonneg = psf, mask, b, mu, truth, nonneg
        self.backend, self.solver_seed = backend, solver_seed
        self.origin = (psf.shape[0] // 2, psf.shape[1] // 2)

    def operator(self):
        return self.device_operator(lambda: ConvMap(self.b.shape, self.psf, mask=self.mask))

    def objective(self, x):
        r = self.operator()(x) - self.b
        return .5 * float(np.sum(r * r)) + (0.0 if self.nonneg else self.mu * float(np.abs(x).sum()))

    def relative_error(self, x):
        return float(la.norm(x - self.truth) / la.norm(self.truth))

    def solve(self, x0, fasta_options=None):
        opts = dict(verbose=False)
        opts.update(fasta_options or {})
        if self.solver_seed is not None:
            np.random.seed(self.solver_seed)
        if self.backend == "closures":
            fwd, adj = conv_closures(self.psf, self.origin, self.mask)
            A = LinearMap(fwd, adj, self.b.shape, self.b.shape)
            f = lambda z: .5 * la.norm((z - self.b).ravel()) ** 2
            gradf = lambda z: z - self.b
            if self.nonneg:
                g, proxg = (lambda x: 0), (lambda x, t: np.maximum(x, 0))
            else:
                g, proxg = (lambda x: self.mu * la.norm(x.ravel(), 1)), (lambda x, t: proximal.shrink(x, t * self.mu))
            c = fasta(A, f, gradf, g, proxg, x0, **opts)
        else:
            loss, reg = LeastSquares(self.b), (NonNeg() if self.nonneg else Shrink(self.mu))
            c = fasta(self.operator(), loss.f, loss.gradf, reg.g, reg.prox, x0, backend=self.backend, **opts)
        return c.solution, c

    @staticmethod
    def construct(shape=(64, 64), psf=7, sigma=0.8, noise=0.01, mu=0.2, stars=None, missing=0.0, nonneg=False, seed=None, backend="hip"):
        """stars=None: one pixel in fifty.  Draws, in this order, from RandomState(seed): the star positions and magnitudes, the noise, the mask."""
        rng = np.random.RandomState(seed)
        shape = tuple(int(k) for k in shape)
        truth = star_field(shape, max(1, int(np.prod(shape)) // 50) if stars is None else int(stars), rng)
        k = gaussian_psf(psf, sigma)
        blurred = conv_closures(k, (psf // 2, psf // 2), None)[0](truth)
        b = blurred + noise * rng.randn(*shape)
        mask = None
        if missing > 0.0:
            mask = (rng.rand(*shape) >= missing).astype(np.float64)
            b = mask * b
        return DeconvolutionProblem(k, mask, b, mu, truth=truth, nonneg=nonneg, backend=backend), np.zeros(shape)


def _cli_value(argv, flag, count, cast, default):
    if flag not in argv:
        return default
    at = argv.index(flag)
    vals = [cast(v) for v in argv[at + 1:at + 1 + count]]
    if len(vals) != count:
        raise SystemExit(f"{flag} takes {count} value(s)")
    return vals[0] if count == 1 else tuple(vals)


def main(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    shape = _cli_value(argv, "--shape", 2, int, (64, 64))
    psf = _cli_value(argv, "--psf", 1, int, 7)
    sigma = _cli_value(argv, "--sigma", 1, float, 0.8)
    mu = _cli_value(argv, "--mu", 1, float, 0.2)
    missing = _cli_value(argv, "--missing", 1, float, 0.0)
    backend = cli_backend(argv)
    if "--closures" in argv:
        if backend != "numpy":
            raise SystemExit("--closures goes with --backend numpy")
        backend = "closures"
    problem, x0 = DeconvolutionProblem.construct(shape=shape, psf=psf, sigma=sigma, mu=mu, missing=missing, nonneg="--nonneg" in argv,
                                                 seed=0, backend=backend)
    problem.solver_seed = 1
    print("Constructed deconvolution problem: {} x {}, {} x {} point-spread function, {}{}.".format(
        *shape, psf, psf, "x >= 0" if problem.nonneg else f"mu = {mu}", f", {missing:.0%} of the pixels missing" if missing > 0.0 else ""))
    results = test_modes(problem, x0, {"max_iters": 500})
    for label, (x, c) in zip(("adaptive", "accelerated", "plain"), results):
        print("{:12s} {:4d} iterations, {:3d} backtracks, objective {:.9e}, relative error {:.4f}".format(
            label, c.iteration_count, c.backtracks, problem.objective(x), problem.relative_error(x)))
    problem.close()
    return results


if __name__ == "__main__":
    main()

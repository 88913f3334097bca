"""Volumetric total-variation denoising: min_X mu*TV(X) + .5*||X - M||^2 over a (D, H, W) volume through its dual,
min_Y .5*||div(Y) - M/mu||^2 with ||Y_p|| <= 1 for every voxel's 3-vector -- the N = 3 case of the reference's N-dimensional `grad` / `div`
(fasta/examples/tv_denoising.py:26-63) and of its recipe (:85-103 solve, :105-125 construct).  The volume is synthetic and seeded:
{0, 1} blocks, or spheres, plus Gaussian noise; nothing is downloaded.

    python -m fasta.examples.tv_denoising3d [--backend hip|numpy] [--shape D H W] [--mu 0.1] [--sigma 0.1] [--spheres]

backend "hip" runs the 3-D stencil kernels (csrc/fh_tv3d.h) through `GradDivMap((D, H, W))`, "numpy" the reference's closures on the host loop."""

import sys

import numpy as np
from numpy import linalg as la

from .. import GradDivMap, LeastSquares, TVDualBall, fasta
from . import ExampleProblem, cli_backend, test_modes
from .tv_denoising import div, grad

__all__ = ["TVDenoising3DProblem", "blocks", "spheres"]


def blocks(shape, side):
    """{0, 1} blocks of `side` voxels: the 3-D checkerboard."""
    idx = np.indices(shape)
    return (sum(i // side for i in idx) % 2).astype(float)


def spheres(shape, count, seed):
    """`count` solid balls at seeded centres, radii between an eighth and a quarter of the smallest dimension, valued 1 on a 0 background."""
    rng = np.random.RandomState(seed)
    idx = np.indices(shape).astype(float)
    out = np.zeros(shape)
    for _ in range(count):
        centre = [rng.uniform(0, n) for n in shape]
        radius = rng.uniform(0.125, 0.25) * min(shape)
        out[sum((i - c) ** 2 for i, c in zip(idx, centre)) <= radius ** 2] = 1.0
    return out


class TVDenoising3DProblem(ExampleProblem):
    def __init__(self, M, mu, backend="hip"):
        self.M, self.mu, self.backend = M, mu, backend

    def solve(self, Y0, fasta_options=None):
        opts = dict(verbose=False)
        opts.update(fasta_options or {})
        if self.backend == "numpy":                 # the reference's closures and bare-function operator pair (tv_denoising.py:85-99)
            f = lambda Z: .5 * la.norm((Z - self.M / self.mu).ravel()) ** 2
            gradf = lambda Z: Z - self.M / self.mu
            g = lambda Y: 0

            def proxg(Y, t):
                lengths = np.maximum(la.norm(Y, axis=Y.ndim - 1), 1)
                return Y / lengths[..., np.newaxis]

            c = fasta(div, grad, f, gradf, g, proxg, Y0, **opts)
            return self.M - self.mu * div(c.solution), c            # tv_denoising.py:101
        op = self.device_operator(lambda: GradDivMap(self.M.shape))
        loss, reg = LeastSquares(self.M / self.mu), TVDualBall()
        c = fasta(op, op.H, loss.f, loss.gradf, reg.g, reg.prox, Y0, backend="hip", **opts)
        return self.M - self.mu * div(c.solution), c

    @staticmethod
    def construct(sigma=0.1, mu=0.1, shape=(32, 32, 32), side=8, seed=None, backend="hip", balls=0):
        """balls = 0: blocks of `side` voxels; balls = k > 0: k seeded spheres.  Noise from the global RNG (seeded by `seed` when given)."""
        if seed is not None:
            np.random.seed(seed)
        M = spheres(shape, balls, 0 if seed is None else seed) if balls else blocks(shape, side)
        M /= max(np.max(M), 1.0)
        M += sigma * np.random.randn(*M.shape)
        return TVDenoising3DProblem(M, mu, backend=backend), np.zeros(M.shape + (3,))


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
    shape = _cli_value(argv, "--shape", 3, int, (32, 32, 32))
    mu = _cli_value(argv, "--mu", 1, float, 0.1)
    sigma = _cli_value(argv, "--sigma", 1, float, 0.1)
    problem, Y0 = TVDenoising3DProblem.construct(sigma=sigma, mu=mu, shape=shape, side=max(1, min(shape) // 4), seed=0,
                                                 backend=cli_backend(argv), balls=3 if "--spheres" in argv else 0)
    print("Constructed volumetric total-variation denoising problem: {} x {} x {}, mu = {}.".format(*shape, mu))
    np.random.seed(1)
    results = test_modes(problem, Y0, {"max_iters": 300})
    problem.close()
    return results


if __name__ == "__main__":
    main()

"""Democratic representation (l-infinity-penalised least squares): min_x mu*||x||_inf + .5*||Ax - b||^2 with A a randomly subsampled
orthonormal DCT -- a solution of low dynamic range.  Recipe: fasta/examples/democratic_representation.py:42-45 (closures), :61-82 (construct:
the same draws from the global RNG in the same order; the operator is `mask * dct(x, norm='ortho')` / `idct(mask * x, norm='ortho')`).

    python -m fasta.examples.democratic_representation [--backend hip|numpy] [--points N] [--samples M] [--mu MU]

backend "hip" runs the transform on the device through `DCTMap(N, mask)` (csrc/fh_dct.h: no matrix is stored, so N = 2^16 ... 2^22 is in reach),
"numpy" the reference's closures on the host loop."""

import sys

import numpy as np
from numpy import linalg as la
from scipy.fftpack import dct, idct

from .. import DCTMap, LeastSquares, LinearMap, LinfProx, fasta, proximal
from . import ExampleProblem, cli_backend, test_modes

__all__ = ["DemocraticRepresentationProblem"]


class DemocraticRepresentationProblem(ExampleProblem):
    def __init__(self, mask, b, mu, backend="hip", solver_seed=None):
        """solver_seed: the global RNG is seeded with it before every solve (the solver's two step-size probes draw from it), so that the three
        modes of one command line are each a reproducible run."""
        self.mask, self.b, self.mu, self.backend, self.solver_seed = mask, b, mu, backend, solver_seed
        # the reference's operator (:80-82): what backend "numpy" runs
        self.A = LinearMap(lambda x: mask * dct(x, norm='ortho'), lambda x: idct(mask * x, norm='ortho'), b.shape)

    def solve(self, x0, fasta_options=None):
        opts = dict(verbose=False)
        opts.update(fasta_options or {})
        if self.solver_seed is not None:
            np.random.seed(self.solver_seed)
        if self.backend == "numpy":                 # the reference's closures (:42-45), 6-argument call
            f = lambda z: .5 * la.norm((z - self.b).ravel()) ** 2
            gradf = lambda z: z - self.b
            g = lambda x: self.mu * la.norm(x, np.inf)
            proxg = lambda x, t: proximal.project_Linf_ball(x, t * self.mu)
            c = fasta(self.A, f, gradf, g, proxg, x0, **opts)
        else:
            op = self.device_operator(lambda: DCTMap(len(self.b), self.mask, lazy=True))
            loss, reg = LeastSquares(self.b), LinfProx(self.mu)
            c = fasta(op, loss.f, loss.gradf, reg.g, reg.prox, x0, backend="hip", **opts)
        return c.solution, c

    @staticmethod
    def construct(M=500, N=1000, mu=300.0, seed=None, backend="hip"):
        if seed is not None:
            np.random.seed(seed)
        samples = np.random.permutation(N - 1)[:M] + 1          # a random set of DCT modes ...
        samples[M - 1] = 1                                      # ... the last one replaced by mode 1
        samples.sort()
        mask = np.zeros(N)
        mask[samples] = 1
        b = np.zeros(N)
        b[samples] = np.random.randn(M)
        return DemocraticRepresentationProblem(mask, b, mu, backend=backend), np.zeros(N)


def _cli_value(argv, flag, cast, default):
    if flag not in argv:
        return default
    at = argv.index(flag)
    if at + 1 >= len(argv):
        raise SystemExit(f"{flag} takes a value")
    return cast(argv[at + 1])


def main(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    N = _cli_value(argv, "--points", int, 1000)
    M = _cli_value(argv, "--samples", int, N // 2)
    mu = _cli_value(argv, "--mu", float, 300.0)
    problem, x0 = DemocraticRepresentationProblem.construct(M=M, N=N, mu=mu, seed=7, backend=cli_backend(argv))
    problem.solver_seed = 107
    print("Constructed democratic representation problem.")
    results = test_modes(problem, x0)
    problem.close()
    return results


if __name__ == "__main__":
    main()

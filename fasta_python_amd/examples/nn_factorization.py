"""The l1-penalised non-negative matrix factorisation min_{X, Y} mu ||X||_1 + .5 ||S - X Y^T||^2 with 0 <= Y <= 1
(fasta/examples/nn_factorization.py:1-113).  The two factors are stacked into one unknown Z = [X; Y] (:43), the smooth term is bilinear --
f(Z) = .5 ||S - X Y^T||^2, gradf(Z) = [d Y; d^T X] with d = X Y^T - S (:48-57) -- and the prox shrinks X and clips Y (:59-61).  The problem is
not convex, but FBS is still often effective.  On the device one pass over S gives the value and both halves of the gradient
(losses.Factorization, proximal.RowSplit; csrc/fh_bilinear.h).

    python -m fasta.examples.nn_factorization [--backend hip|numpy] [--rows 800] [--cols 200] [--rank 10]
"""

import numpy as np
from numpy import linalg as la

from .. import Box, Factorization, RowSplit, Shrink, fasta, proximal
from . import ExampleProblem, cli_backend, test_modes
from .sparse_mmv import cli_value

__all__ = ["NNFactorizationProblem"]


class NNFactorizationProblem(ExampleProblem):
    def __init__(self, S, mu, X=None, Y=None, backend="hip"):
        self.S, self.mu, self.X, self.Y, self.backend = S, mu, X, Y, backend

    def solve(self, inits, fasta_options=None):
        """`inits` = (X0, Y0); returns ((X, Y), Convergence)."""
        opts = dict(verbose=False)
        opts.update(fasta_options or {})
        Z0 = np.concatenate(inits)                  # the unknowns as one matrix (:43)
        N = inits[0].shape[0]                       # first N rows of Z are X (:46)
        S, mu = self.S, self.mu
        if self.backend == "numpy":                 # the reference's closures (:48-61)
            f = lambda Z: .5 * la.norm((S - Z[:N, ...] @ Z[N:, ...].T).ravel())**2

            def gradf(Z):
                X = Z[:N, ...]
                Y = Z[N:, ...]
                d = X @ Y.T - S
                return np.concatenate((d @ Y, d.T @ X))

            g = lambda Z: mu * la.norm(Z[:N, ...].ravel(), 1)
            proxg = lambda Z, t: np.concatenate((proximal.shrink(Z[:N, ...], t * mu),
                                                 np.minimum(np.maximum(Z[N:, ...], 0), 1)))
            c = fasta(None, None, f, gradf, g, proxg, Z0, **opts)
        else:
            loss, reg = Factorization(S), RowSplit(N, Shrink(mu), Box(0.0, 1.0))
            c = fasta(None, None, loss.f, loss.gradf, reg.g, reg.prox, Z0, backend="hip", **opts)
        return (c.solution[:N, ...], c.solution[N:, ...]), c

    @staticmethod
    def construct(M=800, N=200, K=10, b=0.75, sigma=0.1, mu=1.0, seed=None, backend="hip"):
        """Two random factors, the first made sparse, their noisy product and an initial guess, in the reference's RNG order (:80-94)."""
        if seed is not None:
            np.random.seed(seed)
        X = np.random.rand(M, K)
        Y = np.random.rand(N, K)
        X *= np.random.rand(M, K) > b
        S = X @ Y.T + sigma * np.random.randn(M, N)
        X0 = np.zeros((M, K))
        Y0 = np.random.rand(N, K)
        return NNFactorizationProblem(S, mu, X=X, Y=Y, backend=backend), (X0, Y0)


if __name__ == "__main__":
    backend = cli_backend()
    M, N, K = cli_value("--rows", 800, int), cli_value("--cols", 200, int), cli_value("--rank", 10, int)
    problem, inits = NNFactorizationProblem.construct(M=M, N=N, K=K, backend=backend)
    print("Constructed non-negative matrix factorization problem.")
    np.random.seed(1)                               # the Lipschitz probes: the same draws for both backends
    results = test_modes(problem, inits)
    print("Iterations (adaptive, accelerated, plain): {}, {}, {}".format(*(c.iteration_count for _, c in results)))
    (X, Y), c = results[0]
    print("Adaptive run: relative misfit ||S - X Y^T|| / ||S|| = {:.4f}, non-zeros of X: {:.1f}%".format(
        la.norm(problem.S - X @ Y.T) / la.norm(problem.S), 100 * np.count_nonzero(X) / X.size))
    problem.close()

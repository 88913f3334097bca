"""The max-norm problem min_X <S, X X^T> subject to ||X_i||_2 <= mu for every row X_i of the (N, K) matrix X -- a relaxation of max-cut used
here to split a two-moons data set (fasta/examples/max_norm.py:22-95).  The smooth term is quadratic on Q = S + S^T, which has negative eigenvalues:
sum(S * (X @ X.T)) = .5 <X, Q X> and gradf(X) = Q X (:49-50), the prox projects every row onto the ball of radius mu (:53-59).  On the device
one product W = Q X per attempt gives both the value and the gradient (losses.Quadratic, proximal.RowBall; csrc/fh_quad.h).

    python -m fasta.examples.max_norm [--backend hip|numpy] [--points 2000] [--rank 10]
"""

import numpy as np
from numpy import linalg as la

from .. import Quadratic, RowBall, fasta
from . import ExampleProblem, cli_backend, test_modes
from .sparse_mmv import cli_value

__all__ = ["MaxNormProblem"]


class MaxNormProblem(ExampleProblem):
    def __init__(self, points, mu, sigma=0.1, delta=0.01, backend="hip"):
        self.points, self.mu, self.backend = points, mu, backend
        # similarity matrix from the distances between the points, then the edge weights (:36-40)
        diff = points[:, None, :] - points[None, :, :]
        distances = np.sqrt(np.sum(diff * diff, axis=2))
        self.S = delta - np.exp(-distances ** 2 / sigma ** 2 / 2)

    def solve(self, X0, fasta_options=None):
        opts = dict(verbose=False)
        opts.update(fasta_options or {})
        S, mu = self.S, self.mu
        if self.backend == "numpy":                 # the reference's closures (:49-59)
            f = lambda X: np.sum(S * (X @ X.T))
            gradf = lambda X: (S + S.T) @ X
            g = lambda X: 0

            def proxg(X, t):
                norms = la.norm(X, axis=1)
                scale = np.maximum(norms, mu) + (norms == 0)
                return mu * X / scale[:, np.newaxis]

            c = fasta(None, None, f, gradf, g, proxg, X0, **opts)
        else:
            loss, reg = Quadratic(S + S.T), RowBall(mu)
            c = fasta(None, None, loss.f, loss.gradf, reg.g, reg.prox, X0, backend="hip", **opts)
        return c.solution, c

    @staticmethod
    def construct(N=2000, D=2, noise=0.15, dx=(1, 0.5), K=10, mu=1.0, seed=None, backend="hip"):
        """Two moons in D dimensions and an initial guess, in the reference's RNG order (:78-93)."""
        if seed is not None:
            np.random.seed(seed)
        theta = np.arange(0, N) / N * 2 * np.pi
        points = np.zeros((N, D))
        points[:, 0] = np.cos(theta)
        points[:, 1] = np.sin(theta)
        points[:N // 2, :2] -= dx
        points += noise * np.random.randn(N, D)
        X0 = np.random.randn(N, K) / np.sqrt(K) / 10
        return MaxNormProblem(points, mu, backend=backend), X0

    def labels(self, solution, seed=0):
        """A random hyperplane rounding of the rows (:102)."""
        return np.sign(solution @ np.random.RandomState(seed).randn(solution.shape[1]))


if __name__ == "__main__":
    backend, N, K = cli_backend(), cli_value("--points", 2000, int), cli_value("--rank", 10, int)
    problem, X0 = MaxNormProblem.construct(N=N, K=K, backend=backend)
    print("Constructed max-norm problem.")
    np.random.seed(1)                               # the Lipschitz probes: the same draws for both backends
    results = test_modes(problem, X0)
    print("Iterations (adaptive, accelerated, plain): {}, {}, {}".format(*(c.iteration_count for _, c in results)))
    lab = problem.labels(results[0][0])
    print("Top moon / bottom moon majority labels: {:+.0f} / {:+.0f}".format(np.sign(lab[:N // 2].sum()), np.sign(lab[N // 2:].sum())))
    problem.close()

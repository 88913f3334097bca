"""LASSO and sparse logistic regression on a SPARSE design matrix: min_x mu*||x||_1 + f(S x) with S a seeded random scipy.sparse matrix
(bag-of-words features, one-hot encodings: the shape these problems arrive in).  The closures are those of
fasta/examples/sparse_least_squares.py:41-44 and sparse_logistic.py:47-50; the operator is what the reference is given for such a matrix,
`LinearMap(lambda x: S @ x, lambda y: S.T @ y, ...)`.  On the device S stays sparse: kept by rows and by columns, both directions gathers
(linalg.SparseMatrixMap, csrc/fh_sparse.h).

    python -m fasta.examples.sparse_design [--backend hip|numpy] [--density 0.01]
"""

import sys

import numpy as np
from numpy import linalg as la

from .. import LeastSquares, LinearMap, LogisticLoss, Shrink, SparseMatrixMap, fasta, proximal
from . import ExampleProblem, cli_backend, test_modes

__all__ = ["SparseDesignProblem"]


class SparseDesignProblem(ExampleProblem):
    def __init__(self, S, b, mu, logistic=False, x=None, backend="hip"):
        self.S, self.b, self.mu, self.logistic, self.x, self.backend = S, b, mu, logistic, x, backend

    def solve(self, x0, fasta_options=None):
        opts = dict(verbose=False)
        opts.update(fasta_options or {})
        S, b, mu = self.S, self.b, self.mu
        if self.backend == "numpy":                 # the reference's closures over the closure LinearMap
            if self.logistic:
                f = lambda z: np.sum(np.log(1 + np.exp(z)) - (b == 1) * z)
                gradf = lambda z: -b / (1 + np.exp(b * z))
            else:
                f = lambda z: .5 * la.norm((z - b).ravel()) ** 2
                gradf = lambda z: z - b
            g = lambda x: mu * la.norm(x.ravel(), 1)
            proxg = lambda x, t: proximal.shrink(x, t * mu)
            A = LinearMap(lambda x: S @ x, lambda y: S.T @ y, (S.shape[1],), (S.shape[0],))
            c = fasta(A, f, gradf, g, proxg, x0, **opts)
        else:
            op = self.device_operator(lambda: SparseMatrixMap(S))
            loss, reg = (LogisticLoss(b) if self.logistic else LeastSquares(b)), Shrink(mu)
            c = fasta(op, op.H, loss.f, loss.gradf, reg.g, reg.prox, x0, backend="hip", **opts)
        return c.solution, c

    @staticmethod
    def construct(M=2000, N=4000, K=20, density=0.01, sigma=0.01, mu=None, logistic=False, seed=0, backend="hip"):
        from scipy import sparse as sp
        rng = np.random.RandomState(seed)
        S = sp.random(M, N, density=density, format="csr", random_state=rng, data_rvs=rng.standard_normal)
        x = np.zeros(N)
        if logistic:
            x[rng.permutation(N)[:K]] = 1
            b = 2.0 * (rng.rand(M) < 1 / (1 + np.exp(-(S @ x)))) - 1
        else:
            x[rng.permutation(N)[:K]] = rng.randn(K)
            b = S @ x + sigma * rng.randn(M)
        if mu is None:
            mu = 1.0 if logistic else 0.1
        return SparseDesignProblem(S, b, mu, logistic=logistic, x=x, backend=backend), np.zeros(N)


def cli_density(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    return float(argv[argv.index("--density") + 1]) if "--density" in argv else 0.01


if __name__ == "__main__":
    backend, density = cli_backend(), cli_density()
    for logistic in (False, True):
        problem, x0 = SparseDesignProblem.construct(density=density, logistic=logistic, backend=backend)
        print("Constructed {} problem on a {} x {} design matrix with {} stored entries.".format(
            "sparse logistic" if logistic else "LASSO", problem.S.shape[0], problem.S.shape[1], problem.S.nnz))
        np.random.seed(1)                           # the Lipschitz probes: the same draws for both backends
        test_modes(problem, x0)
        problem.close()

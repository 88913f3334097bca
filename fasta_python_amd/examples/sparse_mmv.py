"""Multiple measurement vectors through a SPARSE sensing matrix: min_X mu * sum_i ||X_i||_2 + .5*||S X - B||_F^2 over matrices X of shape
(N, L), X_i its rows -- the problem of fasta/examples/mmv.py:49-61 (f, gradf, g, proxg) and :66-94 (construct) with a seeded random
scipy.sparse matrix S in place of the dense A.  The operator is what the reference is given for such a matrix,
`LinearMap(lambda X: S @ X, lambda Y: S.T @ Y, (N, L), (M, L))`.  On the device S stays sparse and the unknown is a matrix: every stored
entry gathers one whole row of X and is read once for all L columns, and the row-wise shrink runs as FH_PROX_GROUP
(linalg.SparseMatrixMap(S, rhs=L), csrc/fh_spmulti.h).

    python -m fasta.examples.sparse_mmv [--backend hip|numpy] [--density 0.05] [--columns 10]
"""

import sys

import numpy as np
from numpy import linalg as la

from .. import GroupShrink, LeastSquares, LinearMap, SparseMatrixMap, fasta, proximal
from . import ExampleProblem, cli_backend, test_modes

__all__ = ["SparseMMVProblem"]


class SparseMMVProblem(ExampleProblem):
    def __init__(self, S, B, mu, X=None, backend="hip"):
        self.S, self.B, self.mu, self.X, self.backend = S, B, mu, X, backend

    def solve(self, X0, fasta_options=None):
        opts = dict(verbose=False)
        opts.update(fasta_options or {})
        S, B, mu = self.S, self.B, self.mu
        (M, N), L = S.shape, np.shape(X0)[1]
        if self.backend == "numpy":                 # the reference's closures over the closure LinearMap
            f = lambda Z: .5 * la.norm((Z - B).ravel()) ** 2
            gradf = lambda Z: Z - B
            g = lambda X: mu * np.sum(np.sqrt(np.sum(X * X, axis=1)))

            def proxg(X, t):
                norms = la.norm(X, axis=1)
                scale = proximal.shrink(norms, mu * t) / (norms + (norms == 0))
                return X * scale[:, np.newaxis]

            A = LinearMap(lambda X: S @ X, lambda Y: S.T @ Y, (N, L), (M, L))
            c = fasta(A, f, gradf, g, proxg, X0, **opts)
        else:
            op = self.device_operator(lambda: SparseMatrixMap(S, rhs=L))
            loss, reg = LeastSquares(B), GroupShrink(mu)
            c = fasta(op, op.H, loss.f, loss.gradf, reg.g, reg.prox, X0, backend="hip", **opts)
        return c.solution, c

    @staticmethod
    def construct(M=400, N=600, L=10, K=12, density=0.05, sigma=0.1, mu=1.0, seed=0, backend="hip"):
        from scipy import sparse as sp
        rng = np.random.RandomState(seed)
        S = sp.random(M, N, density=density, format="csr", random_state=rng, data_rvs=rng.standard_normal)
        X = np.zeros((N, L))                        # K rows carry signal
        X[rng.permutation(N)[:K]] = rng.randn(K, L)
        B = S @ X + sigma * rng.randn(M, L)
        return SparseMMVProblem(S, B, mu, X=X, backend=backend), np.zeros((N, L))


def cli_value(flag, default, kind, argv=None):
    argv = sys.argv[1:] if argv is None else argv
    return kind(argv[argv.index(flag) + 1]) if flag in argv else default


if __name__ == "__main__":
    backend, density, columns = cli_backend(), cli_value("--density", 0.05, float), cli_value("--columns", 10, int)
    problem, X0 = SparseMMVProblem.construct(density=density, L=columns, backend=backend)
    print("Constructed MMV problem with {} columns on a {} x {} sensing matrix with {} stored entries.".format(
        columns, problem.S.shape[0], problem.S.shape[1], problem.S.nnz))
    np.random.seed(1)                               # the Lipschitz probes: the same draws for both backends
    counts = [c.iteration_count for _, c in test_modes(problem, X0)]
    print("Iterations (adaptive, accelerated, plain): {}, {}, {}".format(*counts))
    problem.close()

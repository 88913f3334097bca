"""Multiple measurement vectors: min_X mu * sum_i ||X_i||_2 + .5*||A X - B||_F^2 over matrices X of shape (N, L), X_i its rows --
L sparse signals that share one support, observed through one A.
Recipe: fasta/examples/mmv.py:49-61 (f, gradf, g, proxg: here LeastSquares and GroupShrink), :66-94 (construct).  On the device the unknown is a matrix: A is read once per
pass for all L columns and the row-wise shrink runs as FH_PROX_GROUP (csrc/fh_multi.h)."""

import numpy as np

from .. import DenseMatrixMap, GroupShrink, LeastSquares, fasta
from . import ExampleProblem, cli_backend, test_modes

__all__ = ["MMVProblem"]


class MMVProblem(ExampleProblem):
    def __init__(self, A, At, B, mu, X=None, backend="hip"):
        self.A, self.At, self.B, self.mu, self.X, self.backend = A, At, B, mu, X, backend

    def solve(self, X0, fasta_options=None):
        opts = dict(verbose=False)
        opts.update(fasta_options or {})
        if self.backend == "numpy":                 # the same tagged operands as ordinary callables on the generic host loop
            loss, reg = LeastSquares(self.B), GroupShrink(self.mu)
            c = fasta(self.A, self.At, loss.f, loss.gradf, reg.g, reg.prox, X0, backend="numpy", **opts)
        else:
            L = np.shape(X0)[1]
            op = self.A if isinstance(self.A, DenseMatrixMap) else self.device_operator(lambda: DenseMatrixMap(np.asarray(self.A), rhs=L))
            loss, reg = LeastSquares(self.B), GroupShrink(self.mu)
            c = fasta(op, op.H, loss.f, loss.gradf, reg.g, reg.prox, X0, backend="hip", **opts)
        return c.solution, c

    @staticmethod
    def construct(M=20, N=30, L=10, K=7, sigma=0.1, mu=1.0, seed=None, backend="hip"):
        if seed is not None:
            np.random.seed(seed)
        X = np.zeros((N, L))                        # K rows carry signal (same global-RNG draw order as mmv.py:81-91)
        X[np.random.permutation(N)[:K], ] = np.random.randn(K, L)
        A = np.random.randn(M, N)
        B = A @ X + sigma * np.random.randn(M, L)
        return MMVProblem(A, A.T, B, mu, X=X, backend=backend), np.zeros((N, L))


if __name__ == "__main__":
    problem, X0 = MMVProblem.construct(backend=cli_backend())
    print("Constructed MMV problem.")
    test_modes(problem, X0)
    problem.close()

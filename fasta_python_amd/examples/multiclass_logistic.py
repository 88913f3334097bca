"""Sparse multinomial (multi-class) logistic regression: min_X mu * ||X||_1 + sum_i [logsumexp((A X)_i,:) - (A X)_i,y_i] over weight
matrices X of shape (N, L), one column per class -- or, with --group, mu * sum_j ||X_j||_2 over the rows of X: a feature is kept or dropped
for all classes at once (the "grouped" multinomial of glmnet).  The reference has no multinomial example; this one follows the recipe of
examples/sparse_logistic.py (seeded data, labels drawn from the model, the three modes of test_modes) with the softmax of A X_true for a
row-sparse X_true in place of the sigmoid.  With --sparse DENSITY the design matrix is a seeded scipy.sparse matrix (bag-of-words features,
one-hot encodings) and stays sparse on the device.  On the device the unknown is a matrix (csrc/fh_multi.h, csrc/fh_spmulti.h) and the
loss couples the L columns of a row of A X (losses.SoftmaxLoss, csrc/fh_softmax.h).

    python -m fasta.examples.multiclass_logistic [--backend hip|numpy] [--sparse DENSITY] [--rows M] [--features N] [--classes L] [--group]
"""

import sys

import numpy as np

from .. import DenseMatrixMap, GroupShrink, LinearMap, Shrink, SoftmaxLoss, SparseMatrixMap, fasta
from . import ExampleProblem, cli_backend, test_modes

__all__ = ["MulticlassLogisticProblem"]


class MulticlassLogisticProblem(ExampleProblem):
    def __init__(self, A, y, classes, mu, group=False, X=None, backend="hip"):
        self.A, self.y, self.classes, self.mu, self.group, self.X, self.backend = A, y, classes, mu, group, X, backend

    @property
    def is_sparse(self):
        return not isinstance(self.A, np.ndarray)

    def solve(self, X0, fasta_options=None):
        opts = dict(verbose=False)
        opts.update(fasta_options or {})
        A, L = self.A, self.classes
        M, N = A.shape
        loss = SoftmaxLoss(self.y, classes=L)
        reg = GroupShrink(self.mu) if self.group else Shrink(self.mu)
        if self.backend == "numpy":                 # the tags' host closures over the closure LinearMap, on the generic host loop
            At = A.T.tocsr() if self.is_sparse else A.T
            op = LinearMap(lambda X: A @ X, lambda Y: At @ Y, (N, L), (M, L))
            c = fasta(op, loss.f, loss.gradf, reg.g, reg.prox, X0, **opts)
        else:
            op = self.device_operator(lambda: SparseMatrixMap(A, rhs=L) if self.is_sparse else DenseMatrixMap(A, rhs=L))
            c = fasta(op, op.H, loss.f, loss.gradf, reg.g, reg.prox, X0, backend="hip", **opts)
        return c.solution, c

    def close(self):                                # (A is a host array here, not a device map)
        if self._device_op is not None:
            self._device_op.close()
            self._device_op = None

    @staticmethod
    def construct(M=400, N=200, L=5, K=10, mu=None, sparse=None, group=False, seed=0, backend="hip"):
        """A seeded problem: A is (M, N) -- dense standard normal, or scipy.sparse CSR of density `sparse` -- X_true has K live rows, the
        labels are drawn from the softmax of A X_true.  mu defaults to a tenth of the largest gradient entry (row norm with group) at X = 0."""
        rng = np.random.RandomState(seed)
        if sparse is None:
            A = rng.randn(M, N)
        else:
            from scipy import sparse as sp
            A = sp.random(M, N, density=float(sparse), format="csr", random_state=rng, data_rvs=rng.standard_normal)
            A.sort_indices()
        X = np.zeros((N, L))
        X[rng.permutation(N)[:K]] = 2.0 * rng.randn(K, L)
        Z = A @ X
        P = np.exp(Z - Z.max(axis=1)[:, np.newaxis])
        P /= P.sum(axis=1)[:, np.newaxis]
        u = rng.rand(M)
        y = np.minimum((np.cumsum(P, axis=1) < u[:, np.newaxis]).sum(axis=1), L - 1).astype(np.int64)
        if mu is None:
            G0 = A.T @ SoftmaxLoss(y, classes=L).gradf(np.zeros((M, L)))
            mu = 0.1 * float(np.sqrt((G0 * G0).sum(axis=1)).max() if group else np.abs(G0).max())
        return MulticlassLogisticProblem(A, y, L, mu, group=group, X=X, backend=backend), np.zeros((N, L))


def cli_value(flag, default, kind, argv=None):
    argv = sys.argv[1:] if argv is None else argv
    return kind(argv[argv.index(flag) + 1]) if flag in argv else default


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    backend = cli_backend(argv)
    M, N, L = cli_value("--rows", 400, int, argv), cli_value("--features", 200, int, argv), cli_value("--classes", 5, int, argv)
    sparse, group = cli_value("--sparse", None, float, argv), "--group" in argv
    problem, X0 = MulticlassLogisticProblem.construct(M=M, N=N, L=L, K=max(2, N // 20), sparse=sparse, group=group, backend=backend)
    print("Constructed a {}-class logistic regression on a {} x {} {} design matrix, {} penalty mu = {:.4g}.".format(
        L, M, N, "sparse" if sparse is not None else "dense", "row-wise l2" if group else "l1", problem.mu))
    np.random.seed(1)                               # the Lipschitz probes: the same draws for both backends
    runs = test_modes(problem, X0)
    print("Iterations (adaptive, accelerated, plain): {}, {}, {}".format(*(c.iteration_count for _, c in runs)))
    live = np.abs(runs[0][0]).sum(axis=1) != 0
    print("Features kept by the adaptive solve: {} of {} ({} carry signal).".format(int(live.sum()), N, int((np.abs(problem.X).sum(axis=1) != 0).sum())))
    problem.close()
    return runs


if __name__ == "__main__":
    main()

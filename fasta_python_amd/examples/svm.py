"""The support vector machine min_w .5 ||w||^2 + C h(D w, l) with the hinge loss h, solved through its dual
min_y .5 ||D^T (l * y)||^2 - sum(y) over the box 0 <= y <= C (fasta/examples/svm.py:1-100).  The dual is a box-constrained quadratic
programme: .5 <y, Q y> + <c, y> with Q = (l l^T) * K, c = -1, where K = D D^T is the linear kernel -- the reference's problem (:68-69) -- or
any other symmetric kernel matrix (--kernel rbf).  Q is formed ONCE; on the device one product W = Q y per attempt gives the value and the
gradient (losses.Quadratic, proximal.Box; csrc/fh_quad.h).  w = D^T (l * y) is recovered on the host (:76).

    python -m fasta.examples.svm [--backend hip|numpy] [--kernel linear|rbf] [--points 1000]
"""

import sys

import numpy as np
from numpy import linalg as la

from .. import Box, Quadratic, fasta
from . import ExampleProblem, cli_backend, test_modes
from .sparse_mmv import cli_value

__all__ = ["generate", "kernel_matrix", "SVMProblem"]


def generate(M, N, w):
    """Linearly separable labelled data (:26-43)."""
    permutation = np.random.permutation(M)
    negative = permutation[:M // 2]
    positive = permutation[M // 2:]
    D = 2 * np.random.randn(M, N)
    D[negative] -= w
    D[positive] += w
    L = np.zeros(M)
    L[negative] -= 1.0
    L[positive] += 1.0
    return D, L


def kernel_matrix(D, kernel="linear", gamma=None):
    """K[i, j] = k(D_i, D_j), exactly symmetric: "linear" = D D^T, "rbf" = exp(-gamma ||D_i - D_j||^2) (gamma: 1 / features by default)."""
    if kernel == "linear":
        K = D @ D.T
        return np.triu(K) + np.triu(K, 1).T        # the upper triangle mirrored: symmetric whatever the product routine did
    if kernel != "rbf":
        raise ValueError('kernel must be "linear" or "rbf"')
    gamma = 1.0 / D.shape[1] if gamma is None else gamma
    diff = D[:, None, :] - D[None, :, :]
    return np.exp(-gamma * np.sum(diff * diff, axis=2))


class SVMProblem(ExampleProblem):
    def __init__(self, D, l, C, w=None, kernel="linear", gamma=None, backend="hip"):
        self.D, self.l, self.C, self.w, self.kernel, self.gamma, self.backend = D, l, C, w, kernel, gamma, backend
        self._Q = None

    @property
    def Q(self):
        if self._Q is None:
            self._Q = np.outer(self.l, self.l) * kernel_matrix(self.D, self.kernel, self.gamma)
        return self._Q

    def solve(self, y0, fasta_options=None):
        opts = dict(verbose=False)
        opts.update(fasta_options or {})
        D, l, C = self.D, self.l, self.C
        if self.backend == "numpy" and self.kernel == "linear":        # the reference's closures (:68-71)
            f = lambda y: .5 * la.norm((D.T @ (l * y)).ravel()) ** 2 - np.sum(y)
            gradf = lambda y: l * (D @ (D.T @ (l * y))) - 1
            g = lambda y: 0
            proxg = lambda y, t: np.minimum(np.maximum(y, 0), C)
            c = fasta(None, None, f, gradf, g, proxg, y0, **opts)
        else:
            loss, reg = Quadratic(self.Q, -np.ones(len(l))), Box(0.0, C)
            c = fasta(None, None, loss.f, loss.gradf, reg.g, reg.prox, y0, backend=self.backend, **opts)
        return D.T @ (l * c.solution), c

    @staticmethod
    def construct(M=1000, N=15, C=0.01, separation=1.0, kernel="linear", gamma=None, seed=None, backend="hip"):
        """Random linearly separable training data in the reference's RNG order (:90-100)."""
        if seed is not None:
            np.random.seed(seed)
        w = np.random.randn(N)
        w /= la.norm(w)
        w *= separation
        D, l = generate(M, N, w)
        return SVMProblem(D, l, C, w=w, kernel=kernel, gamma=gamma, backend=backend), np.zeros(M)

    def accuracy(self, solution, M_test=300):
        """Share of freshly generated points the hyperplane `solution` classifies correctly (:109-112)."""
        D_test, l_test = generate(M_test, solution.shape[0], self.w)
        return np.sum(np.sign(D_test @ solution) == l_test) / M_test


if __name__ == "__main__":
    backend, kernel, M = cli_backend(), cli_value("--kernel", "linear", str), cli_value("--points", 1000, int)
    problem, y0 = SVMProblem.construct(M=M, kernel=kernel, backend=backend)
    print("Constructed support vector machine problem ({} kernel).".format(kernel))
    np.random.seed(1)                               # the Lipschitz probes: the same draws for both backends
    results = test_modes(problem, y0)
    print("Iterations (adaptive, accelerated, plain): {}, {}, {}".format(*(c.iteration_count for _, c in results)))
    if kernel == "linear":
        print("Accuracy of the adaptive run's hyperplane on fresh points: {:.1f}%".format(100 * problem.accuracy(results[0][0])))
    problem.close()

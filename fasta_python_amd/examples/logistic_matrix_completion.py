"""1-bit (logistic) matrix completion: min_X mu*||X||_* + sum log(1 + e^X) - (B == 1)*X, the nuclear norm pulling X towards low rank.
Recipe: fasta/examples/logistic_matrix_completion.py:43-48 (closures, `fasta(None, None, f, gradf, g, proxg, X0)`), :62-78 (construct: the same
draws from the global RNG in the same order).

    python -m fasta.examples.logistic_matrix_completion [--backend hip|numpy] [--rows M] [--cols N] [--rank K] [--mu MU]

backend "hip" runs on the device through the identity operator (csrc/fh_nuclear.h): the singular-value thresholding is a block one-sided
Jacobi decomposition there, min(M, N) <= 1024; "numpy" the reference's closures on the host loop.  Plots are not ported."""

import sys

import numpy as np
from numpy import linalg as la

from .. import LogisticLoss, NuclearShrink, fasta, proximal
from . import ExampleProblem, cli_backend, test_modes

__all__ = ["LogisticMatrixCompletionProblem"]


class LogisticMatrixCompletionProblem(ExampleProblem):
    def __init__(self, B, mu, X=None, backend="hip", solver_seed=None):
        """B: the +-1 observations; X: the matrix behind them, if known.  solver_seed: the global RNG is seeded with it before every solve (the
        solver's two step-size probes draw from it), so that the three modes of one command line are each a reproducible run."""
        self.B, self.mu, self.X, self.backend, self.solver_seed = B, mu, X, backend, solver_seed

    def solve(self, X0, fasta_options=None):
        opts = dict(verbose=False)
        opts.update(fasta_options or {})
        if self.solver_seed is not None:
            np.random.seed(self.solver_seed)
        if self.backend == "numpy":                 # the reference's closures (:43-46), 7-argument call
            f = lambda Z: np.sum(np.log(1 + np.exp(Z)) - (self.B == 1) * Z)
            gradf = lambda Z: -self.B / (1 + np.exp(self.B * Z))
            g = lambda X: self.mu * la.norm(np.diag(la.svd(X)[1]), 1)
            proxg = lambda X, t: proximal.project_Lnuc_ball(X, t * self.mu)
            c = fasta(None, None, f, gradf, g, proxg, X0, **opts)
        else:
            loss, reg = LogisticLoss(self.B), NuclearShrink(self.mu)
            c = fasta(None, None, loss.f, loss.gradf, reg.g, reg.prox, X0, backend="hip", **opts)
        return c.solution, c

    @staticmethod
    def construct(M=200, N=1000, K=10, mu=20.0, seed=None, backend="hip"):
        if seed is not None:
            np.random.seed(seed)
        X = np.random.randn(M, N) * 10.0
        U, s, V = la.svd(X)
        S = np.zeros((M, N))                                    # rank K: the K leading singular values only
        S[:K, :K] = np.diag(s[:K])
        X = U @ S @ V
        P = 1 / (1 + np.exp(-X))
        B = 2.0 * (np.random.rand(M, N) < P) - 1
        return LogisticMatrixCompletionProblem(B, mu, X=X, backend=backend), np.zeros((M, N))


def _cli_value(argv, flag, cast, default):
    if flag not in argv:
        return default
    at = argv.index(flag)
    if at + 1 >= len(argv):
        raise SystemExit(f"{flag} takes a value")
    return cast(argv[at + 1])


def main(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    M = _cli_value(argv, "--rows", int, 200)
    N = _cli_value(argv, "--cols", int, 1000)
    K = _cli_value(argv, "--rank", int, 10)
    mu = _cli_value(argv, "--mu", float, 20.0)
    problem, X0 = LogisticMatrixCompletionProblem.construct(M=M, N=N, K=K, mu=mu, seed=7, backend=cli_backend(argv))
    problem.solver_seed = 107
    print("Constructed 1-bit logistic matrix completion problem.")
    results = test_modes(problem, X0)
    problem.close()
    return results


if __name__ == "__main__":
    main()

"""Matrix completion from a SUBSET of the entries: recover a low-rank (M, N) matrix from the entries a 0 / 1 mask W observes,

    min_X  mu*||X||_* + .5 * sum W * (X - B)^2                 (--mu, the default)
    min_X  .5 * sum W * (X - B)^2   subject to ||X||_* <= R    (--radius R)

with B the noisy observed values, or -- with --one-bit -- their +-1 signs under the logistic loss, sum W * (log(1 + e^X) - (B == 1)*X).

    python -m fasta.examples.matrix_completion [--backend hip|numpy] [--rows M] [--cols N] [--rank K] [--observed FRACTION] [--noise S]
                                               [--mu MU | --radius R] [--one-bit]

backend "hip" runs on the device through the identity operator with observation weights (csrc/fh_nuclear.h: fh_set_loss_weights, and the block
one-sided Jacobi decomposition behind NuclearShrink / NuclearBall, min(M, N) <= 1024); "numpy" runs the same tags' host closures on the generic host
loop, a LAPACK SVD per iteration.  Prints, per mode: iterations, objective, rank kept and the relative error on the UNOBSERVED entries."""

import sys

import numpy as np
from numpy import linalg as la

from .. import LeastSquares, LogisticLoss, NuclearBall, NuclearShrink, fasta
from . import ExampleProblem, cli_backend, test_modes

__all__ = ["MatrixCompletionProblem"]


class MatrixCompletionProblem(ExampleProblem):
    def __init__(self, B, W, mu=None, radius=None, one_bit=False, X=None, backend="hip", solver_seed=None):
        """B: the observations (values, or +-1 with one_bit); W: the 0 / 1 mask of the observed entries; exactly one of mu (nuclear-norm penalty) and
        radius (nuclear-norm ball); X: the matrix behind B, if known.  solver_seed: as in LogisticMatrixCompletionProblem."""
        if (mu is None) == (radius is None):
            raise ValueError("MatrixCompletionProblem takes exactly one of mu (penalty) and radius (constraint)")
        self.B, self.W, self.mu, self.radius, self.one_bit, self.X = B, W, mu, radius, one_bit, X
        self.backend, self.solver_seed = backend, solver_seed

    def tags(self):
        loss = (LogisticLoss if self.one_bit else LeastSquares)(self.B, weights=self.W)
        reg = NuclearShrink(self.mu) if self.radius is None else NuclearBall(self.radius)
        return loss, reg

    def solve(self, X0, fasta_options=None):
        opts = dict(verbose=False)
        opts.update(fasta_options or {})
        if self.solver_seed is not None:
            np.random.seed(self.solver_seed)
        loss, reg = self.tags()
        c = fasta(None, None, loss.f, loss.gradf, reg.g, reg.prox, X0, backend=self.backend, **opts)
        return c.solution, c

    def unobserved_error(self, solution):
        """||(1 - W) * (solution - X)||_F / ||(1 - W) * X||_F: the entries the solver never saw.  (With one_bit the scale of X is not identified
        by its signs; the figure is then of a least-squares rescaling of the solution.)"""
        hidden = self.W == 0
        S = solution
        if self.one_bit:
            S = S * (np.sum(S * self.X) / max(np.sum(S * S), 1e-300))
        return la.norm((S - self.X)[hidden]) / max(la.norm(self.X[hidden]), 1e-300)

    @staticmethod
    def construct(M=200, N=1000, K=5, observed=0.3, noise=0.3, mu=None, radius=None, one_bit=False, seed=None, backend="hip"):
        if seed is not None:
            np.random.seed(seed)
        X = np.random.randn(M, K) @ np.random.randn(K, N)          # rank K, entries of variance K
        W = (np.random.rand(M, N) < observed).astype(np.float64)
        if one_bit:
            B = 2.0 * (np.random.rand(M, N) < 1 / (1 + np.exp(-X))) - 1
        else:
            B = (X + noise * np.random.randn(M, N)) * W            # (unobserved entries hold nothing of X)
        if mu is None and radius is None:
            # a fraction of the spectral norm of what the MASK does to the data: entries of root mean square `scale` kept with probability
            # `observed` differ from their mean by a random matrix of norm ~ scale * sqrt(observed * (1 - observed)) * (sqrt(M) + sqrt(N));
            # 0.4 of it leaves rank K at the default size and a fifth of the unobserved entries' norm as the shrinkage's bias
            scale = 1.0 if one_bit else float(np.sqrt(np.mean(B[W != 0] ** 2))) if W.any() else 1.0
            mu = 0.4 * scale * np.sqrt(observed * (1 - observed)) * (np.sqrt(M) + np.sqrt(N))
        return MatrixCompletionProblem(B, W, mu=mu, radius=radius, one_bit=one_bit, X=X, backend=backend), np.zeros((M, N))


def _cli_value(argv, flag, cast, default):
    if flag not in argv:
        return default
    at = argv.index(flag)
    if at + 1 >= len(argv):
        raise SystemExit(f"{flag} takes a value")
    return cast(argv[at + 1])


def main(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    if "--mu" in argv and "--radius" in argv:
        raise SystemExit("--mu (penalty) and --radius (constraint) exclude each other")
    problem, X0 = MatrixCompletionProblem.construct(
        M=_cli_value(argv, "--rows", int, 200), N=_cli_value(argv, "--cols", int, 1000), K=_cli_value(argv, "--rank", int, 5),
        observed=_cli_value(argv, "--observed", float, 0.3), noise=_cli_value(argv, "--noise", float, 0.3),
        mu=_cli_value(argv, "--mu", float, None), radius=_cli_value(argv, "--radius", float, None), one_bit="--one-bit" in argv,
        seed=11, backend=cli_backend(argv))
    problem.solver_seed = 111
    what = f"radius = {problem.radius:g}" if problem.radius is not None else f"mu = {problem.mu:g}"
    print(f"Constructed {'1-bit ' if problem.one_bit else ''}matrix completion problem: {problem.B.shape[0]} x {problem.B.shape[1]}, "
          f"{int(problem.W.sum())} of {problem.W.size} entries observed, {what}.")
    results = test_modes(problem, X0)
    for label, (solution, c) in zip(("adaptive", "accelerated", "plain"), results):
        s = la.svd(solution, compute_uv=False)
        rank = int(np.sum(s > 1e-3 * max(s[0], 1e-300)))
        print(f"{label:12s} iterations {c.iteration_count:4d}  objective {c.objectives[c.iteration_count]:.6e}  rank kept {rank:3d}  "
              f"relative error on the unobserved entries {problem.unobserved_error(solution):.3e}")
    problem.close()
    return results


if __name__ == "__main__":
    main()

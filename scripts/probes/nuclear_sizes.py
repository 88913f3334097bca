"""Times of the nuclear-norm prox (FH_PROX_NUCLEAR, csrc/fh_nuclear.h) and of the example's three modes -> profiles/nuclear_sizes.txt.

    python scripts/probes/nuclear_sizes.py [--out FILE] [--quick]

Per shape and block size: one forward launch (x0 = a seeded low-rank-plus-noise matrix, g0 = 0, tau * mu = a third of its largest singular value)
timed by the host clock around a call that ends in a synchronisation, after one warm-up call; REPS repetitions, median and range; the sweeps,
steps and rotations of the decomposition (fh_nuclear_info); the time the library books under FH_K_LEVEL; and LAPACK's thin SVD (with vectors) of the
same matrix on this box's CPU for scale.  Then examples/logistic_matrix_completion.py at its own size, wall clock per iteration of each mode with
backend="hip" against the same call with backend="numpy" on the same box (seeded alike; the iteration counts are printed beside the times)."""
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import fasta_python_amd as fa                                    # noqa: E402
from fasta_python_amd import hip                                 # noqa: E402
from fasta_python_amd.examples import logistic_matrix_completion as ex      # noqa: E402

SHAPES = ((200, 1000), (1000, 200), (512, 4096), (1024, 1024))
REPS = 5


def matrix(M, N, seed=3, rank=10):
    rng = np.random.RandomState(seed)
    return rng.randn(M, rank) @ rng.randn(rank, N) + 0.5 * rng.randn(M, N)


def prox_times(M, N, Bk, reps, say):
    X = matrix(M, N)
    t0 = time.perf_counter()
    smax = float(np.linalg.svd(X, full_matrices=False)[1][0])
    lapack = time.perf_counter() - t0
    op = fa.IdentityMap((M, N), tuning={hip.TUNE_NUC_BLOCK_ROWS: Bk})
    try:
        c = op.ctx
        c.set_loss_lsq(np.zeros(M * N))
        c.set_prox_nuclear(smax / 3.0, False)
        c.set_vector(hip.VEC_X0, X)
        c.set_vector(hip.VEC_G0, np.zeros(M * N))
        c.fwd(1.0)                                               # warm-up: code objects, workspace
        c.timing_enable(True)
        c.timing_reset()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            c.fwd(1.0)
            ts.append((time.perf_counter() - t0) * 1e3)
        level_ms, level_n = c.timing_get(hip.K_LEVEL)
        info, sh = c.nuclear_info(), c.nuclear_shape()
        say(f"{M:5d} x {N:5d}  Bk {Bk}  prox {statistics.median(ts):9.3f} ms (min {min(ts):.3f}, max {max(ts):.3f}, {reps} runs)  "
            f"FH_K_LEVEL {level_ms / max(level_n, 1):9.3f} ms  sweeps {info.sweeps:2d}  steps {info.steps:6d}  rotations {info.rotations:9d}  "
            f"rank kept {info.rank:4d}  workgroups/step {sh.wgs_per_step:4d}  buffer {sh.bytes / 2 ** 20:7.1f} MiB  | LAPACK thin SVD on this CPU {lapack * 1e3:8.1f} ms")
    finally:
        op.close()


def example_times(say, M=200, N=1000):
    rows = {}
    for backend in ("hip", "numpy"):
        problem, X0 = ex.LogisticMatrixCompletionProblem.construct(M=M, N=N, seed=7, backend=backend)
        problem.solver_seed = 107
        for mode, opts in (("adaptive", dict(adaptive=True, accelerate=False)), ("accelerated", dict(adaptive=False, accelerate=True)),
                           ("plain", dict(adaptive=False, accelerate=False))):
            o = dict(opts, tolerance=1e-5, evaluate_objective=True, verbose=False)
            if backend == "hip":
                problem.solve(X0, dict(o, max_iters=2))          # warm-up
            t0 = time.perf_counter()
            _, conv = problem.solve(X0, o)
            dt = time.perf_counter() - t0
            rows[(backend, mode)] = (dt, conv.iteration_count, conv.backtracks, float(conv.objectives[conv.iteration_count]))
            say(f"example {M} x {N}  {backend:5s} {mode:11s} {conv.iteration_count:4d} iterations, {conv.backtracks:3d} backtracks, {dt:8.3f} s, "
                f"{dt / max(conv.iteration_count, 1) * 1e3:9.2f} ms per iteration, objective {rows[(backend, mode)][3]:.6e}")
        problem.close()
    for mode in ("adaptive", "accelerated", "plain"):
        h, n = rows[("hip", mode)], rows[("numpy", mode)]
        say(f"example {M} x {N}  {mode:11s} hip / numpy per iteration: {h[0] / max(h[1], 1) / (n[0] / max(n[1], 1)):6.2f}")


def main(argv):
    out = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(ROOT, "profiles", "nuclear_sizes.txt")
    quick = "--quick" in argv
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        def say(line):
            print(line, flush=True)
            fh.write(line + "\n")
            fh.flush()
        say(f"# scripts/probes/nuclear_sizes.py on {hip.device_cus(0)} CUs; times in ms: median (min, max) of {REPS} runs behind one warm-up run")
        for M, N in (((24, 60),) if quick else SHAPES):
            for Bk in (8, 1):
                prox_times(M, N, Bk, 2 if quick else REPS, say)
        example_times(say, *((24, 60) if quick else (200, 1000)))


if __name__ == "__main__":
    main(sys.argv[1:])

"""Times of the weighted identity kernels and of the nuclear-norm ball (csrc/fh_nuclear.h) -> profiles/completion_sizes.txt.

    python scripts/probes/completion_sizes.py [--out FILE] [--quick] [--parent-lib PATH]

1. k_id_fwd / k_id_adj UNWEIGHTED at 4096 x 4096 and 64 x 64 on this build and -- with --parent-lib, a libfasta_hip.so built from the parent
   commit -- on that one: one fresh process per (library, round), the two libraries alternating, ROUNDS rounds; in a process LAUNCHES forward
   and adjoint launches behind WARMUP warm-up pairs, timed by the library's own device events (fh_timing_get: FH_K_FWD, FH_K_ADJ), mean per
   launch; reported: the median over the rounds with their range.  The parent's own range is the margin a "no change" claim has.
2. The WEIGHTED pair against the unweighted one, same procedure on this build; achieved TB/s on ALGORITHMIC bytes (forward: x0, g0, b read, xhat,
   xprox, z written = 48 B per entry; adjoint: x0, xprox, xhat, b read, g1 written = 40 B; the weighted form reads 8 B more in each).
3. The ball prox against the shrink prox at 200 x 1000 and 1024 x 1024: a forward launch on a seeded low-rank-plus-noise matrix, the radius set to
   the nuclear norm the threshold leaves, so that both keep the same values; host clock around a call that ends in a synchronisation, and FH_K_LEVEL.
   The level launch's own time is taken where the decomposition is cheapest and repeatable: a 1024 x 1024 DIAGONAL matrix (one sweep, no rotation),
   ball minus shrink, alternating, median of the differences.
4. examples/matrix_completion.py at 200 x 1000, 30 % observed, three modes: wall clock per iteration, backend="hip" against backend="numpy"."""
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

ROUNDS, LAUNCHES, WARMUP, REPS = 5, 200, 10, 5
FWD_BYTES, ADJ_BYTES = 48, 40


def worker(M, N, weighted, launches, warmup):
    """In a fresh process (the library is $FASTA_HIP_LIB or the package's own): mean ms per K-fwd and per K-adj launch, as JSON on stdout."""
    import ctypes
    import fasta_python_amd as fa
    from fasta_python_amd import hip
    if not hasattr(ctypes.CDLL(hip.LIB_PATH), "fh_set_loss_weights"):      # a library of the parent commit: it serves the unweighted form alone
        assert not weighted
        hip.SIGNATURES.pop("fh_set_loss_weights")
    rng = np.random.RandomState(1)
    op = fa.IdentityMap((M, N))
    try:
        c = op.ctx
        c.set_loss_lsq(rng.randn(M * N))
        if weighted:
            c.set_loss_weights((rng.rand(M * N) < 0.3).astype(np.float64))
        c.set_prox(hip.PROX_SHRINK, 0.1)
        c.set_vector(hip.VEC_X0, rng.randn(M * N))
        c.init()
        for _ in range(warmup):
            c.fwd(0.25)
            c.adj(0.25)
        c.timing_enable(True)
        c.timing_reset()
        for _ in range(launches):
            c.fwd(0.25)
            c.adj(0.25)
        (f_ms, f_n), (a_ms, a_n) = c.timing_get(hip.K_FWD), c.timing_get(hip.K_ADJ)
        print(json.dumps(dict(fwd=f_ms / f_n, adj=a_ms / a_n, launches=[f_n, a_n])))
    finally:
        op.close()


def run_worker(lib, M, N, weighted, launches, warmup):
    env = dict(os.environ)
    env.pop("FASTA_HIP_LIB", None)
    if lib:
        env["FASTA_HIP_LIB"] = lib
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", str(M), str(N), str(int(weighted)), str(launches), str(warmup)],
                         env=env, check=True, capture_output=True, text=True, timeout=300).stdout
    return json.loads(out.strip().splitlines()[-1])


def spread(values):
    return f"{statistics.median(values) * 1e3:9.2f} us (min {min(values) * 1e3:.2f}, max {max(values) * 1e3:.2f})"


def kernel_section(say, shapes, parent, rounds, launches, warmup):
    for M, N in shapes:
        forms = [("this build, unweighted", None, False)] + ([("parent commit, unweighted", parent, False)] if parent else []) + [("this build, weighted", None, True)]
        got = {name: dict(fwd=[], adj=[]) for name, _, _ in forms}
        for _ in range(rounds):                                  # the forms alternate within a round
            for name, lib, weighted in forms:
                r = run_worker(lib, M, N, weighted, launches, warmup)
                got[name]["fwd"].append(r["fwd"])
                got[name]["adj"].append(r["adj"])
        for name, _, weighted in forms:
            for k, nbytes in (("fwd", FWD_BYTES), ("adj", ADJ_BYTES)):
                med = statistics.median(got[name][k])
                tbs = (nbytes + (8 if weighted else 0)) * M * N / (med * 1e-3) / 1e12
                say(f"{M:5d} x {N:5d}  k_id_{k}  {name:26s} {spread(got[name][k])}  {rounds} rounds x {launches} launches  {tbs:6.3f} TB/s on algorithmic bytes")
        for k in ("fwd", "adj"):
            u, w = statistics.median(got["this build, unweighted"][k]), statistics.median(got["this build, weighted"][k])
            say(f"{M:5d} x {N:5d}  k_id_{k}  weighted / unweighted time {w / u:6.3f}")
            if parent:
                p = got["parent commit, unweighted"][k]
                say(f"{M:5d} x {N:5d}  k_id_{k}  this build / parent {u / statistics.median(p):6.3f}; the parent's own rounds span {min(p) / statistics.median(p):.3f} .. {max(p) / statistics.median(p):.3f} of its median")


def matrix(M, N, seed=3, rank=10):
    rng = np.random.RandomState(seed)
    return rng.randn(M, rank) @ rng.randn(rank, N) + 0.5 * rng.randn(M, N)


def prox_pair(say, X, label, reps):
    """Forward launches of the shrink prox and of the ball prox that keeps the same values, alternating; returns the per-repetition differences."""
    import fasta_python_amd as fa
    from fasta_python_amd import hip
    M, N = X.shape
    s = np.linalg.svd(X, compute_uv=False)
    thr = float(s[0]) / 3.0
    radius = float(np.sum(np.maximum(s - thr, 0)))
    op = fa.IdentityMap((M, N))
    try:
        c = op.ctx
        c.set_loss_lsq(np.zeros(M * N))
        c.set_vector(hip.VEC_X0, X)
        c.set_vector(hip.VEC_G0, np.zeros(M * N))
        times = {"shrink": [], "ball": []}
        level = {"shrink": [], "ball": []}
        info = {}

        def one(kind):
            if kind == "shrink":
                c.set_prox_nuclear(thr, False)
            else:
                c.set_prox(hip.PROX_NUCBALL, radius)
            c.timing_enable(True)
            c.timing_reset()
            t0 = time.perf_counter()
            sc = c.fwd(1.0)
            dt = (time.perf_counter() - t0) * 1e3
            return dt, c.timing_get(hip.K_LEVEL)[0], c.nuclear_info(), sc

        for kind in ("shrink", "ball"):
            one(kind)                                            # warm-up: code objects, workspace
        for _ in range(reps):
            for kind in ("shrink", "ball"):
                dt, lv, info[kind], sc = one(kind)
                times[kind].append(dt)
                level[kind].append(lv)
        for kind in ("shrink", "ball"):
            i = info[kind]
            say(f"{label:24s} {kind:6s} prox {statistics.median(times[kind]):9.3f} ms (min {min(times[kind]):.3f}, max {max(times[kind]):.3f}, {reps} runs)  "
                f"FH_K_LEVEL {statistics.median(level[kind]):9.3f} ms  sweeps {i.sweeps:2d}  steps {i.steps:6d}  rotations {i.rotations:9d}  rank kept {i.rank:4d}")
        return [b - a for a, b in zip(level["shrink"], level["ball"])]
    finally:
        op.close()


def example_times(say, M, N):
    from fasta_python_amd.examples import matrix_completion as ex
    rows = {}
    for backend in ("hip", "numpy"):
        problem, X0 = ex.MatrixCompletionProblem.construct(M=M, N=N, observed=0.3, seed=11, backend=backend)
        problem.solver_seed = 111
        for mode, opts in (("adaptive", dict(adaptive=True, accelerate=False)), ("accelerated", dict(adaptive=False, accelerate=True)),
                           ("plain", dict(adaptive=False, accelerate=False))):
            o = dict(opts, tolerance=1e-5, evaluate_objective=True, verbose=False)
            if backend == "hip":
                problem.solve(X0, dict(o, max_iters=2))          # warm-up
            t0 = time.perf_counter()
            solution, conv = problem.solve(X0, o)
            dt = time.perf_counter() - t0
            rows[(backend, mode)] = (dt, conv.iteration_count)
            say(f"example {M} x {N}, 30 % observed  {backend:5s} {mode:11s} {conv.iteration_count:4d} iterations, {conv.backtracks:3d} backtracks, {dt:8.3f} s, "
                f"{dt / max(conv.iteration_count, 1) * 1e3:9.2f} ms per iteration, objective {float(conv.objectives[conv.iteration_count]):.6e}, "
                f"error on the unobserved entries {problem.unobserved_error(solution):.3e}")
        problem.close()
    for mode in ("adaptive", "accelerated", "plain"):
        h, n = rows[("hip", mode)], rows[("numpy", mode)]
        say(f"example {M} x {N}  {mode:11s} hip / numpy per iteration: {h[0] / max(h[1], 1) / (n[0] / max(n[1], 1)):6.2f}")


def main(argv):
    if argv and argv[0] == "--worker":
        M, N, weighted, launches, warmup = (int(a) for a in argv[1:6])
        return worker(M, N, bool(weighted), launches, warmup)
    from fasta_python_amd import hip
    out = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(ROOT, "profiles", "completion_sizes.txt")
    parent = os.path.abspath(argv[argv.index("--parent-lib") + 1]) if "--parent-lib" in argv else None
    if parent and not os.path.exists(parent):
        raise SystemExit(f"--parent-lib {parent}: no such file")
    quick = "--quick" in argv
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        def say(line):
            print(line, flush=True)
            fh.write(line + "\n")
            fh.flush()
        say(f"# scripts/probes/completion_sizes.py on {hip.device_cus(0)} CUs; kernel times: device events, mean per launch in a fresh process, median (min, max) over the rounds")
        say("# parent commit: " + ("a library built from it, alternating with this build" if parent else "not measured (no --parent-lib)"))
        kernel_section(say, ((64, 64),) if quick else ((4096, 4096), (64, 64)), parent, 2 if quick else ROUNDS, 20 if quick else LAUNCHES, 2 if quick else WARMUP)
        reps = 2 if quick else REPS
        for M, N in (((24, 60),) if quick else ((200, 1000), (1024, 1024))):
            prox_pair(say, matrix(M, N), f"{M} x {N} low rank + noise", reps)
        n = 64 if quick else 1024
        diffs = prox_pair(say, np.diag(np.linspace(1.0, 2.0, n)), f"{n} x {n} diagonal", 3 if quick else 15)
        say(f"{n} x {n} diagonal: FH_K_LEVEL of the ball minus that of the shrink (the level launch k_nuc_ball, p = {n}): median {statistics.median(diffs) * 1e3:8.1f} us "
            f"(min {min(diffs) * 1e3:.1f}, max {max(diffs) * 1e3:.1f}, {len(diffs)} alternating pairs)")
        example_times(say, *((24, 60) if quick else (200, 1000)))


if __name__ == "__main__":
    main(sys.argv[1:])

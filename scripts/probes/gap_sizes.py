"""What does one duality-gap certificate (fh_dual_gap, csrc/fh_gap.h) cost next to one iteration of the same context, and what does the stop rule
stopping.DualityGap(every=10) add to a solve?  One MI355X, one process, data from seeded generators.

    python scripts/probes/gap_sizes.py [--out profiles/gap_sizes.txt] [--calls 200] [--jobs dense4096,dense65536,csr,dct,small]

Per job, on ONE context at a committed state a few plain iterations into a LASSO solve:
  certificate  wall clock around HipContext.dual_gap() -- the call ends in a stream synchronisation and the copy of its 8 doubles -- median (min, max)
               of `--calls` calls after 10 warm-up calls; the bytes it moves, (2 n + 2 m) L 8 (one more m-side read for the logistic loss), and the
               rate that is of the median;
  iteration    wall clock of K iterations of the library loop on the same context over K, warm, median of 3 (plain FBS, no stop);
  rule         the same solve of N iterations under stop_rule=DualityGap(0.0, every=10) (the gap is checked N / 10 + 1 times and never met) and
               under stop_rule=hybrid_residual at tolerance 0 (never met), alternating, 5 times each: median wall clock per iteration of either
               and their difference.
Jobs: dense 4096^2 and 65536^2 (generated in HBM; the second also with the logistic loss at 4096^2), CSR 20000 x 40000 at the density of
examples/sparse_design.py (0.01), DCTMap(2^20), and the 64 x 128 fixture size, where a launch latency is all there is."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def make(job, fa, synthetic):
    """(label, operator, loss, L)"""
    rng = np.random.RandomState(0)
    if job.startswith("dense"):
        n = int(job[5:])
        op = fa.DenseMatrixMap.synthetic(n, n, seed=0, scale=synthetic.lasso_scale(n, n))
        b = synthetic.lasso_observation(op, synthetic.sparse_signal(n, seed=1), seed_noise=2, sigma=0.01)
        return f"dense {n} x {n} (generated)", op, b
    if job == "csr":
        from scipy import sparse as sp
        S = sp.random(20000, 40000, density=0.01, format="csr", random_state=rng, data_rvs=rng.standard_normal)
        x = np.zeros(40000)
        x[rng.permutation(40000)[:200]] = rng.randn(200)
        return f"CSR 20000 x 40000, density 0.01 ({S.nnz} entries)", fa.SparseMatrixMap(S), S @ x + 0.01 * rng.randn(20000)
    if job == "dct":
        N = 1 << 20
        mask = (rng.rand(N) < 0.5).astype(np.float64)
        op = fa.DCTMap(N, mask=mask)
        x = np.zeros(N)
        x[rng.permutation(N)[:1000]] = rng.randn(1000)
        return "DCTMap(2^20), half the coefficients kept", op, np.asarray(op(x)) + 0.01 * rng.randn(N)
    if job == "small":
        A = rng.randn(64, 128) / 8.0
        x = np.zeros(128)
        x[:5] = 1.0
        return "dense 64 x 128", fa.DenseMatrixMap(A), A @ x + 0.01 * rng.randn(64)
    raise SystemExit(f"unknown job {job}")


def stats(v):
    v = np.asarray(v) * 1e3
    return f"{np.median(v):.4f} ms  (min {v.min():.4f}, max {v.max():.4f})"


def solve(fa, op, loss, reg, x0, iters, rule, tolerance=0.0):
    np.random.seed(1)
    solver = fa.FBSolver(op, loss, reg, x0, verbose=False, adaptive=False, max_iters=iters, tolerance=tolerance, stop_rule=rule).setup()
    t0 = time.perf_counter()
    solver.run()
    dt = time.perf_counter() - t0
    assert solver.i == iters, (solver.i, iters)
    return dt / iters


def measure(job, calls, fa, synthetic, out):
    from fasta_python_amd import stopping
    label, op, b = make(job, fa, synthetic)
    try:
        m, n = b.shape[0], op.Vshape[0]
        big = job == "dense65536"          # (a 32 GiB matrix: 5 ms per iteration; the rule is timed on the others)
        K = 20 if big else 50
        for logistic in ((False, True) if job == "dense4096" else (False,)):
            loss = fa.LogisticLoss(np.where(b > np.median(b), 1.0, -1.0)) if logistic else fa.LeastSquares(b)
            x0 = np.zeros(n)
            c = op.ctx
            loss.bind(c)
            c.set_prox(1, 1.0)
            c.set_vector(0, x0)
            c.init()
            reg = fa.Shrink(0.1 * c.dual_gap().dual_norm)
            np.random.seed(1)
            solver = fa.FBSolver(op, loss, reg, x0, verbose=False, adaptive=False, max_iters=10 ** 4, tolerance=0.0, stop_rule=stopping.residual).setup()
            solver.advance(5)
            for _ in range(10):
                cert = c.dual_gap()
            t = []
            for _ in range(calls):
                t0 = time.perf_counter()
                c.dual_gap()
                t.append(time.perf_counter() - t0)
            it = []
            for _ in range(3):
                t0 = time.perf_counter()
                solver.advance(K)
                c.sync()
                it.append((time.perf_counter() - t0) / K)
            nbytes = (2 * n + 2 * m + (m if logistic else 0)) * 8
            out(f"{label}, {'logistic' if logistic else 'least squares'}, Shrink: {'three' if logistic else 'two'} launches, {nbytes} bytes")
            out(f"  certificate  {stats(t)}   ->  {nbytes / np.median(t) / 1e9:.1f} GB/s of its bytes; relative gap there {cert.relative:.3e}")
            out(f"  iteration    {stats(it)}   (library loop, plain FBS, {K} iterations per timing)   certificate / iteration = {np.median(t) / np.median(it):.3f}")
            if not big:
                N = 200
                g, h = [], []
                for _ in range(5):
                    g.append(solve(fa, op, loss, reg, x0, N, fa.DualityGap(0.0, every=10)))
                    h.append(solve(fa, op, loss, reg, x0, N, stopping.hybrid_residual))
                out(f"  rule         DualityGap(every=10) {stats(g)} per iteration; hybrid_residual {stats(h)}; difference of the medians "
                    f"{(np.median(g) - np.median(h)) * 1e3:+.4f} ms per iteration ({N} iterations, 21 certificates)")
            out("")
    finally:
        op.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--jobs", default="small,dense4096,csr,dct,dense65536")
    a = ap.parse_args()
    import fasta_python_amd as fa
    from fasta_python_amd import synthetic
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)
    out("duality-gap certificate (csrc/fh_gap.h), one MI355X, one process; wall clock around calls that end in a stream synchronisation")
    out(f"certificate: median (min, max) of {a.calls} calls after 10 warm-up calls; iteration: median of 3 timings; rule: 5 alternating solves each")
    out("")
    for job in a.jobs.split(","):
        measure(job, a.calls, fa, synthetic, out)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

"""What do the pieces of gap-safe screening cost (csrc/fh_screen.h), and what does a screened path gain or lose?  One MI355X, one process, data from
seeded generators.

    python scripts/probes/screen_sizes.py [--out profiles/screen_sizes.txt] [--repeats 7] [--path-repeats 3] [--jobs norms,gather,paths]

norms   fh_column_norms on a generated dense matrix of 4096 x 65536, 16384^2 and 65536^2: HIP-event time of its two launches (FH_K_AUX), `--repeats`
        fresh runs (fh_set_rhs(0) drops the kept norms in between), median (min, max), next to fh_stream_read_ms over the same buffer in the same
        process (median of 3 calls of 5 passes); ratio = stream-read time / norms time.
gather  fh_gather_columns out of 4096 x 65536 keeping every 2nd, 8th and 64th column: HIP-event time of the launch on the destination, `--repeats`
        runs, next to the stream-read time of the source plus that of the destination (the destination's read rate standing in for its write).
paths   fasta.path, 20 points, ratio 1e-2, gap_tolerance 1e-6, adaptive FBS, on generated dense 4096 x 65536 and 2048 x 131072 and on the CSR
        operator of examples/sparse_design.py (2000 x 4000, density 0.01): screen=False and screen=True alternating, `--path-repeats` times each, in one process:
        wall clock (median, min, max), total iterations, launches that read the full-width A (forward, adjoint and one-pass launches of the full
        context), columns kept per point.  The parent commit's path is screen=False here: the same code (tests/test_gpu_screen.py holds it to a
        plain loop of solves, bit for bit)."""
import argparse
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def stats(v, unit="ms"):
    v = np.asarray(v, dtype=float)
    return f"{np.median(v):.4f} {unit} (min {v.min():.4f}, max {v.max():.4f})"


def read_ms(c):
    t = [c.stream_read_ms(5) for _ in range(3)]
    return float(np.median([a for a, _ in t])), t[0][1]


def norms(repeats, fa, hip, synthetic, out):
    for m, n in ((4096, 65536), (16384, 16384), (65536, 65536)):
        with hip.HipContext(0) as c:
            c.generate_matrix(m, n, 0, 0, synthetic.synth_coef(synthetic.lasso_scale(m, n)))
            c.timing_enable()
            c.column_norms()                                # warm-up: code objects, the workspace
            t = []
            for _ in range(repeats):
                c.set_rhs(0)
                c.timing_reset()
                c.column_norms()
                t.append(c.timing_get(hip.K_AUX)[0])
            rd, nbytes = read_ms(c)
            sh = hip.screen_shape_for(m, n)
            out(f"norms {m} x {n} ({nbytes / 2 ** 30:.1f} GiB; {sh.tiles} tiles x {sh.nslab} slabs of {sh.slab} rows): {stats(t)} -> "
                f"{nbytes / np.median(t) / 1e6:.0f} GB/s; stream read {rd:.4f} ms -> {nbytes / rd / 1e6:.0f} GB/s; ratio {rd / np.median(t):.3f}")


def gather(repeats, fa, hip, synthetic, out):
    m, n = 4096, 65536
    with hip.HipContext(0) as src, hip.HipContext(0) as dst:
        src.generate_matrix(m, n, 0, 0, synthetic.synth_coef(synthetic.lasso_scale(m, n)))
        rd_src, bytes_src = read_ms(src)
        dst.timing_enable()
        for every in (2, 8, 64):
            idx = np.arange(0, n, every, dtype=np.int32)
            dst.gather_columns(src, idx)                    # warm-up
            t = []
            for _ in range(repeats):
                dst.timing_reset()
                dst.gather_columns(src, idx)
                t.append(dst.timing_get(hip.K_AUX)[0])
            rd_dst, bytes_dst = read_ms(dst)
            out(f"gather {m} x {n} keeping 1/{every} ({idx.size} columns, {bytes_dst / 2 ** 20:.0f} MiB written): {stats(t)}; stream read of the source "
                f"{rd_src:.4f} ms + of the destination {rd_dst:.4f} ms = {rd_src + rd_dst:.4f} ms; ratio {(rd_src + rd_dst) / np.median(t):.3f}; "
                f"bytes written + the kept columns' bytes read over the time: {2 * bytes_dst / np.median(t) / 1e6:.0f} GB/s")


def full_reads(c, hip):
    return sum(int(c.timing_get(k)[1]) for k in (hip.K_FWD, hip.K_ADJ, hip.K_FUSED))


def paths(repeats, fa, hip, synthetic, out, path_repeats=3):
    jobs = []
    for m, n in ((4096, 65536), (2048, 131072)):
        def dense(m=m, n=n):
            op = fa.DenseMatrixMap.synthetic(m, n, seed=0, scale=synthetic.lasso_scale(m, n))
            return op, synthetic.lasso_observation(op, synthetic.sparse_signal(n, seed=1), seed_noise=2, sigma=0.01)
        jobs.append((f"dense {m} x {n} (generated)", dense))

    def csr():
        from fasta_python_amd.examples.sparse_design import SparseDesignProblem
        prob, _ = SparseDesignProblem.construct()
        return fa.SparseMatrixMap(prob.S), prob.b
    jobs.append(("CSR 2000 x 4000, density 0.01 (examples/sparse_design.py)", csr))
    for label, make in jobs:
        op, b = make()
        try:
            loss = fa.LeastSquares(b)
            c = op.ctx
            c.timing_enable()
            wall, info = {False: [], True: []}, {}
            for _ in range(path_repeats):
                for screen in (False, True):
                    np.random.seed(1)
                    c.timing_reset()
                    with warnings.catch_warnings():
                        warnings.simplefilter("ignore")
                        t0 = time.perf_counter()
                        pts = fa.path(op, loss, fa.Shrink, n_mus=20, ratio=1e-2, gap_tolerance=1e-6, backend="hip", max_iters=5000, screen=screen)
                        c.sync()
                        wall[screen].append(time.perf_counter() - t0)
                    info[screen] = (sum(p.iteration_count for p in pts), full_reads(c, hip), max(p.certificate.relative for p in pts),
                                    [getattr(p, "kept", op.Vshape[0]) for p in pts], [getattr(p, "rounds", 0) for p in pts])
            out(label)
            for screen in (False, True):
                it, reads, worst, kept, rounds = info[screen]
                out(f"  screen={screen!s:5}  wall {stats(wall[screen], 's')}; {it} iterations; {reads} launches over the full-width A; worst relative gap {worst:.2e}")
                if screen:
                    out(f"               kept per point {kept}")
                    out(f"               rounds per point {rounds}")
            out(f"  screen=True / screen=False (medians): {np.median(wall[True]) / np.median(wall[False]):.3f}")
        finally:
            op.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--path-repeats", type=int, default=3)
    ap.add_argument("--jobs", default="norms,gather,paths")
    a = ap.parse_args()
    import fasta_python_amd as fa
    from fasta_python_amd import hip, synthetic
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)
    out("gap-safe screening (csrc/fh_screen.h), one MI355X, one process; kernel times from HIP events (FH_K_AUX), paths by the wall clock")
    out("")
    for job in a.jobs.split(","):
        if job == "paths":
            paths(a.repeats, fa, hip, synthetic, out, a.path_repeats)
        else:
            {"norms": norms, "gather": gather}[job](a.repeats, fa, hip, synthetic, out)
        out("")
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

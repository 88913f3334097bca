"""What does fh_standardize (csrc/fh_standardize.h) cost, launch by launch, next to the context's own stream probe and to fh_column_norms, and next to
what a user does without it: preprocess.standardize on the host plus one upload?  One MI355X, one process, matrices generated in HBM.

    python scripts/probes/standardize_sizes.py [--out profiles/standardize_sizes.txt] [--reps 7] [--sizes 4096x65536,16384x16384,65536x65536] [--host 16384]

Per size and storage (float64, float32), on ONE context, device-event times (FH_K_AUX: the events bracket the launches, not the host's wait):
  whole call   standardize(center, scale) for (1, 1), (1, 0), (0, 1): (1, 1) issues the sums, the centred squares and the rewrite; (1, 0) leaves
               the centred squares out, (0, 1) the sums.  `--reps` calls of each, interleaved, after one warm-up round; median (min, max).  A call
               standardises what the call before left: the values change, the bytes and the operation counts do not.
  per launch   from those medians: sums = T11 - T01, centred squares = T11 - T10, rewrite = T10 + T01 - T11 (the small closing launches over ld
               columns ride along with the pass they follow).  The spread of a difference is the spreads of its terms.
  host wall    perf_counter around the (1, 1) call (it ends in a stream synchronisation and two copies of n doubles).
  norms        fh_column_norms on the same block, launched again after each call (the rewrite drops the kept norms).
  stream       fh_stream_read_ms over the same block: the rate a read-only pass of this context reaches.
FASTA_HIP_LIB=fasta_python_amd/libfasta_hip_stdmul.so (make -C fasta_python_amd/csrc stdmul: the rewrite multiplies by the reciprocal of the scale
instead of dividing -- NOT the statement, an A/B build that prices the division) runs the same probe on that library; --host 0 leaves the host part out.
The rewrite reads and writes the block once each; its rate is 2 x bytes over its time, to be held against the stream probe's read rate and the
6.29 TB/s of a float4 copy (profiles/r03_mixprobe.txt: 6.70 with non-temporal accesses on both sides).
--host N: the N x N float64 comparison -- NumPy matrix on the host, (a) preprocess.standardize + one upload of the result, (b) one upload of the
raw matrix + standardize() on the device; wall clock of each, once (seconds of host work: the spread is not the question)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def spread(v):
    v = np.asarray(v)
    return f"{np.median(v):9.4f} ms  (min {v.min():.4f}, max {v.max():.4f})"


def aux(c, hip):
    return c.timing_get(hip.K_AUX)[0]


def measure(m, n, storage, reps, fa, hip, synthetic, out):
    op = fa.DenseMatrixMap.synthetic(m, n, seed=0, scale=synthetic.lasso_scale(m, n), storage=storage)
    try:
        c = op.ctx
        c.timing_enable()
        elem = 4 if storage == "f32" else 8
        mp, ld = (m + 15) // 16 * 16, (n + (31 if storage == "f32" else 15)) // (32 if storage == "f32" else 16) * (32 if storage == "f32" else 16)
        nbytes = mp * ld * elem
        modes = ((True, True), (True, False), (False, True))
        t = {k: [] for k in modes}
        wall, norms = [], []
        for r in range(reps + 1):
            for k in modes:
                t0 = aux(c, hip)
                w0 = time.perf_counter()
                c.standardize(center=k[0], scale=k[1])
                w = time.perf_counter() - w0
                dt = aux(c, hip) - t0
                t0 = aux(c, hip)
                c.column_norms()
                dn = aux(c, hip) - t0
                if r:                                   # (round 0 warms every launch up)
                    t[k].append(dt)
                    norms.append(dn)
                    if k == (True, True):
                        wall.append(w * 1e3)
        ms, got = c.stream_read_ms(5)
        T11, T10, T01 = (float(np.median(t[k])) for k in modes)
        sums, css, rew = T11 - T01, T11 - T10, T10 + T01 - T11
        rate = lambda b, x: b / (x * 1e-3) / 1e9 if x > 0 else float("nan")      # bytes over milliseconds, in GB/s
        sh = hip.screen_shape_for(m, n, 0, storage, c.cu_count()[0])
        out(f"{m} x {n} {storage}: block {nbytes / 2 ** 30:.2f} GiB, {sh.tiles} tiles x {sh.nslab} slabs of {sh.slab} rows = {sh.grid} workgroups")
        out(f"  call (1, 1)        {spread(t[modes[0]])}   host wall {spread(wall)}")
        out(f"  call (1, 0)        {spread(t[modes[1]])}")
        out(f"  call (0, 1)        {spread(t[modes[2]])}")
        out(f"  sums               {sums:9.4f} ms   {rate(nbytes, sums):7.0f} GB/s read")
        out(f"  centred squares    {css:9.4f} ms   {rate(nbytes, css):7.0f} GB/s read")
        out(f"  rewrite            {rew:9.4f} ms   {rate(2 * nbytes, rew):7.0f} GB/s read + written")
        out(f"  fh_column_norms    {spread(norms)}   {rate(nbytes, float(np.median(norms))):7.0f} GB/s read")
        out(f"  stream probe       {ms:9.4f} ms   {rate(got, ms):7.0f} GB/s read ({got / 2 ** 30:.2f} GiB)")
        out("")
    finally:
        op.close()


def host_comparison(N, fa, hip, out):
    from fasta_python_amd import preprocess
    rng = np.random.RandomState(0)
    A = rng.standard_normal((N, N)) * 10.0 ** rng.uniform(-3, 3, size=N) + rng.standard_normal(N)
    with hip.HipContext(0) as c:
        c.set_matrix(A[:64])                            # (the context and its first upload are warm)
        t0 = time.perf_counter()
        Z, st = preprocess.standardize(A)
        t_host = time.perf_counter() - t0
        t0 = time.perf_counter()
        c.set_matrix(Z)
        c.sync()
        t_up_z = time.perf_counter() - t0
        del Z
        t0 = time.perf_counter()
        c.set_matrix(A)
        c.sync()
        t_up = time.perf_counter() - t0
        t0 = time.perf_counter()
        means, scales = c.standardize()
        t_dev = time.perf_counter() - t0
        worst = float(np.max(np.abs(scales - st.scales) / st.scales))
    out(f"host comparison, {N} x {N} float64 ({A.nbytes / 2 ** 30:.2f} GiB), wall clock, once each:")
    out(f"  today    preprocess.standardize on the host {t_host:8.3f} s + upload of the result {t_up_z:7.3f} s = {t_host + t_up_z:8.3f} s (and a second host copy)")
    out(f"  device   upload of the raw matrix {t_up:7.3f} s + standardize() {t_dev * 1e3:8.3f} ms = {t_up + t_dev:8.3f} s")
    out(f"  (largest relative difference of the two sets of scales: {worst:.2e})")
    out("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sizes", default="4096x65536,16384x16384,65536x65536")
    ap.add_argument("--host", type=int, default=16384)
    a = ap.parse_args()
    import fasta_python_amd as fa
    from fasta_python_amd import hip, synthetic
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:                                       # (written as it goes: a run cut short leaves what it measured)
            with open(a.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")
    out("fh_standardize (csrc/fh_standardize.h), one MI355X, one process; device-event times under FH_K_AUX unless a line says wall")
    if os.environ.get("FASTA_HIP_LIB"):
        out(f"library: {os.environ['FASTA_HIP_LIB']}")
    out(f"median (min, max) of {a.reps} calls of each kind, interleaved, after one warm-up round; per-launch lines are differences of those medians")
    out("")
    for size in [s for s in a.sizes.split(",") if s]:
        m, n = (int(v) for v in size.split("x"))
        for storage in ("f64", "f32"):
            measure(m, n, storage, a.reps, fa, hip, synthetic, out)
    if a.host:
        host_comparison(a.host, fa, hip, out)


if __name__ == "__main__":
    main()

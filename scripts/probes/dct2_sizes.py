"""What does the 2-D DCT operator (csrc/fh_dct2.h) sustain, and how does it stand beside the 1-D operator and the host?  Per image shape, in a
process of its own: HIP-event time of K-fwd (mode 0, shrink) and K-adj -- median, min and max of `--launches` pairs after a warm-up -- the
algorithmic bytes the launch chain moves over that time, against the 8 TB/s of the data sheet; in the SAME process the 1-D operator's pair at
the same element count N = H * W (two row passes and the transposes as well, plus the six-step twiddle, on complex intermediates); and one
iteration of the same plain solve, wall clock and warm, on the device loop and on the generic host loop over scipy.fftpack's dctn / idctn.

    python scripts/probes/dct2_sizes.py [--out profiles/dct2_sizes.txt] [--launches 30] [--shapes 256x256,512x512,...]

Bytes per element (8-byte doubles), algorithmic -- the twiddle tables (one pair per axis, H + W entries) are not counted:
  K-fwd 112: first row launch x0, g0, x_accel0 read, xhat, xprox and the real rows written (48); transpose 8 + 8; second row launch 8 + 8;
             last launch the rows, d, b read, z written (32)
  K-adj 104: first launch z, b, d read, the transposed residual written (32); row launch 8 + 8; transpose 8 + 8; last row launch the rows, x0,
             xprox, xhat read, g1 written (40)
  the 1-D operator's two-level pair at the same N: 208 / 216 (scripts/probes/dct_sizes.py)
Data from seeded generators."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
PEAK = 8.0e12            # bytes per second, data sheet
DEFAULT_SHAPES = "256x256,512x512,1024x1024,2048x2048,64x2048"
HOST_REPEATS = 5
BYTES = (112, 104)
BYTES_1D = {1: (80, 72), 2: (208, 216)}


def problem(shape, seed=0):
    rng = np.random.RandomState(seed)
    mask = (rng.rand(*shape) < 0.5).astype(np.float64)
    return mask, mask * rng.standard_normal(shape), rng.standard_normal(shape) * 0.5


def timed(c, hip, tau, launches):
    for _ in range(3):
        c.fwd(tau)
        c.adj(tau)
    c.timing_enable(True)
    f, a = [], []
    for _ in range(launches):
        c.timing_reset()
        c.fwd(tau)
        c.adj(tau)
        f.append(c.timing_get(hip.K_FWD)[0])
        a.append(c.timing_get(hip.K_ADJ)[0])
    c.timing_enable(False)
    return np.array(f), np.array(a)


def row(label, ms, nbytes):
    med = float(np.median(ms))
    rate = nbytes / (med * 1e-3)
    return f"  {label:24s} {med:8.4f} ms  (min {ms.min():.4f}, max {ms.max():.4f})  {nbytes / 2**20:9.2f} MiB  {rate / 1e9:7.1f} GB/s = {100 * rate / PEAK:5.2f} % of 8 TB/s"


def iters_for(N):
    """Iterations per timed solve: enough that the solver's set-up is a small share."""
    return 200 if N <= 1 << 16 else (40 if N <= 1 << 20 else 12)


def per_iteration_ms(op, b, x0, backend, iters):
    import fasta_python_amd as fa
    ls, reg = fa.LeastSquares(b), fa.Shrink(0.1)

    def solve(k):
        t0 = time.perf_counter()
        fa.fasta(op, ls.f, ls.gradf, reg.g, reg.prox, x0, backend=backend, verbose=False, adaptive=False, accelerate=False, backtrack=False,
                 max_iters=k, tolerance=0.0, L=1.0, tau0=0.5)
        return (time.perf_counter() - t0) * 1e3 / k
    solve(min(iters, 20))                                   # warm-up, discarded
    return float(np.median([solve(iters) for _ in range(HOST_REPEATS)]))


def child(shape, launches):
    import fasta_python_amd as fa
    from fasta_python_amd import hip
    H, W = shape
    N = H * W
    mask, b, x0 = problem(shape)
    tau = 0.5
    op = fa.DCTMap(shape, mask, lazy=True)
    c = op.ctx
    sh = c.dct2_shape()
    lines = [f"{H} x {W} (N = {N}): radices {sh.radices_h} / {sh.radices_w}, rows per workgroup {sh.rows_h} / {sh.rows_w}, grids {sh.grid_h} / {sh.grid_w} "
             f"and {sh.tiles} tiles, LDS {sh.lds_bytes} B, {sh.launches} launches per direction"]
    c.set_loss_lsq(b)
    c.set_prox(hip.PROX_SHRINK, 0.1)
    c.set_vector(hip.VEC_X0, x0)
    c.init()
    f, a = timed(c, hip, tau, launches)
    fb, ab = BYTES[0] * N, BYTES[1] * N
    lines.append(row("K-fwd", f, fb))
    lines.append(row("K-adj", a, ab))
    pair = float(np.median(f) + np.median(a))
    spread = float((f + a).max() - (f + a).min())
    rate = (fb + ab) / (pair * 1e-3)
    lines.append(f"  pair {pair:.4f} ms (run-to-run spread of the pair {spread:.4f} ms): {rate / 1e9:.1f} GB/s = {100 * rate / PEAK:.2f} % of 8 TB/s")
    iters = iters_for(N)
    dev_iter = per_iteration_ms(op, b, x0, "hip", iters)
    op.close()
    # the 1-D operator at the same element count, the same process, the same prox
    one = fa.DCTMap(N, mask.ravel(), lazy=True)
    c1 = one.ctx
    s1 = c1.dct_shape()
    c1.set_loss_lsq(b.ravel())
    c1.set_prox(hip.PROX_SHRINK, 0.1)
    c1.set_vector(hip.VEC_X0, x0.ravel())
    c1.init()
    f1, a1 = timed(c1, hip, tau, launches)
    one.close()
    pair1 = float(np.median(f1) + np.median(a1))
    spread1 = float((f1 + a1).max() - (f1 + a1).min())
    lines.append(f"  the 1-D operator at N = {N} ({s1.N1} x {s1.N2}, {s1.launches} launches per direction, {sum(BYTES_1D[s1.levels])} bytes per element and pair): "
                 f"K-fwd {np.median(f1):.4f} ms, K-adj {np.median(a1):.4f} ms, pair {pair1:.4f} ms (spread {spread1:.4f} ms) = {pair1 / pair:.2f} x the 2-D pair")
    host = per_iteration_ms(fa.DCTMap(shape, mask, lazy=True), b, x0, "numpy", iters)
    lines.append(f"  one iteration of the same plain solve, wall clock, warm, median of {HOST_REPEATS} solves of {iters} iterations: device loop {dev_iter:.4f} ms, "
                 f"host loop (scipy.fftpack dctn / idctn, this box's CPU) {host:.4f} ms = {host / dev_iter:.1f} x")
    print("DCT2_SIZES " + json.dumps(dict(lines=lines)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dct2_sizes.txt"))
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--shapes", default=DEFAULT_SHAPES)
    ap.add_argument("--child", default=None)
    args = ap.parse_args()
    if args.child:
        return child(tuple(int(k) for k in args.child.split("x")), args.launches)
    lines = ["2-D DCT operator (csrc/fh_dct2.h), one process per shape, HIP events",
             f"median (min, max) of {args.launches} K-fwd + K-adj pairs after 3 warm-up pairs; bytes per element: {BYTES} (K-fwd, K-adj)", ""]
    for spec in [s for s in args.shapes.split(",") if s]:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", spec, "--launches", str(args.launches)], capture_output=True, text=True, timeout=600)
        got = [ln for ln in r.stdout.splitlines() if ln.startswith("DCT2_SIZES ")]
        if r.returncode != 0 or not got:
            lines += [f"{spec}: FAILED (exit status {r.returncode})", r.stderr[-2000:], ""]
            print("\n".join(lines[-3:]))
            raise SystemExit(1)                       # nothing more is started on the device after a failed step
        new = json.loads(got[0][len("DCT2_SIZES "):])["lines"]
        lines += new + [""]
        print("\n".join(new), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()

"""What does the convolution operator (csrc/fh_conv.h) sustain, and against which bound?  Per shape and kernel, in a process of its own: HIP-event
time of K-fwd (mode 0, shrink) and K-adj through fh_timing_* -- median, min and max of `--launches` pairs after a warm-up -- against the two
bounds a pass cannot beat on this chip:

  bytes       its algorithmic bytes (below) at the stream-read rate fh_stream_read_ms measures in the same process (a dense 8192 x 8192 matrix);
  arithmetic  2 * kh * kw * H * W flop at HALF the FP64 vector peak of 78.6 Tflop/s: the contract forbids FMA, so a tap is two instructions.

    python scripts/probes/conv_sizes.py [--out profiles/conv_sizes.txt] [--launches 30] [--jobs 1024x1024:3x3,...]

Bytes per pixel (8-byte doubles), algorithmic -- the halo a neighbouring tile reads again is served by the caches and counted once:
  K-fwd 56: x0, g0, x_accel0 read, xhat, xprox written, b read, z written          (64 with a diagonal)
  K-adj 48: z, b read, x0, xprox, xhat read for the n-side epilogue, g1 written    (56 with a diagonal)
In the first process of each pixel count the unchanged 2-D TV two-launch pair (fused=False: k_fwd_tv_step / k_adj_tv_step, 112 bytes per
pixel, csrc/fh_tv.h) runs on an image of the same pixel count as the memory-bound yardstick.  Every process also times one iteration of a plain
solve, wall clock: the library loop on the device, the generic host loop over ConvMap's roll closures and over scipy.ndimage on this box's
CPU -- the host loops only up to 2^27 pixels x taps, where an iteration over the roll closures still takes seconds.  Data from seeded generators.
Registers, LDS and scratch of each instantiation: `make -C fasta_python_amd/csrc resources` (the compiler's remarks), copied into DESIGN.md."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
FP64_PEAK = 78.6e12
DEFAULT_JOBS = ",".join(f"{n}x{n}:{k}x{k}" for n in (1024, 4096, 8192) for k in (3, 9, 16)) + f",{1 << 22}:15"
FWD_BYTES, ADJ_BYTES, TV2_PAIR_BYTES = 56, 48, 112
STREAM_N = 8192
HOST_LIMIT = 1 << 27          # pixels x taps up to which the host loops are timed beside the device


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


def parse(job):
    s, k = job.split(":")
    shape, kshape = tuple(int(v) for v in s.split("x")), tuple(int(v) for v in k.split("x"))
    return shape, kshape


def wall_per_iteration(fa, op, b, backend, iters, repeats=3):
    ls, reg = fa.LeastSquares(b), fa.Shrink(0.01)
    x0 = np.zeros(b.shape)

    def solve(k):
        t0 = time.perf_counter()
        fa.fasta(op, ls.f, ls.gradf, reg.g, reg.prox, x0, backend=backend, verbose=False, adaptive=False, accelerate=False, backtrack=False,
                 max_iters=k, tolerance=0.0, L=1.0, tau0=0.5)
        return (time.perf_counter() - t0) * 1e3 / k
    solve(min(iters, 3))                                    # warm-up, discarded
    return float(np.median([solve(iters) for _ in range(repeats)]))


def child(job, launches, yardstick):
    import scipy.ndimage
    import fasta_python_amd as fa
    from fasta_python_amd import hip
    shape, kshape = parse(job)
    n = int(np.prod(shape))
    taps = int(np.prod(kshape))
    rng = np.random.RandomState(0)
    K = rng.rand(*kshape)
    K /= K.sum()
    b, x0 = rng.standard_normal(shape), rng.standard_normal(shape) * 0.5
    tau = 0.5
    # the stream-read rate of this process
    with hip.HipContext(0) as d:
        d.generate_matrix(STREAM_N, STREAM_N, 0, 1, 1e-3)
        sms, sbytes = d.stream_read_ms(5)
    stream = sbytes / (sms * 1e-3)
    op = fa.ConvMap(shape, K)
    c = op.ctx
    sh = c.conv_shape()
    lines = [f"{'x'.join(map(str, shape))} under {'x'.join(map(str, kshape))}: tile {sh.tile_h} x {sh.tile_w}, grid {sh.grid}, LDS {sh.lds_bytes} B; "
             f"stream-read rate of this process {stream / 1e9:.0f} GB/s"]
    c.set_loss_lsq(b)
    c.set_prox(hip.PROX_SHRINK, 0.01)
    c.set_vector(hip.VEC_X0, x0)
    c.init()
    f, a = timed(c, hip, tau, launches)
    flop_ms = 2.0 * taps * n / (FP64_PEAK / 2) * 1e3
    for label, ms, per in (("K-fwd", f, FWD_BYTES), ("K-adj", a, ADJ_BYTES)):
        med = float(np.median(ms))
        byte_ms = per * n / stream * 1e3
        bound, which = max(byte_ms, flop_ms), ("bytes" if byte_ms >= flop_ms else "arithmetic")
        lines.append(f"  {label} {med:9.4f} ms  (min {ms.min():.4f}, max {ms.max():.4f})   bounds: bytes {byte_ms:.4f} ms, arithmetic {flop_ms:.4f} ms   "
                     f"-> {med / bound:5.2f} x the {which} bound   ({per * n / (med * 1e-3) / 1e9:.0f} GB/s, {2.0 * taps * n / (med * 1e-3) / 1e12:.2f} Tflop/s)")
    pair = float(np.median(f) + np.median(a))
    iters = 50 if n <= 1 << 22 else 20
    dev = wall_per_iteration(fa, op, b, "hip", iters)
    op.close()
    if yardstick:
        H, W = (shape if len(shape) == 2 else (1 << (n.bit_length() // 2), n >> (n.bit_length() // 2)))
        op2 = fa.GradDivMap((H, W))
        d = op2.ctx
        d.set_loss_lsq(rng.standard_normal(H * W))
        d.set_prox(hip.PROX_TVBALL)
        d.set_vector(hip.VEC_X0, rng.standard_normal(2 * H * W) * 0.5)
        d.init()
        df, da = timed(d, hip, tau, launches)
        dpair = float(np.median(df) + np.median(da))
        lines.append(f"  yardstick: the 2-D TV two-launch pair on {H} x {W}: K-fwd {np.median(df):.4f} ms, K-adj {np.median(da):.4f} ms, pair {dpair:.4f} ms = "
                     f"{TV2_PAIR_BYTES * H * W / (dpair * 1e-3) / 1e9:.0f} GB/s on its {TV2_PAIR_BYTES} bytes per pixel; this pair {pair:.4f} ms = "
                     f"{(FWD_BYTES + ADJ_BYTES) * n / (pair * 1e-3) / 1e9:.0f} GB/s on its {FWD_BYTES + ADJ_BYTES}")
        op2.close()
    lines.append(f"  one iteration of the same plain solve, wall clock, warm, on the device (the library loop, median of 3 solves of {iters} iterations): {dev:.4f} ms")
    if n * taps <= HOST_LIMIT:
        host_iters = 3 if n * taps > 1 << 24 else 20
        host = wall_per_iteration(fa, fa.ConvMap(shape, K), b, "numpy", host_iters, repeats=2)
        if len(shape) == 2:
            nd = fa.LinearMap(lambda x: scipy.ndimage.convolve(x, K, mode="wrap"), lambda w: scipy.ndimage.correlate(w, K, mode="wrap"), shape, shape)
        else:
            nd = fa.LinearMap(lambda x: scipy.ndimage.convolve1d(x, K, mode="wrap"), lambda w: scipy.ndimage.correlate1d(w, K, mode="wrap"), shape, shape)
        ndi = wall_per_iteration(fa, nd, b, "numpy", host_iters, repeats=2)
        lines.append(f"  the generic host loop on this box's CPU ({host_iters} iterations): over the roll closures {host:.2f} ms = {host / dev:.0f} x, "
                     f"over scipy.ndimage {ndi:.2f} ms = {ndi / dev:.0f} x")
    else:
        lines.append("  the host loops are not timed at this size (an iteration over the roll closures takes tens of seconds)")
    print("CONV_SIZES " + json.dumps(dict(lines=lines)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conv_sizes.txt"))
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--jobs", default=DEFAULT_JOBS)
    ap.add_argument("--child", default=None)
    ap.add_argument("--yardstick", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.launches, args.yardstick)
    lines = ["convolution operator (csrc/fh_conv.h), one MI355X, one process per shape and kernel, HIP events through fh_timing_*",
             f"median (min, max) of {args.launches} K-fwd + K-adj pairs after 3 warm-up pairs; bytes per pixel: K-fwd {FWD_BYTES}, K-adj {ADJ_BYTES}; "
             f"arithmetic bound: 2 kh kw H W flop at {FP64_PEAK / 2e12:.1f} Tflop/s (half the FP64 vector peak: no FMA)", ""]
    seen = set()
    for job in [j for j in args.jobs.split(",") if j]:
        n = int(np.prod(parse(job)[0]))
        cmd = [sys.executable, os.path.abspath(__file__), "--child", job, "--launches", str(args.launches)] + ([] if n in seen else ["--yardstick"])
        seen.add(n)
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        got = [ln for ln in r.stdout.splitlines() if ln.startswith("CONV_SIZES ")]
        if r.returncode != 0 or not got:
            lines += [f"{job}: FAILED (exit status {r.returncode})", r.stderr[-2000:], ""]
            print("\n".join(lines[-3:]))
            with open(args.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")
            raise SystemExit(1)                       # nothing more is started on the device after a failed step
        new = json.loads(got[0][len("CONV_SIZES "):])["lines"]
        lines += new + [""]
        print("\n".join(new), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()

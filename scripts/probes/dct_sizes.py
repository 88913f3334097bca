"""What does the DCT operator (csrc/fh_dct.h) sustain, and what does it replace?  Per length N, in a process of its own: HIP-event time of K-fwd
(mode 0, l-infinity prox; the level search is timed beside it) and K-adj -- median, min and max of `--launches` pairs after a warm-up -- the
bytes the chosen launch sequence moves over that time, against the 8 TB/s of the data sheet; beside it the HOST alternative, one iteration of
the generic host loop over the reference's scipy.fftpack closures (the only thing that serves these lengths without this operator) -- WARM:
one whole solve is discarded first (the first call imports scipy.fftpack and plans the transform), then the median of `HOST_REPEATS` solves of
`host_iters(N)` iterations each, so that the solver's set-up is a small share; and the two transforms alone, median of many calls; for
`--dense` lengths the DENSE path on the explicit N x N matrix diag(mask) * C (the only device alternative, where it exists); and, for every
length of the accuracy list, the device's error against a longdouble O(N^2) transform beside scipy's on the same input.

    python scripts/probes/dct_sizes.py [--out profiles/dct_sizes.txt] [--launches 30] [--sizes 1000,2048,...] [--dense 4096,16384]

Bytes per element (8-byte doubles, 16-byte complex), algorithmic -- a table or a vector read twice by one launch is counted once:
  one row   K-fwd 80: x0, g0, x_accel0 read, xhat, xprox written, the post-twiddle (16), d, b read, z written
            K-adj 72: z, b, d and the post-twiddle (16) read, x0, xprox, xhat read for the n-side epilogue, g1 written
  two level K-fwd 208: prologue 24 read, 16 + 8 (real rows) written; rows of N1 8 read, 16 written, six-step twiddle 16; transpose 16 + 16; rows of
            N2 16 + 16; last launch 16 + post-twiddle 16 + d, b 16 read, z 8 written
            K-adj 216: first launch z, b, d 24 + post-twiddle 16 read, 16 written; rows 16 + 16 + twiddle 16; transpose 32; rows 32; last launch 16
            read, x0, xprox, xhat 24 read, g1 8 written
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
DEFAULT_SIZES = f"1000,2048,{1 << 16},{1 << 20},{1 << 22},{3 << 20}"
DEFAULT_DENSE = "4096,16384"
ACCURACY = "1,2,3,4,5,6,8,9,15,16,25,30,45,64,96,125,1000,1024,2048,4096,6000,60:16,96:16,150:16,250:25,1000:40"      # N or N:row cap
HOST_REPEATS = 5
BYTES = {1: (80, 72), 2: (208, 216)}


def problem(N, seed=0):
    rng = np.random.RandomState(seed)
    mask = (rng.rand(N) < 0.5).astype(np.float64)
    return mask, mask * rng.standard_normal(N), rng.standard_normal(N) * 0.5


def timed(c, hip, tau, launches):
    for _ in range(3):
        c.fwd(tau)
        c.adj(tau)
    c.timing_enable(True)
    f, a, lv = [], [], []
    for _ in range(launches):
        c.timing_reset()
        c.fwd(tau)
        c.adj(tau)
        f.append(c.timing_get(hip.K_FWD)[0])
        a.append(c.timing_get(hip.K_ADJ)[0])
        lv.append(c.timing_get(hip.K_LEVEL)[0])
    c.timing_enable(False)
    return np.array(f), np.array(a), np.array(lv)


def row(label, ms, nbytes):
    med = float(np.median(ms))
    rate = nbytes / (med * 1e-3)
    return f"  {label:24s} {med:8.4f} ms  (min {ms.min():.4f}, max {ms.max():.4f})  {nbytes / 2**20:9.2f} MiB  {rate / 1e9:7.1f} GB/s = {100 * rate / PEAK:5.2f} % of 8 TB/s"


def host_iters(N):
    """Iterations per timed host solve: enough that the solver's set-up (one initial pass, a few allocations) is a small share."""
    return 200 if N <= 1 << 16 else (40 if N <= 1 << 20 else 12)


def host_iteration_ms(N, mask, b, x0):
    """(ms per iteration of the generic host loop -- plain FBS, no backtracking, over the reference's closures: two scipy.fftpack transforms, the
    l-infinity projection and the loop's vector passes --, ms of the two transforms alone): one solve discarded, then the median of HOST_REPEATS
    solves of host_iters(N) iterations; the transforms: median of the same number of calls."""
    import fasta_python_amd as fa
    op = fa.DCTMap(N, mask, lazy=True)
    ls, reg = fa.LeastSquares(b), fa.LinfProx(1.0)
    iters = host_iters(N)

    def solve(k):
        t0 = time.perf_counter()
        fa.fasta(op, ls.f, ls.gradf, reg.g, reg.prox, x0, backend="numpy", verbose=False, adaptive=False, accelerate=False, backtrack=False,
                 max_iters=k, tolerance=0.0, L=1.0, tau0=0.5)
        return (time.perf_counter() - t0) * 1e3 / k
    solve(min(iters, 20))                                   # warm-up, discarded
    per_iter = float(np.median([solve(iters) for _ in range(HOST_REPEATS)]))
    pair = []
    for _ in range(iters):
        t0 = time.perf_counter()
        op.H(op(x0))
        pair.append((time.perf_counter() - t0) * 1e3)
    return per_iter, float(np.median(pair))


def child(N, launches):
    import fasta_python_amd as fa
    from fasta_python_amd import hip
    mask, b, x0 = problem(N)
    tau = 0.5
    op = fa.DCTMap(N, mask, lazy=True)
    c = op.ctx
    sh = c.dct_shape()
    lines = [f"N = {N}: " + (f"one row, radices {sh.radices1}, LDS {sh.lds_bytes} B, 1 launch per direction" if sh.levels == 1 else
                             f"{sh.N1} x {sh.N2}, radices {sh.radices1} / {sh.radices2}, rows per workgroup {sh.rows1} / {sh.rows2}, grids {sh.grid1} / {sh.grid2} "
                             f"and {sh.tiles} tiles, LDS {sh.lds_bytes} B, {sh.launches} launches per direction")]
    c.set_loss_lsq(b)
    c.set_prox(hip.PROX_LINF, 1.0)
    c.set_vector(hip.VEC_X0, x0)
    c.init()
    f, a, lv = timed(c, hip, tau, launches)
    fb, ab = BYTES[sh.levels][0] * N, BYTES[sh.levels][1] * N
    lines.append(row("K-fwd", f, fb))
    lines.append(row("K-adj", a, ab))
    pair = float(np.median(f) + np.median(a))
    rate = (fb + ab) / (pair * 1e-3)
    lines.append(f"  pair {pair:.4f} ms: {rate / 1e9:.1f} GB/s = {100 * rate / PEAK:.2f} % of 8 TB/s; the level search of the l-infinity prox beside it: {np.median(lv):.4f} ms")
    # the same solve end to end on the device (the library's host-side loop: launches, level search, scalar round trips), wall clock per iteration
    ls, reg = fa.LeastSquares(b), fa.LinfProx(1.0)
    iters = host_iters(N)

    def device_solve(k):
        t0 = time.perf_counter()
        fa.fasta(op, ls.f, ls.gradf, reg.g, reg.prox, x0, backend="hip", verbose=False, adaptive=False, accelerate=False, backtrack=False,
                 max_iters=k, tolerance=0.0, L=1.0, tau0=0.5)
        return (time.perf_counter() - t0) * 1e3 / k
    device_solve(min(iters, 20))
    dev_iter = float(np.median([device_solve(iters) for _ in range(HOST_REPEATS)]))
    op.close()
    host, host_pair = host_iteration_ms(N, mask, b, x0)
    lines.append(f"  one iteration of the same plain solve, wall clock, warm, median of {HOST_REPEATS} solves of {iters} iterations: device loop {dev_iter:.4f} ms, "
                 f"host loop (scipy.fftpack, this box's CPU) {host:.4f} ms = {host / dev_iter:.1f} x")
    lines.append(f"  the two transforms alone on the host, warm: {host_pair:.4f} ms = {host_pair / pair:.1f} x the device pair's kernel time")
    print("DCT_SIZES " + json.dumps(dict(lines=lines)))


def dense_child(N, launches):
    """The dense path on the explicit matrix diag(mask) * C: K-fwd + K-adj of the dense operator, the same prox and data."""
    import scipy.fftpack
    import fasta_python_amd as fa
    from fasta_python_amd import hip
    mask, b, x0 = problem(N)
    A = scipy.fftpack.dct(np.eye(N), axis=0, norm="ortho")
    A *= mask[:, None]
    tau = 0.5
    lines = []
    for label, make in (("DCT operator", lambda: fa.DCTMap(N, mask, lazy=True)), ("dense N x N matrix", lambda: fa.DenseMatrixMap(A))):
        op = make()
        c = op.ctx
        c.set_loss_lsq(b)
        c.set_prox(hip.PROX_LINF, 1.0)
        c.set_vector(hip.VEC_X0, x0)
        c.init()
        f, a, _ = timed(c, hip, tau, launches)
        lines.append(f"  N = {N}: {label:20s} K-fwd {np.median(f):.4f} ms, K-adj {np.median(a):.4f} ms, pair {np.median(f) + np.median(a):.4f} ms"
                     + (f"   ({8 * N * N / 2**20:.0f} MiB of matrix)" if "dense" in label else ""))
        op.close()
    print("DCT_SIZES " + json.dumps(dict(lines=lines)))


def exact_dct(x):
    """The orthonormal DCT-II by the direct O(N^2) sum in longdouble, 256 rows at a time."""
    N = len(x)
    pi = np.longdouble("3.14159265358979323846264338327950288")
    xl = np.asarray(x, dtype=np.longdouble)
    n = np.arange(N, dtype=np.int64)[None, :]
    out = np.empty(N, dtype=np.longdouble)
    for k0 in range(0, N, 256):
        k = np.arange(k0, min(k0 + 256, N), dtype=np.int64)[:, None]
        out[k0:k0 + 256] = np.cos(((k * (2 * n + 1)) % (4 * N)).astype(np.longdouble) * (pi / np.longdouble(2 * N))) @ xl
    out *= np.sqrt(np.longdouble(2) / N)
    out[0] *= np.sqrt(np.longdouble(0.5))
    return out


def accuracy_child(sizes):
    import scipy.fftpack
    import fasta_python_amd as fa
    lines = ["  N        device |err|_inf   scipy.fftpack |err|_inf   ratio     (error of the forward transform of one Gaussian vector against longdouble)"]
    from fasta_python_amd import hip
    for spec in sizes:
        N, _, cap = spec.partition(":")
        N, cap = int(N), int(cap or 0)
        x = np.random.RandomState(N).standard_normal(N)
        want = exact_dct(x)
        op = fa.DCTMap(N, lazy=True, tuning={hip.TUNE_DCT_ROW_CAP: cap} if cap else None)
        sh = op.ctx.dct_shape()
        dev = float(np.max(np.abs(op.device_apply(x) - want)))
        op.close()
        ref = float(np.max(np.abs(scipy.fftpack.dct(x, norm="ortho") - want)))
        form = "one row" if sh.levels == 1 else f"{sh.N1} x {sh.N2}" + (f" (cap {cap})" if cap else "")
        lines.append(f"  {N:6d}   {dev:.3e}          {ref:.3e}                  {dev / ref if ref else float('inf'):6.2f}    {form}")
    print("DCT_SIZES " + json.dumps(dict(lines=lines)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dct_sizes.txt"))
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--sizes", default=DEFAULT_SIZES)
    ap.add_argument("--dense", default=DEFAULT_DENSE)
    ap.add_argument("--accuracy", default=ACCURACY)
    ap.add_argument("--child", default=None)
    args = ap.parse_args()
    if args.child:
        kind, _, spec = args.child.partition(":")
        if kind == "size":
            return child(int(spec), args.launches)
        if kind == "dense":
            return dense_child(int(spec), args.launches)
        return accuracy_child(spec.split(","))
    lines = ["DCT operator (csrc/fh_dct.h), one process per length, HIP events",
             f"median (min, max) of {args.launches} K-fwd + K-adj pairs after 3 warm-up pairs; bytes per element: one row {BYTES[1]}, two levels {BYTES[2]} (K-fwd, K-adj)", ""]
    jobs = [f"size:{n}" for n in args.sizes.split(",") if n] + [f"dense:{n}" for n in args.dense.split(",") if n] + ([f"accuracy:{args.accuracy}"] if args.accuracy else [])
    for job in jobs:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", job, "--launches", str(args.launches)], capture_output=True, text=True, timeout=900)
        got = [ln for ln in r.stdout.splitlines() if ln.startswith("DCT_SIZES ")]
        if r.returncode != 0 or not got:
            lines += [f"{job}: FAILED (exit status {r.returncode})", r.stderr[-2000:], ""]
            print("\n".join(lines[-3:]))
            raise SystemExit(1)                       # nothing more is started on the device after a failed step
        new = json.loads(got[0][len("DCT_SIZES "):])["lines"]
        if job.startswith("dense:") and not any("dense path" in ln for ln in lines):
            lines.append("the dense path on the explicit matrix diag(mask) * C, the same prox and data:")
        if job.startswith("accuracy:"):
            lines += ["", "accuracy:"]
        lines += new + ([""] if job.startswith("size:") else [])
        print("\n".join(new), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()

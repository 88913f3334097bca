"""Where do the multi-column dense kernels (csrc/fh_multi.h) leave the bandwidth limit?  For LB = 2, 4, 8, 16 columns per row at 16384^2 and
65536 x 16384: HIP-event time of one K-fwd (prologue + matrix kernel) and one K-adj launch -- median, min and max of `--launches` launches
after a warm-up, all in one process on one matrix -- the bytes the algorithm moves (m*n*8 for A plus the vector traffic of the launch) over
that time against the 8 TB/s of the data sheet, the unchanged vector kernels' figures from the same run, and the registers of every
instantiation (hipcc -Rpass-analysis=kernel-resource-usage).

    python scripts/probes/mmv_columns.py [--out profiles/mmv_columns.txt] [--launches 30] [--shapes 16384x16384,65536x16384]
"""
import argparse
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
PEAK = 8.0e12            # bytes per second, data sheet


def registers():
    """{kernel: (VGPRs, AGPRs, scratch bytes per lane, waves per SIMD)} of the instantiations in fh_multi_part.hip"""
    csrc = os.path.join(ROOT, "fasta_python_amd", "csrc")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-unused-function", "-c", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", "-o", os.devnull, "fh_multi_part.hip"], cwd=csrc, capture_output=True, text=True)
    out, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
        for key, pat in (("v", r" VGPRs: (\d+)"), ("a", r"AGPRs: (\d+)"), ("s", r"ScratchSize \[bytes/lane\]: (\d+)"), ("o", r"Occupancy \[waves/SIMD\]: (\d+)")):
            m = re.search(pat, line)
            if m and name:
                out[name][key] = int(m.group(1))
    return {k: v for k, v in out.items() if "k_mc_" in k}


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
    return f"  {label:22s} {med:8.3f} ms  (min {ms.min():.3f}, max {ms.max():.3f})  {nbytes / 2**30:7.2f} GiB  {rate / 1e12:5.2f} TB/s = {100 * rate / PEAK:5.1f} % of 8 TB/s"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mmv_columns.txt"))
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--shapes", default="16384x16384,65536x16384")
    args = ap.parse_args()
    import fasta_python_amd as fa
    from fasta_python_amd import hip
    lines = ["multi-column dense kernels (csrc/fh_multi.h) against the vector kernels (csrc/fh_dense.h), one process per table, HIP events",
             f"median (min, max) of {args.launches} launches after 3 warm-up launches; bytes = m*n*8 + the launch's vector traffic (slab partials of K-adj not counted)", ""]
    tau = 1e-3
    for shape in args.shapes.split(","):
        m, n = (int(v) for v in shape.split("x"))
        op = fa.DenseMatrixMap.synthetic(m, n, seed=3, scale=1.0 / 128)
        c = op.ctx
        rng = np.random.RandomState(0)
        lines.append(f"{m} x {n}  (A = {m * n * 8 / 2**30:.1f} GiB)")
        c.set_loss_lsq(rng.randn(m))
        c.set_prox(hip.PROX_SHRINK, 0.01)
        c.set_vector(hip.VEC_X0, rng.randn(n) * 0.01)
        c.init()
        f, a = timed(c, hip, tau, args.launches)
        A8 = m * n * 8
        lines.append(row("vector K-fwd", f, A8 + (4 * n + 2 * m) * 8))
        lines.append(row("vector K-adj", a, A8 + (2 * m + 4 * n) * 8))
        base = float(np.median(f) + np.median(a))
        for L in (2, 4, 8, 16):
            c.set_rhs(L)
            c.set_loss_lsq(rng.randn(m, L))
            c.set_prox(hip.PROX_GROUP, 0.01)
            c.set_vector(hip.VEC_X0, rng.randn(n, L) * 0.01)
            c.init()
            f, a = timed(c, hip, tau, args.launches)
            lines.append(row(f"LB = {L:2d}  K-fwd", f, A8 + (5 * n + 2 * m) * L * 8))
            lines.append(row(f"LB = {L:2d}  K-adj", a, A8 + (2 * m + 4 * n) * L * 8))
            pair = float(np.median(f) + np.median(a))
            # host <-> device transfer of an (m, L) matrix (outside the timed kernels, inside every solve and fh_apply): wall clock per call
            import time
            Bh = rng.randn(m, L)
            ts, tg = [], []
            for _ in range(7):
                t0 = time.perf_counter(); c.set_vector(hip.VEC_B, Bh); t1 = time.perf_counter(); c.get_vector(hip.VEC_B, m * L); t2 = time.perf_counter()
                ts.append(t1 - t0); tg.append(t2 - t1)
            lines.append(f"  LB = {L:2d}  set_vector / get_vector of ({m}, {L}): {1e3 * np.median(ts):.3f} / {1e3 * np.median(tg):.3f} ms per call (host clock, median of 7)")
            lines.append(f"  LB = {L:2d}  pair {pair:.3f} ms = {pair / base:.2f} x the vector pair: {L * base / pair:.2f} x faster than {L} vector passes; "
                         f"{2 * 2 * m * n * L / (pair * 1e-3) / 1e12:.1f} TFLOP/s float64")
        lines.append("")
        op.close()
    lines.append("registers of the instantiations (VGPRs, AGPRs, scratch bytes per lane, waves per SIMD):")
    for k, v in sorted(registers().items()):
        lines.append(f"  {k:44s} {v.get('v', 0):4d} {v.get('a', 0):4d} {v.get('s', 0):4d} {v.get('o', 0):2d}")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    print(text)


if __name__ == "__main__":
    main()

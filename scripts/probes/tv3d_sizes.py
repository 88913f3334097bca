"""What do the 3-D stencil kernels (csrc/fh_tv3d.h) sustain?  K-fwd (mode 0, TV-ball prox), K-adj (mode 0) and the pair, per volume in a process of
its own: HIP-event time -- median, min and max of `--launches` launches after a warm-up -- the bytes the launch has to move over that time,
against the 8 TB/s of the data sheet; the pair a second and third time with plain / non-temporal stores of xhat, xprox and g1
(FH_TUNE_NT_LOADS = 0 / 1).  In the 512^3 process the unchanged 2-D two-launch pair (fused=False: k_fwd_tv_step / k_adj_tv_step) runs on an
8192^2 image as the yardstick, as GB/s on its own algorithmic bytes (112 per pixel, csrc/fh_tv.h).  Registers of every instantiation at the end.

    python scripts/probes/tv3d_sizes.py [--out profiles/tv3d_sizes.txt] [--launches 30] [--shapes 128x128x128,...]

Algorithmic bytes per voxel, P = D * H * W voxels of 8-byte doubles:
  K-fwd  17 * 8: x0, g0 and the acceleration history x_accel0 (the restart dot) read, 3 each; xhat, xprox written, 3 each; b read, z written
  K-adj  14 * 8: z, b read; g1 written, 3; x0, xprox, xhat read for the n-side epilogue, 3 each
Halo re-reads (a tile's h+1 row and w+1 column, a chunk's extra plane) are NOT counted: they are the kernel's overhead.  Data from seeded generators."""
import argparse
import json
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
PEAK = 8.0e12            # bytes per second, data sheet
DEFAULT_SHAPES = "128x128x128,256x256x256,512x512x512,64x2048x2048"
FWD_BYTES, ADJ_BYTES, TV2_PAIR_BYTES = 17 * 8, 14 * 8, 112


def registers():
    """{kernel: VGPRs, scratch bytes per lane, waves per SIMD, LDS bytes} of the instantiations in fh_tv3d_part.hip"""
    csrc = os.path.join(ROOT, "fasta_python_amd", "csrc")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-unused-function", "-c", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", "-o", os.devnull, "fh_tv3d_part.hip"], cwd=csrc, capture_output=True, text=True)
    out, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
        for key, pat in (("v", r" VGPRs: (\d+)"), ("s", r"ScratchSize \[bytes/lane\]: (\d+)"), ("o", r"Occupancy \[waves/SIMD\]: (\d+)"), ("l", r"LDS Size \[bytes/block\]: (\d+)")):
            m = re.search(pat, line)
            if m and name:
                out[name][key] = int(m.group(1))
    return {k: v for k, v in out.items() if "k_tv3_" in k}


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
    return f"  {label:22s} {med:8.3f} ms  (min {ms.min():.3f}, max {ms.max():.3f})  {nbytes / 2**20:9.1f} MiB  {rate / 1e9:7.1f} GB/s = {100 * rate / PEAK:5.1f} % of 8 TB/s"


def child(spec, launches):
    """One volume, this process: the lines of its table on stdout as JSON."""
    import fasta_python_amd as fa
    from fasta_python_amd import hip
    shape = tuple(int(k) for k in spec.split("x"))
    P = int(np.prod(shape))
    tau = 0.05
    rng = np.random.RandomState(0)
    op = fa.GradDivMap(shape)
    c = op.ctx
    sh = c.tv3d_shape()
    lines = [f"{spec}: {P} voxels, n = {3 * P}; tiles of {sh.tile_h} x {sh.tile_w}, {sh.planes} planes per workgroup, grid {sh.chunks} x {sh.tiles_h} x {sh.tiles_w} = {sh.grid} workgroups"]
    c.set_loss_lsq(rng.standard_normal(P))
    c.set_prox(hip.PROX_TVBALL)
    c.set_vector(hip.VEC_X0, rng.standard_normal(3 * P) * 0.5)
    c.init()
    f, a = timed(c, hip, tau, launches)
    fb, ab = FWD_BYTES * P, ADJ_BYTES * P
    lines.append(row("3-D K-fwd (TV ball)", f, fb))
    lines.append(row("3-D K-adj", a, ab))
    pair = float(np.median(f) + np.median(a))
    rate3 = (fb + ab) / (pair * 1e-3)
    lines.append(f"  3-D pair {pair:.3f} ms: {rate3 / 1e9:.1f} GB/s = {100 * rate3 / PEAK:.1f} % of 8 TB/s")
    for nt in (0, 1):
        c.set_tuning(hip.TUNE_NT_LOADS, nt)
        f2, a2 = timed(c, hip, tau, launches)
        lines.append(f"  {'non-temporal' if nt else 'plain':12s} stores: K-fwd {np.median(f2):.3f} ms, K-adj {np.median(a2):.3f} ms, pair {np.median(f2) + np.median(a2):.3f} ms"
                     + ("" if nt else "   <- the default"))
    op.close()
    verdict = None
    if spec == "512x512x512":
        n2 = 8192
        op2 = fa.GradDivMap((n2, n2))
        d = op2.ctx
        d.set_loss_lsq(rng.standard_normal(n2 * n2))
        d.set_prox(hip.PROX_TVBALL)
        d.set_vector(hip.VEC_X0, rng.standard_normal(2 * n2 * n2) * 0.5)
        d.init()
        df, da = timed(d, hip, tau, launches)
        dpair = float(np.median(df) + np.median(da))
        rate2 = TV2_PAIR_BYTES * n2 * n2 / (dpair * 1e-3)
        lines.append(f"  yardstick: 2-D two-launch pair on 8192^2: K-fwd {np.median(df):.3f} ms, K-adj {np.median(da):.3f} ms, pair {dpair:.3f} ms: "
                     f"{rate2 / 1e9:.1f} GB/s on its {TV2_PAIR_BYTES} bytes per pixel")
        verdict = rate3 / rate2
        lines.append(f"  the 3-D pair at 512^3 runs at {100 * verdict:.0f} % of the yardstick's rate" + ("" if verdict >= 0.5 else "  -- LESS THAN HALF: find out why"))
        op2.close()
    print("TV3D_SIZES " + json.dumps(dict(lines=lines, verdict=verdict)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tv3d_sizes.txt"))
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--shapes", default=DEFAULT_SHAPES)
    ap.add_argument("--child", default=None)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.launches)
    lines = ["3-D stencil kernels (csrc/fh_tv3d.h), one process per volume, HIP events",
             f"median (min, max) of {args.launches} launches after 3 warm-up launches; bytes per voxel: K-fwd {FWD_BYTES}, K-adj {ADJ_BYTES} (halo re-reads not counted)", ""]
    for spec in args.shapes.split(","):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", spec, "--launches", str(args.launches)], capture_output=True, text=True, timeout=600)
        got = [ln for ln in r.stdout.splitlines() if ln.startswith("TV3D_SIZES ")]
        if r.returncode != 0 or not got:
            lines += [f"{spec}: FAILED (exit status {r.returncode})", r.stderr[-2000:], ""]
            print("\n".join(lines[-3:]))
            raise SystemExit(1)                       # nothing more is started on the device after a failed step
        lines += json.loads(got[0][len("TV3D_SIZES "):])["lines"] + [""]
        print("\n".join(lines[-(len(json.loads(got[0][len('TV3D_SIZES '):])['lines']) + 1):]), flush=True)
    lines.append("registers (hipcc -Rpass-analysis=kernel-resource-usage):")
    for name, r in sorted(registers().items()):
        lines.append(f"  {name:40s} VGPRs {r.get('v')}, scratch {r.get('s')} B/lane, {r.get('o')} waves/SIMD, LDS {r.get('l')} B")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()

"""What does a matrix unknown cost on a sparse operator (csrc/fh_spmulti.h)?  Per shape of DESIGN section 10's table, in a process of its
own: the unchanged vector sparse pair (k_sp_fwd / k_sp_adj with their prologue launches) and, on the same matrix, the multi-column pair at
L = 1, 2, 4, 8, 16 columns.  HIP-event time -- median, min and max of `--launches` launches after a warm-up -- and the bytes the launch has
to move (12 per stored entry: 8 value + 4 index; 8 per row offset; the launch's vector traffic at LB columns per row, every gathered operand
counted ONCE) over that time, against the 8 TB/s of the data sheet.  The figure the form exists for is the last column: the pair at L
columns against L vector pairs.  Reported, not gated.  Registers of every instantiation at the end.

    python scripts/probes/sparse_columns.py [--out profiles/sparse_columns.txt] [--launches 30] [--shapes uniform:65536:0.001,...] [--columns 1,2,4,8,16]

Matrices and their generators are those of scripts/probes/sparse_rows.py.  Timing only: run it under a profiler's kernel trace, if at all,
separately from any counter collection."""
import argparse
import importlib.util
import json
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
PEAK = 8.0e12            # bytes per second, data sheet
DEFAULT_SHAPES = "uniform:65536:0.001,uniform:65536:0.01,uniform:65536:0.05,perrow:1048576:16,powerlaw:1048576:16"


def rows_probe():
    spec = importlib.util.spec_from_file_location("sparse_rows", os.path.join(ROOT, "scripts", "probes", "sparse_rows.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def registers():
    """{kernel: (VGPRs, AGPRs, scratch bytes per lane, waves per SIMD)} of the instantiations in fh_spmulti_part.hip"""
    csrc = os.path.join(ROOT, "fasta_python_amd", "csrc")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-unused-function", "-c", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", "-o", os.devnull, "fh_spmulti_part.hip"], cwd=csrc, capture_output=True, text=True)
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
    return {k: v for k, v in out.items() if "k_spmc_" in k}


def lb_of(L):
    return 2 if L <= 2 else 4 if L <= 4 else 8 if L <= 8 else 16


def lanes_per_row(nnz, rows, C):
    """The host's choice of G (csrc/fasta_hip.hip: sp_upload_side): the smallest of max(4, C)..64 with 2 * (G / C) >= the mean row length."""
    G = max(4, C)
    while G < 64 and 2.0 * (G // C) < nnz / max(rows, 1):
        G *= 2
    return G


def child(spec, launches, columns):
    """One shape, this process: the lines of its table on stdout as JSON."""
    import fasta_python_amd as fa
    from fasta_python_amd import hip
    sr = rows_probe()
    kind, n, arg = spec.split(":")
    n, arg = int(n), float(arg)
    S = sr.build(kind, n, arg)
    m, nnz = S.shape[0], int(S.nnz)
    lens = np.diff(S.indptr)
    tau = 1e-3
    rng = np.random.RandomState(0)
    lines = [f"{spec}: {m} x {n}, nnz {nnz} ({100.0 * nnz / (m * n):.4f} %), entries per row mean {lens.mean():.1f} max {lens.max()}"]

    def fmt(label, f, a, cols, note=""):
        fb = 12 * nnz + 8 * (m + 1) + (6 * n + 2 * m) * 8 * cols          # x0, g0, xacc0 in; xhat, xprox out; xprox gathered; b in, z out
        ab = 12 * nnz + 8 * (n + 1) + (4 * m + 5 * n) * 8 * cols          # z, b in, r out, r gathered; x0, xprox, xhat in; g1 out
        fm, am = float(np.median(f)), float(np.median(a))
        pair = fm + am
        rate = (fb + ab) / (pair * 1e-3)
        return pair, (f"  {label:14s} K-fwd {fm:7.3f} ms ({f.min():.3f}-{f.max():.3f})  K-adj {am:7.3f} ms ({a.min():.3f}-{a.max():.3f})  pair {pair:7.3f} ms  "
                      f"{(fb + ab) / 2**20:8.1f} MiB  {rate / 1e9:7.1f} GB/s = {100 * rate / PEAK:4.1f} %{note}")

    op = fa.SparseMatrixMap(S)
    c = op.ctx
    c.set_loss_lsq(rng.randn(m))
    c.set_prox(hip.PROX_SHRINK, 0.01)
    c.set_vector(hip.VEC_X0, rng.randn(n) * 0.01)
    c.init()
    f, a = sr.timed(c, hip, tau, launches)
    vpair, text = fmt("vector", f, a, 1, f"  G {lanes_per_row(nnz, m, 1)} / {lanes_per_row(nnz, n, 1)}")
    lines.append(text)
    op.close()
    per_col = {}
    for L in columns:
        LB = lb_of(L)
        op = fa.SparseMatrixMap(S, rhs=L)
        c = op.ctx
        c.set_loss_lsq(rng.randn(m, L))
        c.set_prox(hip.PROX_SHRINK, 0.01)
        c.set_vector(hip.VEC_X0, rng.randn(n, L) * 0.01)
        c.init()
        f, a = sr.timed(c, hip, tau, launches)
        pair, text = fmt(f"L = {L} (LB {LB})", f, a, LB, f"  G {lanes_per_row(nnz, m, LB // 2)} / {lanes_per_row(nnz, n, LB // 2)}"
                         f"  {pair / vpair:5.2f} x one vector pair, {L * vpair / pair:5.2f} x faster than {L} vector pairs, {pair / L:.3f} ms per column")
        per_col[L] = pair / L
        lines.append(text)
        op.close()
    print("SPARSE_COLUMNS " + json.dumps(dict(lines=lines)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparse_columns.txt"))
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--shapes", default=DEFAULT_SHAPES)
    ap.add_argument("--columns", default="1,2,4,8,16")
    ap.add_argument("--child", default=None)
    args = ap.parse_args()
    columns = [int(k) for k in args.columns.split(",")]
    if args.child:
        return child(args.child, args.launches, columns)
    lines = ["matrix unknowns on a sparse operator (csrc/fh_spmulti.h) against the vector sparse pair (csrc/fh_sparse.h), one process per shape, HIP events",
             f"median (min-max) of {args.launches} launches after 3 warm-up launches; bytes = 12 * nnz + 8 per row offset + the launch's vector traffic at LB columns (gathered operand counted once); % of 8 TB/s",
             "G = lanes per row of A / of A^T", ""]
    for spec in args.shapes.split(","):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", spec, "--launches", str(args.launches), "--columns", args.columns],
                           capture_output=True, text=True, timeout=1100)
        got = [ln for ln in r.stdout.splitlines() if ln.startswith("SPARSE_COLUMNS ")]
        if r.returncode != 0 or not got:
            lines += [f"{spec}: FAILED (exit status {r.returncode})", r.stderr[-2000:], ""]
            print("\n".join(lines[-3:]))
            raise SystemExit(1)                       # nothing more is started on the device after a failed step
        rec = json.loads(got[0][len("SPARSE_COLUMNS "):])
        lines += rec["lines"] + [""]
        print("\n".join(rec["lines"]), flush=True)
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

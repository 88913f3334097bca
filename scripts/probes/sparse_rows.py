"""What do the sparse-operator kernels (csrc/fh_sparse.h) sustain?  K-fwd (prologue + gather over A), K-adj (residual launch + gather over A^T)
and the pair, per shape in a process of its own: HIP-event time -- median, min and max of `--launches` launches after a warm-up -- the
bytes the launch has to move (12 per stored entry: 8 value + 4 index; 8 per row offset; the launch's vector traffic, every gathered operand
counted ONCE) over that time, against the 8 TB/s of the data sheet.  In the 65536^2 process the unchanged dense vector pair
k_fwd_dense / k_adj_dense runs on a 65536^2 dense matrix for comparison.  Registers of every instantiation at the end.

    python scripts/probes/sparse_rows.py [--out profiles/sparse_rows.txt] [--launches 30] [--shapes uniform:65536:0.001,...]

Matrices: `uniform:n:density` -- every row holds round(density * n) entries, one column drawn from each of that many equal stretches of the
row; `perrow:n:k` -- the same with k entries per row; `powerlaw:n:k` -- row lengths from a Pareto law (shape 1.2) scaled to about k * n entries
in all, columns uniform; `powerlaw_t:n:k` -- its transpose (the long rows are on the A^T copy).  For every shape the pair is timed a second
and third time with the streaming loads of values and indices forced plain / non-temporal (FH_TUNE_NT_LOADS = 0 / 1): plain is the default because of these rows.  Values standard normal, all from seeded generators.
"""
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
DEFAULT_SHAPES = "uniform:65536:0.001,uniform:65536:0.01,uniform:65536:0.05,perrow:1048576:16,powerlaw:1048576:16,powerlaw_t:1048576:16"


def registers():
    """{kernel: (VGPRs, AGPRs, scratch bytes per lane, waves per SIMD)} of the instantiations in fh_sparse_part.hip"""
    csrc = os.path.join(ROOT, "fasta_python_amd", "csrc")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-unused-function", "-c", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", "-o", os.devnull, "fh_sparse_part.hip"], cwd=csrc, capture_output=True, text=True)
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
    return {k: v for k, v in out.items() if "k_sp_" in k}


def lanes_per_row(nnz, rows):
    """The host's choice of G (csrc/fasta_hip.hip: sp_upload_side): the smallest of 4..64 with 2 G >= the mean row length."""
    G = 4
    while G < 64 and 2.0 * G < nnz / max(rows, 1):
        G *= 2
    return G


def build(kind, n, arg, seed=5):
    from scipy import sparse as sp
    rng = np.random.RandomState(seed)
    if kind in ("uniform", "perrow"):
        k = max(1, int(round(arg * n))) if kind == "uniform" else int(arg)
        stretch = n // k
        cols = (rng.randint(0, stretch, size=(n, k), dtype=np.int32) + (np.arange(k, dtype=np.int32) * stretch)).ravel()
        return sp.csr_matrix((rng.standard_normal(n * k), cols, np.arange(n + 1, dtype=np.int64) * k), shape=(n, n))
    raw = rng.pareto(1.2, size=n) + 1.0
    lens = np.clip(np.round(raw * (arg * n / raw.sum())), 1, n // 4).astype(np.int64)
    rows = np.repeat(np.arange(n, dtype=np.int32), lens)
    S = sp.coo_matrix((rng.standard_normal(rows.size), (rows, rng.randint(0, n, size=rows.size, dtype=np.int32))), shape=(n, n)).tocsr()
    S.sum_duplicates()
    S.sort_indices()
    if kind == "powerlaw_t":
        S = S.T.tocsr()
        S.sort_indices()
    return S


def long_threshold(nnz, rows):
    """Entries beyond which a row gets a workgroup of its own (sp_upload_side): max(64 G, 16 mean rows)."""
    return max(64 * lanes_per_row(nnz, rows), int(16.0 * nnz / max(rows, 1)))


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
    """One shape, this process: the lines of its table on stdout as JSON."""
    import fasta_python_amd as fa
    from fasta_python_amd import hip
    kind, n, arg = spec.split(":")
    n, arg = int(n), float(arg)
    S = build(kind, n, arg)
    m, nnz = S.shape[0], int(S.nnz)
    lens, clens = np.diff(S.indptr), np.bincount(S.indices, minlength=n)
    tau = 1e-3
    rng = np.random.RandomState(0)
    lines = [f"{spec}: {m} x {n}, nnz {nnz} ({100.0 * nnz / (m * n):.4f} %), entries per row mean {lens.mean():.1f} max {lens.max()}, per column max {clens.max()}; "
             f"G = {lanes_per_row(nnz, m)} lanes per row of A, {lanes_per_row(nnz, n)} per row of A^T; "
             f"rows with a workgroup of their own: {int((lens > long_threshold(nnz, m)).sum())} of A, {int((clens > long_threshold(nnz, n)).sum())} of A^T"]
    op = fa.SparseMatrixMap(S)
    c = op.ctx
    c.set_loss_lsq(rng.randn(m))
    c.set_prox(hip.PROX_SHRINK, 0.01)
    c.set_vector(hip.VEC_X0, rng.randn(n) * 0.01)
    c.init()
    f, a = timed(c, hip, tau, launches)
    fb = 12 * nnz + 8 * (m + 1) + (6 * n + 2 * m) * 8          # x0, g0, xacc0 in; xhat, xprox out; xprox gathered; b in, z out
    ab = 12 * nnz + 8 * (n + 1) + (4 * m + 5 * n) * 8          # z, b in, r out, r gathered; x0, xprox, xhat in; g1 out (+ x1 when accelerating)
    lines.append(row("sparse K-fwd", f, fb))
    lines.append(row("sparse K-adj", a, ab))
    pair = float(np.median(f) + np.median(a))
    lines.append(f"  sparse pair {pair:.3f} ms: {(fb + ab) / (pair * 1e-3) / 1e9:.1f} GB/s = {100 * (fb + ab) / (pair * 1e-3) / PEAK:.1f} % of 8 TB/s")
    for nt in (0, 1):
        c.set_tuning(hip.TUNE_NT_LOADS, nt)
        f2, a2 = timed(c, hip, tau, launches)
        lines.append(f"  {'non-temporal' if nt else 'plain':12s} streaming loads: K-fwd {np.median(f2):.3f} ms, K-adj {np.median(a2):.3f} ms, pair {np.median(f2) + np.median(a2):.3f} ms"
                     + ("" if nt else "   <- the default"))
    op.close()
    verdict = None
    if kind == "uniform" and n == 65536 and abs(arg - 0.01) < 1e-12:
        dop = fa.DenseMatrixMap.synthetic(n, n, seed=3, scale=1.0 / 128)
        d = dop.ctx
        d.set_loss_lsq(rng.randn(n))
        d.set_prox(hip.PROX_SHRINK, 0.01)
        d.set_vector(hip.VEC_X0, rng.randn(n) * 0.01)
        d.init()
        df, da = timed(d, hip, tau, launches)
        A8 = n * n * 8
        lines.append(row("dense k_fwd_dense", df, A8 + (4 * n + 2 * n) * 8))
        lines.append(row("dense k_adj_dense", da, A8 + (2 * n + 4 * n) * 8))
        dpair = float(np.median(df) + np.median(da))
        verdict = pair < dpair
        lines.append(f"  dense vector pair {dpair:.3f} ms; the sparse pair at 1 % density moves {100.0 * (fb + ab) / (2 * A8):.2f} % of its bytes in {100.0 * pair / dpair:.2f} % of its time"
                     f" -- {'FASTER' if verdict else 'NOT FASTER'} than the dense pair ({dpair / pair:.1f} x)")
        dop.close()
    print("SPARSE_ROWS " + json.dumps(dict(lines=lines, verdict=verdict)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparse_rows.txt"))
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--shapes", default=DEFAULT_SHAPES)
    ap.add_argument("--child", default=None)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.launches)
    lines = ["sparse-operator kernels (csrc/fh_sparse.h), one process per shape, HIP events",
             f"median (min, max) of {args.launches} launches after 3 warm-up launches; bytes = 12 * nnz + 8 per row offset + the launch's vector traffic (gathered operand counted once)", ""]
    verdict = None
    for spec in args.shapes.split(","):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", spec, "--launches", str(args.launches)], capture_output=True, text=True, timeout=900)
        got = [ln for ln in r.stdout.splitlines() if ln.startswith("SPARSE_ROWS ")]
        if r.returncode != 0 or not got:
            lines += [f"{spec}: FAILED (exit status {r.returncode})", r.stderr[-2000:], ""]
            print("\n".join(lines[-3:]))
            raise SystemExit(1)                       # nothing more is started on the device after a failed step
        rec = json.loads(got[0][len("SPARSE_ROWS "):])
        lines += rec["lines"] + [""]
        print("\n".join(rec["lines"]), flush=True)
        if rec["verdict"] is not None:
            verdict = rec["verdict"]
    lines.append("registers of the instantiations (VGPRs, AGPRs, scratch bytes per lane, waves per SIMD):")
    for k, v in sorted(registers().items()):
        lines.append(f"  {k:36s} {v.get('v', 0):4d} {v.get('a', 0):4d} {v.get('s', 0):4d} {v.get('o', 0):2d}")
    if verdict is not None:
        lines += ["", f"condition (65536^2, 1 %: sparse pair faster than the dense vector pair of the same run): {'HOLDS' if verdict else 'FAILS'}"]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    print(text)
    if verdict is False:
        raise SystemExit(2)


if __name__ == "__main__":
    main()

"""What does an attempt of the step cost with the bilinear smooth term (csrc/fh_bilinear.h)?  Per shape (m, n, K), in a process of its own:
HIP-event time -- median, min and max of `--launches` launches after a warm-up -- of
  fh_fwd, value and gradient   = k_bl_prologue + k_bl_pass<GRAD = 1>   (what an adaptive / plain attempt launches: ONE read of S)
  fh_fwd, value alone          = k_bl_prologue + k_bl_pass<GRAD = 0>   (what an accelerated attempt launches first)
  fh_adj, plain                = k_bl_grad                             (elementwise: the partial reduction and the n-side sums; never reads S)
  fh_adj, accelerated          = k_bl_extrap + k_bl_pass<1> + k_bl_grad (the second pass, at the extrapolated point)
and the per-attempt totals.  The yardsticks are taken in the same process: fh_stream_read_ms over the same bytes, and fh_fwd of the unchanged
multi-column dense form (k_mc_prologue + k_mc_fwd, csrc/fh_multi.h) on an A of S's shape with L = K.
Per row: achieved bytes / s on m * n * 8 plus the partials the launch writes or reads, against the 8 TB/s of the data sheet, and for the
passes flop / s on 6 K m n (value alone: 2 K m n + 2 m n), against the FP64 vector peak of 78.6 Tflop/s (half the FP32 vector rate of
157.3 Tflop/s the data sheet gives).  Reported, not gated.

    python scripts/probes/factor_sizes.py [--out profiles/factor_sizes.txt] [--launches 30] [--shapes 16384x16384,32768x32768,65536x4096]
                                          [--columns 1,2,4,8,10,16]

Timing only: run it under a profiler's kernel trace, if at all, separately from any counter collection."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
PEAK_BW = 8.0e12            # bytes per second, data sheet
PEAK_F64 = 78.6e12          # flop per second, FP64 vector, data sheet


def timed(c, launches, prepare, call, kernel):
    for _ in range(3):
        prepare()
        call()
    c.timing_enable(True)
    ms = []
    for _ in range(launches):
        prepare()
        c.timing_reset()
        call()
        ms.append(c.timing_get(kernel)[0])
    c.timing_enable(False)
    return np.array(ms)


def child(m, n, K, launches):
    """One shape, this process: the lines of its table on stdout as JSON."""
    import fasta_python_amd as fa
    from fasta_python_amd import hip
    rng = np.random.RandomState(0)
    S = np.add.outer(rng.rand(m), rng.rand(n))        # (the values do not matter to a stream)
    Z0 = np.concatenate((rng.rand(m, K) * (rng.rand(m, K) > 0.75), rng.rand(n, K)))
    tau = 1e-6
    mat = m * n * 8

    def row(label, ms, nbytes, flops=0.0, note=""):
        med = float(np.median(ms))
        rate = nbytes / (med * 1e-3)
        text = f"  {label:50s} {med:8.4f} ms ({ms.min():.4f}-{ms.max():.4f})  {nbytes / 2**20:9.1f} MiB  {rate / 1e9:7.1f} GB/s = {100 * rate / PEAK_BW:4.1f} %"
        if flops:
            fr = flops / (med * 1e-3)
            text += f"  {fr / 1e12:6.2f} Tflop/s = {100 * fr / PEAK_F64:4.1f} % of FP64 vector peak"
        return med, text + note

    c = hip.HipContext(0)
    c.set_factorization(S, K)
    del S
    sh = c.bilinear_shape()
    part = sh.gx_bytes + sh.gy_bytes
    vec = (m + n) * sh.LB * 8
    lines = [f"S {m} x {n}, K = {K} (LB {sh.LB}): S {mat / 2**30:.2f} GiB, k_bl_pass<{sh.LB}, ., {sh.NT}> on {sh.grid} workgroups, {sh.row_panels} panels of "
             f"{sh.tile_rows} rows x {sh.col_tiles} tiles of {sh.tile_cols} columns, {sh.tiles_max} tiles per workgroup; partials {part / 2**20:.1f} MiB = "
             f"{100 * part / mat:.2f} % of S (the rule promises LB (1/512 + 1/PR) = {100 * sh.LB * (1 / 512 + 1 / sh.tile_rows):.2f} %); elementwise launches of {sh.nelem} workgroups"]
    c.set_prox_split(m, hip.PROX_SHRINK, 1.0, 0.0, 0.0, hip.PROX_BOX, 0.0, 1.0)
    c.set_vector(hip.VEC_X0, Z0)
    c.init()
    nothing = lambda: None
    fg = timed(c, launches, lambda: c.adj(tau), lambda: c.fwd(tau), hip.K_FWD)                                  # (a plain adjoint launch before: the next pass takes the gradient)
    fv = timed(c, launches, lambda: c.adj(tau, accel=True, coef=0.5), lambda: c.fwd(tau), hip.K_FWD)            # (an accelerated one before: value alone)
    c.fwd(tau)
    ap = timed(c, launches, lambda: (c.adj(tau), c.fwd(tau)), lambda: c.adj(tau), hip.K_ADJ)
    aa = timed(c, launches, nothing, lambda: c.adj(tau, accel=True, coef=0.5), hip.K_ADJ)
    fgm, text = row("fh_fwd: k_bl_prologue + k_bl_pass, value and gradient", fg, mat + part + 5 * vec, 6.0 * K * m * n)
    lines.append(text)
    fvm, text = row("fh_fwd: k_bl_prologue + k_bl_pass, value alone", fv, mat + 5 * vec, 2.0 * K * m * n + 2.0 * m * n)
    lines.append(text)
    apm, text = row("fh_adj plain: k_bl_grad (partials summed, n-side sums)", ap, part + 4 * vec)
    lines.append(text)
    aam, text = row("fh_adj accelerated: k_bl_extrap + k_bl_pass + k_bl_grad", aa, mat + 2 * part + 8 * vec, 6.0 * K * m * n)
    lines.append(text)
    lines.append(f"  {'attempt, adaptive / plain: fh_fwd(gradient) + fh_adj':50s} {fgm + apm:8.4f} ms")
    lines.append(f"  {'attempt, accelerated: fh_fwd(value) + fh_adj(accel)':50s} {fvm + aam:8.4f} ms")
    c.close()
    op = fa.DenseMatrixMap.synthetic(m, n, seed=1, scale=1.0, rhs=K)
    d = op.ctx
    sms, sbytes = d.stream_read_ms(launches)
    lines.append(f"  {'yardstick fh_stream_read_ms':50s} {sms:8.4f} ms per pass  {sbytes / 2**20:9.1f} MiB  {sbytes / (sms * 1e-3) / 1e9:7.1f} GB/s = {100 * sbytes / (sms * 1e-3) / PEAK_BW:4.1f} %")
    d.set_loss_lsq(np.zeros((m, K)))
    d.set_prox(hip.PROX_BOX, 0.0, 0.0, 1.0)
    d.set_vector(hip.VEC_X0, Z0[m:])
    d.init()
    y = timed(d, launches, nothing, lambda: d.fwd(tau), hip.K_FWD)
    ym, text = row("yardstick fh_fwd: k_mc_prologue + k_mc_fwd, L = K", y, mat + (5 * n + 2 * m) * sh.LB * 8, 2.0 * K * m * n)
    lines.append(text)
    spread = float(y.max() - y.min())
    for label, v in (("value and gradient", fgm), ("value alone", fvm)):
        verdict = "within" if abs(v - ym) <= spread else ("SLOWER than the yardstick by more than" if v > ym else "faster than the yardstick by more than")
        lines.append(f"  fh_fwd ({label}) - yardstick = {v - ym:+.4f} ms ({v / ym:.2f} x): {verdict} the yardstick's own min-max spread of {spread:.4f} ms")
    op.close()
    print("FACTOR_SIZES " + json.dumps(dict(lines=lines)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "factor_sizes.txt"))
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--shapes", default="16384x16384,32768x32768,65536x4096")
    ap.add_argument("--columns", default="1,2,4,8,10,16")
    ap.add_argument("--child", default=None)
    args = ap.parse_args()
    if args.child:
        m, n, K = (int(k) for k in args.child.split(":"))
        return child(m, n, K, args.launches)
    lines = ["bilinear smooth term (csrc/fh_bilinear.h) against the stream-read ceiling and the multi-column dense K-fwd (csrc/fh_multi.h), one MI355X, one process per shape, HIP events",
             f"median (min-max) of {args.launches} launches after 3 warm-up launches; bytes = m * n * 8 + the partials and vectors the launch moves; % of 8 TB/s; "
             "flop = 6 K m n (value alone: 2 K m n + 2 m n); % of 78.6 Tflop/s", ""]
    status = 0
    for shape in args.shapes.split(","):
        m, n = (int(k) for k in shape.split("x"))
        for K in (int(k) for k in args.columns.split(",")):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", f"{m}:{n}:{K}", "--launches", str(args.launches)],
                               capture_output=True, text=True, timeout=600)
            got = [ln for ln in r.stdout.splitlines() if ln.startswith("FACTOR_SIZES ")]
            if r.returncode != 0 or not got:
                lines += [f"S {m} x {n}, K = {K}: FAILED (exit status {r.returncode})", r.stderr[-2000:], ""]
                print("\n".join(lines[-3:]))
                status = 1                            # nothing more is started on the device after a failed step
                break
            rec = json.loads(got[0][len("FACTOR_SIZES "):])
            lines += rec["lines"] + [""]
            print("\n".join(rec["lines"]), flush=True)
        if status:
            break
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    raise SystemExit(status)


if __name__ == "__main__":
    main()

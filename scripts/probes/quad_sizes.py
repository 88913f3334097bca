"""What does an attempt of the step cost with a quadratic smooth term (csrc/fh_quad.h)?  Per shape (n, L), in a process of its own: HIP-event
time -- median, min and max of `--launches` launches after a warm-up -- of
  fh_fwd   = k_qd_prologue + k_qd_fwd   (the prox, then W = Q xprox and the loss: the ONE read of Q an attempt costs)
  fh_apply = k_mc_pack + k_qd_fwd       (the product alone; fh_fwd minus this is what the prologue adds over a pack launch)
  fh_adj   = k_qd_grad                  (the second direction: elementwise, never reads Q)
and, in the same process, the yardstick: fh_fwd of the unchanged multi-column dense form (k_mc_prologue + k_mc_fwd, csrc/fh_multi.h) on an
(n, n) matrix with the same L -- the same streaming loop, so equality is the expectation.  Bytes: n^2 * 8 for the matrix plus the launch's
vector traffic at LB columns per row, over the time, against the 8 TB/s of the data sheet.  Reported, not gated.

    python scripts/probes/quad_sizes.py [--out profiles/quad_sizes.txt] [--launches 30] [--sizes 16384,32768] [--columns 1,2,4,8,10,16]

Timing only: run it under a profiler's kernel trace, if at all, separately from any counter collection."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
PEAK = 8.0e12            # bytes per second, data sheet


def lb_of(L):
    return 2 if L <= 2 else 4 if L <= 4 else 8 if L <= 8 else 16


def timed(c, hip, launches, call, kernel):
    for _ in range(3):
        call()
    c.timing_enable(True)
    ms = []
    for _ in range(launches):
        c.timing_reset()
        call()
        ms.append(c.timing_get(kernel)[0])
    c.timing_enable(False)
    return np.array(ms)


def child(n, L, launches):
    """One shape, this process: the lines of its table on stdout as JSON."""
    import fasta_python_amd as fa
    from fasta_python_amd import hip
    LB = lb_of(L)
    rng = np.random.RandomState(0)
    v = rng.randn(n) / n
    Q = np.add.outer(v, v)                            # exactly symmetric (a + b == b + a); the values do not matter to a stream
    X0, cvec = rng.randn(n, L) * 0.01, rng.randn(n, L)
    tau = 1e-3
    mat = n * n * 8

    def row(label, ms, nbytes, note=""):
        med = float(np.median(ms))
        rate = nbytes / (med * 1e-3)
        return med, f"  {label:44s} {med:8.4f} ms ({ms.min():.4f}-{ms.max():.4f})  {nbytes / 2**20:9.1f} MiB  {rate / 1e9:7.1f} GB/s = {100 * rate / PEAK:4.1f} %{note}"

    lines = [f"n = {n}, L = {L} (LB {LB}): Q {mat / 2**30:.2f} GiB"]
    c = hip.HipContext(0)
    c.set_quadratic(Q, cvec, L)
    sh = c.quad_shape()
    lines[0] += f", k_qd_fwd<{sh.LB}, {sh.CH}, {sh.R}, {sh.NT}> on {sh.fwd_grid} workgroups, {sh.ntrip} trips, {sh.pass_max} passes; elementwise launches of {sh.ngrad} workgroups"
    c.set_prox(hip.PROX_BOX, 0.0, -0.005, 0.005)
    c.set_vector(hip.VEC_X0, X0)
    c.init()
    vec = n * LB * 8
    f = timed(c, hip, launches, lambda: c.fwd(tau), hip.K_FWD)
    a = timed(c, hip, launches, lambda: c.adj(tau), hip.K_ADJ)
    p = timed(c, hip, launches, lambda: c.apply(X0), hip.K_FWD)
    fm, text = row("fh_fwd: k_qd_prologue + k_qd_fwd", f, mat + 9 * vec)          # x0, g0, xacc0 in; xhat, xprox, xs out; xs, xprox, c in; w out
    lines.append(text)
    pm, text = row("fh_apply: k_mc_pack + k_qd_fwd (no loss)", p, mat + 4 * vec)
    lines.append(text)
    am, text = row("fh_adj: k_qd_grad", a, 6 * vec)                                # w, c, x0, xprox, xhat in; g1 out
    lines.append(text)
    lines.append(f"  {'prologue over a pack launch (difference)':44s} {fm - pm:8.4f} ms")
    lines.append(f"  {'attempt: fh_fwd + fh_adj':44s} {fm + am:8.4f} ms")
    c.close()
    del Q
    op = fa.DenseMatrixMap.synthetic(n, n, seed=1, scale=1.0, rhs=L)
    d = op.ctx
    d.set_loss_lsq(cvec)
    d.set_prox(hip.PROX_BOX, 0.0, -0.005, 0.005)
    d.set_vector(hip.VEC_X0, X0)
    d.init()
    y = timed(d, hip, launches, lambda: d.fwd(tau), hip.K_FWD)
    ym, text = row("yardstick fh_fwd: k_mc_prologue + k_mc_fwd", y, mat + 9 * vec)
    lines.append(text)
    spread = float(y.max() - y.min())
    verdict = "within" if abs(fm - ym) <= spread else ("SLOWER than the yardstick by more than" if fm > ym else "faster than the yardstick by more than")
    lines.append(f"  fh_fwd - yardstick = {fm - ym:+.4f} ms: {verdict} the yardstick's own min-max spread of {spread:.4f} ms")
    op.close()
    print("QUAD_SIZES " + json.dumps(dict(lines=lines)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quad_sizes.txt"))
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--sizes", default="16384,32768")
    ap.add_argument("--columns", default="1,2,4,8,10,16")
    ap.add_argument("--child", default=None)
    args = ap.parse_args()
    if args.child:
        n, L = (int(k) for k in args.child.split(":"))
        return child(n, L, args.launches)
    lines = ["quadratic smooth term (csrc/fh_quad.h) against the multi-column dense K-fwd (csrc/fh_multi.h), one MI355X, one process per shape, HIP events",
             f"median (min-max) of {args.launches} launches after 3 warm-up launches; bytes = n^2 * 8 + the launch's vector traffic at LB columns per row; % of 8 TB/s", ""]
    for n in (int(k) for k in args.sizes.split(",")):
        for L in (int(k) for k in args.columns.split(",")):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", f"{n}:{L}", "--launches", str(args.launches)],
                               capture_output=True, text=True, timeout=600)
            got = [ln for ln in r.stdout.splitlines() if ln.startswith("QUAD_SIZES ")]
            if r.returncode != 0 or not got:
                lines += [f"n = {n}, L = {L}: FAILED (exit status {r.returncode})", r.stderr[-2000:], ""]
                print("\n".join(lines[-3:]))
                raise SystemExit(1)                   # nothing more is started on the device after a failed step
            rec = json.loads(got[0][len("QUAD_SIZES "):])
            lines += rec["lines"] + [""]
            print("\n".join(rec["lines"]), flush=True)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()

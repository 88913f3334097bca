"""What does the softmax loss (csrc/fh_softmax.h) add to an iteration over the least-squares loss on the SAME operator, shape and prox?  It adds
two short m-side launches per iteration (the row pass behind K-fwd, value only; the row pass in front of K-adj, plus a one-workgroup launch
behind the dense K-adj) and about 5 * mv * LB * 8 bytes, against one read of A per direction.  Per shape, in a process of its own, on ONE
context whose loss is switched: HIP-event time of the K-fwd + K-adj pair (fh_fwd_adj: FH_K_FWD + FH_K_ADJ, which bracket every launch of a
direction) and the wall clock of one iteration as the separate-launch loop issues it (fh_fwd, fh_adj, fh_commit) -- median, min and max of
`--pairs` after a warm-up -- for losses.LeastSquares first, losses.SoftmaxLoss second.  Reported, not gated; no ratio is fixed in advance.

    python scripts/probes/softmax_sizes.py [--out profiles/softmax_sizes.txt] [--pairs 30]

Shapes: dense 16384^2 x {4, 16} columns (synthetic matrix generated in HBM); sparse 65536^2 with 16 entries per row x 8 columns.
Timing only: run it under a profiler's kernel trace, if at all, separately from any counter collection."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
SHAPES = ["dense:16384:4", "dense:16384:16", "sparse:65536:8"]


def lb_of(L):
    return 2 if L <= 2 else 4 if L <= 4 else 8 if L <= 8 else 16


def measure(c, hip, pairs, tau):
    """(pair ms by HIP events, iteration ms by the wall clock), `pairs` samples each after 3 warm-up rounds"""
    for _ in range(3):
        c.fwd_adj(tau)
    c.timing_enable(True)
    ev = []
    for _ in range(pairs):
        c.timing_reset()
        c.fwd_adj(tau)
        ev.append(c.timing_get(hip.K_FWD)[0] + c.timing_get(hip.K_ADJ)[0])
    c.timing_enable(False)
    wall = []
    for k in range(pairs + 3):
        t0 = time.perf_counter()
        c.fwd(tau)
        c.adj(tau)
        c.commit(False)
        wall.append((time.perf_counter() - t0) * 1e3)
    return np.array(ev), np.array(wall[3:])


def child(kind, n, L, pairs):
    import fasta_python_amd as fa
    from fasta_python_amd import hip
    rng = np.random.RandomState(0)
    if kind == "dense":
        op = fa.DenseMatrixMap.synthetic(n, n, seed=1, scale=1.0, rhs=L)
        what = f"dense {n} x {n}, L = {L} (LB {lb_of(L)}): A {n * n * 8 / 2**30:.2f} GiB"
    else:
        from scipy import sparse as sp
        offs = np.sort(rng.permutation(n)[:16])
        idx = (np.arange(n)[:, None] + offs[None, :]) % n
        idx.sort(axis=1)
        S = sp.csr_matrix((rng.randn(n * 16), idx.ravel().astype(np.int32), np.arange(0, n * 16 + 1, 16, dtype=np.int64)), shape=(n, n))
        op = fa.SparseMatrixMap(S, rhs=L)
        what = f"sparse {n} x {n}, 16 entries per row, L = {L} (LB {lb_of(L)}): {S.nnz * 12 / 2**20:.1f} MiB of index and value per direction"
    c = op.ctx
    X0 = rng.randn(n, L) * (0.01 if kind == "dense" else 0.1)
    tau, mu = 1e-6, 1e-3                                   # (a step well inside 2 / ||A||^2 for both operators: the iterates stay finite)
    m_side = n * lb_of(L) * 8
    lines = [what + f"; one (mv, LB) m-side matrix {m_side / 2**20:.1f} MiB"]
    med = {}
    for name, bind in (("LeastSquares", lambda: c.set_loss_lsq(rng.randn(n, L))), ("SoftmaxLoss", lambda: c.set_loss_softmax(rng.randint(0, L, n)))):
        bind()
        c.set_prox(hip.PROX_GROUP, mu)
        c.set_vector(hip.VEC_X0, X0)
        c.init()
        ev, wall = measure(c, hip, pairs, tau)
        med[name] = (float(np.median(ev)), float(np.median(wall)))
        lines.append(f"  {name:13s} K-fwd + K-adj pair {np.median(ev):8.4f} ms ({ev.min():.4f}-{ev.max():.4f})   iteration (fwd, adj, commit) {np.median(wall):8.4f} ms ({wall.min():.4f}-{wall.max():.4f})")
    (pl, il), (ps, is_) = med["LeastSquares"], med["SoftmaxLoss"]
    lines.append(f"  softmax - least squares: pair {ps - pl:+.4f} ms = {100 * (ps / pl - 1):+.1f} %, iteration {is_ - il:+.4f} ms = {100 * (is_ / il - 1):+.1f} %")
    op.close()
    print("SOFTMAX_SIZES " + json.dumps(dict(lines=lines)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "softmax_sizes.txt"))
    ap.add_argument("--pairs", type=int, default=30)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--child", default=None)
    args = ap.parse_args()
    if args.child:
        kind, n, L = args.child.split(":")
        return child(kind, int(n), int(L), args.pairs)
    lines = ["softmax loss (csrc/fh_softmax.h) against least squares on the same operator, shape and prox (GroupShrink), one MI355X, one process per shape",
             f"median (min-max) of {args.pairs} samples after 3 warm-up rounds; pair: HIP events around every launch of the two directions (fh_fwd_adj); iteration: wall clock of fh_fwd, fh_adj, fh_commit", ""]
    for shape in args.shapes.split(","):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", shape, "--pairs", str(args.pairs)], capture_output=True, text=True, timeout=300)
        got = [ln for ln in r.stdout.splitlines() if ln.startswith("SOFTMAX_SIZES ")]
        if r.returncode != 0 or not got:
            lines += [f"{shape}: FAILED (exit status {r.returncode})", r.stderr[-2000:], ""]
            print("\n".join(lines[-3:]))
            raise SystemExit(1)                       # nothing more is started on the device after a failed step
        rec = json.loads(got[0][len("SOFTMAX_SIZES "):])
        lines += rec["lines"] + [""]
        print("\n".join(rec["lines"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

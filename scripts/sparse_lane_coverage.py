#!/usr/bin/env python3
"""Which instantiation of the sparse gather kernels each GPU test reaches, as a table: (G, LB) x direction x mode for the matrix form
(csrc/fh_spmulti.h), G x direction x mode for the vector form (csrc/fh_sparse.h).  Host-only: the matrices of the GPU tests are rebuilt on
the CPU and put through the host's rule as tests/sparse_lanes.py:lanes_of restates it (the GPU tests themselves ask the library:
fh_sparse_lanes).  "before": tests/test_gpu_sparse.py and tests/test_gpu_sparse_mmv.py; "after": with tests/test_gpu_sparse_lanes.py.

    python scripts/sparse_lane_coverage.py            # markdown on stdout

Modes: `apply A` / `apply A^T` (fh_apply: the plain gather), `fwd` (a step's K-fwd on the A copy: prologue, gather, loss terms,
finaliser), `adj` (the mode-0 K-adj on the A^T copy: owner-lane epilogue, Barzilai-Borwein sums, x1), `adj+group` (the same with
FH_PROX_GROUP: the row norm over the column lanes)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scipy import sparse as sp                       # noqa: E402

from tests import sparse_lanes as SL                 # noqa: E402
from tests import test_gpu_sparse as TV              # noqa: E402
from tests import test_gpu_sparse_mmv as TM          # noqa: E402

MODES = ("apply A", "apply A^T", "fwd", "adj", "adj+group")


def reach(table, S, LB, modes, group=False):
    a, at = SL.both_lanes(sp.csr_matrix(S), LB)
    for mode in modes:
        if mode == "step":
            table.add((a.G, LB, "fwd"))
            table.add((at.G, LB, "adj"))
            if group:
                table.add((at.G, LB, "adj+group"))
        else:
            table.add(((a if mode == "apply A" else at).G, LB, mode))


def existing():
    """Every matrix the two existing GPU files put on the device, with what they run on it."""
    t = set()
    both = ("apply A", "apply A^T")
    # vector form (tests/test_gpu_sparse.py)
    for make in TV.APPLY.values():
        reach(t, make(), 0, both)
    reach(t, TV.random_sparse(3000, 2000, 0.01, 21), 0, both)
    for kind, matrix in (("shrink", "uniform"), ("shrink", "long_col"), ("shrink", "long_both")):
        reach(t, TV.STEP_MATRICES[matrix](), 0, ("step",))
    reach(t, TV.random_sparse(40, 1003, 0.05, 18), 0, ("step",))
    for name in TV.CASES:
        reach(t, TV.capture_script().matrix_of(TV.load(name)[2]), 0, ("step",))
    reach(t, TV.long_both() * 0.05, 0, ("step",))
    reach(t, TV.random_sparse(400, 300, 0.05, 23), 0, both)
    reach(t, TV.random_sparse(64, 96, 0.1, 31), 0, both)
    reach(t, TV.banded_random(1 << 20, 16, 41), 0, ("step",))
    reach(t, TV.random_sparse(600, 1200, 0.02, 0), 0, ("step",))          # the example's matrix (examples/sparse_design.py: seed 0)
    # matrix form (tests/test_gpu_sparse_mmv.py)
    for make in TM.SMALL.values():
        for L in TM.ALL_L:
            reach(t, make(), SL.lb_of(L), both)
    for make in TM.LARGE.values():
        for L in (2, 16):
            reach(t, make(), SL.lb_of(L), both)
    for L in (3, 4, 5, 8):
        reach(t, TV.random_sparse(203, 1001, 0.02, 3), SL.lb_of(L), both)
    reach(t, TV.long_both(), 8, both)
    reach(t, TV.banded_random(1 << 18, 16, 41), 4, both)
    reach(t, TV.random_sparse(64, 96, 0.1, 31), 4, both + ("fwd",))
    a = SL.both_lanes(TV.random_sparse(40, 403, 0.05, 18), 8)[0]
    t.add((a.G, 8, "fwd"))
    for L, kind, matrix in [(5, "group", "uniform"), (16, "group", "uniform"), (3, "shrink", "uniform"), (2, "nonneg", "uniform"), (9, "box", "uniform"),
                            (1, "none", "uniform"), (8, "group", "long_both"), (2, "shrink", "long_both")]:
        reach(t, TM.STEP_MATRICES[matrix](), SL.lb_of(L), ("step",), group=kind == "group")
    for name in TM.CASES:
        meta, z, d = TM.load(name)
        reach(t, TM.capture_script().matrix_of(d), SL.lb_of(d["B"].shape[1]), ("step",), group=meta["kind"] == "mmv")
    reach(t, TV.capture_script().matrix_of(TV.load("lasso_200x400_adaptive")[2]), 8, ("step",), group=True)
    reach(t, TV.random_sparse(200, 300, 0.05, 0), 8, ("step",), group=True)       # the example's matrix (examples/sparse_mmv.py: seed 0)
    return t


def added():
    t = set()
    both = ("apply A", "apply A^T")
    for G, LB, L in SL.apply_cases():
        reach(t, SL.exact_matrix(G, LB), LB, both)
    for G, LB, L, kind in SL.step_cases():
        reach(t, SL.exact_matrix(G, LB), LB, ("step",))
    for G, LB, L in SL.group_cases():
        reach(t, SL.exact_matrix(G, LB), LB, ("step",), group=True)
    for LB in (0,) + SL.ALL_LB:
        reach(t, SL.long_matrix(LB), LB, both + ("step",), group=LB > 0)
    for LB in (0, 2, 16):
        reach(t, SL.staircase(), LB, both + ("step",))
    return t


def table(before, after):
    rows = ["| form | G | LB | " + " | ".join(MODES) + " |", "|---|---|---|" + "---|" * len(MODES)]
    counts = {m: [0, 0, 0] for m in MODES}
    for G, LB in [(G, 0) for G in SL.VECTOR_G] + SL.PAIRS:
        cells = []
        for mode in MODES:
            if LB == 0 and mode == "adj+group":
                cells.append("n/a")
                continue
            b, a = (G, LB, mode) in before, (G, LB, mode) in after
            cells.append("before" if b else ("NEW" if a else "never"))
            if LB:
                counts[mode][0] += b
                counts[mode][1] += a or b
                counts[mode][2] += 1
        rows.append(f"| {'vector' if LB == 0 else 'matrix'} | {G} | {LB or '-'} | " + " | ".join(cells) + " |")
    rows.append("")
    rows.append("matrix form, pairs reached (before -> after, of 19): " + ", ".join(f"{m} {c[0]} -> {c[1]}" for m, c in counts.items()))
    return "\n".join(rows)


if __name__ == "__main__":
    before = existing()
    print(table(before, before | added()))

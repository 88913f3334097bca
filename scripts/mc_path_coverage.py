#!/usr/bin/env python3
"""Which loop of the multi-column dense kernels (csrc/fh_multi.h) each GPU test reaches, as a table: path x (LB, NT).  Host-only: every
shape a test puts on the device goes through the library's own launch rule in its pure form (fh_multi_shape_for, the function both
launchers call; the GPU tests themselves ask the context: fh_multi_shape) and tests/mc_paths.py:paths_of reads the loops off the geometry.
"before": the asserting tests of tests/test_gpu_mmv.py; "after": with tests/test_gpu_mc_paths.py.

    python scripts/mc_path_coverage.py            # markdown on stdout

Paths: `several stages` (a slab of k_mc_adj longer than the 2048 / LB rows staged at a time), `short last stage`, `ragged last slab`,
`ncc > 1` (more than one column chunk), `clamped chunk` (lanes of the last chunk past the row), `K-fwd second pass` (the grid-stride loop
of k_mc_fwd comes round), `uneven passes` (... for some workgroups once more than for others), `accelerated adjoint` (fh_adj with accel:
residual from the extrapolated Z, x1 written).  tests/test_gpu_mmv.py:test_eight_columns_cost_less_than_eight_vector_passes runs
16384^2 at LB = 8 but asserts only a time; it is not counted."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np                                   # noqa: E402

from fasta_python_amd import hip                     # noqa: E402
from tests import mc_paths as MC                     # noqa: E402
from tests import test_gpu_mmv as TM                 # noqa: E402

COLUMNS = [(LB, nt) for LB in MC.ALL_LB for nt in (0, 1)]


def reach(table, m, n, L, accel, slab=0, cap=0, nt=-1):
    sh = hip.multi_shape(m, n, L, slab, cap, nt)
    for path, yes in MC.paths_of(sh, m, n).items():
        if yes and path in MC.PATHS:
            table.add((sh.LB, sh.NT, path))
    if accel:
        table.add((sh.LB, sh.NT, "accelerated adjoint"))
    return sh


def existing():
    """Every shape tests/test_gpu_mmv.py compares against a reference, under the automatic rules."""
    t = set()
    for m, n in TM.APPLY_SHAPES:
        for L in (1, 2, 3, 5, 8, 9, 16):
            reach(t, m, n, L, accel=False)
    reach(t, 16400, 16390, 5, accel=False)
    for L in (5, 16, 3, 2, 9):
        reach(t, 96, 200, L, accel=True)                                  # test_single_step_scalars_match_numpy
    for name in TM.CASES:
        meta, z = TM.load(name)
        (m, n), L = z["in_A"].shape, z["in_B"].shape[1]
        reach(t, m, n, L, accel=bool(meta["options"].get("accelerate")))
    for L in (3, 8):
        reach(t, 120, 90, L, accel=False)                                 # test_columns_of_a_separable_problem_...
    reach(t, 40, 24, 4, accel=False)
    return t


def added():
    t = set()
    for c in MC.cases():
        for nt in (0, 1):
            reach(t, c.m, c.n, c.L, True, c.slab, c.cap, nt)
    return t


def table(before, after):
    rows = ["| path | " + " | ".join(f"LB {LB}, NT {nt}" for LB, nt in COLUMNS) + " |", "|---|" + "---|" * len(COLUMNS)]
    counts = np.zeros(3, dtype=int)
    for path in MC.PATHS:
        cells = []
        for LB, nt in COLUMNS:
            b, a = (LB, nt, path) in before, (LB, nt, path) in after
            cells.append("before" if b else ("NEW" if a else "never"))
            counts += (b, a or b, 1)
        rows.append(f"| {path} | " + " | ".join(cells) + " |")
    rows.append("")
    rows.append(f"cells reached: {counts[0]} -> {counts[1]} of {counts[2]}")
    return "\n".join(rows)


if __name__ == "__main__":
    before = existing()
    print(table(before, before | added()))

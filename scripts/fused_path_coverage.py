#!/usr/bin/env python3
"""Which instantiation and which path of the one-pass dense kernels (csrc/fh_fused.h: k_fused_dense; csrc/fh_setup.h: k_setup_dense) the cases of
tests/fused_paths.py reach, as tables.  Host-only: every case goes through the library's own launch rule in its pure form
(fh_fused_launch_shape_for / fh_setup_shape_for, the functions the launchers call; the GPU tests ask the context) and
tests/fused_paths.py:paths_of reads the paths off the geometry.

    python scripts/fused_path_coverage.py            # markdown on stdout
    python scripts/fused_path_coverage.py --proof    # ... and per case: the bits the worst sum of the launch needed in integer arithmetic

Tables: row-side and finaliser paths per loop form of the body (cases that reach each; `unreachable` with the reason below the table, `NEVER` = a
gap); column-side paths per row of the two instance tables (`n/a`: no width of that row reaches the path)."""
import collections
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import fused_paths as FP                  # noqa: E402
from tests import test_fused_paths_cpu as CPU        # noqa: E402


def reached():
    forms, columns = collections.Counter(), collections.Counter()
    for c in FP.cases():
        sh = FP.shape_query(c)
        for path, yes in FP.paths_of(sh, c.m, c.n).items():
            if not yes:
                continue
            if path in FP.COLUMN_PATHS:
                columns[(c.what, FP.row_of(sh), path)] += 1
            elif c.what == "step":
                forms[(FP.form_of(sh), path)] += 1
    return forms, columns


def tables():
    forms, columns = reached()
    out = [f"{len(FP.step_cases())} step cases ({len(FP.logistic_cases())} logistic), {len(FP.setup_cases())} set-up cases", "",
           "| rows and finaliser | " + " | ".join(FP.FORMS) + " |", "|---|" + "---|" * len(FP.FORMS)]
    gaps = 0
    for path in FP.ROW_PATHS + FP.FIN_PATHS:
        cells = []
        for form in FP.FORMS:
            if (form, path) in FP.UNREACHABLE:
                cells.append("unreachable" if not forms[(form, path)] else f"LISTED, yet {forms[(form, path)]}")
            else:
                cells.append(str(forms[(form, path)]) if forms[(form, path)] else "NEVER")
                gaps += not forms[(form, path)]
        out.append(f"| {path} | " + " | ".join(cells) + " |")
    out += ["", "Unreachable on at most 256 CUs:", ""] + [f"- {form}, {path}: {why}" for (form, path), why in FP.UNREACHABLE.items()]
    reachable = CPU._reachable_column_paths()
    for what, table, key in (("step", FP.fused_table(), "PPT, PIPE, TEAM, XLDS, NBO, F32"), ("setup", FP.setup_table(), "MPP, PIPE, TEAM, threads, NR, F32")):
        out += ["", f"| {what}: {key} | " + " | ".join(FP.COLUMN_PATHS) + " |", "|---|" + "---|" * len(FP.COLUMN_PATHS)]
        for row in table:
            cells = []
            for path in FP.COLUMN_PATHS:
                k = columns[(what, row, path)]
                cells.append(str(k) if k else ("NEVER" if (what, row, path) in reachable else "n/a"))
                gaps += not k and (what, row, path) in reachable
            out.append(f"| {', '.join(str(v) for v in row)} | " + " | ".join(cells) + " |")
    out += ["", f"uncovered cells: {gaps}"]
    return "\n".join(out), gaps


def proof():
    out = ["", "| case | teams x rows | grid | worst sum | bits |", "|---|---|---|---|---|"]
    for c in FP.cases():
        if c.loss != "lsq":
            continue
        bits, where = FP.prove(c) if c.what == "step" else FP.prove_setup(c)
        sh = FP.shape_query(c)
        out.append(f"| {FP.case_id(c)} | {sh.nteams} x {sh.rows_per_team} | {sh.grid} | {where} | {bits} |")
    return "\n".join(out)


if __name__ == "__main__":
    text, gaps = tables()
    print(text)
    if "--proof" in sys.argv[1:]:
        print(proof())
    sys.exit(1 if gaps else 0)

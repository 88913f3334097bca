#!/usr/bin/env python3
"""Which path of the device-side loop kernel (csrc/fh_run.h: k_run_dense<PPT>) the cases of tests/run_paths.py reach, as tables.  Host-only:
every case goes through the library's own launch rule in its pure form (fh_run_shape_for, the function fh_run itself calls; the GPU tests ask
the context: fh_run_shape) and tests/run_paths.py:paths_of reads the paths off the geometry.

    python scripts/run_path_coverage.py            # markdown on stdout
    python scripts/run_path_coverage.py --proof    # ... and per case: iterations proven exact in integer arithmetic, the bits the worst sum needed

Tables: lane paths per table entry PPT; row-block and phase-B paths per NB (the row buffers: 6 for PPT <= 4, 5 for 5 / 6, 4 for 7 / 8, 3 beyond);
the controller's paths and the options, with the number of cases that take each."""
import collections
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import run_paths as RP                    # noqa: E402


def reached():
    lanes, blocks, options = collections.defaultdict(int), collections.defaultdict(int), collections.Counter()
    for c in RP.cases():
        sh = RP.shape_query(c)
        mdl = RP.model(c)
        for path, yes in RP.paths_of(sh, c.m, c.n).items():
            if yes:
                if path in RP.LANE_PATHS:
                    lanes[(path, sh.PPT)] += 1
                else:
                    blocks[(path, sh.NB)] += 1
        for name, yes in RP.controller_paths(c, mdl).items():
            options[name] += bool(yes)
        options[f"mode {c.mode}{', restart' if c.restart else ''}"] += 1
        options[f"prox {c.kind}, {'BIG' if sh.BIG else 'not BIG'}"] += 1
        options[f"NT = {sh.NT}"] += 1
        options[f"evaluate_objective = {c.evalobj}"] += 1
    return lanes, blocks, options


def tables():
    lanes, blocks, options = reached()
    out = ["| lanes | " + " | ".join(f"PPT {p}" for p in RP.RUN_TABLE) + " |", "|---|" + "---|" * len(RP.RUN_TABLE)]
    for path in RP.LANE_PATHS:
        out.append(f"| {path} | " + " | ".join(str(lanes[(path, p)]) if lanes[(path, p)] else ("n/a" if path == "idle piece" and p not in (4, 10, 12, 14) else "never")
                                              for p in RP.RUN_TABLE) + " |")
    out += ["", "| rows and phase B | NB 6 | NB 5 | NB 4 | NB 3 |", "|---|---|---|---|---|"]
    for path in RP.ROW_PATHS + RP.PHASE_B_PATHS:
        out.append(f"| {path} | " + " | ".join(str(blocks[(path, nb)]) if blocks[(path, nb)] else "never" for nb in (6, 5, 4, 3)) + " |")
    out += ["", "| controller and options | cases |", "|---|---|"]
    for name in sorted(options):
        out.append(f"| {name} | {options[name] or 'never'} |")
    return "\n".join(out)


def proof():
    out = ["", "| case | shape | iterations compared | proven exact | retries per iteration | worst sum | bits |", "|---|---|---|---|---|---|---|"]
    for c in RP.cases():
        proven, bits, where, failed = RP.prove(c)
        sh = RP.shape_query(c)
        out.append(f"| {RP.case_id(c)} | PPT {sh.PPT}, G {sh.G} x {sh.rows_per_team} | {c.steps} | {proven}{' (' + failed[1] + ')' if failed else ''} | "
                   f"{RP.model(c).retries} | {where} | {bits} |")
    return "\n".join(out)


if __name__ == "__main__":
    print(tables())
    if "--proof" in sys.argv[1:]:
        print(proof())

#!/usr/bin/env python3
"""Which instantiation of the 2-D stencil kernels (csrc/fh_tv.h) each GPU test file reaches: the 30 k_tv_onepass<IDENT, ACCEL, U, NT, NB> the
host can dispatch and the 22 of the two-launch family (k_fwd_tv_step<IDENT, U, NT>, k_adj_tv_step<U, NT>, k_fwd_tv<4, NT>, k_adj_tv<4, NT>).
Host-only: the tuning every launch of a test runs under goes through the host's dispatch rule as tests/tv_paths.py restates it
(onepass_instantiation, two_launch_instantiations; tests/test_tv_paths_cpu.py holds that restatement against csrc/fh_host_launch.h).
"before": tests/test_gpu_prox_tv.py and tests/test_gpu_experimental.py, which set none of FH_TUNE_TV_U / _PIPE / _NT / _XCD (the experimental
file sets FH_TUNE_TV_ROWS, which selects no instantiation); "after": with tests/test_gpu_tv_paths.py.

    python scripts/tv_path_coverage.py            # markdown on stdout"""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import test_gpu_prox_tv as OLD            # noqa: E402
from tests import tv_paths as T                      # noqa: E402


SELECTING_KEYS = ("TUNE_TV_U", "TUNE_TV_PIPE", "TUNE_TV_NT", "TUNE_TV_XCD")
OLD_FILES = ("test_gpu_prox_tv.py", "test_gpu_experimental.py")


def old_files_set_no_selecting_key():
    """The premise of existing(): neither earlier file names a tuning key that selects an instantiation (read as text: the experimental file
    imports only against its own library)."""
    for name in OLD_FILES:
        text = open(os.path.join(ROOT, "tests", name)).read()
        for key in SELECTING_KEYS:
            assert not re.search(rf"\b{key}\b", text), f"tests/{name} sets {key}: count its launches in existing()"


def existing():
    """Every launch of the two earlier files, all under the automatic rules (no tuning key that selects an instantiation is ever set: checked)."""
    old_files_set_no_selecting_key()
    one, two = set(), set()
    if OLD.ONE_PASS_SHAPES:                                                 # test_one_pass_tv_step_equals_two_launch_step: TV-ball, fh_step | fh_fwd + fh_adj
        one.add(T.onepass_instantiation(T.TVBALL, 0))
        two |= T.two_launch_instantiations(T.TVBALL)
    if OLD.ONE_PASS_ACCEL_SHAPES:                                           # ..._accelerated_...: both prox kinds, fh_step_accel | fh_fwd + fh_adj(accel)
        for prox in (T.TVBALL, T.IDENTITY):
            one.add(T.onepass_instantiation(prox, 1))
            two |= T.two_launch_instantiations(prox)
    # the solves (golden parity, denoising, with / without the one-pass kernel, the 8192^2 iterations): TV-ball, plain and accelerated
    one |= {T.onepass_instantiation(T.TVBALL, 0), T.onepass_instantiation(T.TVBALL, 1)}
    two |= T.two_launch_instantiations(T.TVBALL)
    if OLD.TV_SHAPES:                                                       # test_stencil_pair_matches_numpy_rolls: fh_apply, and every fh_init
        two |= T.plain_pair_instantiations()
    return one, two


def added():
    return T.reached_onepass(), T.reached_two_launch()


def name_of(i):
    return f"k_tv_onepass<{', '.join(str(k) for k in i)}>" if isinstance(i[0], int) else f"{i[0]}<{', '.join(str(k) for k in i[1:])}>"


def table(before, after):
    rows = ["| instantiation | reached |", "|---|---|"]
    for family, every, b, a in (("one-pass", T.ONEPASS_ALL, before[0], after[0]), ("two-launch", T.TWO_LAUNCH_ALL, before[1], after[1])):
        for i in sorted(every, key=str):
            rows.append(f"| `{name_of(i)}` | {'before' if i in b else ('NEW' if i in a else 'never')} |")
    rows.append("")
    for family, every, b, a in (("one-pass", T.ONEPASS_ALL, before[0], after[0]), ("two-launch", T.TWO_LAUNCH_ALL, before[1], after[1])):
        rows.append(f"{family} instantiations reached: {len(b & every)} -> {len((a | b) & every)} of {len(every)}")
    return "\n".join(rows)


if __name__ == "__main__":
    print(table(existing(), added()))

"""Take the fixture tests/golden/refusals/front_end.json: ask solver._unrecognised -- and, where it has no objection, solver._recognise -- about
every case of tests/front_end_cases.py and record the answers, together with the commit they were taken on.  No device is needed, the built
library is (the DCT and the convolution operator ask it for their refusals):

    python scripts/make_front_end_golden.py <commit> [--out <path>]

Run it on the commit whose behaviour is to be pinned -- before a change to the recognition code that is meant to keep every answer -- and commit
the file; tests/test_front_end_cpu.py asks the same list and compares with `==`."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import front_end_cases as FC             # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("commit", help="the commit the answers are taken on")
    ap.add_argument("--out", default=FC.GOLDEN)
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    cases, answers = FC.dump_golden(args.out, args.commit, {cid: FC.answer(cid) for cid in FC.ids()})
    print("wrote", args.out, cases, "cases,", answers, "distinct answers")


if __name__ == "__main__":
    main()

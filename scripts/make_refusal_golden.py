"""Take the fixture tests/golden/refusals/c_abi.json: replay every case of tests/refusal_cases.py through fasta_python_amd.hip on the GPU and
record, per call, the status and the text of fh_last_error (0 and "" on success), together with the commit the library was built from:

    python scripts/make_refusal_golden.py <commit> [--out <path>]

Run it on the commit whose behaviour is to be pinned -- before a change to the host text that is meant to keep every answer -- and commit the
file; tests/test_gpu_refusals.py replays the same list and compares with `==`."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fasta_python_amd import hip                    # noqa: E402
from tests import refusal_cases as RC               # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("commit", help="the commit the library under fasta_python_amd/ was built from")
    ap.add_argument("--out", default=RC.GOLDEN)
    args = ap.parse_args()
    lib = hip.load_library()
    cases = {}
    for case in RC.CASES:
        cases[case[0]] = {"calls": [name for name, _ in case[2]], "got": RC.replay(lib, case)}
        print(case[0], sum(1 for status, _ in cases[case[0]]["got"] if status), "refusals of", len(cases[case[0]]["got"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"commit": args.commit, "cases": cases}, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote", args.out, len(cases), "cases")


if __name__ == "__main__":
    main()

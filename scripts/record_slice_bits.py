"""Prints (or writes with --out FILE) the sha256 of the output bytes of every case of tests/slice_tail_defs.py BIT_CASES as JSON.

tests/golden/hub_slices_parent_bits.json is this script's output on the commit BEFORE the sliced aggregation's tail was re-scheduled
(counter reset in the gather, non-temporal row stores, two rows per wave in the combine, the "slice_front" block schedule); on any
later tree it must print the same hashes, which tests/test_slice_tail_gpu.py::test_bits_of_the_parent checks.  Needs an MI355X.

    python scripts/record_slice_bits.py [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import pgl_amd
    import slice_tail_defs as S
    ops, built, hashes = pgl_amd.ops, {}, {}
    for case in S.BIT_CASES:
        if case[0] not in built:
            built[case[0]] = S.device_index(pgl_amd, case[0])
        index, n = built[case[0]][:2]
        hashes[S.case_id(case)] = S.bits(S.run_case(ops, index, n, case)[0])
    text = json.dumps(hashes, indent=1, sort_keys=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Records what the CPU tests need to know about the reference (TEST
INFRASTRUCTURE): run once against a reference tree, commit the results.

usage: python3 oracle/record_reference_facts.py REFERENCE_DIR

Writes
  tests/golden/ref_optable.json     the (op, type) pairs that have a kernel in
                                    ompi_op_base_functions / _3buff_functions
                                    (tests/ref_optable.py)
  tests/golden/ref_abi_layout.json  member lists, offsets and sizes of the
                                    plugin-ABI structs and the names the
                                    headers declare (tests/ref_abi.py)
Both hold names and numbers only.  Needs gcc (the offsets come from probe
programs that include the reference's headers).
"""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ref_abi       # noqa: E402
import ref_optable   # noqa: E402


def main():
    if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "ompi")):
        sys.exit(__doc__)
    ref = os.path.abspath(sys.argv[1])
    with tempfile.TemporaryDirectory() as tmp:
        abi = ref_abi.record(ref, tmp)
    for path, d in ((ref_optable.GOLDEN, ref_optable.record(ref)), (ref_abi.GOLDEN, abi)):
        with open(path, "w") as f:
            json.dump(d, f, indent=0, sort_keys=True)
            f.write("\n")
        print(f"{os.path.relpath(path, ROOT)}: {os.path.getsize(path)} B")


if __name__ == "__main__":
    main()

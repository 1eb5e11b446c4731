#!/usr/bin/env python3
"""Writes tests/golden/moe_bits.json: the SHA-256 of the output bytes of every case of tests/test_gpu_moe_bits.py, from the library
NS_LIB_PATH names (default: the tree's).  Needs the GPU.  Every case runs twice, in two passes over all of them; nothing is written when the
two passes differ in any digest, or when a case was not served by the path it is named for.

    NS_LIB_PATH=/path/to/parent/libns_hip.so python tests/golden/make_moe_bits.py [out.json [passes]]

(passes = 1: the single pass tests/test_gpu_moe_bits.py runs in a child process and compares with the committed file.)

The committed file was written by the build in front of the family's split into files by role (docs/kernels/other.md, "MoE: files and paths")."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]

import __graft_entry__ as ge  # noqa: E402
import test_gpu_moe_bits as T  # noqa: E402

if __name__ == "__main__":
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "moe_bits.json")
    pkg = ge.load_package()
    nso = ge.load_oracle()
    L = pkg.lib()
    first = T.run_all(L, pkg, nso)
    second = T.run_all(L, pkg, nso) if len(sys.argv) < 3 or int(sys.argv[2]) > 1 else first
    differ = sorted(c for c in first if first[c] != second.get(c))
    if differ or len(first) != len(second):
        sys.exit("two runs differ, nothing written: %s" % differ)
    with open(out_path, "w") as f:
        json.dump(first, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote %s (%d digests) from %s" % (out_path, len(first), pkg.LIB_PATH))

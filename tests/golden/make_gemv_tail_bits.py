#!/usr/bin/env python3
"""Writes tests/golden/gemv_tail_bits.json: the SHA-256 of the output bytes of every case of tests/test_gpu_gemv_tail.py, from the library
NS_LIB_PATH names (default: the tree's).  Needs the GPU.  Every case is also held to the test's other yardsticks on the way, so a file is
written only by a library that passes them.

    NS_LIB_PATH=/path/to/parent/libns_hip.so python tests/golden/make_gemv_tail_bits.py [out.json]

The committed file was written by the build in front of the launch-tail change of round 14 (docs/kernels/gemv.md, "launch tail")."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]

import __graft_entry__ as ge  # noqa: E402
import test_gpu_gemv_tail as T  # noqa: E402

if __name__ == "__main__":
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "gemv_tail_bits.json")
    pkg = ge.load_package()
    nso = ge.load_oracle()
    L = pkg.lib()
    bits = {}
    for cfg in T.WCFG:
        bits.update(T.run_config(L, pkg, nso, cfg))
        print("%s: %d cases so far" % (cfg[0], len(bits)), flush=True)
    with open(out_path, "w") as f:
        json.dump(bits, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote %s (%d digests) from %s" % (out_path, len(bits), pkg.LIB_PATH))

#!/usr/bin/env python3
"""Writes tests/golden/device_bits.json: the SHA-256 of the output bytes of every case of tests/test_gpu_device_bits.py, from the library
NS_LIB_PATH names (default: the tree's).  Needs the GPU.  Every case is recorded twice, in two separate processes; a case whose two
recordings differ is written as null - tests/test_gpu_device_bits.py does not hold it to a digest - and named on standard output.

    NS_LIB_PATH=/path/to/parent/libns_hip.so python tests/golden/make_device_bits.py [out.json]

(With a second argument `once`: one pass in this process, whatever it gives - what the two child processes run.)

The committed file was written by the build in front of the device backend's split into files by role (docs/kernels/device_backend.md,
"Files")."""
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]


def once(out_path):
    import __graft_entry__ as ge
    import test_gpu_device_bits as T
    pkg = ge.load_package()
    with open(out_path, "w") as f:
        json.dump(T.run_all(pkg.lib(), pkg), f, indent=0, sort_keys=True)
        f.write("\n")
    return pkg.LIB_PATH


if __name__ == "__main__":
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "device_bits.json")
    if len(sys.argv) > 2 and sys.argv[2] == "once":
        once(out_path)
        sys.exit(0)
    passes = []
    with tempfile.TemporaryDirectory() as tmp:
        for i in range(2):
            part = os.path.join(tmp, "pass%d.json" % i)
            subprocess.run([sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), part, "once"], check=True, timeout=600)
            with open(part) as f:
                passes.append(json.load(f))
    first, second = passes
    if sorted(first) != sorted(second):
        sys.exit("the two passes ran different cases, nothing written")
    differ = sorted(c for c in first if first[c] != second[c])
    with open(out_path, "w") as f:
        json.dump({c: (None if c in differ else first[c]) for c in first}, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote %s (%d digests, %d cases whose two recordings differ: %s) from %s" % (out_path, len(first) - len(differ), len(differ), differ,
                                                                                        os.environ.get("NS_LIB_PATH", "the tree's library")))

"""Worker of tests/test_gpu_attn_block_paged.py: one ns_hip_attn_block_paged call of a named case in a process of its own.

  attn_block_paged_worker.py <case name> <out.npz>

NS_ATTN_DYN_RANGES is read once per process, so the ranges as laid out can only be had from a fresh process with the variable set by the parent.
The inputs are a function of the case alone: the parent draws the same ones."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import __graft_entry__ as ge
    import test_gpu_attn_block_paged as t
    pkg = ge.load_package()
    name = sys.argv[1]
    c = t.Rag(None, *t.CASES[name][:7])  # (no oracle here: the parent checks)
    p = t.rag_pools(c, *t.CASES[name][7:]).upload()
    out = t.run_block(pkg.lib(), pkg, c, p)[0]
    np.savez(sys.argv[2], out=out)
    print("ATTN_BLOCK_PAGED_WORKER_OK DYN_RANGES=%s" % os.environ.get("NS_ATTN_DYN_RANGES"))

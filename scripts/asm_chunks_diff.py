#!/usr/bin/env python3
"""Device assembly of two builds of one kernel file (hipcc --cuda-device-only -S), compared without regard to the ORDER in which the
compiler emitted the template instantiations: host code that reaches the same instantiations along another path changes that order
and nothing else.

    python scripts/asm_chunks_diff.py parent/ns_gemm.s new/ns_gemm.s

The text is cut at every `.section` directive (each kernel's code, its kernel descriptor and its .AMDGPU.csdata lie in sections of
their own) and at every entry of the amdhsa.kernels metadata list; the two multisets of chunks are compared.  Lines that carry the
translation unit's __hip_cuid_ are dropped, and local labels lose their file-wide running numbers (.LBB17_4 -> .LBB_4, .Lfunc_end17, .Lpost_getpc6).  Exit status 0: the same chunks, byte for byte; 1: not."""
import collections
import re
import sys


# local labels, and the comments that name them, carry the index of their function in the file: .LBB17_4, .Lfunc_end17 -> .LBB_4, .Lfunc_end
LABEL = re.compile(r"(BB|func_end|func_begin|post_getpc)\d+")
PAD = re.compile(r"[ \t]+;")  # a label's trailing comment is aligned to a column: the padding depends on the label's length


def chunks(path):
    out, cur = collections.Counter(), []
    with open(path) as f:
        for line in f:
            if "__hip_cuid_" in line:
                continue
            line = PAD.sub(" ;", LABEL.sub(r"\1", line))
            if line.startswith("\t.section\t") or re.match(r"  - \.", line) or line.startswith("amdhsa.target") or line.startswith("\t.amdgpu_metadata"):
                out["".join(cur)] += 1
                cur = []
            cur.append(line)
    out["".join(cur)] += 1
    return out


if __name__ == "__main__":
    a, b = chunks(sys.argv[1]), chunks(sys.argv[2])
    only_a, only_b = a - b, b - a
    print("%s: %d chunks / %d chunks, %d only in the first, %d only in the second" %
          (sys.argv[2].split("/")[-1], sum(a.values()), sum(b.values()), sum(only_a.values()), sum(only_b.values())))
    for c in list(only_a)[:2] + list(only_b)[:2]:
        print("   ", c[:200].replace("\n", "\n    "))
    sys.exit(1 if only_a or only_b else 0)

#!/usr/bin/env python3
"""Device assembly of two builds of one kernel file (hipcc --cuda-device-only -S), compared without regard to the ORDER in which the
compiler emitted the template instantiations: host code that reaches the same instantiations along another path changes that order
and nothing else.

    python scripts/asm_chunks_diff.py parent/ns_gemm.s new/ns_gemm.s
    python scripts/asm_chunks_diff.py parent/ns_attn.s -- new/ns_attn_decode.s new/ns_attn_prefill.s new/ns_kvcache.s   (a file that was split:
        several files on either side of `--`; the chunks are then compared as sets, since every file repeats its frame)

The text is cut at every `.section` directive (each kernel's code, its kernel descriptor and its .AMDGPU.csdata lie in sections of
their own) and at every entry of the amdhsa.kernels metadata list; the two multisets of chunks are compared.  Lines that carry the
translation unit's __hip_cuid_ are dropped, and local labels lose their file-wide running numbers (.LBB17_4 -> .LBB_4, .Lfunc_end17, .Lpost_getpc6).  Exit status 0: the same chunks, byte for byte; 1: not."""
import collections
import re
import sys


# local labels, and the comments that name them, carry the index of their function in the file: .LBB17_4, .Lfunc_end17 -> .LBB_4, .Lfunc_end
LABEL = re.compile(r"(BB|func_end|func_begin|post_getpc)\d+")
PAD = re.compile(r"[ \t]+;")  # a label's trailing comment is aligned to a column: the padding depends on the label's length


def chunks(*paths):
    """the chunks of several files together: a kernel file that was split compares against the files it was split into"""
    out = collections.Counter()
    for path in paths:
        out += chunks_of(path)
    return out


def chunks_of(path):
    out, cur = collections.Counter(), []
    with open(path) as f:
        for line in f:
            if "__hip_cuid_" in line:
                continue
            line = PAD.sub(" ;", LABEL.sub(r"\1", line))
            if line.startswith("\t.section\t") or line == "\t.text\n" or re.match(r"  - \.", line) or line.startswith("amdhsa.target") or line.startswith("\t.amdgpu_metadata"):
                out["".join(cur)] += 1
                cur = []
            cur.append(line)
    out["".join(cur)] += 1
    return out


if __name__ == "__main__":
    args = sys.argv[1:]
    cut = args.index("--") if "--" in args else 1
    a, b = chunks(*args[:cut]), chunks(*[x for x in args[cut:] if x != "--"])
    if cut != 1 or len(args) > 2:
        # what every file carries once (target line, metadata frame) counts once; a file's own frame is left out: its table of
        # address-significant symbols (.note.GNU-stack: the LDS arrays of the kernels IN that file) and a section directive with nothing behind it
        frame = lambda c: c.startswith('\t.section\t".note.GNU-stack"') or len(c.strip().split("\n")) <= 1
        a, b = (collections.Counter(c for c in set(x) if not frame(c)) for x in (a, b))
    only_a, only_b = a - b, b - a
    print("%s: %d chunks / %d chunks, %d only in the first, %d only in the second" %
          (" + ".join(x.split("/")[-1] for x in args[cut:] if x != "--"), sum(a.values()), sum(b.values()), sum(only_a.values()), sum(only_b.values())))
    for c in list(only_a)[:2] + list(only_b)[:2]:
        print("   ", c[:200].replace("\n", "\n    "))
    sys.exit(1 if only_a or only_b else 0)

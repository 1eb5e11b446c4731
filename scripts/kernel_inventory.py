#!/usr/bin/env python3
"""The kernels of two builds of libns_hip.so, compared name by name — the guard against an instantiation appearing, vanishing or changing
when host-side launch code is rewritten.

    python scripts/kernel_inventory.py parent/libns_hip.so neural-speed_amd/libns_hip.so

How: llvm-objdump --offloading extracts the device code objects (gfx950); per code object llvm-readelf -s -W gives the FUNC symbols (name,
code size) and llvm-readelf --notes the amdhsa.kernels metadata.  Per kernel name: code size, .vgpr_count, .sgpr_count, .vgpr_spill_count,
.sgpr_spill_count, .group_segment_fixed_size (LDS), .private_segment_fixed_size (scratch).  A name held by two code objects is reported."""
import collections
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
FIELDS = (".vgpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".group_segment_fixed_size", ".private_segment_fixed_size")


def run(*cmd, cwd=None):
    return subprocess.run(cmd, cwd=cwd, check=True, capture_output=True, text=True).stdout


def inventory(lib):
    """{kernel name: [(code size, metadata values) per code object that holds it]}, number of code objects"""
    kernels = collections.defaultdict(list)
    with tempfile.TemporaryDirectory() as tmp:
        shutil.copy(lib, os.path.join(tmp, "lib.so"))
        run(os.path.join(LLVM, "llvm-objdump"), "--offloading", "lib.so", cwd=tmp)
        objs = sorted(f for f in os.listdir(tmp) if "amdgcn" in f)
        for obj in objs:
            path = os.path.join(tmp, obj)
            size = {}
            for line in run(os.path.join(LLVM, "llvm-readelf"), "-s", "-W", path).splitlines():
                c = line.split()
                if len(c) >= 8 and c[3] == "FUNC":
                    size[c[7]] = int(c[2])
            meta, cur = [], None
            for line in run(os.path.join(LLVM, "llvm-readelf"), "--notes", path).splitlines():
                if line.startswith("amdhsa.kernels:"):
                    cur = {}
                elif cur is not None and re.match(r"\S", line):
                    cur = None  # the next top-level key: amdhsa.target, amdhsa.version
                if cur is None:
                    continue
                if line.startswith("  - "):  # an entry of the kernel list (the entries of a kernel's .args list are indented further)
                    cur = {}
                    meta.append(cur)
                m = re.match(r"  (?:- |  )(\.\w+):\s*(\S+)", line)
                if m:
                    cur[m.group(1)] = m.group(2)
            for k in meta:
                if ".name" in k and ".vgpr_count" in k:
                    kernels[k[".name"]].append((size.get(k[".name"], -1),) + tuple(int(k.get(f, -1)) for f in FIELDS))
    return kernels, len(objs)


def family(name):
    m = re.match(r"_ZN2ns(?:12_GLOBAL__N_1)?(\d+)", name)
    return name[m.end():][:int(m.group(1))] if m else name


if __name__ == "__main__":
    a, na = inventory(sys.argv[1])
    b, nb = inventory(sys.argv[2])
    row = lambda what, x, y: print("%-58s %14s %14s" % (what, x, y))
    row("", "parent", "new")
    row("code objects", na, nb)
    row("kernel names", len(a), len(b))
    row("names only in this build", len(set(a) - set(b)), len(set(b) - set(a)))
    row("names in more than one code object", sum(len(v) > 1 for v in a.values()), sum(len(v) > 1 for v in b.values()))
    row("sum of code sizes (bytes)", sum(v[0][0] for v in a.values()), sum(v[0][0] for v in b.values()))
    for i, f in enumerate(FIELDS):
        agg = sum if "spill" in f else max
        row(("sum of " if "spill" in f else "largest ") + f, agg(v[0][1 + i] for v in a.values()), agg(v[0][1 + i] for v in b.values()))
    fa, fb = collections.Counter(family(n) for n in a), collections.Counter(family(n) for n in b)
    for fam in sorted(set(fa) | set(fb)):
        row("  " + fam, fa[fam], fb[fam])
    diff = [n for n in sorted(set(a) & set(b)) if a[n] != b[n]]
    print("\nkernels whose code size or one of the six metadata values differs between the builds: %d" % len(diff))
    for n in diff[:40]:
        print("  %s: %s -> %s" % (n, a[n], b[n]))
    for n in sorted(set(a) ^ set(b))[:40]:
        print("  only in %s: %s" % ("parent" if n in a else "new", n))
    sys.exit(1 if diff or set(a) != set(b) else 0)

"""The host decisions of the reference's device backend (neural-speed_amd/csrc/ns_device_plan.cpp), checked without a GPU.

KvMirrorTable keeps the records of the fp16 kv mirrors: which record holds a cache range, which ones a new range evicts, the hull, what a
foreign write resets and which positions an attention call converts again.  mha_f32_plan says which of the three servers of
ns_hip_mha_f32_device_layout takes a call and, for the context-split kernel, into which row chunks; binary_plan and lazy_mul_plan say which
kernel a binary node runs on and what the lazy peephole makes of a multiply.  A host program (tests/tools/device_plan_main.cpp, nothing
launched, every address made up) answers one command per line; the rules it must follow - ns_device_plan.h, csrc/ns_route.h - are restated
here independently: the table's as the expected answer of every command, the three plans as Python functions.  The program is plain C++:
it is built once with the library's compiler and once with g++ under the address and undefined-behaviour sanitizers."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "neural-speed_amd", "csrc")
SOURCES = [os.path.join(ROOT, "tests", "tools", "device_plan_main.cpp"), os.path.join(CSRC, "ns_device_plan.cpp")]


def compiler():
    """HIPCC of the library's Makefile (the environment's HIPCC wins there too)"""
    with open(os.path.join(CSRC, "Makefile")) as f:
        default = re.search(r"^HIPCC\s*\?=\s*(\S+)", f.read(), re.M).group(1)
    path = os.environ.get("HIPCC", default)
    return path if os.path.exists(path) else shutil.which(path)


def run_program(exe, commands):
    out = subprocess.run([exe], input="".join(c + "\n" for c in commands), check=True, capture_output=True, text=True, timeout=120)
    assert out.stderr == "", out.stderr
    lines = out.stdout.splitlines()
    assert len(lines) == len(commands)
    return lines


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    hipcc = compiler()
    if not hipcc:
        pytest.skip("the library's compiler is not installed")
    exe = str(tmp_path_factory.mktemp("device_plan") / "device_plan")
    subprocess.run([hipcc, "-std=c++20", "-x", "hip", "--offload-arch=gfx950", "--cuda-host-only", "-Wall", "-Werror", "-I", CSRC] + SOURCES + ["-o", exe],
                   check=True, capture_output=True, text=True, timeout=300)
    return exe


# ---- the mirror table -------------------------------------------------------------------------------------------------------------------------
# heads_kv 2, hs 8, n_ctx 16: one slot is 2 * 16 * 8 * 4 = 1024 bytes (256 elements); two slots, K at 0x10000, V at 0x20000.  The program
# hands out the fp16 "allocations" 0x1000000 (K) / 0x1800000 (V) to the first record, 0x2000000 / 0x2800000 to the second, ...
K, V, SLOT = 0x10000, 0x20000, 1024
GEO = "2 8 16"
TWO = "get %d %d 2 %s" % (K, V, GEO)
K16, V16 = 0x1000000, 0x1800000


def table_script():
    """(command, expected answer)"""
    s = []
    add = lambda c, w: s.append((c, w))
    # -- lookup --
    add("reset", "ok")
    add(TWO, "hit=0 evicted= rec=0 slot0=0")
    add(TWO, "hit=1 rec=0 slot0=0")
    add("get %d %d 1 %s" % (K, V, GEO), "hit=1 rec=0 slot0=0")                      # slot 0 alone
    add("get %d %d 1 %s" % (K + SLOT, V + SLOT, GEO), "hit=1 rec=0 slot0=1")        # slot 1
    add("lookup %d %d 1 %s" % (K + SLOT, V + SLOT, GEO), "rec=0 slot0=1")
    add("lookup %d %d 2 %s" % (K + SLOT, V + SLOT, GEO), "none")                    # two slots from slot 1: past the record
    add("lookup %d %d 1 %s" % (K + 512, V + 512, GEO), "none")                      # an offset that is no slot multiple
    add("lookup %d %d 2 2 4 32" % (K, V), "none")                                   # the same addresses and bytes, another geometry
    add("lookup %d %d 1 %s" % (K + SLOT, V, GEO), "none")                           # V at the wrong offset
    add("state 0", "valid=0,0 fresh=0,0")
    add("get %d %d 1 %s" % (K + SLOT, V, GEO), "hit=0 evicted=0 rec=1 slot0=0")     # ... evicts and starts anew
    add("hull", "lo=%d hi=%d" % (K + SLOT, V + SLOT))
    add("state 1", "valid=0 fresh=0,0")
    add("get %d %d 1 %s" % (V + 512, 0x30000, GEO), "hit=0 evicted=1 rec=2 slot0=0")  # a new K range over an old V range
    add("reset", "ok")
    add(TWO, "hit=0 evicted= rec=0 slot0=0")
    add("get %d %d 2 2 4 32" % (K, V), "hit=0 evicted=0 rec=1 slot0=0")             # another geometry at the same address
    add("get %d %d 1 %s" % (K + 512, V + 512, GEO), "hit=0 evicted=1 rec=2 slot0=0")  # no slot multiple of the record: a mirror of its own
    # several records: every overlapping one goes, newest first; the others stay
    add("reset", "ok")
    add("get %d %d 1 %s" % (K, V, GEO), "hit=0 evicted= rec=0 slot0=0")
    add("get %d %d 1 %s" % (0x40000, 0x50000, GEO), "hit=0 evicted= rec=1 slot0=0")
    add("get %d %d 1 %s" % (0x60000, 0x70000, GEO), "hit=0 evicted= rec=2 slot0=0")
    add("get %d %d 1 %s" % (0x60000 + 4, K + 1020, GEO), "hit=0 evicted=2,0 rec=3 slot0=0")   # K over rec 2's K, V over rec 0's last K cell
    add("lookup %d %d 1 %s" % (0x40000, 0x50000, GEO), "rec=1 slot0=0")
    # -- hull after add and after erase --
    add("reset", "ok")
    add("hull", "lo=0 hi=0")
    add(TWO, "hit=0 evicted= rec=0 slot0=0")
    add("hull", "lo=%d hi=%d" % (K, V + 2 * SLOT))
    add("get %d %d 1 %s" % (0x40000, 0x50000, GEO), "hit=0 evicted= rec=1 slot0=0")
    add("hull", "lo=%d hi=%d" % (K, 0x50000 + SLOT))
    add("erase 1", "ok")
    add("hull", "lo=%d hi=%d" % (K, V + 2 * SLOT))
    add("erase 0", "ok")
    add("hull", "lo=0 hi=0")
    add("cell %d" % K, "none")
    add("write %d 4" % K, "hit=0")
    # -- args_for_cell --
    add("reset", "ok")
    add(TWO, "hit=0 evicted= rec=0 slot0=0")
    kcell = "base=%d m16=%d elems=512 n_ctx=16 hs=8 transposed=0" % (K, K16)
    add("cell %d" % K, kcell)                                                         # the first byte
    add("cell %d" % (K + 2 * SLOT - 1), kcell)                                        # the last byte
    add("cell %d" % (K + 2 * SLOT), "none")                                           # one past the end (inside the hull)
    add("cell %d" % (K - 1), "none")
    add("cell %d" % (V + 4), "base=%d m16=%d elems=512 n_ctx=16 hs=8 transposed=1" % (V, V16))   # inside V: elems = bytes / 4
    add("cell %d" % (V + 2 * SLOT), "none")
    # -- foreign writes --
    mark = ["set_valid %d 5" % K, "set_valid %d 7" % (K + SLOT + 8), "fresh 0 3 9"]
    for c in mark:
        add(c, "ok")
    add("state 0", "valid=5,7 fresh=3,9")
    add("write %d 256" % (K - 256), "hit=0")                                          # ends exactly at the base
    add("write %d 256" % (K + 2 * SLOT), "hit=0")                                     # between K and V, inside the hull
    add("write %d 64" % (V + 2 * SLOT), "hit=0")                                      # starts at the hull's end
    add("state 0", "valid=5,7 fresh=3,9")
    add("write %d 1" % (V + 2 * SLOT - 1), "hit=1")                                   # the last byte
    add("state 0", "valid=0,0 fresh=0,0")                                             # a hit clears every valid and fresh
    for c in mark:
        add(c, "ok")
    add("write %d 0" % (K + 4), "hit=1")                                              # bytes = 0 counts as 1
    add("state 0", "valid=0,0 fresh=0,0")
    for c in mark:
        add(c, "ok")
    add("write %d 512" % (K - 256), "hit=1")                                          # over the base
    add("state 0", "valid=0,0 fresh=0,0")
    # -- set_valid --
    add("set_valid %d 99" % (K + SLOT), "ok")                                         # above n_ctx: clamped
    add("set_valid %d 3" % (K + SLOT - 4), "ok")
    add("set_valid %d 9" % V, "ok")                                                   # a V address names no slot
    add("set_valid %d 9" % (K - 4), "ok")
    add("state 0", "valid=3,16 fresh=0,0")
    # -- convert_from(rec, slot0, batch, seq, seq_all, executing) --
    add("convert 0 0 1 4 16 0", "lo=0")                                               # not executing: everything live
    add("state 0", "valid=16,16 fresh=0,0")
    add("set_valid %d 12" % K, "ok")
    add("convert 0 0 1 4 16 1", "lo=12")                                              # valid == seq_all - seq
    add("set_valid %d 5" % K, "ok")
    add("convert 0 0 1 4 16 1", "lo=5")                                               # a smaller valid
    add("set_valid %d 14" % K, "ok")
    add("convert 0 0 1 4 16 1", "lo=12")                                              # a larger valid: the rows this evaluation wrote go again
    add("set_valid %d 12" % K, "ok")
    add("fresh 0 12 16", "ok")
    add("convert 0 0 1 4 16 1", "lo=16")                                              # fresh covers [lo, seq_all): nothing to convert
    add("state 0", "valid=16,16 fresh=0,0")
    add("set_valid %d 12" % K, "ok")
    add("fresh 0 12 16", "ok")
    add("convert 0 0 1 4 16 0", "lo=0")                                               # ... but only for the route's own launches
    add("state 0", "valid=16,16 fresh=0,0")
    add("set_valid %d 12" % K, "ok")
    add("fresh 0 13 16", "ok")
    add("convert 0 0 1 4 16 1", "lo=12")                                              # fresh starts behind lo
    add("set_valid %d 12" % K, "ok")
    add("fresh 0 12 15", "ok")
    add("convert 0 0 1 4 16 1", "lo=12")                                              # fresh ends in front of seq_all
    add("state 0", "valid=16,16 fresh=0,0")
    add("set_valid %d 12" % (K + SLOT), "ok")
    add("set_valid %d 2" % K, "ok")
    add("fresh 0 12 16", "ok")
    add("convert 0 1 1 4 16 1", "lo=12")                                              # slot0 = 1: the mark is slot 0's, ignored
    add("state 0", "valid=2,16 fresh=0,0")                                            # ... and cleared; slot 0 untouched
    add("set_valid %d 12" % K, "ok")
    add("set_valid %d 12" % (K + SLOT), "ok")
    add("fresh 0 12 16", "ok")
    add("convert 0 0 2 4 16 1", "lo=12")                                              # batch 2: ignored
    add("state 0", "valid=16,16 fresh=0,0")                                           # every slot of the batch
    add("set_valid %d 3" % (K + SLOT), "ok")
    add("convert 0 0 2 4 16 1", "lo=3")                                               # several slots: the smallest mark
    add("convert 0 0 1 16 16 1", "lo=0")                                              # a first prompt
    # -- producer kv16 K V heads_kv hs n_ctx n_past m --
    add("fresh 0 0 0", "ok")
    add("producer 0 %d %d %s 12 4" % (K, V, GEO), "refused")                          # kv16 off
    add("producer 1 %d %d %s -1 4" % (K, V, GEO), "refused")
    add("producer 1 %d %d %s 12 0" % (K, V, GEO), "refused")
    add("producer 1 %d %d %s 13 4" % (K, V, GEO), "refused")                          # n_past + m > n_ctx
    add("state 0", "valid=16,16 fresh=0,0")
    add("producer 1 %d %d %s 2 3" % (K + SLOT, V + SLOT, GEO), "rec=0 slot0=1 k16=%d v16=%d" % (K16 + 512, V16 + 512))
    add("state 0", "valid=16,16 fresh=0,0")                                            # fresh is slot 0's alone
    add("producer 1 %d %d %s 12 4" % (K, V, GEO), "rec=0 slot0=0 k16=%d v16=%d" % (K16, V16))
    add("state 0", "valid=16,16 fresh=12,16")
    add("reset", "ok")
    add("producer 1 %d %d %s 0 16" % (K, V, GEO), "rec=0 slot0=0 k16=%d v16=%d" % (K16, V16))   # makes the mirror when there is none
    add("state 0", "valid=0 fresh=0,16")
    add("convert 0 0 1 16 16 1", "lo=16")
    return s


def test_the_mirror_table_follows_its_rules(program):
    script = table_script()
    got = run_program(program, [c for c, _ in script])
    wrong = [(i, c, w, g) for i, ((c, w), g) in enumerate(zip(script, got)) if w != g]
    assert not wrong, wrong


# ---- which server takes an attention call -------------------------------------------------------------------------------------------------------
SHAPES = [  # batch, seq, seq_all, heads, heads_kv, head_size, n_ctx, masked: the cases of tests/test_gpu_device_mha.py
    (1, 1, 2048, 32, 32, 128, 2048, 1), (1, 1, 777, 8, 2, 64, 1024, 1), (1, 5, 300, 4, 4, 128, 512, 1), (2, 1, 513, 4, 1, 256, 600, 0),
    (1, 3, 1001, 4, 2, 128, 1001, 1), (1, 2, 100, 4, 4, 128, 256, 1), (1, 1, 400, 6, 3, 80, 512, 1), (1, 700, 900, 32, 32, 128, 1024, 1),
    (1, 64, 64, 8, 8, 128, 128, 1), (1, 200, 333, 8, 2, 64, 512, 1), (2, 130, 130, 4, 4, 96, 256, 0), (1, 40, 1000, 4, 4, 256, 1024, 1),
    (1, 31, 400, 4, 4, 128, 512, 1), (1, 1, 1, 32, 32, 128, 2048, 1)]
LONG = (1, 520, 520, 32, 32, 256, 520, 1)
MHA_ORDER = ["batch", "seq", "seq_all", "heads", "heads_kv", "head_size", "n_ctx", "masked", "q16", "k16", "v16", "moving", "attn_supported", "executing",
             "kv16", "no_split", "inlaunch_off"]
ERR_MOVING_SHAPE = "mha_f32: a moving context length needs the context-split kernel (decode step, head size 64 / 128 / 256)"
ERR_MOVING_PAST = "mha_f32: the moving-length form needs 16-byte aligned q / k and scratch for the partials"
ERR_TOO_LONG = "mha_f32: context too long for the device-layout attention kernel"


def mha_case(shape, **kw):
    d = dict(zip(MHA_ORDER[:8], shape), q16=1, k16=1, v16=1, moving=0, attn_supported=1, executing=0, kv16=0, no_split=0, inlaunch_off=0)
    assert set(kw) <= set(d)
    d.update(kw)
    return d


def mha_cases():
    c = {}
    for i, s in enumerate(SHAPES):
        for kv16 in (0, 1):
            c["shape%d-kv%d" % (i, kv16)] = mha_case(s, kv16=kv16)
        c["shape%d-kv1-unsupported" % i] = mha_case(s, kv16=1, attn_supported=0)
        c["shape%d-kv1-executing" % i] = mha_case(s, kv16=1, executing=1)
        c["shape%d-no-split" % i] = mha_case(s, no_split=1)
    c["keys128"] = mha_case((1, 1, 128, 4, 4, 128, 256, 1))
    c["keys129"] = mha_case((1, 1, 129, 4, 4, 128, 256, 1))
    c["hs80"] = mha_case((1, 1, 400, 6, 3, 80, 512, 1))
    for kv16 in (0, 1):
        c["q-misaligned-kv%d" % kv16] = mha_case((1, 1, 300, 4, 4, 128, 512, 1), q16=0, kv16=kv16)
        c["k-misaligned-kv%d" % kv16] = mha_case((1, 1, 300, 4, 4, 128, 512, 1), k16=0, kv16=kv16)
        c["v-misaligned-kv%d" % kv16] = mha_case((1, 1, 300, 4, 4, 128, 512, 1), v16=0, kv16=kv16)   # the split kernel takes it element-wise
    c["rows65535"] = mha_case((1, 65535, 65535, 1, 1, 64, 65535, 0))
    c["rows65536"] = mha_case((2, 32768, 32768, 1, 1, 64, 32768, 0))
    c["heads65535"] = mha_case((1, 1, 256, 65535, 1, 64, 256, 1))
    c["heads65536"] = mha_case((1, 1, 256, 65536, 1, 64, 256, 1))
    c["whole-lds-exact"] = mha_case((1, 1, 40704, 1, 1, 80, 40704, 1))     # (40704 + 256) * 4 = 160 KiB
    c["whole-40705"] = mha_case((1, 1, 40705, 1, 1, 80, 40705, 1))
    c["whole-40706"] = mha_case((1, 1, 40706, 1, 1, 80, 40706, 1))
    c["long-masked"] = mha_case(LONG)
    c["long-unmasked"] = mha_case(LONG[:7] + (0,))
    c["long-batch2"] = mha_case((2,) + LONG[1:])
    for kv16 in (0, 1):
        c["moving-kv%d" % kv16] = mha_case((1, 1, 300, 32, 32, 128, 2048, 1), moving=1, kv16=kv16, executing=1)
        c["moving-seq2-kv%d" % kv16] = mha_case((1, 2, 300, 32, 32, 128, 2048, 1), moving=1, kv16=kv16, executing=1)
        c["moving-hs80-kv%d" % kv16] = mha_case((1, 1, 300, 6, 3, 80, 2048, 1), moving=1, kv16=kv16, executing=1)
    c["moving-no-inlaunch"] = mha_case((1, 1, 300, 32, 32, 128, 2048, 1), moving=1, inlaunch_off=1)
    c["moving-no-inlaunch-kv1"] = mha_case((1, 1, 300, 32, 32, 128, 2048, 1), moving=1, inlaunch_off=1, kv16=1)
    c["moving-no-split"] = mha_case((1, 1, 300, 32, 32, 128, 2048, 1), moving=1, no_split=1)      # the switch is ignored
    c["moving-one-range"] = mha_case((1, 1, 5, 4, 4, 64, 128, 1), moving=1)
    c["moving-65536-pairs"] = mha_case((2, 1, 300, 32768, 1, 64, 512, 1), moving=1)
    c["moving-65538-pairs"] = mha_case((2, 1, 300, 32769, 1, 64, 512, 1), moving=1)
    c["moving-q-misaligned"] = mha_case((1, 1, 300, 32, 32, 128, 2048, 1), moving=1, q16=0)
    c["mirror-hs-260"] = mha_case((1, 1, 300, 2, 2, 264, 512, 1), kv16=1)
    c["mirror-hs-12"] = mha_case((1, 1, 300, 2, 2, 12, 512, 1), kv16=1)
    c["mirror-batch-kv-heads"] = mha_case((2, 1, 130, 32768, 32768, 8, 130, 1), kv16=1)
    c["mirror-q-step"] = mha_case((1, 16384, 16384, 512, 1, 256, 16384, 0), kv16=1)     # seq x heads x head_size = 2^31
    c["mirror-k-step"] = mha_case((1, 1, 8, 128, 128, 256, 65536, 1), kv16=1)
    return c


def want_mha(d):
    """the rule of ns_hip_mha_f32_device_layout, restated"""
    hs, seq, seq_all, batch, heads = d["head_size"], d["seq"], d["seq_all"], d["batch"], d["heads"]
    mirror = (d["kv16"], hs % 8 != 0 or hs > 256 or not (d["q16"] and d["k16"] and d["v16"]) or batch * d["heads_kv"] > 65535 or
              seq * heads * hs >= 2 ** 31 or d["n_ctx"] * d["heads_kv"] * hs >= 2 ** 31 or (d["moving"] and seq != 1) or not d["attn_supported"])
    keys = d["n_ctx"] if d["moving"] else seq_all
    nsplit = -(-keys // 128)
    split_hs = hs in (64, 128, 256)
    split_error = ERR_MOVING_SHAPE if d["moving"] and not (seq == 1 and split_hs and d["n_ctx"] >= seq_all) else "-"
    split = ((not d["no_split"] or d["moving"]) and (nsplit >= 2 or d["moving"]),
             not split_hs or batch * seq > 65535 or heads > 65535 or not d["q16"] or not d["k16"])
    per_row = heads * nsplit * (2 + hs) * 4
    chunk = seq
    if batch == 1 and d["masked"] and seq * per_row > 64 << 20:
        chunk = max(1, (64 << 20) // per_row)
    tickets = bool(d["moving"] and seq == 1 and not d["inlaunch_off"] and batch * heads <= 65536)
    chunks = []
    for r0 in range(0, seq, chunk):
        nr = min(chunk, seq - r0)
        sa = seq_all if chunk == seq else seq_all - seq + r0 + nr
        ns_c = nsplit if d["moving"] else -(-sa // 128)
        chunks.append("%d:%d:%d:%d:%d:%d:%d" % (r0, nr, sa, ns_c, tickets, not tickets and (ns_c > 1 or bool(d["moving"])), bool(d["moving"]) and seq == 1))
    lds = ((seq_all + 3) // 4 * 4 + 256) * 4
    whole_error = ERR_MOVING_PAST if d["moving"] else ERR_TOO_LONG if lds > 160 * 1024 else "-"
    return "mirror=%d,%d split=%d,%d whole=1,%d o16=%d inlaunch=%d nsplit=%d per_row=%d chunk=%d bytes=%d lds=%d chunks=%s|%s|%s" % (
        mirror[0], mirror[1], split[0], split[1], whole_error != "-", d["executing"], 0 if d["inlaunch_off"] else 1, nsplit, per_row, chunk,
        batch * chunk * per_row, lds, ",".join(chunks), split_error, whole_error)


def parse_mha(line):
    fields, split_error, whole_error = line.split("|")
    p = dict(kv.split("=") for kv in fields.split())
    for k in ("mirror", "split", "whole"):
        tried, refused = p[k].split(",")
        p[k] = tried == "1" and refused == "0"          # offered
    p["chunks"] = [tuple(int(x) for x in c.split(":")) for c in p["chunks"].split(",")]
    p["split_error"], p["whole_error"] = split_error, whole_error
    return p


def server(p):
    """who serves when the run time refuses nobody (a mirror and scratch can be allocated)"""
    if p["mirror"]:
        return "mirror"
    if p["split_error"] != "-":
        return "error: " + p["split_error"]
    if p["split"]:
        return "split"
    return "whole" if p["whole_error"] == "-" else "error: " + p["whole_error"]


def run_mha(exe):
    cases = mha_cases()
    return dict(zip(cases, run_program(exe, ["mha " + " ".join(str(int(d[k])) for k in MHA_ORDER) for d in cases.values()])))


def test_the_server_of_every_attention_call_follows_the_rule(program):
    got = run_mha(program)
    for name, d in mha_cases().items():
        assert got[name] == want_mha(d), name


def test_the_attention_cases_are_what_they_are_named_for(program):
    p = {n: parse_mha(l) for n, l in run_mha(program).items()}
    srv = {n: server(v) for n, v in p.items()}
    # the 14 shapes: the mirror takes every one; without it the split from two ranges on for head sizes 64 / 128 / 256, else the whole kernel
    assert [srv["shape%d-kv1" % i] for i in range(14)] == ["mirror"] * 14
    fp32 = ["split", "split", "split", "split", "split", "whole", "whole", "split", "whole", "split", "whole", "split", "split", "whole"]
    assert [srv["shape%d-kv0" % i] for i in range(14)] == fp32
    assert [srv["shape%d-kv1-unsupported" % i] for i in range(14)] == fp32
    assert [srv["shape%d-no-split" % i] for i in range(14)] == ["whole"] * 14
    assert all(p["shape%d-kv1-executing" % i]["o16"] == "1" and p["shape%d-kv1" % i]["o16"] == "0" for i in range(14))
    assert (srv["keys128"], p["keys128"]["nsplit"], srv["keys129"], p["keys129"]["nsplit"]) == ("whole", "1", "split", "2")
    assert srv["hs80"] == "whole"
    assert [srv["%s-misaligned-kv%d" % (w, kv)] for w in "qkv" for kv in (0, 1)] == ["whole", "whole", "whole", "whole", "split", "split"]
    assert (srv["rows65535"], srv["rows65536"], srv["heads65535"], srv["heads65536"]) == ("split", "whole", "split", "whole")
    assert p["whole-lds-exact"]["lds"] == str(160 * 1024) and srv["whole-lds-exact"] == "whole"
    assert srv["whole-40705"] == srv["whole-40706"] == "error: " + ERR_TOO_LONG
    # the chunked prompt: 32 heads x 5 ranges x 258 floats per row, 520 rows = 85.9 MB against the 64 MB cap
    q = p["long-masked"]
    assert (q["per_row"], q["chunk"], q["chunks"]) == ("165120", "406", [(0, 406, 406, 4, 0, 1, 0), (406, 114, 520, 5, 0, 1, 0)])
    assert int(q["bytes"]) == 406 * 165120 <= 64 << 20 < 520 * 165120
    assert p["long-unmasked"]["chunks"] == [(0, 520, 520, 5, 0, 1, 0)] and p["long-batch2"]["chunks"] == [(0, 520, 520, 5, 0, 1, 0)]
    assert int(p["long-batch2"]["bytes"]) == 2 * 520 * 165120
    # a moving length: the layout of the longest context, tickets up to 65536 (row, head) pairs, a merge launch only without them
    assert srv["moving-kv1"] == "mirror" and p["moving-kv1"]["inlaunch"] == "1" and p["moving-no-inlaunch-kv1"]["inlaunch"] == "0"
    assert srv["moving-kv0"] == "split" and p["moving-kv0"]["nsplit"] == "16" and p["moving-kv0"]["chunks"] == [(0, 1, 300, 16, 1, 0, 1)]
    assert p["moving-no-inlaunch"]["chunks"] == [(0, 1, 300, 16, 0, 1, 1)]
    assert srv["moving-no-split"] == "split" and srv["moving-one-range"] == "split" and p["moving-one-range"]["chunks"] == [(0, 1, 5, 1, 1, 0, 1)]
    assert p["moving-65536-pairs"]["chunks"][0][4:6] == (1, 0) and p["moving-65538-pairs"]["chunks"][0][4:6] == (0, 1)
    assert srv["moving-seq2-kv0"] == srv["moving-seq2-kv1"] == srv["moving-hs80-kv0"] == "error: " + ERR_MOVING_SHAPE
    assert srv["moving-hs80-kv1"] == "mirror"          # (the error stands behind it: a call without a mirror ends there)
    assert p["moving-hs80-kv1"]["split_error"] == ERR_MOVING_SHAPE
    assert srv["moving-q-misaligned"] == "error: " + ERR_MOVING_PAST
    assert [srv[n] for n in ("mirror-hs-260", "mirror-hs-12", "mirror-batch-kv-heads", "mirror-q-step", "mirror-k-step")] == ["whole", "whole", "whole", "split", "whole"]


def test_the_partials_are_sized_by_one_function(program):
    """mha_f32_partials_bytes is what both the attention entry and the route's prepare_plan_device ask: batch * chunk * per_row of the plan"""
    cases, got = mha_cases(), run_mha(program)
    names = [n for n in cases if not n.startswith("whole-")]
    cmds = []
    for n in names:
        d, p = cases[n], parse_mha(got[n])
        cmds.append("partials %d %d %d %d %d" % (d["batch"], int(p["chunk"]), d["heads"], d["head_size"], d["n_ctx"] if d["moving"] else d["seq_all"]))
    for n, line in zip(names, run_program(program, cmds)):
        p = parse_mha(got[n])
        assert int(line) == int(p["bytes"]) == cases[n]["batch"] * int(p["chunk"]) * int(p["per_row"]), n
    # the route sizes a plan's scratch for the longest context: 32 heads x 16 ranges x 130 floats
    assert run_program(program, ["partials 1 1 32 128 2048"]) == [str(32 * 16 * 130 * 4)]


# ---- binary nodes and the lazy peephole -----------------------------------------------------------------------------------------------------------
def packed_nb(ne):
    nb, s = [], 4
    for e in ne:
        nb.append(s)
        s *= e
    return nb


def binary_cases():
    """name -> (aligned16, dense_off, ne0, nb0, ne1, nb1, nbd)"""
    c = {}

    def add(name, ne0, ne1=None, nb0=None, nb1=None, nbd=None, aligned16=1, dense_off=0):
        ne1 = ne1 or ne0
        c[name] = (aligned16, dense_off, list(ne0), nb0 or packed_nb(ne0), list(ne1), nb1 or packed_nb(ne1), nbd or packed_nb(ne0))

    add("total-4095", (4095, 1, 1, 1))
    add("total-4092", (4, 1023, 1, 1))
    add("total-4096", (4, 1024, 1, 1))
    add("64x64", (64, 64, 1, 1))
    add("64x64-4d", (64, 4, 4, 4))
    add("ne00-62", (62, 68, 1, 1))
    add("60x68", (60, 68, 1, 1))
    add("60x69", (60, 69, 1, 1))
    add("rowvec", (64, 64, 1, 1), ne1=(64, 1, 1, 1))
    add("rowvec-zero-strides", (64, 64, 1, 1), ne1=(64, 1, 1, 1), nb1=[4, 0, 0, 0])       # as ne hands a broadcast operand over
    add("rowvec-zero-extents", (64, 64, 1, 1), ne1=(64, 0, 0, 0), nb1=[4, 0, 0, 0])       # an extent below 1 counts as 1
    add("rowvec-stride-8", (64, 64, 1, 1), ne1=(64, 1, 1, 1), nb1=[8, 512, 512, 512])
    add("colvec", (64, 64, 1, 1), ne1=(1, 64, 1, 1))
    add("broadcast-dim1", (64, 64, 2, 1), ne1=(64, 1, 2, 1))
    add("misaligned", (64, 64, 1, 1), aligned16=0)
    add("src0-row-stride", (64, 64, 1, 1), nb0=[4, 272, 272 * 64, 272 * 64])
    add("src1-row-stride", (64, 64, 1, 1), nb1=[4, 272, 272 * 64, 272 * 64])
    add("dst-row-stride", (64, 64, 1, 1), nbd=[4, 272, 272 * 64, 272 * 64])
    add("one-row-any-stride", (4096, 1, 1, 1), nb0=[4, 99, 77, 55])                       # the stride of an extent of 1 is never used
    add("switched-off", (64, 64, 1, 1), dense_off=1)
    return c


def want_binary(aligned16, dense_off, ne0, nb0, ne1, nb1, nbd):
    ne1 = [max(e, 1) for e in ne1]

    def dense(ne, nb):
        want = packed_nb(ne)
        return all(e == 1 or b == w for e, b, w in zip(ne, nb, want))

    total = ne0[0] * ne0[1] * ne0[2] * ne0[3]
    same = ne1 == list(ne0)
    rowvec = ne1 == [ne0[0], 1, 1, 1] and nb1[0] == 4
    ok = bool(not dense_off and total >= 4096 and ne0[0] % 4 == 0 and dense(ne0, nb0) and dense(ne0, nbd) and ((same and dense(ne1, nb1)) or rowvec) and aligned16)
    return "dense=%d bcols4=%d" % (ok, ne0[0] // 4 if ok and not same else 0)


def test_binary_nodes_take_the_dense_kernel_inside_its_conditions(program):
    cases = binary_cases()
    got = dict(zip(cases, run_program(program, ["binary " + " ".join(str(x) for part in c for x in (part if isinstance(part, list) else [part]))
                                                for c in cases.values()])))
    for name, c in cases.items():
        assert got[name] == want_binary(*c), name
    dense = sorted(n for n in cases if got[n].startswith("dense=1"))
    assert dense == sorted(["total-4096", "64x64", "64x64-4d", "60x69", "rowvec", "rowvec-zero-strides", "rowvec-zero-extents", "one-row-any-stride"])
    assert got["64x64"] == "dense=1 bcols4=0" and got["rowvec"] == "dense=1 bcols4=16" and got["60x68"] == "dense=0 bcols4=0"   # 4080 elements


NODE_SRC, NODE_DST, OTHER, OUT, GAMMA = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000


def lazy_cases():
    """name -> (kind, src, dst, cols, n, same_stream, a, b, d, ne0, nb0, ne1, nb1, nbd)"""
    c = {}
    rows, cols = 3, 64
    full, vec = [cols, rows, 1, 1], [cols, 1, 1, 1]

    def add(name, kind, a, b, d, ne1=None, nb1=None, ne0=None, nb0=None, nbd=None, same_stream=1, n=rows * cols):
        ne0 = ne0 or full
        ne1 = ne1 or ne0
        c[name] = (kind, NODE_SRC, NODE_DST, cols, n, same_stream, a, b, d, ne0, nb0 or packed_nb(ne0), ne1, nb1 or packed_nb(ne1), nbd or packed_nb(ne0))

    add("norm-then-weight", 1, NODE_DST, GAMMA, OUT, ne1=vec)
    add("norm-then-weight-zero-strides", 1, NODE_DST, GAMMA, OUT, ne1=vec, nb1=[4, 0, 0, 0])
    add("norm-in-place", 1, NODE_DST, GAMMA, NODE_DST, ne1=vec)
    add("norm-over-its-input", 1, NODE_DST, GAMMA, NODE_SRC, ne1=vec)
    add("norm-as-second-operand", 1, GAMMA, NODE_DST, OUT, ne1=vec)
    add("norm-times-full-tensor", 1, NODE_DST, OTHER, OUT)
    add("norm-weight-stride-8", 1, NODE_DST, GAMMA, OUT, ne1=vec, nb1=[8, 512, 512, 512])
    add("norm-other-size", 1, NODE_DST, GAMMA, OUT, ne1=vec, n=2 * cols)
    add("norm-other-stream", 1, NODE_DST, GAMMA, OUT, ne1=vec, same_stream=0)
    add("norm-not-consumed", 1, OTHER, GAMMA, OUT, ne1=vec)
    add("norm-strided-dst", 1, NODE_DST, GAMMA, OUT, ne1=vec, nbd=[4, 272, 816, 816])
    add("silu-first", 2, NODE_DST, OTHER, OUT)
    add("silu-second", 2, OTHER, NODE_DST, OUT)
    add("silu-both", 2, NODE_DST, NODE_DST, OUT)
    add("silu-in-place", 2, NODE_DST, OTHER, NODE_DST)
    add("silu-over-its-input", 2, OTHER, NODE_DST, NODE_SRC)
    add("silu-times-row-vector", 2, NODE_DST, GAMMA, OUT, ne1=vec)
    add("silu-strided-up", 2, NODE_DST, OTHER, OUT, nb1=[4, 272, 816, 816])
    add("silu-other-stream", 2, NODE_DST, OTHER, OUT, same_stream=0)
    add("silu-not-consumed", 2, OTHER, GAMMA, OUT)
    add("nothing-recorded", 0, NODE_DST, OTHER, OUT)
    add("null-operand", 2, NODE_DST, 0, OUT)
    return c


def want_lazy(kind, src, dst, cols, n, same_stream, a, b, d, ne0, nb0, ne1, nb1, nbd):
    total = ne0[0] * ne0[1] * ne0[2] * ne0[3]
    if not (kind and a and b and d and same_stream and nb0 == packed_nb(ne0) and nbd == packed_nb(ne0) and total == n) or d in (src, dst):
        return "plain"
    if kind == 1:
        return "norm_mul" if a == dst and ne0[0] == cols and ne1[0] == cols and max(ne1[1:]) <= 1 and nb1[0] == 4 else "plain"
    if list(ne1) != list(ne0) or nb1 != packed_nb(ne1) or (a == dst) == (b == dst):
        return "plain"
    return "silu_first" if a == dst else "silu_second"


def test_the_lazy_multiply_fuses_only_what_consumes_the_recorded_node(program):
    cases = lazy_cases()
    got = dict(zip(cases, run_program(program, ["lazy " + " ".join(str(x) for part in c for x in (part if isinstance(part, list) else [part]))
                                                for c in cases.values()])))
    for name, c in cases.items():
        assert got[name] == want_lazy(*c), name
    fused = {n: g for n, g in got.items() if g != "plain"}
    assert fused == {"norm-then-weight": "norm_mul", "norm-then-weight-zero-strides": "norm_mul", "silu-first": "silu_first", "silu-second": "silu_second"}


def test_the_program_is_clean_under_the_sanitizers(tmp_path, program):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path / "device_plan_san")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC] + SOURCES + ["-o", exe], check=True, capture_output=True, text=True, timeout=300)
    script = [c for c, _ in table_script()]
    assert run_program(exe, script) == run_program(program, script)
    assert run_mha(exe) == run_mha(program)
    for cases, word in ((binary_cases(), "binary"), (lazy_cases(), "lazy")):
        cmds = [word + " " + " ".join(str(x) for part in c for x in (part if isinstance(part, list) else [part])) for c in cases.values()]
        assert run_program(exe, cmds) == run_program(program, cmds)

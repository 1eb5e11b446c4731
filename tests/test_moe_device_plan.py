"""The host side of the block entries' device-grouped pass (neural-speed_amd/csrc/ns_moe_plan.cpp), checked without a GPU.

moe_ffn_plan gains a candidate `device` between the fused launches and the grouped pass: with the key "moe_ffn_device_rows" at 0 every
decision is what it was (the fact grid of tests/test_moe_plan.py, its rule want_ffn), with the key set the candidate follows the rule restated
here (want_device).  moe_chunk_plan is the layout moe_pair_sort_kernel must reproduce on the device - the pair layout of moe_pair_plan cut
into chunks of at most R rows of one expert - and moe_chunk_slots the host's bound of its chunk count; moe_chunk_rows the rows a workgroup
can stage.  A host program (tests/tools/moe_device_plan_main.cpp) prints them; it is built once with the library's compiler and once with
g++ under the address and undefined-behaviour sanitizers."""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

from test_moe_plan import CSRC, FACTS, KNOBS, ORDER, ROOT, compiler, decisions, want_ffn

SOURCES = [os.path.join(ROOT, "tests", "tools", "moe_device_plan_main.cpp"), os.path.join(CSRC, "ns_moe_plan.cpp")]
PAD = 1 << 20
RS = [1, 2, 3, 7, 16]
ORDER_DEV = ORDER[:4] + ["ffn_device_rows"] + ORDER[4:] + ["gu_kstep", "dn_kstep", "i8_mode"]
DEV = dict(ffn_device_rows=0, gu_kstep=128, dn_kstep=128, i8_mode=0)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    hipcc = compiler()
    if not hipcc:
        pytest.skip("the library's compiler is not installed")
    exe = str(tmp_path_factory.mktemp("moe_device_plan") / "moe_device_plan")
    subprocess.run([hipcc, "-std=c++20", "-x", "hip", "--offload-arch=gfx950", "--cuda-host-only", "-Wall", "-Werror", "-I", CSRC] + SOURCES + ["-o", exe],
                   check=True, capture_output=True, text=True, timeout=300)
    return exe


def run(exe, mode, text):
    out = subprocess.run([exe, mode], input=text, check=True, capture_output=True, text=True, timeout=120)
    assert out.stderr == "", out.stderr
    return out.stdout.splitlines()


# ---- which server takes a call ---------------------------------------------------------------------------------------------------------------
def device_cases():
    """knobs + facts of every case: today's grid with the key at 0, then the key set"""
    cases = [dict(d, **DEV) for entry, d in decisions() if entry == "ffn"]
    base = dict(KNOBS, **FACTS)

    def add(**kw):
        d = dict(base, **DEV)
        assert set(kw) <= set(d)
        d.update(kw)
        cases.append(d)

    for rows in (9, 31, 64):
        for m in (1, 8, 9, 16, 31, 32, 33, 64, 65):
            for cap in (0, 1):
                add(ffn_device_rows=rows, m=m, capturing=cap)
            for which in ("gate_f8", "up_f8", "down_f8"):
                add(ffn_device_rows=rows, m=m, **{which: 1})
            add(ffn_device_rows=rows, m=m, single_span=0)
            add(ffn_device_rows=rows, m=m, gate_up_one_format=0)
            add(ffn_device_rows=rows, m=m, i8_mode=1)
            add(ffn_device_rows=rows, m=m, k=192)                          # one and a half 4-bit k-steps ...
            add(ffn_device_rows=rows, m=m, k=192, gu_kstep=64)             # ... three 8-bit ones
            add(ffn_device_rows=rows, m=m, ff=528)
            add(ffn_device_rows=rows, m=m, ff=576, dn_kstep=64)
            add(ffn_device_rows=rows, m=m, ff=576, dn_kstep=128)
            add(ffn_device_rows=rows, m=m, k=96, ff=96)
            add(ffn_device_rows=rows, m=m, ffn_fused=0)
            add(ffn_device_rows=rows, m=m, ffn_grouped_rows=16)
            add(ffn_device_rows=rows, m=m, gemv_rows=-1)
    for m, n_used in ((512, 2), (513, 2), (128, 8), (129, 8), (1024, 1), (1025, 1)):     # the sort's 1024 pairs
        add(ffn_device_rows=2000, m=m, n_used=n_used)
    add(ffn_device_rows=-1, m=9)
    return cases


def want_device(d):
    tried = d["ffn_device_rows"] > 0 and d["m"] <= d["ffn_device_rows"]
    whole = d["gu_kstep"] > 0 and d["dn_kstep"] > 0 and d["k"] % d["gu_kstep"] == 0 and d["ff"] % d["dn_kstep"] == 0
    refused = bool(d["gate_f8"] or d["up_f8"] or d["down_f8"] or not d["single_span"] or not d["gate_up_one_format"] or not whole or
                   d["m"] * d["n_used"] > 1024 or d["i8_mode"])
    return tried, refused


def run_decisions(exe):
    return run(exe, "plans", "".join(" ".join(str(int(d[k])) for k in ORDER_DEV) + "\n" for d in device_cases()))


def test_the_servers_of_a_block_call_follow_the_rule(program):
    cases, got = device_cases(), run_decisions(program)
    assert len(got) == len(cases)
    seen = set()
    for d, line in zip(cases, got):
        fused, device, grouped = line.split()
        assert fused + " " + grouped == want_ffn(d), (d, line)            # today's two candidates: untouched by the new key
        tried, refused = want_device(d)
        if d["ffn_device_rows"] == 0:
            assert device.split("=")[1].split(",")[0] == "0", (d, line)   # never tried: every decision is today's
        else:
            assert device == "device=%d,%d" % (tried, refused), (d, line)
            seen.add((tried, refused))
    assert seen == {(False, False), (False, True), (True, False), (True, True)}


# ---- the layout ------------------------------------------------------------------------------------------------------------------------------
def by_counts(counts, rng=None):
    """one selection per row, count[e] rows of expert e, shuffled"""
    col = [e for e, c in enumerate(counts) for _ in range(c)]
    if rng is not None:
        rng.shuffle(col)
    return np.asarray(col, np.int64).reshape(-1, 1)


def tables():
    """(name, ids [m][n_used], n_as, ids_stride)"""
    rng = np.random.default_rng(11)
    t = []
    t.append(("random_2_of_4", np.stack([rng.permutation(4)[:2] for _ in range(12)]), 4, 2))
    t.append(("random_2_of_8", np.stack([rng.permutation(8)[:2] for _ in range(31)]), 8, 3))
    t.append(("random_with_repeats", rng.integers(0, 5, (17, 3)), 5, 3))
    t.append(("all_on_one_expert", np.full((9, 2), 2), 4, 2))
    t.append(("row_e_e", np.array([[1, 1], [0, 1], [1, 1], [3, 3]]), 4, 2))
    t.append(("bad_ids", np.array([[-1, 2], [4, 4], [0, -1], [4, 1], [-1, -1], [2, 0]]), 4, 3))
    t.append(("all_bad", np.array([[-1, 9], [9, -1]]), 4, 2))
    t.append(("an_expert_with_none", np.array([[0, 1], [3, 0], [1, 3], [0, 3]]), 4, 2))
    for R in RS:                                                               # groups of exactly R, R + 1 and 2 R pairs (and one of 1)
        t.append(("counts_R_R1_2R_for_%d" % R, by_counts([R, R + 1, 2 * R, 1], rng), 4, 1))
    t.append(("m_1", np.array([[3, 0]]), 4, 2))
    t.append(("most_pairs", np.stack([rng.permutation(8)[:2] for _ in range(512)]), 8, 2))
    return [(n, np.asarray(i, np.int64), a, s) for n, i, a, s in t]


def chunk_input():
    lines, keys = [], []
    for name, ids, n_as, stride in tables():
        m, n_used = ids.shape
        full = np.full((m, stride), PAD, np.int64)
        full[:, :n_used] = ids
        for R in RS:
            lines.append("%d %d %d %d %d %s" % (m, n_used, n_as, stride, R, " ".join(str(int(v)) for v in full.reshape(-1))))
            keys.append((name, ids, n_as, R))
    # refused: no rows, no selections, no experts, a short stride, R outside 1 .. 16 (m * ids_stride ids each)
    for bad in ("0 2 4 2 3", "2 0 4 2 3 0 0 0 0", "2 2 0 2 3 0 0 0 0", "2 3 4 2 3 0 0 0 0", "2 2 4 2 0 0 0 0 0", "2 2 4 2 17 0 0 0 0"):
        lines.append(bad)
        keys.append(None)
    return "\n".join(lines) + "\n", keys


def parse(line):
    if line == "refused":
        return None
    d = {}
    for kv in line.split():
        k, v = kv.split("=")
        d[k] = v
    ints = lambda s: [int(x) for x in s.split(",")] if s else []
    out = {k: ints(d[k]) for k in ("offset", "count", "src_row", "pos")}
    out["pairs"], out["slots"] = int(d["pairs"]), int(d["slots"])
    out["chunks"] = [tuple(int(x) for x in c.split(":")) for c in d["chunks"].split(",")] if d["chunks"] else []
    return out


def restate(ids, n_as, R):
    """ns_moe_plan.h, moe_chunk_plan: group order, stable; chunks by expert, then by position"""
    m, n_used = ids.shape
    good = [(t, i) for t in range(m) for i in range(n_used) if 0 <= ids[t, i] < n_as]
    order = sorted(good, key=lambda ti: int(ids[ti]))                # (sorted is stable: (row, selection) ascending inside a group)
    src_row = [t for t, _ in order] + [-1] * (m * n_used - len(order))
    pos = [-1] * (m * n_used)
    for j, (t, i) in enumerate(order):
        pos[t * n_used + i] = j
    count = [sum(1 for ti in good if ids[ti] == e) for e in range(n_as)]
    offset = [sum(count[:e]) for e in range(n_as)]
    chunks = [(e, offset[e] + c, min(R, count[e] - c)) for e in range(n_as) for c in range(0, count[e], R)]
    return dict(pairs=len(order), offset=offset, count=count, src_row=src_row, pos=pos, chunks=chunks)


@pytest.fixture(scope="module")
def chunk_plans(program):
    text, keys = chunk_input()
    got = [parse(line) for line in run(program, "chunks", text)]
    assert len(got) == len(keys)
    return got


def test_the_chunk_plan_follows_the_rule(chunk_plans):
    _, keys = chunk_input()
    for key, p in zip(keys, chunk_plans):
        if key is None:
            assert p is None
            continue
        name, ids, n_as, R = key
        assert p is not None, (name, R)
        want = restate(ids, n_as, R)
        for field, v in want.items():
            assert p[field] == v, (name, R, field)
        m, n_used = ids.shape
        P = m * n_used
        assert p["slots"] == (P + min(n_as, P) * (R - 1)) // R and len(p["chunks"]) <= p["slots"], (name, R)
        # the chunks tile [0, pairs) in order, each inside one expert's group and no longer than R
        at = 0
        for e, first, rows in p["chunks"]:
            assert first == at and 1 <= rows <= R and p["offset"][e] <= first and first + rows <= p["offset"][e] + p["count"][e], (name, R)
            at += rows
        assert at == p["pairs"], (name, R)


def test_the_cases_cover_what_they_are_named_for(chunk_plans):
    _, keys = chunk_input()
    by = {(k[0], k[3]): p for k, p in zip(keys, chunk_plans) if k is not None}
    assert by[("all_on_one_expert", 7)]["chunks"] == [(2, 0, 7), (2, 7, 7), (2, 14, 4)]
    assert by[("all_bad", 3)]["chunks"] == [] and by[("all_bad", 3)]["src_row"] == [-1] * 4
    assert by[("bad_ids", 2)]["pairs"] == 5 and by[("bad_ids", 2)]["pos"][8:10] == [-1, -1]
    p = by[("row_e_e", 16)]
    assert p["pos"][0] + 1 == p["pos"][1] and p["src_row"][p["pos"][0]] == p["src_row"][p["pos"][1]] == 0
    assert by[("an_expert_with_none", 3)]["count"][2] == 0
    for R in RS:
        p = by[("counts_R_R1_2R_for_%d" % R, R)]
        rows = lambda e: [r for ee, _, r in p["chunks"] if ee == e]
        assert rows(0) == [R] and rows(1) == [R, 1] and rows(2) == [R, R] and rows(3) == [1]
    assert by[("most_pairs", 16)]["pairs"] == 1024


def test_the_slot_bound_holds_for_every_small_table(program):
    """moe_chunk_slots against every id table with ids in [-1, n_as) of up to 4 rows, 2 selections, 3 experts: the program enumerates the
    tables through moe_chunk_plan, the most chunks any count vector gives are restated here"""
    cases = [(m, n_used, n_as, R) for m in (1, 2, 3, 4) for n_used in (1, 2) for n_as in (1, 2, 3) for R in RS]
    got = run(program, "maxchunks", "".join("%d %d %d %d\n" % c for c in cases))
    assert len(got) == len(cases)
    for (m, n_used, n_as, R), line in zip(cases, got):
        most, slots = (int(kv.split("=")[1]) for kv in line.split())
        P = m * n_used
        want = max(sum(-(-c // R) for c in counts) for counts in itertools.product(range(P + 1), repeat=n_as) if sum(counts) <= P)
        assert most == want, (m, n_used, n_as, R)
        assert slots == (P + min(n_as, P) * (R - 1)) // R and most <= slots, (m, n_used, n_as, R)


def test_chunk_rows(program):
    """min(16, cap or 16, floor(64 KiB / ((ks * kstep + 8) * 2))), at least 1"""
    cases = [((256, 128, 0), 16), ((4096, 128, 0), 7), ((14336, 128, 0), 2), ((14336, 64, 0), 2), ((4096, 128, 3), 3), ((4096, 128, 16), 7),
             ((256, 128, 1), 1), ((256, 64, 5), 5), ((40000, 128, 0), 1), ((2040, 128, 0), 15), ((2048, 128, 0), 15), ((1920, 128, 0), 16)]
    got = run(program, "rows", "".join("%d %d %d\n" % c for c, _ in cases))
    assert [int(x) for x in got] == [w for _, w in cases]
    for (k, kstep, cap), w in cases:
        ks = -(-k // kstep)
        assert w == max(1, min(16, cap or 16, (64 * 1024) // ((ks * kstep + 8) * 2)))


def test_the_program_is_clean_under_the_sanitizers(tmp_path, program, chunk_plans):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path / "moe_device_plan_san")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC] + SOURCES + ["-o", exe], check=True, capture_output=True, text=True, timeout=300)
    text, _ = chunk_input()
    assert [parse(line) for line in run(exe, "chunks", text)] == chunk_plans
    assert run_decisions(exe) == run_decisions(program)
    small = "".join("%d %d %d %d\n" % c for c in [(4, 2, 3, 2), (3, 2, 2, 16), (4, 1, 3, 1)])
    assert run(exe, "maxchunks", small) == run(program, "maxchunks", small)

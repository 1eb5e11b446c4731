"""attn_plan (neural-speed_amd/csrc/ns_attn_plan.cpp) is the one place that decides which attention kernel serves a call: path, template
arguments, grid, LDS, context ranges, partials.  A host program (tests/tools/attn_plan_main.cpp, built with the library's compiler, nothing
launched) prints the plan for a grid of calls; the rule it must follow — the table "What tests which launch path" of
docs/kernels/attention.md — is written out here independently."""
import importlib.util
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "neural-speed_amd", "csrc")
MAIN = os.path.join(ROOT, "tests", "tools", "attn_plan_main.cpp")
CAUSAL, ALIBI, TANH = 1, 2, 8  # NS_ATTN_FLAG_IS_* (include/ns_bestla.h)
DEFAULTS = dict(attn_stream=1, attn_mfma2_rows=128, attn_inlaunch=0, attn_heads_first=-1, wg_target=1024, min_keys=128, wg_target_s=256, min_keys_s=32,
                pipe=1, pvar=-1, no_mfma=0, no_xcd_map=0, v1=0, dyn_ranges=1, no_partials=0, alibi_heads=0)
TICKET_CAP = 65536


def compiler():
    """HIPCC of the library's Makefile (the environment's HIPCC wins there too)"""
    with open(os.path.join(CSRC, "Makefile")) as f:
        default = re.search(r"^HIPCC\s*\?=\s*(\S+)", f.read(), re.M).group(1)
    path = os.environ.get("HIPCC", default)
    return path if os.path.exists(path) else shutil.which(path)


def num(v):
    try:
        return int(v)
    except ValueError:
        try:
            return float(v)
        except ValueError:
            return v


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    hipcc = compiler()
    if not hipcc:
        pytest.skip("the library's compiler is not installed")
    exe = str(tmp_path_factory.mktemp("attn_plan") / "attn_plan")
    subprocess.run([hipcc, "-std=c++20", "-x", "hip", "--offload-arch=gfx950", "--cuda-host-only", "-Wall", "-Werror", "-I", CSRC, MAIN, "-o", exe],
                   check=True, capture_output=True, text=True, timeout=300)
    out = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=120).stdout
    rows = []
    for line in out.splitlines():
        call, plan = line.split(" | ")
        plan, why = plan.split(" why=")
        i = {k: num(v) for k, v in (kv.split("=") for kv in call.split())}
        o = {k: num(v) for k, v in (kv.split("=") for kv in plan.split())}
        o["why"] = why
        rows.append((i, o))
    return rows


def ceil_div(a, b):
    return -(-a // b)


def knobs_of(i):
    kn = dict(DEFAULTS)
    if i["knob"] != "none":
        kn[i["knob"]] = i["kval"]
    return kn


def strides(i):
    """(k_head_size, k_sl, k_head_num, k_bs), (v ...) in halves"""
    rows = i["cap"] or i["slkv"]
    row = {2: i["hs"] + 4, 4: 1 << 24}.get(i["klay"], i["hs"])
    k = v = (1, row, rows * row, i["hkv"] * rows * row)
    if i["klay"] == 1:
        k = (rows, 1, k[2], k[3])
    if i["klay"] in (3, 4):
        k = v = (1, i["hkv"] * i["hs"] if i["klay"] == 3 else row, i["hs"], k[3] if i["klay"] == 3 else i["hkv"] * i["hs"])
    if i["klay"] == 5:
        k = v = (1, i["ksl"] or i["hkv"] * i["hs"], i["hs"], i["kbs"] or i["hkv"] * rows * i["hs"])
    return k, v


def in32(sl_kv, k_sl, v_sl):
    return (sl_kv * k_sl + 256) * 2 < 1 << 32 and (sl_kv * v_sl + 256) * 2 < 1 << 32


def range_rule(kn, blocks, ring, batch_keys, heavy):
    target = kn["wg_target_s"] if ring else kn["wg_target"]
    if ring and heavy and blocks >= 64:
        target *= 2
    return dict(target=target, min_keys=kn["min_keys_s"] if ring else kn["min_keys"], batch_keys=batch_keys if ring else 0,
                single_below=128 if ring and blocks >= 32 else 0)


def nsplit_of(r, blocks, sl_kv):
    if sl_kv <= r["single_below"]:
        return 1
    n = min(ceil_div(r["target"], blocks), max(1, ceil_div(sl_kv, r["min_keys"])), 64)
    if r["batch_keys"] > 0 and n > 1:
        kps = ceil_div(ceil_div(sl_kv, n), r["batch_keys"]) * r["batch_keys"]
        if ceil_div(sl_kv, kps) * blocks >= 128:
            n = ceil_div(sl_kv, kps)
    return n


def groups(g_full):
    G = 1 if g_full <= 1 else 2 if g_full == 2 else 4 if g_full <= 4 else 8
    return G, ceil_div(g_full, G)


def ws_bytes(kn, i):
    """bestla_fusion_attn_workspace_size: the most any rule asks for"""
    _, chunks = groups(i["hn"] // max(1, i["hkv"]))
    blocks = i["hkv"] * chunks * i["slq"] * i["bs"]
    sl_kv = i["cap"] or i["slkv"]
    n = max(nsplit_of(range_rule(kn, blocks, ring, 0, heavy), blocks, sl_kv) for ring, heavy in ((False, False), (True, False), (True, True)))
    return i["bs"] * i["slq"] * i["hn"] * n * (2 + i["hs"]) * 4 if n > 1 else 0


def stage_bytes(hs):
    return 64 * hs * 2 + (hs // 16) * (64 * 32 + 128)


def expected(i):
    """the fields of the plan the rule determines (a refusal: path and why)"""
    kn = knobs_of(i)
    hs, slq, slkv, hn, hkv, bs, flags = (i[k] for k in ("hs", "slq", "slkv", "hn", "hkv", "bs", "flags"))
    refuse = lambda why: dict(path="REFUSED", why=why)
    if hs < 1 or hs > 256:
        return refuse("attention: head_size must be 1..256")
    if hkv < 1 or hn % hkv:
        return refuse("attention: head_num must be a multiple of heads_kv")
    if flags & CAUSAL and slq > slkv:
        return refuse("attention: causal needs sl_q <= sl_kv")
    if slq < 1 or slkv < 1:
        return refuse("attention: empty sequence")
    all_heads = kn["alibi_heads"] if kn["alibi_heads"] > 0 else hn
    off = kn["alibi_heads"] - hn if kn["alibi_heads"] > 0 else 0
    if off < 0 or off + hn > all_heads:
        return refuse("attention: head partition (ns_hip_attn_set_head_partition) does not contain this call's heads")
    if hn > 65535 or bs > 65535:
        return refuse("attention: head_num / batch_size above the grid limit")
    if i["cap"] and (slq != 1 or i["cap"] < slkv):
        return refuse("attention: a moving context length is served for decode steps (one query row) within the cache's capacity")
    e = dict(why="", phs=64 if hs <= 64 else 128 if hs <= 128 else 256, off=off, lf=1 << int(math.floor(math.log2(all_heads))))
    k, v = strides(i)
    rows_ok = k[0] == 1 and v[0] == 1 and all(s % 8 == 0 for s in k[1:] + v[1:])  # (K and V themselves are aligned in every case)
    biased = bool(flags & (ALIBI | TANH))
    exact = hs in (64, 128)
    only128 = biased or not exact
    nqb = ceil_div(slq, 128)
    rows128 = slq >= (16 if only128 else kn["attn_mfma2_rows"]) and nqb * hn * bs < 1 << 31 and (biased or i["scale"] > 0)
    if not kn["no_mfma"] and slq >= 16 and hs % 8 == 0 and rows_ok and (not only128 or rows128):
        e.update(block=256, hsp=e["phs"], G=0, lpk=0, dpl=0)
        if not rows128:  # 16 .. 127 rows of head size 64 / 128 without bias (or any number of rows under a score scale that is not positive)
            return dict(e, path="ROWS64", grid=(ceil_div(slq, 64), hn, bs), lds=0, sb=0, pad=0, nqb=0, al=0, xcd=0)
        aligned = int(bool(i["dal"]) and i["d16"] != 2)  # (the row strides of dst are multiples of 4 floats in every case)
        xcd = int(not kn["no_xcd_map"] and (hkv * bs) % 8 == 0)
        e.update(grid=(nqb * hn * bs, 1, 1), lds=2 * stage_bytes(e["phs"]), sb=int(biased), pad=int(not exact and hs != 256), nqb=nqb, al=aligned)
        if kn["pipe"] and not biased and exact and in32(ceil_div(slkv, 64) * 64, k[1], v[1]):  # (whole 64-key tiles: the kernel requests the last one whole)
            pvar = kn["pvar"] if kn["pvar"] >= 0 else (3 if slkv >= 3072 else 0)
            return dict(e, path="PIPELINED", xcd=xcd | pvar << 8)
        return dict(e, path="ROWS128", xcd=xcd)
    G, chunks = groups(hn // hkv)
    dpl = 8 if hs <= 128 else 16
    blocks = hkv * slq * chunks
    e.update(block=256, hsp=0, sb=0, pad=0, nqb=0, al=0, xcd=0)
    if kn["v1"] or not rows_ok or hs % dpl or blocks > 65535:
        return dict(e, path="GENERIC", grid=(slq, hn, bs), lds=0, G=0, lpk=0, dpl=0)
    rule_kv = i["cap"] or slkv
    stream = 32 < hs <= 128 and in32(rule_kv, k[1], v[1]) and bool(i["qal"]) and kn["attn_stream"] != 0  # (Q's strides are multiples of 4 floats)
    lpk = 16 if hs > 64 else 8
    batch_keys = (4 if G * 8 <= 16 else 2) * 4 * (64 // lpk)
    rule = range_rule(kn, blocks * bs, stream or hs > 128, batch_keys if stream else 0, stream and G >= 4)
    n = 1 if kn["no_partials"] else nsplit_of(rule, blocks * bs, rule_kv)
    moving = bool(i["cap"])
    dyn = (rule["min_keys"], rule["batch_keys"], rule["single_below"]) if moving and n > 1 and kn["dyn_ranges"] and slq == 1 else (0, 0, 0)
    tick = int(n > 1 and (kn["attn_inlaunch"] != 0 or (moving and i["affil"] != 0)) and blocks * bs <= TICKET_CAP)
    hf = int(k[2] < k[1]) if kn["attn_heads_first"] < 0 else int(kn["attn_heads_first"] != 0)
    return dict(e, path="RING" if stream else "SPLIT_REGS", G=G, lpk=lpk if stream else 16, dpl=8 if stream else dpl,
                lds=65536 if stream else 4 * G * 16 * dpl * 4, nsplit=n, kps=ceil_div(rule_kv, n), chunks=chunks, gfull=hn // hkv, hf=hf, dyn=dyn,
                tick=tick, merge=int(n > 1 and not tick), pbytes=bs * slq * hn * n * (2 + hs) * 4 if n > 1 else 0,
                grid=(blocks, n, bs) if hf else (n, blocks, bs), kmove=int(moving), kdelta=1 if moving else 0)


def got(o, key):
    v = o[key]
    return tuple(int(x) for x in v.split(",")) if key in ("grid", "dyn") else v


def test_the_grid_of_cases_holds_what_it_should(plans):
    seen = lambda key: {i[key] for i, _ in plans}
    assert seen("hs") >= {24, 32, 40, 64, 80, 128, 160, 256} and seen("slq") >= {1, 4, 15, 16, 64, 127, 128, 257}
    assert seen("slkv") >= {1, 128, 129, 600, 2048, 3071, 3072, 5000} and seen("bs") >= {1, 2, 8} and seen("flags") >= {0, CAUSAL, ALIBI, TANH}
    assert {(i["hn"], i["hkv"]) for i, _ in plans} >= {(8, 8), (8, 4), (8, 2), (8, 1), (71, 1)}
    assert seen("klay") >= {0, 1, 2, 3, 4} and seen("qal") == {0, 1} and seen("dal") == {0, 1} and seen("cap") >= {0, 2048}
    assert {i["knob"] for i, _ in plans} == set(DEFAULTS) | {"none"}  # every knob at another value than its default
    assert all(i["kval"] != DEFAULTS[i["knob"]] for i, _ in plans if i["knob"] != "none")
    assert {o["path"] for _, o in plans} == {"REFUSED", "GENERIC", "SPLIT_REGS", "RING", "ROWS64", "ROWS128", "PIPELINED"}


def test_path_selectors_and_launch_shape_follow_the_rule(plans):
    wrong = []
    for i, o in plans:
        e = expected(i)
        bad = {k: (got(o, k), v) for k, v in e.items() if got(o, k) != v}
        if bad:
            wrong.append((i, bad))
    assert not wrong, (len(wrong), wrong[:3])


def test_rows_beyond_a_32_bit_descriptor_take_the_register_staged_kernels(plans):
    """the row of the path table that no GPU test reaches: in32 false"""
    far = [(i, o) for i, o in plans if i["klay"] == 4]
    by = {(i["slq"], i["slkv"]): (o["path"], o["hsp"], o["sb"], o["pad"]) for i, o in far}
    assert by[(128, 128)] == by[(257, 128)] == ("ROWS128", 128, 0, 0)  # attn_mfma2_kernel<128, false, false>
    # 127 keys lie inside a descriptor, the 128 rows of their two tiles do not: attn_mfma3_kernel requests whole tiles, and a row past the last key
    # whose offset wraps is read from inside the descriptor (tests/test_gpu_attn_far_addresses.py, the slab rule's boundary)
    assert by[(128, 127)] == by[(257, 127)] == ("ROWS128", 128, 0, 0)
    assert by[(128, 64)] == by[(257, 64)] == ("PIPELINED", 128, 0, 0)
    assert by[(1, 128)][0] == "SPLIT_REGS" and by[(1, 127)][0] == "RING"


def test_the_addresses_of_the_far_address_tests_take_the_paths_they_assert(plans):
    """tests/test_gpu_attn_far_addresses.py asserts these paths through ns_hip_attn_stats on buffers of 4 GiB and more; if a 32-bit rule moves, this
    fails first and says which number moved.  The numbers are those of tests/tools/attn_far_layout.py."""
    spec = importlib.util.spec_from_file_location("attn_far_layout", os.path.join(ROOT, "tests", "tools", "attn_far_layout.py"))
    FL = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(FL)
    far = {(i["hs"], i["slq"], i["slkv"], i["bs"], i["ksl"], i["kbs"]): o["path"] for i, o in plans if i["klay"] == 5}
    assert all((i["hn"], i["hkv"], i["flags"]) == (FL.HN, FL.HKV, CAUSAL) for i, _ in plans if i["klay"] == 5)
    n = FL.EDGE_KEYS
    (k_below, k_above), (t_below, t_above) = FL.edge_steps(n), FL.edge_steps(FL.tile_rows(n))
    assert FL.tile_rows(n) == 320 and t_above < k_below
    for hs in (64, 128):
        assert far[(hs, 1, n, 1, k_below, 0)] == "RING" and far[(hs, 1, n, 1, k_above, 0)] == "SPLIT_REGS"  # test_slab_rule_boundary_decode
        assert far[(hs, 130, n, 1, t_below, 0)] == "PIPELINED"  # test_slab_rule_boundary_prefill: below, above, between_keys_and_tiles
        assert far[(hs, 130, n, 1, t_above, 0)] == "ROWS128" and far[(hs, 130, n, 1, k_below, 0)] == "ROWS128"
        got = [far[(hs, slq, 200, 3, 0, FL.SLAB_STEP)] for slq in (1, 5, 40, 130)]  # test_forward_on_far_slabs: the batch step is no part of a rule
        assert got == ["RING", "RING", "ROWS64", "PIPELINED"], got


def test_refusals_say_why(plans):
    whys = {o["why"] for _, o in plans if o["path"] == "REFUSED"}
    assert whys == {"attention: head_size must be 1..256", "attention: head_num must be a multiple of heads_kv", "attention: causal needs sl_q <= sl_kv",
                    "attention: empty sequence", "attention: head partition (ns_hip_attn_set_head_partition) does not contain this call's heads",
                    "attention: head_num / batch_size above the grid limit",
                    "attention: a moving context length is served for decode steps (one query row) within the cache's capacity"}
    assert all(o["why"] == "" for _, o in plans if o["path"] != "REFUSED")


def test_grid_limits_and_lds_of_the_instantiation(plans):
    for i, o in plans:
        if o["path"] == "REFUSED":
            continue
        x, y, z = got(o, "grid")
        assert 1 <= x < 1 << 31 and 1 <= y <= 65535 and 1 <= z <= 65535, (i, o)
        lds = {"GENERIC": 0, "ROWS64": 0, "RING": 4 * 8 * 2048, "SPLIT_REGS": 4 * o["G"] * 16 * o["dpl"] * 4}.get(o["path"], 2 * stage_bytes(o["hsp"]))
        assert o["lds"] == lds <= 160 * 1024, (i, o)


def test_partials_fit_the_workspace_the_size_query_answers(plans):
    for i, o in plans:
        if o["path"] != "REFUSED":
            assert o["ws"] == ws_bytes(knobs_of(i), i), (i, o)
            assert o["pbytes"] <= o["ws"], (i, o)
    assert any(o["pbytes"] == o["ws"] > 0 for _, o in plans) and any(0 < o["pbytes"] < o["ws"] for _, o in plans)


def test_every_live_length_of_a_moving_plan_stays_inside_its_layout(plans):
    """for L in 1 .. cap: attn_live_splits(L) <= nsplit (no range past the partials) and attn_live_splits(L) * attn_live_kps(L) >= L (every key in a
    range) — counted by the program with the functions the kernels run; their values are checked against this model through a checksum"""
    moving = [(i, o) for i, o in plans if i["cap"] and o["path"] in ("RING", "SPLIT_REGS") and o["nsplit"] > 1]
    assert len(moving) > 500 and any(got(o, "dyn")[0] == 0 for _, o in moving) and any(got(o, "dyn")[1] > 1 for _, o in moving)
    for i, o in moving:
        assert o["viol"] == 0, (i, o)
        L = np.arange(1, i["cap"] + 1, dtype=np.int64)
        mk, bk, below = got(o, "dyn")
        if mk <= 0:
            kps = np.full_like(L, o["kps"])
        else:
            want = np.maximum(1, np.minimum(o["nsplit"], -(-L // mk)))
            kps = -(-L // want)
            if bk > 1:
                kps = np.where(want > 1, -(-kps // bk) * bk, kps)
            kps = np.where(L <= below, np.maximum(L, 1), kps)
        n = np.maximum(1, -(-L // kps))
        assert n.max() <= o["nsplit"] and (n * kps >= L).all(), (i, o)
        assert int(((n * 65537 + kps) * L).sum()) == o["sum"], (i, o)


def test_a_knob_changes_the_fields_the_table_says(plans):
    key = lambda i: tuple(v for k, v in sorted(i.items()) if k not in ("knob", "kval"))
    base = {key(i): o for i, o in plans if i["knob"] == "none"}
    ranges = {"path", "lpk", "lds", "grid", "nsplit", "kps", "pbytes", "merge", "tick", "dyn", "ws", "sum"}
    may = {"pipe": {"path", "xcd"}, "pvar": {"xcd"}, "attn_stream": ranges, "attn_mfma2_rows": {"path", "grid", "lds", "nqb", "al", "xcd"},
           "attn_heads_first": {"hf", "grid"}}
    must = {"pipe": lambda b: b["path"] == "PIPELINED", "pvar": lambda b: b["path"] == "PIPELINED", "attn_stream": lambda b: b["path"] == "RING"}
    counts = dict.fromkeys(may, 0)
    for i, o in plans:
        if i["knob"] in may and key(i) in base:
            b = base[key(i)]
            changed = {k for k in o if o[k] != b[k]}
            assert changed <= may[i["knob"]], (i, changed)
            if i["knob"] in must:
                assert bool(changed) == must[i["knob"]](b), (i, changed)
            counts[i["knob"]] += bool(changed)
    assert all(counts.values()), counts

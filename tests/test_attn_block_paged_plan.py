"""The plan of ns_hip_attn_block_paged (attn_block_paged_plan, neural-speed_amd/csrc/ns_attn_plan.cpp), the workspace size function and the live rule
its range workgroups and its merge run (attn_block_live, ns_attn.h).  A host program (tests/tools/attn_block_paged_plan_main.cpp, built with the
library's compiler, nothing launched) prints the plans of a grid of calls, the refusals, and (keys per range, live ranges) for every live length of
a few plans; the rules are written out again here.

The range rule is the block-split kernel's (docs/kernels/attention.md): ceil(512 / workgroups per range) ranges, 128 keys or more each, 64 at the
most, whole 64-key blocks, none that starts at or past the capacity; workgroups per range = kv heads * slot blocks of max_q rows * requests."""
import os
import subprocess

import pytest

from test_attn_plan import CSRC, ROOT, compiler, num

MAIN = os.path.join(ROOT, "tests", "tools", "attn_block_paged_plan_main.cpp")
BLOCKS = (16, 32, 128, 256)
TARGET, MIN_KEYS = 512, 128  # AttnKnobs: "attn_block_wg_target" / "attn_block_min_keys"


def ceil_div(a, b):
    return -(-a // b)


def kv(text):
    return {k: num(v) for k, v in (x.split("=") for x in text.split())}


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    hipcc = compiler()
    if not hipcc:
        pytest.skip("the library's compiler is not installed")
    exe = str(tmp_path_factory.mktemp("attn_block_paged_plan") / "attn_block_paged_plan")
    subprocess.run([hipcc, "-std=c++20", "-x", "hip", "--offload-arch=gfx950", "--cuda-host-only", "-Wall", "-Werror", "-I", CSRC, MAIN, "-o", exe],
                   check=True, capture_output=True, text=True, timeout=300)
    out = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=120).stdout
    res = {"plan": [], "refuse": [], "live": []}
    for line in out.splitlines():
        kind, rest = line.split(" ", 1)
        head, tail = rest.split(" |", 1)
        if kind == "live":
            res[kind].append((kv(head), [tuple(int(x) for x in cell.split(":")) for cell in tail.split()]))
        else:
            body, why = tail.split(" why=")
            o = kv(body)
            o["why"] = why.strip()
            res[kind].append((kv(head), o))
    return res


def rule(bs, hn, hkv, hs, max_q, cap):
    """the plan's fields, written out"""
    g = hn // hkv
    slot_blocks = ceil_div(max_q * g, 64)
    base = hkv * slot_blocks * bs
    ns = min(ceil_div(TARGET, base), max(1, ceil_div(cap, MIN_KEYS)), 64)
    kps = ceil_div(ceil_div(cap, ns), 64) * 64
    nsplit = ceil_div(cap, kps)
    return dict(grid=(slot_blocks * hkv, nsplit, bs), mgrid=(hn, max_q, bs), nsplit=nsplit, kps=kps, gfull=g, pbytes=bs * max_q * hn * nsplit * (2 + hs) * 4)


def test_the_grid(lines):
    seen = {(i["bs"], i["hn"], i["hkv"], i["hs"], i["maxq"], i["cap"], i["bk"]) for i, _ in lines["plan"]}
    want = {(bs, hn, hkv, hs, mq, ceil_div(cap, bk) * bk, bk) for bk in BLOCKS for bs in (1, 2, 8, 33) for hn, hkv in ((8, 8), (8, 2), (8, 1), (71, 1))
            for hs in (64, 128) for mq in (1, 2, 16, 17, 64, 127, 300) for cap in (1, 255, 256, 300, 2048, 8192)}
    assert seen == want and len(lines["plan"]) == 4 * 4 * 4 * 2 * 7 * 6
    assert {i["hm"] for i, _ in lines["plan"]} == {0, 1}
    assert any(o["nsplit"] == 1 for _, o in lines["plan"]) and any(o["nsplit"] > 8 for _, o in lines["plan"])


def test_the_plan_fields_follow_the_rule(lines):
    for i, o in lines["plan"]:
        r = rule(i["bs"], i["hn"], i["hkv"], i["hs"], i["maxq"], i["cap"])
        assert o["ok"] == 1 and o["why"] == "", (i, o)
        assert tuple(int(x) for x in str(o["grid"]).split(",")) == r["grid"], (i, o, r)
        assert tuple(int(x) for x in str(o["mgrid"]).split(",")) == r["mgrid"], (i, o, r)
        assert (o["nsplit"], o["kps"], o["gfull"], o["pbytes"]) == (r["nsplit"], r["kps"], r["gfull"], r["pbytes"]), (i, o, r)
        assert (o["block"], o["hspad"], o["slq"], o["slkv"], o["kdelta"], o["dyn"]) == (256, i["hs"], i["maxq"], i["cap"], 1, MIN_KEYS), (i, o)
        assert 1 << o["shift"] == i["bk"]
        # the layout: whole 64-key blocks, no range that starts at or past the capacity, every key in a range
        assert o["kps"] % 64 == 0 and (o["nsplit"] - 1) * o["kps"] < i["cap"] <= o["nsplit"] * o["kps"] and 1 <= o["nsplit"] <= 64, (i, o)
        assert r["grid"][0] <= 65535


def test_the_workspace_size_function_is_the_plans_partial_bytes(lines):
    for i, o in lines["plan"]:
        assert o["ws"] == o["pbytes"] > 0, (i, o)


def test_each_refusal_names_its_reason(lines):
    got = {i["what"]: o for i, o in lines["refuse"]}
    assert got.pop("none")["ok"] == 1 and got.pop("grid_limit_below")["ok"] == 1
    assert all(o["ok"] == 0 for o in got.values()), got
    want = {"null_qstart": "dQStart is null", "null_lens": "dKvLens is null", "head_size_80": "head_size must be 64 or 128",
            "head_size_256": "head_size must be 64 or 128", "alibi": "ALiBi and the tanh cap are not served", "tanh": "ALiBi and the tanh cap are not served",
            "max_q_0": "sl_q is max_q", "grid_limit": "above the grid limit of 65535", "head_group": "head_num must be a multiple of heads_kv",
            "block_keys_48": "block_keys must be a power of two from 16 to 256", "block_keys_8": "block_keys must be a power of two from 16 to 256",
            "block_keys_512": "block_keys must be a power of two from 16 to 256", "capacity": "must equal table_stride * block_keys",
            "null_table": "block table is null", "pool_blocks": "pool_blocks must be at least 1", "block_step_small": "do not fit inside block_step",
            "block_step_unaligned": "block_step must be a positive multiple of 8", "kv_rows_unaligned": "contiguous in the head dimension and 16-byte aligned"}
    assert set(got) == set(want)
    for what, text in want.items():
        assert text in got[what]["why"], (what, got[what])


def test_the_live_ranges_tile_every_live_length(lines):
    """for every live length 0 .. capacity: the live ranges [i * kps, min((i + 1) * kps, n)) tile [0, n) exactly once, kps is a multiple of 64, there
    are no more of them than laid out; with the dynamic ranges off they are the laid-out ones; with them on, the rule written out"""
    assert len(lines["live"]) == 12 and {h["dyn"] for h, _ in lines["live"]} == {0, 1}
    assert any(h["nsplit"] >= 4 for h, _ in lines["live"])
    for h, cells in lines["live"]:
        assert len(cells) == h["cap"] + 1
        assert h["minkeys"] == (MIN_KEYS if h["dyn"] else 0)
        for n, (kps, live) in enumerate(cells):
            assert kps % 64 == 0 and kps > 0 and 0 <= live <= h["nsplit"], (h, n, kps, live)
            covered = [(i * kps, min((i + 1) * kps, n)) for i in range(live)]
            assert all(a < b for a, b in covered), (h, n, covered)  # no empty live range
            assert sum(b - a for a, b in covered) == n and (not covered or (covered[0][0] == 0 and covered[-1][1] == n)), (h, n, covered)
            assert all(covered[i][1] == covered[i + 1][0] for i in range(live - 1))
            if not h["dyn"]:
                assert kps == h["kps"] and live == ceil_div(n, h["kps"]), (h, n)
            elif n > 0:
                want = min(h["nsplit"], max(1, ceil_div(n, MIN_KEYS)))
                k = ceil_div(ceil_div(n, want), 64) * 64
                assert (kps, live) == (k, ceil_div(n, k)), (h, n)
        # at the capacity the dynamic rule needs no more workgroups than the layout has, and a short request fewer
        assert cells[h["cap"]][1] <= h["nsplit"] and cells[1][1] == 1 and cells[0][1] == 0

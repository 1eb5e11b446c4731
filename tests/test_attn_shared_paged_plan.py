"""The plan of ns_hip_attn_decode_paged_shared (attn_shared_paged_plan, ns_attn_plan.cpp), the workspace size function and the live rule its range
workgroups and its merge run (attn_block_live, ns_attn.h), printed by a host program (tests/tools/attn_shared_paged_plan_main.cpp, nothing launched); the
rules are written out again here.  Both kinds of range follow the block-split kernel's rule: ceil(512 / workgroups per range) ranges, 128 keys or more
each, 64 at the most, whole 64-key blocks; workgroups per range: prefix kv heads * ceil(max_group * g / 64) * groups, suffix kv heads * ceil(g / 64) *
(groups * max_group).  The records of a (request, head) are laid out for ONE group, so the workspace is a function of the shape alone."""
import importlib.util
import os
import subprocess

import pytest

from test_attn_plan import CSRC, ROOT, compiler, num

MAIN = os.path.join(ROOT, "tests", "tools", "attn_shared_paged_plan_main.cpp")
TARGET, MIN_KEYS = 512, 128  # AttnKnobs: "attn_block_wg_target" / "attn_block_min_keys"


def ceil_div(a, b):
    return -(-a // b)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    hipcc = compiler()
    if not hipcc:
        pytest.skip("the library's compiler is not installed")
    exe = str(tmp_path_factory.mktemp("attn_shared_paged_plan") / "attn_shared_paged_plan")
    subprocess.run([hipcc, "-std=c++20", "-x", "hip", "--offload-arch=gfx950", "--cuda-host-only", "-Wall", "-Werror", "-I", CSRC, MAIN, "-o", exe],
                   check=True, capture_output=True, text=True, timeout=300)
    return exe


@pytest.fixture(scope="module")
def lines(exe):
    return parse(subprocess.run([exe], check=True, capture_output=True, text=True, timeout=120).stdout)


def parse(out):
    res = {"plan": [], "refuse": [], "live": [], "far": []}
    for line in out.splitlines():
        kind, rest = line.split(" ", 1)
        head, tail = rest.split(" |", 1)
        body, _, why = tail.partition(" why=")
        o = {k: (tuple(int(x) for x in v.replace(":", ",").split(",")) if ":" in v or "," in v else num(v)) for k, v in (x.split("=") for x in body.split())}
        o["why"] = why.strip()
        res[kind].append(({k: num(v) for k, v in (x.split("=") for x in head.split())}, o))
    return res


def ranges(base, cap):
    ns = min(ceil_div(TARGET, base), max(1, ceil_div(cap, MIN_KEYS)), 64)
    kps = ceil_div(ceil_div(cap, ns), 64) * 64
    return ceil_div(cap, kps), kps


def test_the_plan_follows_the_rule_and_the_workspace_is_its_partials(lines):
    assert len(lines["plan"]) == 5 * 5 * 3
    for i, o in lines["plan"]:
        g = i["hn"] // i["hkv"]
        sbp, sbs = ceil_div(i["maxg"] * g, 64), ceil_div(g, 64)
        nsp, kpsp = ranges(i["hkv"] * sbp * i["groups"], i["cap"])
        nss, kpss = ranges(i["hkv"] * sbs * i["groups"] * i["maxg"], i["cap"])
        one_p, one_s = ranges(i["hkv"] * sbp, i["cap"])[0], ranges(i["hkv"] * sbs * i["maxg"], i["cap"])[0]
        assert o["ok"] == 1 and o["why"] == "", (i, o)
        assert o["pgrid"] == (sbp * i["hkv"], nsp, i["groups"]) and o["sgrid"] == (sbs * i["hkv"], nss, i["groups"] * i["maxg"]), (i, o)
        assert o["mgrid"] == (i["hn"], i["bs"], 1) and (o["block"], o["hspad"], o["gfull"], o["dyn"]) == (256, i["hs"], g, MIN_KEYS * i["dynon"]), (i, o)
        assert (o["nsp"], o["kpsp"], o["nss"], o["kpss"]) == (nsp, kpsp, nss, kpss) and kpsp % 64 == 0 and kpss % 64 == 0, (i, o)
        assert (o["sufoff"], o["stride"]) == (one_p, one_p + one_s) and nsp <= one_p and nss <= one_s, (i, o)
        assert o["pbytes"] == o["ws"] == i["bs"] * i["hn"] * (one_p + one_s) * (2 + i["hs"]) * 4 > 0, (i, o)
        assert max(o["pgrid"] + o["sgrid"] + o["mgrid"]) <= 65535
    assert any(o["nsp"] > 8 for _, o in lines["plan"]) and {1, 2} <= {o["nss"] for _, o in lines["plan"]}


def test_each_refusal_names_its_reason(lines):
    got = {i["what"]: o for i, o in lines["refuse"]}
    assert got.pop("none")["ok"] == 1 and all(o["ok"] == 0 for o in got.values()), got
    want = {"null_start": "dGroupStart is null", "null_prefix": "dPrefixKeys is null", "null_lens": "dKvLens is null", "groups_0": "groups must be 1 .. 65535",
            "max_group_0": "max_group, the most requests of one group", "sl_q_2": "sl_q must be 1", "head_size_80": "head_size must be 64 or 128",
            "alibi": "ALiBi and the tanh cap are not served", "grid_limit_members": "groups * max_group above the grid limit",
            "capacity": "must equal table_stride * block_keys"}
    assert set(got) == set(want) and all(text in got[what]["why"] for what, text in want.items()), got


def test_the_pools_of_the_far_address_tests_take_the_kernels_they_assert(exe):
    """tests/test_gpu_attn_far_addresses.py asserts attn_shared_kernel<64 / 128> through ns_hip_attn_decode_paged_shared_stats on pools of 1.4 * 2^31
    elements — position-major, and head-major with a gap behind every block: both are accepted as they are (the plan has no 32-bit rule: the kernels
    read through 64-bit pointers), with the caller's block_step and strides.  The numbers are those of tests/tools/attn_far_layout.py."""
    spec = importlib.util.spec_from_file_location("attn_far_layout", os.path.join(ROOT, "tests", "tools", "attn_far_layout.py"))
    FL = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(FL)
    live = [ceil_div(n, FL.SHARED_BK) for n in FL.SHARED_LENS]
    for hs in FL.SHARED_HS:
        for layout, gap in (("pm", False), ("hm", True)):
            g = FL.paged_layout("over", hs, FL.SHARED_BK, live, layout, gap)
            assert not FL.page_in32(g["pool_blocks"], g["block_step"]) and (g["block_step"] > g["cells"]) == gap
            args = ["far", hs, FL.SHARED_BK, FL.SHARED_CAP, len(FL.SHARED_LENS), len(FL.SHARED_PREFIX), FL.SHARED_MAX_GROUP, g["pool_blocks"], g["block_step"],
                    g["step_sl"], g["step_head"]]
            (i, o), = parse(subprocess.run([exe] + [str(x) for x in args], check=True, capture_output=True, text=True, timeout=60).stdout)["far"]
            assert (o["ok"], o["why"], o["hspad"]) == (1, "", hs) and i["blocks"] == g["pool_blocks"], (hs, layout, o)
            assert (o["bstep"], o["ksl"], o["khead"]) == (g["block_step"], g["step_sl"], g["step_head"]), (hs, layout, o)
            assert o["pgrid"][2] == 1 and o["sgrid"][2] == FL.SHARED_MAX_GROUP  # one group, three member slots


def test_the_live_ranges_tile_the_prefix_and_the_suffix(lines):
    """for every (P, len) on a coarse grid of six plans: the live prefix ranges, cut at the member's limit min(P, len), cover [0, min(P, len)) exactly once;
    the live suffix ranges, which start at P + i * kps, cover [P, len) exactly once and none is empty; every range starts at a multiple of 16"""
    assert len({(o["nsp"], o["kpsp"], o["nss"], o["kpss"], h["bk"]) for h, o in lines["live"]}) == 6 and {h["dyn"] for h, _ in lines["live"]} == {0, 1}
    for h, o in lines["live"]:
        P, n = h["P"], h["len"]
        assert P % h["bk"] == 0
        for kind, origin, end, span, laid in (("prefix", 0, min(P, n), P, (o["nsp"], o["kpsp"])), ("suffix", P, n, n - P, (o["nss"], o["kpss"]))):
            kps, live = o[kind]
            assert kps % 64 == 0 and kps > 0 and live <= laid[0] and (h["dyn"] or kps == laid[1]) and live == ceil_div(max(span, 0), kps), (h, o)
            cover = [(origin + i * kps, min(origin + (i + 1) * kps, end)) for i in range(live)]
            assert all(a % 16 == 0 for a, _ in cover) and sum(max(0, b - a) for a, b in cover) == max(0, end - origin), (h, kind, cover)
            assert all(cover[i][1] in (cover[i + 1][0], end) for i in range(live - 1)) and (kind == "prefix" or all(a < b for a, b in cover)), (h, kind, cover)

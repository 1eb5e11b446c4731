"""The opt-in context-split block path of attn_plan (neural-speed_amd/csrc/ns_attn_plan.cpp, AP_BLOCK_SPLIT behind AttnKnobs::block_split): a host
program (tests/tools/attn_block_plan_main.cpp, built with the library's compiler, nothing launched) prints, for a grid of calls, the plan with the
key at a value and the plan of the same call with the key at 0.  The envelope and the range rule — docs/kernels/attention.md, "A short block of
query rows over a long cache" — are written out here independently: inside the envelope the path and its launch shape, outside it every
printed field equal to the key-at-0 plan (which tests/test_attn_plan.py pins)."""
import os
import subprocess

import pytest

from test_attn_plan import CSRC, ROOT, compiler, num

MAIN = os.path.join(ROOT, "tests", "tools", "attn_block_plan_main.cpp")
CAUSAL, ALIBI, TANH = 1, 2, 8  # NS_ATTN_FLAG_IS_* (include/ns_bestla.h)
TARGET, MIN_KEYS = 512, 128    # the range rule's constants as shipped (docs/kernels/attention.md: the measured sweep)


@pytest.fixture(scope="module")
def pairs(tmp_path_factory):
    """[(call, plan with the key on, plan with the key at 0)]"""
    hipcc = compiler()
    if not hipcc:
        pytest.skip("the library's compiler is not installed")
    exe = str(tmp_path_factory.mktemp("attn_block_plan") / "attn_block_plan")
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
    assert len(rows) % 2 == 0
    res = []
    for (i_on, o_on), (i_off, o_off) in zip(rows[0::2], rows[1::2]):
        assert i_off["bsplit"] == 0 and i_on["bsplit"] == i_on["want"] and {k: v for k, v in i_on.items() if k != "bsplit"} == {k: v for k, v in i_off.items() if k != "bsplit"}
        res.append((i_on, o_on, o_off))
    return res


def ceil_div(a, b):
    return -(-a // b)


def ranges(i):
    """the range rule: (nsplit, keys per range)"""
    slot_blocks = ceil_div(i["slq"] * (i["hn"] // i["hkv"]), 64)
    base = i["hkv"] * slot_blocks * i["bs"]
    n = min(ceil_div(i["target"], base), max(1, ceil_div(i["slkv"], i["minkeys"])), 64)
    kps = ceil_div(ceil_div(i["slkv"], n), 64) * 64
    return ceil_div(i["slkv"], kps), kps


def inside(i):
    """the envelope of the path"""
    slot_blocks = ceil_div(i["slq"] * (i["hn"] // i["hkv"]), 64)
    rows_ok = i["klay"] != 2  # (a row stride of hs + 4 halves: rows that are not 16-byte aligned)
    return (i["bsplit"] > 0 and 2 <= i["slq"] <= 127 and i["hs"] in (64, 128) and not i["flags"] & (ALIBI | TANH) and rows_ok and not i["cap"]
            and i["knob"] == "none" and i["slkv"] >= max(i["bsplit"], 256) and i["hkv"] * slot_blocks <= 65535 and ranges(i)[0] >= 2)


def grid(o):
    return tuple(int(x) for x in o["grid"].split(","))


def test_the_grid_of_cases_holds_what_it_should(pairs):
    seen = lambda key: {i[key] for i, _, _ in pairs}
    assert seen("slq") >= {1, 2, 5, 15, 16, 64, 127, 128} and seen("slkv") >= {255, 256, 257, 300, 1000, 2048, 8192}
    assert {(i["hn"], i["hkv"]) for i, _, _ in pairs} >= {(8, 8), (8, 2), (8, 1), (71, 1)} and seen("hs") >= {64, 80, 128, 256}
    assert seen("flags") >= {0, CAUSAL, ALIBI, TANH} and seen("bs") >= {1, 2, 8} and seen("cap") >= {0, 4096} and seen("klay") >= {0, 2, 3}
    assert seen("knob") == {"none", "no_mfma", "v1", "no_partials"} and seen("bsplit") >= {-5, 1, 1024}
    full = [i for i, _, _ in pairs if i["bsplit"] == 1 and i["klay"] == 0 and not i["cap"] and i["knob"] == "none" and i["target"] == TARGET and i["minkeys"] == MIN_KEYS]
    assert len({(i["slq"], i["slkv"], i["hn"], i["hkv"], i["hs"], i["flags"], i["bs"]) for i in full}) >= 8 * 7 * 4 * 4 * 4 * 3
    taken = [i for i, o, _ in pairs if o["path"] == "BLOCK_SPLIT"]
    assert len(taken) > 500 and len(taken) < len(pairs) // 2
    assert {i["slq"] for i in taken} == {2, 5, 15, 16, 64, 100, 127} and {i["hs"] for i in taken} == {64, 128} and {i["flags"] for i in taken} == {0, CAUSAL}


def test_the_path_is_taken_exactly_inside_its_envelope(pairs):
    wrong = [(i, o["path"]) for i, o, _ in pairs if (o["path"] == "BLOCK_SPLIT") != inside(i)]
    assert not wrong, (len(wrong), wrong[:3])
    assert all(off["path"] != "BLOCK_SPLIT" for _, _, off in pairs)


def test_outside_the_envelope_the_plan_is_the_plan_with_the_key_at_zero(pairs):
    outside = [(i, o, off) for i, o, off in pairs if not inside(i)]
    assert len(outside) > 1000
    wrong = [(i, {k: (o[k], off[k]) for k in o if o[k] != off[k]}) for i, o, off in outside if o != off]
    assert not wrong, (len(wrong), wrong[:3])
    # ... among them calls the path would take but for ONE condition
    near = lambda **kw: [i for i, _, _ in outside if all(i[k] == v for k, v in kw.items())]
    assert near(slq=16, slkv=2048, hs=128, flags=ALIBI) and near(slq=16, slkv=2048, hs=128, flags=TANH) and near(slq=16, slkv=2048, hs=80, flags=0)
    assert near(slq=1, slkv=2048, hs=128, flags=0) and near(slq=128, slkv=2048, hs=128, flags=0) and near(slq=16, slkv=255, hs=128, flags=0)
    assert near(slq=16, slkv=2048, klay=2) and near(slq=16, slkv=2048, knob="no_mfma") and near(slq=16, slkv=2048, knob="v1")
    assert near(slq=16, slkv=2048, knob="no_partials") and near(slq=16, slkv=2048, bsplit=-5) and near(slq=1, cap=4096)
    assert near(hn=40000, slq=127) and near(hn=64, bs=8, slkv=4096)  # the grid limit; so many workgroups that the rule gives one range


def test_launch_shape_and_ranges_on_the_path(pairs):
    taken = [(i, o) for i, o, _ in pairs if o["path"] == "BLOCK_SPLIT"]
    for i, o in taken:
        g_full = i["hn"] // i["hkv"]
        slot_blocks = ceil_div(i["slq"] * g_full, 64)
        n, kps = o["nsplit"], o["kps"]
        assert (n, kps) == ranges(i), (i, o)
        assert 2 <= n <= 64 and kps % 64 == 0 and (n - 1) * kps < i["slkv"] <= n * kps, (i, o)
        x, y, z = grid(o)
        assert (x, y, z) == (slot_blocks * i["hkv"], n, i["bs"]) and 1 <= x < 1 << 31 and y <= 65535 and z <= 65535, (i, o)
        assert o["block"] == 256 and o["hsp"] == i["hs"] and o["gfull"] == g_full and o["lds"] == 0, (i, o)
        assert o["pbytes"] == i["bs"] * i["slq"] * i["hn"] * n * (2 + i["hs"]) * 4, (i, o)
        assert o["merge"] == 1 and o["tick"] == 0 and o["kmove"] == 0 and o["dyn"] == "0,0,0" and o["why"] == "", (i, o)
    # the rule's three limits each decide somewhere: the workgroup target, the keys per range, 64 ranges
    base = lambda i: i["hkv"] * ceil_div(i["slq"] * (i["hn"] // i["hkv"]), 64) * i["bs"]
    assert any(ceil_div(i["target"], base(i)) < ceil_div(i["slkv"], i["minkeys"]) for i, o in taken)
    assert any(ceil_div(i["target"], base(i)) > ceil_div(i["slkv"], i["minkeys"]) for i, o in taken)
    assert any(o["nsplit"] == 64 for i, o in taken) and any(i["slkv"] % o["kps"] for i, o in taken)
    assert any(i["target"] != TARGET for i, o in taken) and any(i["minkeys"] != MIN_KEYS for i, o in taken) and any(i["klay"] == 3 for i, o in taken)


def test_the_size_query_does_not_know_the_path(pairs):
    """bestla_fusion_attn_workspace_size stays the reference's contract: the same answer with the key on and at 0 — and there are calls whose partials
    do not fit it (launch_attn then takes the stream's scratch) as well as calls whose partials do"""
    assert all(o["ws"] == off["ws"] for _, o, off in pairs)
    taken = [o for _, o, _ in pairs if o["path"] == "BLOCK_SPLIT"]
    assert any(o["pbytes"] > o["ws"] for o in taken) and any(o["pbytes"] <= o["ws"] for o in taken)


def test_the_key_is_a_threshold_on_the_context_length(pairs):
    by = {(i["slq"], i["slkv"], i["hn"], i["hkv"]): o["path"] for i, o, _ in pairs
          if i["bsplit"] == 1024 and i["klay"] == 0 and not i["cap"] and i["knob"] == "none" and i["target"] == TARGET}
    assert by[(16, 1000, 8, 8)] == "ROWS64" and by[(16, 1023, 8, 8)] == "ROWS64" and by[(16, 1024, 8, 8)] == by[(16, 2048, 8, 8)] == "BLOCK_SPLIT"
    assert by[(2, 1000, 8, 2)] == "RING" and by[(2, 2048, 8, 2)] == "BLOCK_SPLIT"
    assert by[(1, 2048, 8, 8)] == "RING" and by[(100, 2048, 71, 1)] == "BLOCK_SPLIT"
    low = {(i["slq"], i["slkv"]): o["path"] for i, o, _ in pairs if i["bsplit"] == 1 and i["hn"] == 8 and i["hkv"] == 8 and i["hs"] == 128 and i["flags"] == CAUSAL
           and i["bs"] == 1 and i["klay"] == 0 and not i["cap"] and i["knob"] == "none" and i["target"] == TARGET and i["minkeys"] == MIN_KEYS}
    assert low[(16, 255)] == "ROWS64" and low[(16, 256)] == low[(16, 257)] == "BLOCK_SPLIT"  # (never below 256 keys)

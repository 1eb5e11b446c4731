"""The per-request form of attn_plan (neural-speed_amd/csrc/ns_attn_plan.cpp, Affine::rows: what ns_hip_attn_decode_rows builds — one live context
length per batch entry, sl_kv the capacity of a request's slab): a host program (tests/tools/attn_rows_plan_main.cpp, built with the library's
compiler, nothing launched) prints, for a grid of decode calls, that plan and the plan of the existing moving-length form of the same shape, and walks
every live length 0 .. capacity of a request through the functions the kernels run (attn_live_kv<true>, attn_live_kps, attn_live_splits; ns_attn.h).
The per-request form only changes where the length comes from: the launch is the moving-length plan's, and the live ranges tile [0, len) exactly once."""
import os
import subprocess

import pytest

from test_attn_plan import CSRC, ROOT, compiler, num

MAIN = os.path.join(ROOT, "tests", "tools", "attn_rows_plan_main.cpp")
# what the issue names (path, template arguments, grid, LDS, nsplit, keys per range, partial bytes) and the rest of the launch's shape
SAME = ("path", "G", "lpk", "dpl", "grid", "block", "lds", "nsplit", "kps", "pbytes", "chunks", "gfull", "hf", "dyn", "tick", "merge", "ws")


@pytest.fixture(scope="module")
def pairs(tmp_path_factory):
    """[(call, per-request plan, moving-length plan)]"""
    hipcc = compiler()
    if not hipcc:
        pytest.skip("the library's compiler is not installed")
    exe = str(tmp_path_factory.mktemp("attn_rows_plan") / "attn_rows_plan")
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
    for (i_r, o_r), (i_m, o_m) in zip(rows[0::2], rows[1::2]):
        assert i_r["form"] == "rows" and i_m["form"] == "moving" and {k: v for k, v in i_r.items() if k != "form"} == {k: v for k, v in i_m.items() if k != "form"}
        res.append((i_r, o_r, o_m))
    return res


def served(pairs):
    return [(i, o, m) for i, o, m in pairs if o["path"] != "REFUSED"]


def test_the_grid_of_cases_holds_what_it_should(pairs):
    full = {(i["bs"], i["hn"], i["hkv"], i["hs"], i["cap"]) for i, _, _ in pairs
            if i["slq"] == 1 and i["klay"] == 0 and i["dynr"] == 1 and i["stream"] == 1 and i["inl"] == 0 and i["flags"] == 0 and i["bias"] == 1}
    want = {(bs, hn, hkv, hs, cap) for bs in (1, 2, 8, 33) for hn, hkv in ((8, 8), (8, 2), (8, 1), (71, 1)) for hs in (32, 64, 80, 128, 256)
            for cap in (1, 255, 256, 300, 2048, 8192)}
    assert full >= want and len(want) == 480
    seen = lambda key: {i[key] for i, _, _ in pairs}
    assert seen("dynr") == {0, 1} and seen("stream") == {0, 1} and seen("inl") == {0, 1} and seen("klay") == {0, 1, 2, 3} and seen("bias") == {0, 1}
    paths = {o["path"] for _, o, _ in pairs}
    assert paths == {"RING", "SPLIT_REGS", "REFUSED"}, paths
    assert any(o["nsplit"] > 1 for _, o, _ in pairs) and any(o["nsplit"] == 1 for _, o, _ in served(pairs)) and any(o["nsplit"] == 64 for _, o, _ in pairs)


def test_the_launch_is_that_of_the_moving_length_plan(pairs):
    ok = served(pairs)
    assert len(ok) == len(pairs) - 4
    wrong = [(i, {k: (o[k], m[k]) for k in SAME if o[k] != m[k]}) for i, o, m in ok if any(o[k] != m[k] for k in SAME)]
    assert not wrong, (len(wrong), wrong[:3])
    for i, o, m in ok:
        # ... and only where the length comes from differs: an array with one entry per request, its bias, the capacity as the clamp's upper end
        assert (o["kmove"], o["rows"], o["kdelta"], o["slkv"]) == (1, 1, i["bias"], i["cap"]), (i, o)
        assert (m["kmove"], m["rows"], m["kdelta"]) == (1, 0, 1), (i, m)
        assert o["path"] == ("RING" if 32 < i["hs"] <= 128 and i["stream"] else "SPLIT_REGS"), (i, o)
        assert o["tick"] == (1 if i["inl"] and o["nsplit"] > 1 else 0) and o["merge"] == (1 if o["nsplit"] > 1 and not o["tick"] else 0), (i, o)
        assert o["why"] == "" and m["why"] == "", (i, o, m)


def test_live_ranges_tile_the_live_keys_exactly_once_at_every_length(pairs):
    """viol (counted by the tool over every length 0 .. capacity and both ends of the clamp): a range without a key, keys covered twice or not at all,
    more live ranges than the launch has workgroups for, a length the clamp does not give back"""
    ok = served(pairs)
    assert all(o["viol"] == 0 for _, o, _ in ok), [(i, o["viol"]) for i, o, _ in ok if o["viol"]][:3]
    # with the range rule applied per request the ranges differ from the ones laid out at some length of every plan that has ranges at all ...
    dyn = [(i, o) for i, o, _ in ok if i["dynr"] == 1 and o["nsplit"] > 1]
    assert dyn and all(o["dyn"] != "0,0,0" and o["laid"] > 0 for _, o in dyn), [(i, o["laid"]) for i, o in dyn if not o["laid"]][:3]
    # ... and NS_ATTN_DYN_RANGES=0 keeps them as laid out, at every length
    laid = [(i, o) for i, o, _ in ok if i["dynr"] == 0]
    assert len(laid) >= 54 and any(o["nsplit"] > 1 for _, o in laid)
    assert all(o["dyn"] == "0,0,0" and o["laid"] == 0 for _, o in laid), [(i, o["laid"]) for i, o in laid if o["laid"]][:3]
    # a plan of one range has one live range at every length
    assert all(o["laid"] == 0 for _, o, _ in ok if o["nsplit"] == 1)


def test_each_refusal_names_its_reason(pairs):
    refused = {(i["slq"], i["klay"], i["cap"]): o["why"] for i, o, _ in pairs if o["path"] == "REFUSED"}
    assert set(refused) == {(2, 0, 2048), (1, 2, 2048), (1, 1, 2048), (1, 0, 0)}
    assert "one query row" in refused[(2, 0, 2048)]
    assert "contiguous in the head dimension" in refused[(1, 2, 2048)] and "16-byte aligned" in refused[(1, 2, 2048)]
    assert "contiguous in the head dimension" in refused[(1, 1, 2048)]
    assert "empty sequence" in refused[(1, 0, 0)]
    # the moving-length form of the replayed route still gives such rows to the generic kernel: the refusal belongs to the per-request form
    assert {m["path"] for i, o, m in pairs if o["path"] == "REFUSED" and i["klay"] in (1, 2)} == {"GENERIC"}

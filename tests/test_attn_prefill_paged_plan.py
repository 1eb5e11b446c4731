"""The plan of ns_hip_attn_prefill_paged (attn_prefill_paged_plan, neural-speed_amd/csrc/ns_attn_plan.cpp) and the row -> cell rule by which its kernel
stages K / V rows from the pools (attn_prefill_tile_key and attn_page_at, ns_attn.h).  A host program (tests/tools/attn_prefill_paged_plan_main.cpp,
built with the library's compiler, nothing launched) prints the plans of a grid of calls, the refusals, and — for a few tables with junk behind the
live blocks and bad ids inside them — every (tile, thread, staging step) of the kernel's staging geometry with the key it clamps to, the table slot
its wave reads and the offset that comes out; the rules are written out again here.

The plan: one launch of the 128-row kernel's PAGED instantiation, ceil(max_q / 128) query blocks x heads x requests workgroups of 256 threads and two
LDS stages; the instantiation is (padded head size 64 / 128, biased, padded).  Head sizes above 128 are refused: the 256-wide PAGED form spills."""
import os
import subprocess

import pytest

from test_attn_plan import CSRC, ROOT, compiler, num

MAIN = os.path.join(ROOT, "tests", "tools", "attn_prefill_paged_plan_main.cpp")
CAUSAL, ALIBI, TANH = 1, 2, 8
KB = 64  # keys per tile (kA2KB)


def ceil_div(a, b):
    return -(-a // b)


def kv(text):
    return {k: num(v) for k, v in (x.split("=") for x in text.split())}


def stage_bytes(hs_pad):
    """a2_stage_bytes: a K tile of 64 rows and hs_pad / 16 V subtiles of 64 x 16 halves + 128 bytes"""
    return KB * hs_pad * 2 + (hs_pad // 16) * (KB * 32 + 128)


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    hipcc = compiler()
    if not hipcc:
        pytest.skip("the library's compiler is not installed")
    exe = str(tmp_path_factory.mktemp("attn_prefill_paged_plan") / "attn_prefill_paged_plan")
    subprocess.run([hipcc, "-std=c++20", "-x", "hip", "--offload-arch=gfx950", "--cuda-host-only", "-Wall", "-Werror", "-I", CSRC, MAIN, "-o", exe],
                   check=True, capture_output=True, text=True, timeout=300)
    out = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=120).stdout
    res = {"plan": [], "refuse": [], "walk": []}
    for line in out.splitlines():
        kind, rest = line.split(" ", 1)
        head, tail = rest.split(" |", 1)
        if kind == "walk":
            res[kind].append((kv(head), [tuple(int(x) for x in cell.split(":")) for cell in tail.split()]))
        else:
            body, why = tail.split(" why=")
            o = kv(body)
            o["why"] = why.strip()
            res[kind].append((kv(head), o))
    return res


def test_the_grid(lines):
    seen = {(i["bs"], i["hn"], i["hkv"], i["hs"], i["maxq"], i["cap"], i["bk"], i["flags"]) for i, _ in lines["plan"]}
    want = {(bs, hn, hkv, hs, mq, ceil_div(cap, bk) * bk, bk, fl) for bk in (16, 64, 256) for bs in (1, 3, 8) for hn, hkv in ((8, 8), (8, 2), (71, 1))
            for hs in (40, 64, 80, 96, 128, 160, 256) for mq in (1, 16, 127, 128, 129, 2048) for cap in (200, 2048)
            for fl in (0, CAUSAL, CAUSAL | ALIBI, CAUSAL | TANH)}
    assert seen == want and len(lines["plan"]) == len(want)
    served = [(i, o) for i, o in lines["plan"] if o["ok"]]
    for key in ("hm", "dsto", "d16", "dstadd", "noxcd"):  # every variation occurs among the served calls
        assert len({i[key] for i, _ in served}) > 1, key
    assert {i["scale"] for i, _ in served} == {0.125, -0.125, 0}
    assert {(o["hspad"], o["sb"], o["pad"]) for _, o in served} == {(h, s, p) for h in (64, 128) for s in (0, 1) for p in (0, 1)}
    assert {o["aligned"] for _, o in served} == {0, 1} and {o["xcd"] for _, o in served} == {0, 1}


def test_the_plan_fields_follow_the_rule(lines):
    for i, o in lines["plan"]:
        if i["hs"] > 128:
            assert o["ok"] == 0 and "head sizes above 128 are not served" in o["why"], (i, o)
            continue
        assert o["ok"] == 1 and o["why"] == "", (i, o)
        hs_pad = 64 if i["hs"] <= 64 else 128
        nqb = ceil_div(i["maxq"], 128)
        biased = bool(i["flags"] & (ALIBI | TANH))
        assert (o["hspad"], o["sb"], o["pad"]) == (hs_pad, int(biased or not i["scale"] > 0), int(i["hs"] != hs_pad)), (i, o)
        assert (o["grid"], o["block"], o["nqb"]) == ("%d,1,1" % (nqb * i["hn"] * i["bs"]), 256, nqb), (i, o)
        assert o["lds"] == 2 * stage_bytes(hs_pad) and o["lds"] <= 160 * 1024, (i, o)
        # 16-byte stores: dst, its row and head steps (packed rows: no batch step), 8-byte stores of the shadow
        row = i["hn"] * i["hs"] + i["dstadd"]
        aligned = i["dsto"] % 16 == 0 and row % 4 == 0 and i["hs"] % 4 == 0 and i["d16"] != 2
        assert o["aligned"] == int(aligned), (i, o)
        assert o["xcd"] == int(not i["noxcd"] and (i["hkv"] * i["bs"]) % 8 == 0), (i, o)
        assert (o["slq"], o["slkv"], o["kdelta"], 1 << o["shift"]) == (i["maxq"], i["cap"], 1, i["bk"]), (i, o)
        assert (o["bsteps"], o["qstart"], o["lens"]) == (0, 1, 1), (i, o)  # no batch step reaches the kernel; the two arrays do


def test_each_refusal_names_its_reason(lines):
    got = {i["what"]: o for i, o in lines["refuse"]}
    for served in ("none", "grid_limit_below", "alibi_partition_fits", "partition_without_alibi"):
        assert got.pop(served)["ok"] == 1, served
    assert all(o["ok"] == 0 for o in got.values()), got
    want = {"null_qstart": "dQStart is null", "null_lens": "dKvLens is null", "layout": "only ATTN_FWD_LAYOUT_PLAIN tensors are supported",
            "no_requests": "batch_size (the requests) must be at least 1", "head_size_84": "head_size must be a multiple of 8, at most 256",
            "head_size_264": "head_size must be a multiple of 8, at most 256", "head_size_136": "head sizes above 128 are not served",
            "head_size_256": "head sizes above 128 are not served", "head_group": "head_num must be a multiple of heads_kv", "max_q_0": "sl_q is max_q",
            "capacity_0": "sl_kv is the capacity of a request (at least 1 key)", "block_keys_48": "block_keys must be a power of two from 16 to 256",
            "block_keys_8": "block_keys must be a power of two from 16 to 256", "block_keys_512": "block_keys must be a power of two from 16 to 256",
            "capacity": "must equal table_stride * block_keys", "null_table": "block table is null", "pool_blocks": "pool_blocks must be at least 1",
            "block_step_small": "do not fit inside block_step", "block_step_unaligned": "block_step must be a positive multiple of 8",
            "kv_rows_unaligned": "contiguous in the head dimension and 16-byte aligned", "grid_limit": "must stay below 2^31 workgroups",
            "alibi_partition": "head partition (ns_hip_attn_set_head_partition) does not contain this call's heads"}
    assert set(got) == set(want)
    for what, text in want.items():
        assert text in got[what]["why"], (what, got[what])


def test_the_walk_turns_no_cell_behind_the_live_length_and_no_bad_id_into_an_address(lines):
    """Every row of every tile is staged exactly once for K and once for V; the key is the row clamped to kv_len - 1; the table slot the wave reads is
    the clamped key's, and lies among the live blocks (the junk behind them is never read); the offset is that of the key's cell in the block the
    table names there, inside the pool — or -1, no access, for an id that is no block of the pool."""
    assert len(lines["walk"]) == 6
    bad_inside = 0
    for h, cells in lines["walk"]:
        table = [int(x) for x in str(h["table"]).split(",")]
        n, bk, hs = h["kvlen"], h["bk"], h["hs"]
        ku = hs // 32
        live_blocks = ceil_div(n, bk)
        tiles = ceil_div(n, KB)
        assert len(cells) == tiles * 256 * ku * 2
        staged = {}
        for pos0, tid, u, which, row, group, key, slot, ident, offset in cells:
            w = tid >> 6
            assert group == u * (64 // ku) + w * (16 // ku) and group <= row < group + 16 // ku, (h, pos0, tid, u, which, row, group)
            assert key == min(pos0 + row, n - 1) and 0 <= key < n
            assert slot == key >> (bk.bit_length() - 1), (h, pos0, row, key, slot)  # the entry is the clamped key's
            assert slot < live_blocks and ident == table[slot]
            if 0 <= ident < h["blocks"]:
                assert offset == ident * h["step"] + (key % bk) * h["stepsl"]
                assert 0 <= offset and offset + 2 * hs <= h["blocks"] * h["step"]  # the row of both kv heads lies inside the pool
            else:
                assert offset == -1
                bad_inside += 1
            staged.setdefault((pos0, which, row), []).append(tid)
        # each tile row: all 16-byte chunks of the row, each by one thread (hs / 8 threads), for K and for V
        assert set(staged) == {(t * KB, which, r) for t in range(tiles) for which in (0, 1) for r in range(KB)}
        assert all(len(set(t)) == len(t) == hs // 8 for t in staged.values())
        assert any(not 0 <= x < h["blocks"] for x in table[live_blocks:]) or h["case"] == 5  # (the junk is there)
    assert bad_inside > 0

"""The plan of ns_hip_attn_prefill_paged_wide (attn_prefill_paged_wide_plan, neural-speed_amd/csrc/ns_attn_plan.cpp) and the request rule by which its
kernel moves K / V tiles pool -> LDS by DMA, one buffer descriptor per page and wave (attn_wide_table_slot, attn_wide_desc, attn_wide_k_offset /
attn_wide_v_offset, attn_wide_k_lds / attn_wide_v_lds, ns_attn.h).  A host program (tests/tools/attn_prefill_paged_wide_plan_main.cpp, built with the
library's compiler, nothing launched) prints the plans of a grid of calls, the refusals, and — for a few tables with junk behind the live blocks and
bad ids inside them — every (tile, wave, request, lane) with its descriptor, lane offset and LDS slot; the rules are written out again here."""
import os
import subprocess

import pytest

from test_attn_plan import CSRC, ROOT, compiler
from test_attn_prefill_paged_plan import ceil_div, kv

MAIN = os.path.join(ROOT, "tests", "tools", "attn_prefill_paged_wide_plan_main.cpp")
KB, STAGE, NO_CELL = 64, 65536, 1 << 31  # keys per tile, bytes per stage (K 32 KiB | V 32 KiB), kAwNoCell


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    hipcc = compiler()
    if not hipcc:
        pytest.skip("the library's compiler is not installed")
    exe = str(tmp_path_factory.mktemp("attn_prefill_paged_wide_plan") / "attn_prefill_paged_wide_plan")
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


def test_the_plan_fields_follow_the_rule(lines):
    assert len(lines["plan"]) == 3 * 3 * 3 * 5 * 5 * 2
    for key in ("hm", "dsto", "d16", "dstadd", "noxcd"):  # every variation occurs
        assert len({i[key] for i, _ in lines["plan"]}) > 1, key
    for i, o in lines["plan"]:
        assert o["ok"] == 1 and o["why"] == "", (i, o)
        nqb = ceil_div(i["maxq"], 128)
        assert (o["hspad"], o["pad"]) == (256, int(i["hs"] != 256)), (i, o)
        assert (o["grid"], o["block"], o["nqb"]) == ("%d,1,1" % (nqb * i["hn"] * i["bs"]), 256, nqb), (i, o)
        assert o["lds"] == 2 * STAGE and o["lds"] <= 160 * 1024, (i, o)
        row = i["hn"] * i["hs"] + i["dstadd"]
        aligned = i["dsto"] % 16 == 0 and row % 4 == 0 and i["hs"] % 4 == 0 and i["d16"] != 2
        assert o["aligned"] == int(aligned), (i, o)
        assert o["xcd"] == int(not i["noxcd"] and (i["hkv"] * i["bs"]) % 8 == 0), (i, o)
        assert (o["slq"], o["slkv"], o["kdelta"], 1 << o["shift"]) == (i["maxq"], i["cap"], 1, i["bk"]), (i, o)
        assert (o["bsteps"], o["qstart"], o["lens"]) == (0, 1, 1), (i, o)
    assert {o["aligned"] for _, o in lines["plan"]} == {0, 1} and {o["xcd"] for _, o in lines["plan"]} == {0, 1}


def test_each_refusal_names_its_reason(lines):
    got = {i["what"]: o for i, o in lines["refuse"]}
    for served in ("none", "grid_limit_below", "descriptor_span_head_major"):
        assert got.pop(served)["ok"] == 1, served
    assert all(o["ok"] == 0 for o in got.values()), got
    width = "not built at this width"
    want = {"null_qstart": "dQStart is null", "null_lens": "dKvLens is null", "layout": "only ATTN_FWD_LAYOUT_PLAIN tensors are supported",
            "no_requests": "batch_size (the requests) must be at least 1", "head_size_140": "head_size must be a multiple of 8 from 136 to 256",
            "head_size_264": "head_size must be a multiple of 8 from 136 to 256", "head_size_128": "served by ns_hip_attn_prefill_paged",
            "head_size_64": "served by ns_hip_attn_prefill_paged", "head_group": "head_num must be a multiple of heads_kv", "max_q_0": "sl_q is max_q",
            "capacity_0": "sl_kv is the capacity of a request (at least 1 key)", "block_keys_48": "block_keys must be a power of two from 16 to 256",
            "block_keys_512": "block_keys must be a power of two from 16 to 256", "capacity": "must equal table_stride * block_keys",
            "null_table": "block table is null", "pool_blocks": "pool_blocks must be at least 1", "block_step_small": "do not fit inside block_step",
            "kv_rows_unaligned": "contiguous in the head dimension and 16-byte aligned", "grid_limit": "must stay below 2^31 workgroups", "alibi": width,
            "tanh": width, "scale_0": width, "scale_negative": width, "scale_inf": width, "descriptor_span": "one buffer descriptor per page and head"}
    assert set(got) == set(want)
    for what, text in want.items():
        assert text in got[what]["why"], (what, got[what])


def test_the_walk_requests_every_live_cell_once_and_nothing_else(lines):
    """The design point.  Per (tile, wave): the table slot is that of the group's first key clamped to the last live key — a live block, never the junk
    behind; the descriptor is empty for a bad id or a group behind kv_len and otherwise starts at the group's first row of the walk's kv head.  An
    offset inside num_records addresses one 16-byte chunk of a live key of that head below head_size; all offsets taken together, every such chunk of
    the tile exactly once for K and once for V; and the 16-byte LDS slots written are a permutation of the stage's K and V images, with each chunk in
    the slot the kernel's operand reads expect (the K row's swizzle, V's [column block][key][32 dims])."""
    assert len(lines["walk"]) == 5
    bad_inside = padded = 0
    for h, cells in lines["walk"]:
        table = [int(x) for x in str(h["table"]).split(",")]
        n, bk, hs, step_sl = h["kvlen"], h["bk"], h["hs"], h["stepsl"]
        tiles, live_blocks = ceil_div(n, KB), ceil_div(n, bk)
        assert len(cells) == tiles * 4 * 2 * 8 * 64
        asked, slots = {}, {}
        for pos0, w, which, u, l, slot, ident, base, nbytes, offset, lds in cells:
            first = pos0 + 16 * w
            assert slot == min(first, n - 1) // bk and slot < live_blocks and ident == table[slot]
            live = min(max(n - first, 0), 16)
            if not 0 <= ident < h["blocks"] or live == 0:
                assert nbytes == 0
                bad_inside += live > 0
            else:
                assert base == ident * h["step"] + h["ihkv"] * h["stephead"] + (first % bk) * step_sl
                assert nbytes == ((live - 1) * step_sl + hs) * 2 < NO_CELL
            slots.setdefault((pos0, which), []).append(lds)
            # what the slot must hold: K — row lds / 512 of the tile, chunk (slot in the row) ^ (row & 15); V — column block, key, 16-byte piece
            if which == 0:
                row, chunk = lds // 512, (lds % 512 // 16) ^ (lds // 512 & 15)
            else:
                assert lds >= KB * 512
                v = lds - KB * 512
                row, chunk = v % 4096 // 64, 4 * (v // 4096) + v % 64 // 16
            assert 16 * w <= row < 16 * w + 16
            if 8 * chunk >= hs:
                assert offset == NO_CELL  # outside every descriptor
                padded += 1
                continue
            assert offset == ((row - 16 * w) * step_sl + 8 * chunk) * 2  # the chunk of THAT row the slot expects
            if offset + 16 <= nbytes:  # inside num_records: the cell it addresses
                key = pos0 + row
                assert key < n and 8 * chunk + 8 <= hs
                asked.setdefault((pos0, which, key, chunk), []).append((w, u, l))
            else:
                assert offset >= nbytes and (pos0 + row >= n or not 0 <= ident < h["blocks"])  # wholly outside: zeros
        good = lambda key: 0 <= table[key // bk] < h["blocks"]
        assert set(asked) == {(t * KB, which, key, c) for t in range(tiles) for which in (0, 1) for key in range(t * KB, min(n, t * KB + KB)) if good(key)
                              for c in range(hs // 8)}
        assert all(len(v) == 1 for v in asked.values())
        for (pos0, which), got in slots.items():
            assert sorted(got) == list(range(which * KB * 512, (which + 1) * KB * 512, 16)), (h, pos0, which)
    assert bad_inside > 0 and padded > 0

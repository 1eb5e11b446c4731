"""The plan of ns_hip_attn_prefill_paged_wide (attn_prefill_paged_wide_plan, neural-speed_amd/csrc/ns_attn_plan.cpp) and the request rule by which its
kernel moves K / V tiles pool -> LDS by DMA, one buffer descriptor per page and wave (attn_wide_table_slot, attn_wide_desc, attn_wide_k_offset /
attn_wide_v_offset, attn_wide_k_lds / attn_wide_v_lds, ns_attn.h).  A host program (tests/tools/attn_prefill_paged_wide_plan_main.cpp, built with the
library's compiler, nothing launched) prints the plans of a grid of calls, the refusals, and — for a few tables with junk behind the live blocks and
bad ids inside them — every (tile, wave, request, lane) with its descriptor, lane offset and LDS slot; the rules are written out again here."""
import importlib.util
import os
import subprocess

import pytest

from test_attn_plan import CSRC, ROOT, compiler
from test_attn_prefill_paged_plan import ceil_div, kv

MAIN = os.path.join(ROOT, "tests", "tools", "attn_prefill_paged_wide_plan_main.cpp")
KB, STAGE, NO_CELL = 64, 65536, 1 << 31  # keys per tile, bytes per stage (K 32 KiB | V 32 KiB), kAwNoCell


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    hipcc = compiler()
    if not hipcc:
        pytest.skip("the library's compiler is not installed")
    exe = str(tmp_path_factory.mktemp("attn_prefill_paged_wide_plan") / "attn_prefill_paged_wide_plan")
    subprocess.run([hipcc, "-std=c++20", "-x", "hip", "--offload-arch=gfx950", "--cuda-host-only", "-Wall", "-Werror", "-I", CSRC, MAIN, "-o", exe],
                   check=True, capture_output=True, text=True, timeout=300)
    return exe


def parse(out):
    res = {"plan": [], "refuse": [], "walk": [], "far": []}
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


@pytest.fixture(scope="module")
def lines(exe):
    return parse(subprocess.run([exe], check=True, capture_output=True, text=True, timeout=120).stdout)


def far_layout():
    spec = importlib.util.spec_from_file_location("attn_far_layout", os.path.join(ROOT, "tests", "tools", "attn_far_layout.py"))
    FL = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(FL)
    return FL


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


def far_call(exe, FL, hs, blocks, block_step, step_sl, step_head, bs=3, max_q=130, cap=None):
    args = ["far", hs, FL.WIDE_BK, cap or FL.WIDE_CAP, bs, max_q, blocks, block_step, step_sl, step_head]
    (i, o), = parse(subprocess.run([exe] + [str(x) for x in args], check=True, capture_output=True, text=True, timeout=60).stdout)["far"]
    assert (i["hs"], i["blocks"], i["step"], i["stepsl"], i["stephead"]) == (hs, blocks, block_step, step_sl, step_head)
    return o


def test_the_pools_of_the_far_address_tests_take_the_kernels_they_assert(exe):
    """tests/test_gpu_attn_far_addresses.py asserts these instantiations through ns_hip_attn_prefill_paged_wide_stats on pools of 1.4 * 2^31 elements,
    position-major and head-major, and at the boundary of the descriptor rule: row step s is accepted, s + 8 refused.  If the rule moves, this fails
    first, with the reason; the numbers are those of tests/tools/attn_far_layout.py."""
    FL = far_layout()
    live = [ceil_div(n, FL.WIDE_BK) for n in FL.WIDE_KV]
    for hs in FL.WIDE_HS:
        for layout in ("pm", "hm"):
            g = FL.paged_layout("over", hs, FL.WIDE_BK, live, layout)
            o = far_call(exe, FL, hs, g["pool_blocks"], g["block_step"], g["step_sl"], g["step_head"])
            assert (o["ok"], o["pad"], o["why"]) == (1, int(hs != 256), ""), (hs, layout, o)
    s, t = FL.wide_edge_steps(256)
    assert (15 * s + 256) * 2 < NO_CELL <= (15 * t + 256) * 2  # the plan's rule restated: last = 15 at blocks of 16
    for step_sl, ok in ((s, 1), (t, 0)):
        g = FL.wide_edge_layout(256, step_sl)
        o = far_call(exe, FL, 256, g["pool_blocks"], g["block_step"], g["step_sl"], g["step_head"], bs=2, max_q=max(FL.EDGE_Q), cap=2 * FL.EDGE_BK)
        assert o["ok"] == ok and o["pad"] == 0, (step_sl, o)
        assert o["why"] == "" if ok else "a block's rows of one kv head must lie within 2 GiB" in o["why"], (step_sl, o)


def test_the_walk_at_the_descriptor_boundary_addresses_every_live_key_in_64_bits(exe):
    """the boundary pools' two requests, both kv heads: for every lane whose 16 bytes lie inside num_records, descriptor base + lane offset is
    attn_page_at of that lane's key (+ the head, + the chunk) — block 2's beyond 2^31 elements, the last rows' offsets just below 2^31 bytes"""
    FL = far_layout()
    g = FL.wide_edge_layout(256)
    s, hs, top = g["step_sl"], 256, 0
    for table, n in zip(FL.EDGE_TABLE, FL.EDGE_KV):
        for ihkv in range(FL.HKV):
            args = ["walk", hs, FL.EDGE_BK, n, g["pool_blocks"], g["block_step"], s, g["step_head"], ihkv] + table
            (h, cells), = parse(subprocess.run([exe] + [str(x) for x in args], check=True, capture_output=True, text=True, timeout=60).stdout)["walk"]
            assert (h["step"], h["stepsl"], h["stephead"]) == (g["block_step"], s, g["step_head"]) and len(cells) == 4 * 2 * 8 * 64
            seen = set()
            for pos0, w, which, u, l, slot, ident, base, nbytes, offset, lds in cells:
                if offset + 16 > nbytes:
                    assert offset >= nbytes  # wholly outside: zeros
                    continue
                if which == 0:
                    row, chunk = lds // 512, (lds % 512 // 16) ^ (lds // 512 & 15)
                else:
                    v = lds - KB * 512
                    row, chunk = v % 4096 // 64, 4 * (v // 4096) + v % 64 // 16
                key = pos0 + row
                assert key < n and ident == table[key // 16] and offset < NO_CELL and nbytes < NO_CELL
                page_at = ident * g["block_step"] + (key % 16) * s  # attn_page_at (ns_attn.h)
                assert 2 * base + offset == 2 * (page_at + ihkv * g["step_head"] + 8 * chunk), (key, ihkv, chunk)
                assert any(o <= base + offset // 2 and base + offset // 2 + 8 <= o + m for o, m in g["extents"] if o // g["block_step"] == ident)
                seen.add((which, key, chunk))
                top = max(top, offset)
            assert seen == {(which, key, c) for which in (0, 1) for key in range(n) for c in range(hs // 8)}
    assert top == (15 * s + hs) * 2 - 16 and top < NO_CELL  # the last offset the rule allows is asked for

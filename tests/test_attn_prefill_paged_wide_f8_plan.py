"""The plan of ns_hip_attn_prefill_paged_wide_f8 (attn_prefill_paged_wide_f8_plan, neural-speed_amd/csrc/ns_attn_plan.cpp) and the request rule by which
its kernel moves tiles of E4M3 codes pool -> registers -> LDS (attn_wide_table_slot, attn_wide8_desc, attn_wide8_k_offset / attn_wide8_v_offset,
attn_wide8_k_lds / attn_wide8_v_lds, ns_attn.h).  A host program (tests/tools/attn_prefill_paged_wide_f8_plan_main.cpp, nothing launched) prints the
plans of a grid of calls beside the fp16 wide plans of the same numbers, the refusals, and every (tile, wave, request, lane) of a few tables with junk
behind the live blocks and bad ids inside them; the rules are written out again here."""
import os
import subprocess

import pytest

from test_attn_plan import CSRC, ROOT, compiler
from test_attn_prefill_paged_plan import ceil_div
from test_attn_prefill_paged_wide_plan import KB, NO_CELL, STAGE, parse

MAIN = os.path.join(ROOT, "tests", "tools", "attn_prefill_paged_wide_f8_plan_main.cpp")


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    hipcc = compiler()
    if not hipcc:
        pytest.skip("the library's compiler is not installed")
    exe = str(tmp_path_factory.mktemp("attn_prefill_paged_wide_f8_plan") / "attn_prefill_paged_wide_f8_plan")
    subprocess.run([hipcc, "-std=c++20", "-x", "hip", "--offload-arch=gfx950", "--cuda-host-only", "-Wall", "-Werror", "-I", CSRC, MAIN, "-o", exe],
                   check=True, capture_output=True, text=True, timeout=300)
    return parse(subprocess.run([exe], check=True, capture_output=True, text=True, timeout=120).stdout)


def test_the_plan_keeps_the_fp16_wide_plans_decisions(lines):
    """... for the same numbers, read as bytes: ok, pad, grid, block, nqb, aligned, xcd_map; f8 is set and lds is the two stages of the fp16 image.  The
    grid's strides and block steps are multiples of 16 with every slack a byte layout may carry: none is refused for alignment."""
    assert len(lines["plan"]) == 8 * 2 * 5 * 3
    for i, o in lines["plan"]:
        nqb = ceil_div(i["maxq"], 128)
        assert (o["ok"], o["f8"], o["lds"], o["why"]) == (1, 1, 2 * STAGE, "") and o["lds"] <= 160 * 1024, (i, o)
        assert o["got"] == o["half"] and str(o["got"]).startswith("1:%d:" % (i["hs"] != 256)) and ":256:%d:" % nqb in str(o["got"]), (i, o)
    assert len({o["got"] for _, o in lines["plan"]}) > 20


def test_each_refusal_names_its_reason(lines):
    got = {i["what"]: o for i, o in lines["refuse"]}
    for served in ("none", "span_1gib"):  # (1 GiB of bytes: the fp16 rule, asked of halves, would refuse it)
        assert got.pop(served)["ok"] == 1, served
    scales, width = "K_sc and V_sc, the pools' scales, must be positive and finite", "not built at this width"
    want = {"k_sc_0": scales, "v_sc_negative": scales, "k_sc_inf": scales, "v_sc_nan": scales,
            "head_size_136": "FP8 paged cache: head_size must be a multiple of 16", "head_size_152": "FP8 paged cache: head_size must be a multiple of 16",
            "head_size_128": "served by ns_hip_attn_prefill_paged_f8", "head_size_272": "head_size must be a multiple of 8 from 136 to 256",
            "row_stride": "FP8 paged cache: the row and head strides must be multiples of 16", "head_stride": "FP8 paged cache: the row and head strides",
            "block_step": "FP8 paged cache: block_step must be a multiple of 16", "base": "FP8 paged cache: the pool bases must be 16-byte aligned",
            "alibi": width, "tanh": width, "score_scale": width, "span_2gib": "a block's rows of one kv head must lie within 2 GiB"}
    assert set(got) == set(want)
    for what, text in want.items():
        assert got[what]["ok"] == 0 and text in got[what]["why"], (what, got[what])


def test_the_walk_requests_every_live_chunk_once_and_builds_the_fp16_image(lines):
    """The design point.  Per (tile, wave): the table slot is that of the group's first key clamped to the last live key; the descriptor is empty for a
    bad id or a group behind kv_len and otherwise starts at the BYTE of the group's first row of the walk's kv head, num_records = (live - 1) * step_sl
    + head_size.  A lane's two LDS pieces name what it must have asked for — by the fp16 kernel's image: K slot -> (row, fp16 chunk = slot ^ row & 15),
    V piece -> (column block, key, piece) — namely fp16 chunks 2 col, 2 col + 1 of one key: the 16 codes at (row, col).  An offset inside num_records
    is one such 16-byte chunk of a live key of that head below head_size; all together, every such chunk of the tile exactly once for K and once for
    V; and the pieces written are a permutation of the stage's K and V images."""
    assert len(lines["walk"]) == 5
    bad_inside = padded = 0
    for h, cells in lines["walk"]:
        table = [int(x) for x in str(h["table"]).split(",")]
        n, bk, hs, step_sl = h["kvlen"], h["bk"], h["hs"], h["stepsl"]
        tiles = ceil_div(n, KB)
        assert len(cells) == tiles * 4 * 2 * 4 * 64
        asked, pieces = {}, {}
        for pos0, w, which, u, l, slot, ident, base, nbytes, offset, lds0, lds1 in cells:
            first = pos0 + 16 * w
            assert slot == min(first, n - 1) // bk and slot < ceil_div(n, bk) and ident == table[slot]
            live = min(max(n - first, 0), 16)
            if not 0 <= ident < h["blocks"] or live == 0:
                assert nbytes == 0
                bad_inside += live > 0
            else:
                assert base == ident * h["step"] + h["ihkv"] * h["stephead"] + (first % bk) * step_sl
                assert nbytes == (live - 1) * step_sl + hs < NO_CELL
            pieces.setdefault((pos0, which), []).extend((lds0, lds1))
            if which == 0:
                where = [(x // 512, (x % 512 // 16) ^ (x // 512 & 15)) for x in (lds0, lds1)]
            else:
                where = [((x - KB * 512) % 4096 // 64, 4 * ((x - KB * 512) // 4096) + (x - KB * 512) % 64 // 16) for x in (lds0, lds1)]
                assert lds0 >= KB * 512
            (row, chunk), col = where[0], where[0][1] // 2
            assert where[1] == (row, chunk + 1) and chunk % 2 == 0 and 16 * w <= row < 16 * w + 16
            if 16 * col >= hs:
                assert offset == NO_CELL  # outside every descriptor
                padded += 1
            elif offset + 16 <= nbytes:  # inside num_records: the cell it addresses
                assert offset == (row - 16 * w) * step_sl + 16 * col and pos0 + row < n and 16 * col + 16 <= hs
                asked.setdefault((pos0, which, pos0 + row, col), []).append((w, u, l))
            else:
                assert offset == (row - 16 * w) * step_sl + 16 * col >= nbytes and (pos0 + row >= n or not 0 <= ident < h["blocks"])  # wholly outside
        good = lambda key: 0 <= table[key // bk] < h["blocks"]
        assert set(asked) == {(t * KB, which, key, c) for t in range(tiles) for which in (0, 1) for key in range(t * KB, min(n, t * KB + KB)) if good(key)
                              for c in range(hs // 16)}
        assert all(len(v) == 1 for v in asked.values())
        for (pos0, which), got in pieces.items():
            assert sorted(got) == list(range(which * KB * 512, (which + 1) * KB * 512, 16)), (h, pos0, which)
    assert bad_inside > 0 and padded > 0

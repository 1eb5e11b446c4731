"""attn_prefill_paged_f8_plan (neural-speed_amd/csrc/ns_attn_plan.cpp: what ns_hip_attn_prefill_paged_f8 launches) and the staging map of the kernel's F8
instantiations (attn_prefill8_*, ns_attn.h).  A host program (tests/tools/attn_prefill_paged_f8_plan_main.cpp, built with the library's compiler, nothing
launched) prints the FP8 plan beside attn_prefill_paged_plan of the same call over 2160 calls, the FP8 plan of each refused call, and every (tile, wave,
step, lane) of the staging map over five tables."""
import os
import subprocess

import pytest

from test_attn_paged_plan import fields
from test_attn_plan import CSRC, ROOT, compiler, num

MAIN = os.path.join(ROOT, "tests", "tools", "attn_prefill_paged_f8_plan_main.cpp")


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    hipcc = compiler()
    if not hipcc:
        pytest.skip("the library's compiler is not installed")
    exe = str(tmp_path_factory.mktemp("attn_prefill_paged_f8_plan") / "attn_prefill_paged_f8_plan")
    subprocess.run([hipcc, "-std=c++20", "-x", "hip", "--offload-arch=gfx950", "--cuda-host-only", "-Wall", "-Werror", "-I", CSRC, MAIN, "-o", exe],
                   check=True, capture_output=True, text=True, timeout=300)
    res = {"plan": [], "refuse": [], "walk": []}
    for line in subprocess.run([exe], check=True, capture_output=True, text=True, timeout=120).stdout.splitlines():
        kind, rest = line.split(" ", 1)
        parts = rest.split(" |")
        head = {k: num(v) for k, v in (kv.split("=") for kv in parts[0].split())}
        if kind == "walk":
            res[kind].append((head, [tuple(int(x) for x in cell.split(":")) for cell in parts[1].split()]))
        else:
            res[kind].append((head,) + tuple(fields(p.strip()) for p in parts[1:]))
    return res


def test_the_f8_plan_is_the_fp16_plan_but_for_the_family(lines):
    """every field: instantiation, grid, LDS, alignment, remap, the page, pointers, strides, the folded scales, the slopes"""
    assert len(lines["plan"]) == 2160
    for i, o, r in lines["plan"]:
        assert o["why"] == "" and r["why"] == "" and (o["ok"], o["f8"], r["ok"], r["f8"]) == (1, 1, 1, 0), (i, o, r)
        diff = {k: (o[k], r[k]) for k in o if k != "f8" and o[k] != r[k]}
        assert not diff, (i, diff)
        assert (o["hspad"], o["pad"]) == (64 if i["hs"] <= 64 else 128, int(i["hs"] not in (64, 128))) and o["qstart"] == o["lens"] == o["table"] == 1
    assert {(o["hspad"], o["sb"], o["pad"]) for _, o, _ in lines["plan"]} == {(h, s, p) for h in (64, 128) for s in (0, 1) for p in (0, 1)}
    assert {o["aligned"] for _, o, _ in lines["plan"]} == {0, 1} and {o["xcd"] for _, o, _ in lines["plan"]} == {0, 1}


def test_each_refusal_names_its_reason(lines):
    """the FP8 pool's refusals come first: head size 40 is refused in the pool's words, not as a shape the fp16 plan would take or name differently"""
    got = {i["what"]: o for i, o in lines["refuse"]}
    none = got.pop("none")
    assert (none["ok"], none["f8"], none["why"]) == (1, 1, "")
    want = {"head_size_40": "FP8 paged cache: head_size must be a multiple of 16", "head_size_144": "head sizes above 128 are not served",
            "step_sl": "row and head strides must be multiples of 16", "block_step": "block_step must be a multiple of 16",
            "base": "pool bases must be 16-byte aligned", "k_scale_zero": "must be positive and finite", "v_scale_inf": "must be positive and finite",
            "null_qstart": "dQStart is null"}
    assert set(got) == set(want)
    for what, text in want.items():
        assert (got[what]["ok"], got[what]["f8"]) == (0, 0) and text in got[what]["why"], (what, got[what])


def test_the_staging_map_addresses_every_row_through_its_own_table_entry(lines):
    """Every (row, 16-dim column) of every tile is staged exactly once for K and once for V; a wave's rows of a step are one aligned group of 1024 / hs
    rows.  Whole tile: the group's base + the lane's part IS attn_page_at of the lane's own row through that row's own entry.  Last tile: the clamped
    key lies in the page of the group's first clamped key, so the group's entry gives the same cell.  A bad id is no address (-1) either way."""
    assert len(lines["walk"]) == 5
    whole_tiles = partial_tiles = bad = 0
    for h, cells in lines["walk"]:
        hs, n = h["hs"], h["kvlen"]
        rpg, tiles = 1024 // hs, -(-n // 64)
        assert len(cells) == tiles * 4 * (hs // 64) * 64 * 2
        staged = {}
        for pos0, w, u, l, kv, row, col, key, whole, got, want in cells:
            first = (4 * u + w) * rpg
            assert first <= row < first + rpg and 0 <= col < hs // 16 and key == min(pos0 + row, n - 1)
            assert whole == int(pos0 + 64 <= n) and (not whole or key == pos0 + row)
            assert key >> (h["bk"].bit_length() - 1) == min(pos0 + first, n - 1) >> (h["bk"].bit_length() - 1)  # one page per group
            assert got == want, (h, pos0, w, u, l, kv, got, want)
            bad += got == -1
            staged.setdefault((pos0, kv, row, col), []).append((w, l))
        assert set(staged) == {(t * 64, kv, r, c) for t in range(tiles) for kv in (0, 1) for r in range(64) for c in range(hs // 16)}
        assert all(len(v) == 1 for v in staged.values())
        whole_tiles, partial_tiles = whole_tiles + n // 64, partial_tiles + (n % 64 != 0)
    assert whole_tiles >= 5 and partial_tiles >= 3 and bad > 0

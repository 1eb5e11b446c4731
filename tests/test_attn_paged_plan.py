"""The paged form of attn_plan (neural-speed_amd/csrc/ns_attn_plan.cpp: what ns_hip_attn_decode_paged builds — the per-request Affine of
ns_hip_attn_decode_rows plus an AttnPage) and the key -> cell translation of a paged cache (attn_page_cell / attn_page_at, ns_attn.h: the functions
the kernels, the append and the store run).  A host program (tests/tools/attn_paged_plan_main.cpp, built with the library's compiler, nothing
launched) prints the plans and walks the translation over every key of a few tables.

The grid is the 480 shapes of tests/test_attn_rows_plan.py times the block sizes 16, 32, 128 and 256.  A paged capacity is table_stride * block_keys,
so each capacity of that grid (1, 255, 256, 300, 2048, 8192) is rounded up to whole blocks, and the per-request plan it is compared with is the one of
that rounded capacity: the same shape and capacity, as the paged entry's contract says."""
import importlib.util
import os
import subprocess

import pytest

from test_attn_plan import CSRC, ROOT, compiler, num
from test_attn_rows_plan import SAME

MAIN = os.path.join(ROOT, "tests", "tools", "attn_paged_plan_main.cpp")
BLOCKS = (16, 32, 128, 256)


def fields(text):
    text, why = text.split(" why=")
    o = {k: num(v) for k, v in (kv.split("=") for kv in text.split())}
    o["why"] = why.strip()
    return o


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    hipcc = compiler()
    if not hipcc:
        pytest.skip("the library's compiler is not installed")
    exe = str(tmp_path_factory.mktemp("attn_paged_plan") / "attn_paged_plan")
    subprocess.run([hipcc, "-std=c++20", "-x", "hip", "--offload-arch=gfx950", "--cuda-host-only", "-Wall", "-Werror", "-I", CSRC, MAIN, "-o", exe],
                   check=True, capture_output=True, text=True, timeout=300)
    out = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=120).stdout
    res = {"plan": [], "refuse": [], "rule32": [], "far32": [], "walk": []}
    for line in out.splitlines():
        kind, rest = line.split(" ", 1)
        parts = rest.split(" | ")
        head = {k: num(v) for k, v in (kv.split("=") for kv in parts[0].split())}
        if kind == "plan":
            res[kind].append((head, fields(parts[1]), fields(parts[2])))
        elif kind in ("refuse", "rule32", "far32"):
            res[kind].append((head, fields(parts[1])))
        else:
            res[kind].append((head, {k: num(v) for k, v in (kv.split("=") for kv in parts[1].split())}))
    return res


def test_the_grid_is_the_rows_grid_times_the_block_sizes(lines):
    seen = {(i["bs"], i["hn"], i["hkv"], i["hs"], i["cap"], i["bk"]) for i, _, _ in lines["plan"]}
    want = {(bs, hn, hkv, hs, -(-cap // bk) * bk, bk) for bk in BLOCKS for bs in (1, 2, 8, 33) for hn, hkv in ((8, 8), (8, 2), (8, 1), (71, 1))
            for hs in (32, 64, 80, 128, 256) for cap in (1, 255, 256, 300, 2048, 8192)}
    assert seen == want and len(lines["plan"]) == 480 * len(BLOCKS)
    assert {i["hm"] for i, _, _ in lines["plan"]} == {0, 1}  # position-major and head-major blocks
    assert {o["path"] for _, o, _ in lines["plan"]} == {"RING", "SPLIT_REGS"}
    assert any(o["nsplit"] > 1 for _, o, _ in lines["plan"]) and any(o["nsplit"] == 1 for _, o, _ in lines["plan"])


def test_the_paged_plan_is_the_rows_plan_of_the_same_shape_and_capacity(lines):
    wrong = [(i, {k: (o[k], r[k]) for k in SAME if o[k] != r[k]}) for i, o, r in lines["plan"] if any(o[k] != r[k] for k in SAME)]
    assert not wrong, (len(wrong), wrong[:3])
    for i, o, r in lines["plan"]:
        assert o["why"] == "" and r["why"] == "", (i, o, r)
        # what differs is what the paging is: the PAGED instantiations, and no batch stride (a request has no slab)
        assert (o["paged"], o["rows"], o["kmove"], o["kdelta"], o["slkv"], o["kbs"]) == (1, 1, 1, 1, i["cap"], 0), (i, o)
        assert (r["paged"], r["rows"]) == (0, 1) and r["kbs"] != 0, (i, r)


def test_each_refusal_names_its_reason(lines):
    got = {i["what"]: o for i, o in lines["refuse"]}
    assert got.pop("none")["path"] == "SERVED"
    assert all(o["path"] == "REFUSED" for o in got.values()), got
    for what in ("block_keys_48", "block_keys_8", "block_keys_512"):
        assert "block_keys must be a power of two from 16 to 256" in got[what]["why"]
    assert "must equal table_stride * block_keys" in got["capacity"]["why"]
    assert "block table is null" in got["null_table"]["why"]
    assert "pool_blocks must be at least 1" in got["pool_blocks"]["why"]
    assert "do not fit inside block_step" in got["block_step_small"]["why"]


def test_the_32_bit_rule_at_its_boundary(lines):
    """The ring kernel addresses a pool through one buffer descriptor: it serves pools of (pool_blocks * block_step + 256) * 2 bytes below 2^32, the
    register kernel (64-bit pointers) every other; nothing is refused and no offset wraps."""
    got = {(i["pool_blocks"], i["block_step"], i["hs"]): (o["path"], o["in32"], o["why"]) for i, o in lines["rule32"]}
    step, limit = 128 * 8 * 128, 2 ** 31 - 256
    assert got[(limit // step, step, 128)] == ("RING", 1, "")
    assert got[(limit // step + 1, step, 128)] == ("SPLIT_REGS", 0, "")
    assert got[(1, limit - 8, 128)] == ("RING", 1, "")
    assert got[(1, limit, 128)] == ("SPLIT_REGS", 0, "")
    assert got[(1, limit + 8, 128)] == ("SPLIT_REGS", 0, "")
    assert got[(limit // step + 1, 2 * step, 256)] == ("SPLIT_REGS", 0, "")
    for (blocks, bstep, _), (_, in32, _) in got.items():
        assert in32 == int((blocks * bstep + 256) * 2 < 2 ** 32)


def test_the_pools_of_the_far_address_tests_take_the_kernels_they_assert(lines):
    """tests/test_gpu_attn_far_addresses.py asserts these kernels through ns_hip_attn_paged_stats on pools of 4 GiB and more: the largest pool the rule
    accepts goes to the ring kernel, 1.4 * 2^31 elements to the register kernel.  If the rule moves, this fails first; the numbers are those of
    tests/tools/attn_far_layout.py."""
    spec = importlib.util.spec_from_file_location("attn_far_layout", os.path.join(ROOT, "tests", "tools", "attn_far_layout.py"))
    FL = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(FL)
    got = {(i["hs"], i["bk"], i["over"]): (i["pool_blocks"], i["block_step"], o["path"], o["in32"], o["why"]) for i, o in lines["far32"]}
    assert len(got) == 2 * len(FL.PAGED_SHAPES)
    for hs, bk in FL.PAGED_SHAPES:
        step = FL.block_step(hs, bk)
        assert got[(hs, bk, 0)] == (FL.pool_blocks("under", step, 0), step, "RING", 1, "")
        assert got[(hs, bk, 1)] == (FL.pool_blocks("over", step, 0), step, "SPLIT_REGS", 0, "")


def test_the_translation_over_every_key_of_a_few_tables(lines):
    """outside: a returned cell whose row leaves the pool or its own block; collide: two different (block, key) pairs at one cell or closer than a row;
    noaccess / wantno: the keys that must get the "no access" answer (-1: an id outside [0, pool_blocks), a key outside the capacity) and those that
    got it; shared: cells named twice by the same (block, key) — the shared prefix, both layouts."""
    got = {i["table"]: o for i, o in lines["walk"]}
    assert set(got) == {"identity", "permutation", "shared_prefix", "out_of_range", "block_256"}
    for name, o in got.items():
        assert o["outside"] == 0 and o["collide"] == 0 and o["noaccess"] == o["wantno"] and o["shared"] == o["sharedwant"], (name, o)
    # 3 requests x 6 blocks x 16 keys, plus one key in front of and one behind each capacity, in both layouts
    assert got["identity"]["keys"] == 2 * 3 * (6 * 16 + 2) and got["identity"]["cells"] == 3 * 6 * 16 and got["identity"]["wantno"] == 2 * 3 * 2
    assert got["permutation"]["cells"] == 3 * 6 * 16
    assert got["shared_prefix"]["cells"] == (2 * 6 - 2) * 16 and got["shared_prefix"]["shared"] == 2 * 2 * 16
    # four bad entries (-1, pool_blocks, INT_MAX, INT_MIN): their 4 x 16 keys get no access, in both layouts
    assert got["out_of_range"]["wantno"] == 2 * (3 * 2 + 4 * 16) and got["out_of_range"]["cells"] == (3 * 6 - 4) * 16
    assert got["block_256"]["cells"] == 4 * 256

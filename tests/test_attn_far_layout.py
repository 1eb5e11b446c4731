"""tests/tools/attn_far_layout.py on its own: the numbers of the far-address cases of the shared-prefix, FP8-block and wide entries, and a check that
those cases CAN fail.  Host arithmetic only: no GPU, no subprocess.

The wide kernel (attn_wide_paged_kernel) is the one paged kernel that does not read through 64-bit pointers: a lane's 16 bytes lie at
    2 * (id * block_step + ihkv * step_head + first row * step_sl)  +  uint32((row in the group * step_sl + 8 * chunk) * 2)
bytes from the pool's base (attn_wide_desc, attn_wide_k_offset / attn_wide_v_offset, ns_attn.h).  lane_address() restates that, and restates it with
one of three mistakes:
    base32       the descriptor's byte offset from the pool kept to 32 bits
    signed       the lane offset sign-extended from 32 bits
    int_product  id * block_step formed in int
What the arithmetic gives, and what is asserted for every lane of every live block of the far and boundary layouts:
    base32       moves every lane of a block at 2^32 bytes or more — onto a trap (the alias at byte offset mod 2^32).
    signed       is the identity below kAwNoCell: THAT is what the plan's rule buys, asserted for every lane at row step s.  At s + 8, which the plan
                 refuses, the last row's offsets reach 2^31 and the mistake moves them 2^32 bytes down — the rule's boundary is where it bites.
    int_product  moves every lane of a block at 2^31 elements or more.  These pools end below 2^32 elements, so the wrapped product is negative and
                 the address lies IN FRONT of the pool, where no trap can lie: asserted to be outside the allocation, never on live data.  On the FP8
                 pool (bytes; live blocks at 2^32 bytes and more) the wrapped product is a low block, and those are traps.
A moved lane never lands on live data, in any layout."""
import importlib.util
import os

import numpy as np
import pytest

_spec = importlib.util.spec_from_file_location("attn_far_layout", os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools", "attn_far_layout.py"))
FL = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(FL)
E31, E32, HKV = FL.E31, FL.E32, FL.HKV


def live_blocks(lens, bk):
    return [-(-n // bk) for n in lens]


def far_layouts():
    """{name: (layout, head size, live block ids, rows per block that hold keys)} of every far pool the GPU cases of the five entries allocate"""
    out = {}
    for hs in FL.SHARED_HS:
        for layout, gap in (("pm", False), ("hm", True)):
            out["shared hs%d %s%s" % (hs, layout, " gapped" if gap else "")] = (
                FL.paged_layout("over", hs, FL.SHARED_BK, live_blocks(FL.SHARED_LENS, FL.SHARED_BK), layout, gap), hs)
    for hs in FL.WIDE_HS:
        for layout in ("pm", "hm"):
            out["wide hs%d %s" % (hs, layout)] = (FL.paged_layout("over", hs, FL.WIDE_BK, live_blocks(FL.WIDE_KV, FL.WIDE_BK), layout), hs)
    return out


def int32(x):
    return (x + E31) % E32 - E31


def lane_address(g, blk, row, ihkv, chunk, mistake=None):
    """byte offset from the pool's base of the 16 bytes lane (row of the block, 16-byte chunk) of kv head ihkv asks for; blocks of 16 keys, so a
    wave's group starts at row 0 of its page"""
    product = blk * g["block_step"]
    if mistake == "int_product":
        product = int32(product)
    base = 2 * (product + ihkv * g["step_head"])
    if mistake == "base32":
        base %= E32
    offset = ((row * g["step_sl"] + 8 * chunk) * 2) % E32
    if mistake == "signed":
        offset = int32(offset)
    return base + offset


def trap_index(g):
    traps = FL.traps_of(g["extents"], g["strip"], g["total"], g["dead"])
    starts = np.array([o for o, _ in traps], np.int64)
    order = np.argsort(starts)
    return starts[order], np.array([n for _, n in traps], np.int64)[order]


def in_a_trap(index, element, span=8):
    """do `span` elements at `element` lie inside one trap (or inside several that touch)"""
    starts, lengths = index
    return bool(np.any((starts <= element) & (element + span <= starts + lengths)))


def lanes(g, hs, blocks, rows=16):
    """every (block, row, kv head) with the first and the last chunk of the head"""
    for blk in blocks:
        for row in range(rows):
            for h in range(HKV):
                for chunk in (0, hs // 8 - 1):
                    yield blk, row, h, chunk


def on_live_data(g, element, span=8):
    return any(o < element + span and element < o + n for o, n in g["extents"])


def test_the_layout_numbers_and_the_wide_rule():
    s, t = FL.wide_edge_steps(256)
    assert (s, t) == (71582768, 71582776) and s % 8 == 0
    assert (15 * s + 256) * 2 < E31 <= (15 * t + 256) * 2  # attn_prefill_paged_wide_plan: last = 15 at blocks of 16
    g = FL.wide_edge_layout(256)
    assert g["block_step"] == 16 * s and 6.8e9 < 2 * g["total"] < 7.0e9 and len(g["extents"]) == 2 * 16 * HKV
    top = max(lane_address(g, 1, 15, 0, c) - 2 * g["block_step"] for c in range(32))
    assert top + 16 == ((15 * s + 256) * 2) and top < E31  # the last offset the rule allows is reached
    assert FL.strides("hm", 128, 16) == (128, 2048) and FL.strides("pm", 128, 16) == (256, 128)
    assert FL.gapped_step(128, 16) == FL.block_step(128, 16) + 8 * 128
    for name, (g, hs) in far_layouts().items():
        high = [i for i in g["ids"].values() if i != 2]
        assert all(i * g["block_step"] > E31 for i in high) and g["total"] < E32, name
        assert FL.traps_of(g["extents"], g["strip"], g["total"], g["dead"])  # (asserts that no trap touches live data)
        if "gapped" in name:  # the gap behind every live block is a trap
            idx = trap_index(g)
            assert all(in_a_trap(idx, i * g["block_step"] + g["cells"], g["block_step"] - g["cells"]) for i in g["ids"].values()), name


@pytest.mark.parametrize("name", list(far_layouts()))
def test_the_three_mistakes_on_the_far_pools(name):
    g, hs = far_layouts()[name]
    idx = trap_index(g)
    high = [i for i in g["ids"].values() if i != 2]
    moved = {"base32": 0, "signed": 0, "int_product": 0}
    for mistake in moved:
        for blk, row, h, chunk in lanes(g, hs, high):
            right, wrong = lane_address(g, blk, row, h, chunk), lane_address(g, blk, row, h, chunk, mistake)
            assert right % 2 == 0 and on_live_data(g, right // 2) and right >= E32
            if mistake == "signed":
                assert wrong == right  # (offsets of a few KiB)
                continue
            assert wrong != right and not on_live_data(g, wrong // 2), (name, mistake, blk, row, h, chunk)
            moved[mistake] += 1
            if mistake == "base32":
                assert in_a_trap(idx, wrong // 2), (name, blk, row, h, chunk, wrong)
            else:
                assert wrong < 0  # in front of the pool: outside the allocation
    assert moved["base32"] == moved["int_product"] == len(high) * 16 * HKV * 2 and moved["signed"] == 0


def test_the_three_mistakes_on_the_boundary_pools():
    s, t = FL.wide_edge_steps(256)
    g = FL.wide_edge_layout(256)
    idx = trap_index(g)
    for blk, row, h, chunk in lanes(g, 256, (1, 2)):
        right = lane_address(g, blk, row, h, chunk)
        assert on_live_data(g, right // 2)
        assert in_a_trap(idx, right // 2 - 8 * chunk + 256, 8)  # the cells hs .. hs + 7 behind the row
        assert lane_address(g, blk, row, h, chunk, "signed") == right  # every offset below 2^31: the rule
        wrong = lane_address(g, blk, row, h, chunk, "base32")
        assert (wrong != right) == (blk == 2) and (blk == 1 or in_a_trap(idx, wrong // 2)), (blk, row, h, chunk)
        wrong = lane_address(g, blk, row, h, chunk, "int_product")
        assert (wrong != right) == (blk == 2) and (blk == 1 or wrong < 0), (blk, row, h, chunk)
        for a in FL.aliases(right // 2, 8, g["total"]):  # offset - 2^31, offset mod 2^32
            assert in_a_trap(idx, a), (blk, row, h, chunk, a)
    assert any(lane_address(g, 1, row, 0, 0) // 2 >= E31 for row in range(16))  # rows of block 1 cross 2^31 elements as well
    # one step further, which the plan refuses: the last row's offsets no longer fit 31 bits, and a signed offset lands 2^32 bytes lower
    e = FL.wide_edge_layout(256, t)
    assert lane_address(e, 1, 15, 0, 31, "signed") == lane_address(e, 1, 15, 0, 31) - E32
    assert lane_address(e, 1, 14, 0, 31, "signed") == lane_address(e, 1, 14, 0, 31)


def test_an_int_product_on_the_fp8_pool_lands_in_the_low_blocks_which_are_traps():
    """FarPools8 (tests/test_gpu_attn_paged_f8.py): blocks of 16 * 2 * 128 bytes, the first and the last 64 blocks 0x7f but for the live ones"""
    step = FL.block_step(128, 16)
    assert step == 4096
    for lens in (FL.SHARED_LENS, FL.BLOCK_KV[16]):
        _, ids = FL.place(live_blocks(lens, 16), FL.PAGED_CAP[16] // 16, FL.F8_BLOCKS)
        high = [i for i in ids.values() if i != 2]
        assert len(high) == len(ids) - 1 and all(i * step >= E32 and i >= FL.F8_BLOCKS - 64 for i in high)
        for i in high:
            for wrapped in (int32(i * step), (i * step) % E32):
                assert 0 <= wrapped < 64 * step and wrapped // step != 2  # a painted block that is not the one low live block

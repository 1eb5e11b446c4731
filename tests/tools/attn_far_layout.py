"""Where tests/test_gpu_attn_far_addresses.py puts its K / V rows: pool sizes, strides, physical block ids, and the places a truncated address would
land (the alias traps).  Host arithmetic only — the CPU plan tests (tests/test_attn_plan.py, tests/test_attn_paged_plan.py, the shared, FP8-block and
wide plan tests) run the plan on the same numbers, so a 32-bit rule that moves fails there with the reason, not on the GPU with a changed path;
tests/test_attn_far_layout.py restates the wide kernel's address with three mistakes in it and looks for the traps they reach.

Offsets are fp16 ELEMENTS from a tensor's base unless a name says bytes."""
import numpy as np

HN, HKV = 4, 2            # query / kv heads of every case: head group 2
E31, E32 = 1 << 31, 1 << 32
TRAP, NAN16 = 0x7F7F, 0xFFFF  # 0x7f bytes (an fp16 NaN as well: a consumed trap shows in a read, a written one in the compare); dead cells of live blocks

# ---- paged pools -----------------------------------------------------------------------------------------------------------------------------------
PAGED_SHAPES = [(64, 16), (64, 128), (128, 16), (128, 128)]  # (head size, keys per block)
PAGED_CAP = {16: 256, 128: 512}                              # a request's capacity by block size: 16 / 4 table entries
PAGED_LENS = {16: [70, 200], 128: [200, 300]}                # live keys: 5 + 13 blocks of 16, 2 + 3 blocks of 128; every length ends inside a block
BLOCK_Q = [1, 5, 40]                                         # query rows of the three requests of the ragged-block cases
BLOCK_KV = {16: [70, 200, 120], 128: [200, 300, 150]}


def block_step(hs, bk):
    """elements of a position-major block [key][kv head][dim]"""
    return bk * HKV * hs


# ---- the shared-prefix, FP8-block and wide cases ------------------------------------------------------------------------------------------------------
SHARED_HS, SHARED_BK, SHARED_CAP = [64, 128], 16, 256
SHARED_START, SHARED_PREFIX, SHARED_MAX_GROUP = [0, 3], [64], 3  # one group: requests 0 .. 2, the leader's first 64 keys
SHARED_LENS = [70, 200, 64, 33]  # the leader ends inside a block, a member beside the capacity, a member with an empty suffix; request 3 is in no group
WIDE_HS, WIDE_BK, WIDE_CAP = [256, 160], 16, 256  # the exact instantiation and a padded one
WIDE_Q, WIDE_KV = [1, 130, 40], BLOCK_KV[16]
F8_BLOCKS = (1 << 20) + 64  # FarPools8 (tests/test_gpu_attn_paged_f8.py): blocks of 4096 bytes; up to 25 high blocks, every second one, all above 2^32 bytes
GAP_ROWS = 8                # a gapped block: GAP_ROWS * hs cells behind a block's own, traps
WIDE_NO_CELL = 1 << 31      # kAwNoCell (ns_attn.h): the wide kernel's lane offsets and num_records stay below it
EDGE_BLOCKS, EDGE_BK, EDGE_Q, EDGE_KV = 3, 16, [20, 1], [20, 17]  # the wide descriptor boundary: block 0 traps, live blocks 1 and 2
EDGE_TABLE = [[1, 2], [2, 1]]  # request 0: keys 0 .. 15 in block 1, 16 .. 19 in rows 0 .. 3 of block 2; request 1: keys 0 .. 15 in block 2, key 16 in row 0 of block 1


def strides(layout, hs, bk):
    """(step_sl, step_head) of a block: "pm" [key][kv head][dim], "hm" [kv head][key][dim]"""
    assert layout in ("pm", "hm")
    return (HKV * hs, hs) if layout == "pm" else (hs, bk * hs)


def gapped_step(hs, bk):
    """block_step of a block with GAP_ROWS * hs cells of gap behind its own"""
    return block_step(hs, bk) + GAP_ROWS * hs


def paged_layout(size, hs, bk, live, layout="pm", gap=False):
    """everything tests/test_gpu_attn_far_addresses.py's Pages is made of: strides, pool size, table, ids, the live blocks' extents (a block's own
    cells: a gap is no part of one) and the arguments traps_of gets — a whole block step as the strip, so a gap lies inside it, and block 0 dead"""
    cells, step = block_step(hs, bk), gapped_step(hs, bk) if gap else block_step(hs, bk)
    step_sl, step_head = strides(layout, hs, bk)
    assert (bk - 1) * step_sl + (HKV - 1) * step_head + hs <= cells
    n = pool_blocks(size, step, sum(live))
    table, ids = place(live, PAGED_CAP[bk] // bk, n)
    extents = [(i * step, cells) for i in ids.values()]
    gaps = [(i * step + cells, step - cells) for i in ids.values()] if gap else []  # (by name: the last block's strip would end behind the pool)
    return dict(cells=cells, block_step=step, step_sl=step_sl, step_head=step_head, pool_blocks=n, table=table, ids=ids, total=n * step, extents=extents,
                strip=step, dead=[(0, step)] + gaps)


def wide_rule(bk, step_sl, hs):
    """attn_prefill_paged_wide_plan's rule restated: the last key's last byte, and every lane offset with it, below kAwNoCell"""
    return ((bk - 1) * step_sl + hs) * 2 < WIDE_NO_CELL


def wide_edge_steps(hs):
    """(the largest row step, a multiple of 8, that keeps the 16 rows of a block of one kv head inside a descriptor below kAwNoCell; the next one)"""
    s = ((WIDE_NO_CELL // 2 - 1 - hs) // (EDGE_BK - 1)) // 8 * 8
    assert (15 * s + hs) * 2 < E31 <= (15 * (s + 8) + hs) * 2
    assert wide_rule(EDGE_BK, s, hs) and not wide_rule(EDGE_BK, s + 8, hs)
    return s, s + 8


def wide_edge_layout(hs, step_sl=None):
    """the boundary pools: EDGE_BLOCKS blocks of 16 rows step_sl apart, kv head 1 hs + 8 cells behind kv head 0, so the 8 cells behind every live row
    of a head are no head's; extents: every (row, kv head) of blocks 1 and 2; dead: those of block 0, where a dropped id lands"""
    step_sl = wide_edge_steps(hs)[0] if step_sl is None else step_sl
    step_head, step = hs + 8, EDGE_BK * step_sl
    assert (EDGE_BK - 1) * step_sl + (HKV - 1) * step_head + hs <= step
    cell = lambda blk: [(blk * step + r * step_sl + h * step_head, hs) for r in range(EDGE_BK) for h in range(HKV)]
    return dict(block_step=step, step_sl=step_sl, step_head=step_head, pool_blocks=EDGE_BLOCKS, total=EDGE_BLOCKS * step, extents=cell(1) + cell(2),
                strip=8, dead=cell(0))


def page_in32(pool_blocks, step):
    """attn_page_in32 (ns_attn.h) restated"""
    return (pool_blocks * step + 256) * 2 < E32


def pool_blocks(size, step, n_live):
    """near: a compact pool; under: the largest pool the ring kernel's descriptor spans; over: about 1.4 * 2^31 elements"""
    if size == "near":
        return 2 * n_live + 6
    if size == "under":
        n = (E31 - 257) // step
        assert page_in32(n, step) and not page_in32(n + 1, step) and (n * step + 256) * 2 < E32
        return n
    n = int(1.4 * E31) // step
    assert size == "over" and not page_in32(n, step)
    return n


def place(live, ts, n_blocks):
    """table [requests][ts] and {(request, logical block): physical id} for live[b] live blocks per request: request 0's first block is the one low
    block (id 2), every other live block is one of the LAST blocks of the pool, every second one so that each has a spare neighbour; table entries
    behind a request's live blocks name block 0, which holds traps"""
    table = np.zeros((len(live), ts), np.int32)
    ids, high = {}, 0
    for b, n in enumerate(live):
        for j in range(n):
            if not ids:
                ids[(b, j)] = 2
            else:
                ids[(b, j)] = n_blocks - 1 - 2 * high
                high += 1
            table[b, j] = ids[(b, j)]
    assert n_blocks - 1 - 2 * high > 3 and len(set(ids.values())) == len(ids)
    return table, ids


# ---- slabs -------------------------------------------------------------------------------------------------------------------------------------------
SLAB_STEP = (1 << 30) + (1 << 21)  # far batch step: entry 2 starts at 2^31 + 2^22 elements, whose alias 2^22 is free (a step of exactly 2^30 would alias entry 0)
HEAD_STEP = 1 << 30                 # far head step: (batch 1, kv head 1) starts at SLAB_STEP + HEAD_STEP = 2^31 + 2^21
ROPE_SL, ROPE_PAST = 1 << 20, 2100  # ns_hip_rope_qkv_append: a padded row step and a position whose row starts at 2100 * 2^20 > 2^31 elements
EDGE_KEYS = 300                     # the slab rule's boundary: 300 keys a very large row step apart
assert SLAB_STEP < E31 and SLAB_STEP % 8 == 0  # (the argument structs carry int steps)


def slab_in32(rows, step_sl):
    """attn_in32 (ns_attn_plan.cpp) restated: `rows` rows of a head inside one 32-bit buffer descriptor"""
    return (rows * step_sl + 256) * 2 < E32


def edge_steps(rows):
    """(the largest row step, a multiple of 8, that keeps `rows` rows inside a descriptor; the next multiple of 8)"""
    s = (E31 - 257) // rows // 8 * 8
    assert slab_in32(rows, s) and not slab_in32(rows, s + 8)
    return s, s + 8


def tile_rows(sl_kv):
    """rows attn_mfma3_kernel requests: whole 64-key tiles"""
    return -(-sl_kv // 64) * 64


# ---- aliases and traps ---------------------------------------------------------------------------------------------------------------------------------
def aliases(e, span, total):
    """where the `span` elements at e would be looked for after a truncation — the element offset mod 2^31 or 2^32, the byte offset mod 2^32 — as far
    as that differs from e and lies inside a tensor of `total` elements"""
    return sorted({a for a in (e % E31, e % E32, (2 * e) % E32 // 2) if a != e and a + span <= total})


def traps_of(extents, strip, total, dead=()):
    """[(offset, length)] to poison around the live extents [(offset, length)]: every alias of an extent, `strip` elements directly before and after
    it, and the `dead` extents with their aliases.  Asserts that no trap touches a live element."""
    traps = set()
    for off, n in extents:
        traps.update((a, n) for a in aliases(off, n, total))
        if off >= strip:
            traps.add((off - strip, strip))
        if off + n + strip <= total:
            traps.add((off + n, strip))
    for off, n in dead:
        if off + n <= total:
            traps.add((off, n))
        traps.update((a, n) for a in aliases(off, n, total))
    traps = sorted(traps)
    starts = np.array([o for o, _ in extents], np.int64)
    ends = starts + np.array([n for _, n in extents], np.int64)
    for off, n in traps:
        hit = (starts < off + n) & (off < ends)
        assert not hit.any(), "a trap at %d (+%d) coincides with live data at %s" % (off, n, starts[hit][:4])
    return traps

"""Where tests/test_gpu_attn_far_addresses.py puts its K / V rows: pool sizes, strides, physical block ids, and the places a truncated address would
land (the alias traps).  Host arithmetic only — the CPU plan tests (tests/test_attn_plan.py, tests/test_attn_paged_plan.py) run the plan on the same
numbers, so a 32-bit rule that moves fails there with the reason, not on the GPU with a changed path.

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

"""Prompt-sized query blocks over an FP8 (E4M3) paged KV cache at head sizes 144 .. 256: ns_hip_attn_prefill_paged_wide_f8 (attn_wide_paged8_kernel: the
fp16 wide kernel from its LDS image on, the codes loaded through registers and decoded once per workgroup).  docs/kernels/attention.md, "Head sizes
144 .. 256 over an FP8 paged cache".  Inputs are Step8's (c.kc / c.vc the codes, c.k / c.v their values in fp16: the fp16 entry takes the same argument
block but for the pool pointers); the uint8 pools hold 0x7f — NaN — behind every live length, in spare blocks and, padded cases, in the odd heads of
pools with twice the kv heads; dst is preset to 7.0.  Every case is checked (1) through check_rag against the fp64 attention over the decoded values
(the fp16 module's bound: rel_l2 < 1e-3, per row max(2^-11, 4 d)) and (2) BIT FOR BIT against ns_hip_attn_prefill_paged_wide over fp16 pools of the
codes' values under the same table: the decode is exact and the LDS images coincide, so equality is derived, not measured.  Largest row error / bound
on an MI355X: 0.416."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_attn_block_paged import LEAD, block_args, block_stats, check_rag
from test_gpu_attn_block_paged_f8 import all_codes
from test_gpu_attn_paged import delta, paged_stats
from test_gpu_attn_paged_f8 import NAN8, FarPools8, Pools8, f8_stats, pools_pair
from test_gpu_attn_prefill_paged import prefill_stats
from test_gpu_attn_prefill_paged_f8 import Step8, prefill8_stats, same
from test_gpu_attn_prefill_paged_wide import run_wide, spaced_pools, wide_stats
from test_gpu_attn_rows import ALIBI, CAUSAL, HM, PM, TANH, attn_stats, stream_ptr

pytestmark = pytest.mark.gpu


def wide8_stats(L):
    out = (C.c_ulonglong * 4)()
    L.ns_hip_attn_prefill_paged_wide_f8_stats(out)
    return list(out)


def others(L):
    return wide_stats(L), prefill8_stats(L), prefill_stats(L), f8_stats(L), paged_stats(L), block_stats(L), attn_stats(L)


class F8Wide:
    """run_wide's library handle with the FP8 entry in the fp16 entry's place"""

    def __init__(self, L):
        self.ns_hip_attn_prefill_paged_wide = L.ns_hip_attn_prefill_paged_wide_f8


def pair(c, bk, layout, padded=0, table_edit=None):
    """the uploaded FP8 pools and the fp16 pools of the decoded values under one table; padded: both with twice the kv heads, the odd ones NaN"""
    if not padded:
        return pools_pair(c, bk, layout, table_edit)
    p8 = Pools8(c.bs, 2 * c.hkv, c.hs, c.cap, bk, layout, 5)
    wide = lambda x: np.stack([x, np.full(x.shape, NAN8, np.uint8)], axis=3).reshape(c.bs, c.cap, 2 * c.hkv, c.hs)
    p8.fill(wide(c.kc), wide(c.vc), c.kvlens)
    p8.step_head *= 2
    p16 = spaced_pools(c, bk, layout)
    assert np.array_equal(p8.table, p16.table)
    return p8.upload(), p16.upload()


def both(L, pkg, c, p8, p16, **kw):
    """the FP8 entry's output (with what run_wide returns beside it) after the housekeeping every run shares, and the fp16 entry's under the same table"""
    o0 = others(L)
    got = run_wide(F8Wide(L), pkg, c, p8, **kw)
    assert others(L) == o0 and p8.guards_intact() and p8.unchanged()  # no other entry's counter moves; the attention writes no cache byte
    return got, run_wide(L, pkg, c, p16, **kw)[0]


# name: ((heads, kv heads, head size, capacity, q lens, kv lens, flags), Step8's keywords, block_keys, layout, padded)
BOUNDARY = (4, 2, 256, 512, [130, 1, 0, 17], [300, 17, 0, 64], CAUSAL)  # two query blocks with a last wave of two rows, a decode row, an idle request, a chunk that ends on a tile
PADDED = lambda hs: (4, 2, hs, 256, [33, 130], [100, 200], CAUSAL)      # a chunk read past head_size, or a byte of the next head, shows as NaN
CASES = {
    "a_query_block_boundary_bk16": (BOUNDARY, {}, 16, PM, 0),    # four pages per tile
    "a_query_block_boundary_bk256": (BOUNDARY, {}, 256, PM, 0),  # four tiles per page
    "c_more_rows_than_keys": ((4, 2, 256, 256, [10, 5, 3, 140], [4, 5, 0, 130], CAUSAL), dict(seed=1), 16, PM, 0),
    "d_gemma_8_on_1_not_causal_head_major": ((8, 1, 256, 1024, [150, 3], [1000, 65], 0), {}, 128, HM, 0),
    "e_head_size_144": (PADDED(144), {}, 16, PM, 1),
    "e_head_size_160": (PADDED(160), {}, 32, HM, 1),
    "e_head_size_240": (PADDED(240), {}, 64, PM, 1),
    "g_all_254_finite_codes": ((4, 2, 256, 256, [16], [100], CAUSAL), dict(scales=(2.0 ** -6, 0.25, 2.0, 4.0), codes=all_codes), 16, PM, 0),
    "i_tensor_scales": ((4, 2, 256, 256, [129, 16], [200, 16], CAUSAL), dict(scales=(0.5, 2.0, 0.25, 4.0), seed=3), 16, PM, 0),
}
_steps = {}


def step8(nso, name):
    """inputs and references of a case, made once and shared"""
    if name not in _steps:
        _steps[name] = Step8(nso, *CASES[name][0], **CASES[name][1])
    return _steps[name]


@pytest.mark.parametrize("name", list(CASES))
def test_f8_wide_prompt_blocks_against_the_reference_and_the_bits_of_the_fp16_entry(L, pkg, nso, name):
    _, _, bk, layout, padded = CASES[name]
    c = step8(nso, name)
    s0 = wide8_stats(L)
    (out, _, _), half = both(L, pkg, c, *pair(c, bk, layout, padded))
    assert delta(s0, wide8_stats(L)) == [1 - padded, padded, 0, 0]
    assert np.all(np.isfinite(out)), name  # no byte behind a live length, no spare block, no neighbouring head was consumed
    check_rag(nso, "f8 wide " + name, c, out)
    assert same(out, half), name


@pytest.mark.parametrize("edge", ["junk_behind_the_live_blocks", "bad_id_minus_one", "bad_id_pool_blocks", "strided_unaligned_dst_with_dst16"])
def test_contract_edges(L, pkg, nso, edge):
    """case (a), blocks of 16.  junk: every entry behind a request's live blocks holds -1, pool_blocks or the id of a NaN block — the clean run's bits.
    bad id: request 0's second block (live) is no block of the pool — request 0 is finite, every other request holds the clean run's bits.  strided
    dst (rows of hs + 3 floats, one float behind a 16-byte boundary): the bits of the 16-byte stores, dst16 the rounded output, paddings still 7.0."""
    c = step8(nso, "a_query_block_boundary_bk16")
    good = both(L, pkg, c, *pair(c, 16, PM))[0][0]

    def change(p):
        if edge.startswith("bad_id"):
            p.table[0, 1] = -1 if edge == "bad_id_minus_one" else p.pool_blocks
            return
        spare = min(set(range(p.pool_blocks)) - set(p.table.ravel().tolist()))  # a block no request names: NaN codes throughout
        for b, n in enumerate(c.kvlens):
            first = -(-n // 16)
            p.table[b, first:] = [(-1, p.pool_blocks, spare)[j % 3] for j in range(p.ts - first)]

    if edge.startswith("strided"):
        p8, p16 = pair(c, 16, PM)
        (plain, s16, _), _ = both(L, pkg, c, p8, p16, dst16=True)
        (out, o16, whole), half = both(L, pkg, c, p8, p16, dst16=True, dst_pad=3)
        live = slice(c.start[0], c.start[-1])
        assert same(plain, good) and same(out, good) and same(out, half) and np.all(whole[..., c.hs:] == 7.0) and np.all(o16[..., c.hs:] == 7.0)
        assert np.array_equal(o16[live, :, :c.hs], out[live].astype(np.float16)) and np.array_equal(s16[live], plain[live].astype(np.float16))
        assert all(np.all(x[:LEAD] == 7.0) and np.all(x[c.start[-1]:] == 7.0) for x in (o16, s16))
        return
    (out, _, _), half = both(L, pkg, c, *pair(c, 16, PM, table_edit=change))
    kept = slice(None) if edge.startswith("junk") else slice(c.start[1], None)
    assert np.all(np.isfinite(out)) and same(out[kept], good[kept]) and same(out, half) and np.all(out[:LEAD] == 7.0)


def test_refusals_are_counted_and_write_nothing(L, pkg, nso):
    """in the entry's order: the scales, the FP8 pool's words (136 and 152 among them), then the wide plan's: -1, the reason, stats [3], nothing written"""
    import torch
    c = step8(nso, "a_query_block_boundary_bk16")
    p = pair(c, 16, PM)[0]
    dq = torch.from_numpy(c.q.copy()).cuda()
    dd = torch.full((c.rows, c.hn, c.hs), 7.0, device="cuda")
    ds = torch.tensor(c.start, dtype=torch.int32, device="cuda")
    dl = torch.tensor(c.kvlens, dtype=torch.int32, device="cuda")

    def call(step=p.block_step, start=True, bk=16, **fields):
        a = block_args(pkg, c, p, dq.data_ptr(), dd.data_ptr(), 130, c.hs)
        for k, v in fields.items():
            setattr(a, k, v)
        return L.ns_hip_attn_prefill_paged_wide_f8(C.byref(a), C.c_void_p(ds.data_ptr()) if start else None, C.c_void_p(dl.data_ptr()), 0,
                                                   C.c_void_p(p.dt.data_ptr()), p.ts, bk, p.pool_blocks, step, None, stream_ptr())

    scales, width = "must be positive and finite", "not built at this width"
    calls = [(scales, dict(K_sc=0.0)), (scales, dict(V_sc=-1.0)), (scales, dict(K_sc=float("inf"))), (scales, dict(V_sc=float("nan"))),
             (scales, dict(K_sc=0.0, head_size=136)), ("FP8 paged cache: head_size must be a multiple of 16", dict(head_size=136)),
             ("FP8 paged cache: head_size must be a multiple of 16", dict(head_size=152)), ("served by ns_hip_attn_prefill_paged_f8", dict(head_size=128)),
             ("multiple of 8 from 136 to 256", dict(head_size=272)), ("strides must be multiples of 16", dict(step_k_sl=p.step_sl + 8)),
             ("block_step must be a multiple of 16", dict(step=p.block_step + 8)), ("pool bases must be 16-byte aligned", dict(K=p.kp + 8)),
             (width, dict(attn_flags=CAUSAL | ALIBI)), (width, dict(attn_flags=CAUSAL | TANH)), (width, dict(QK_scale=-0.0625)), (width, dict(QK_scale=0.0)),
             ("dQStart is null", dict(start=False)), ("power of two from 16 to 256", dict(bk=48))]
    s0, o0 = wide8_stats(L), others(L)
    for n, (text, kw) in enumerate(calls):
        L.ns_hip_reset_error()
        assert call(**kw) == -1, text
        assert text in pkg.last_error(), (text, pkg.last_error())
        assert delta(s0, wide8_stats(L)) == [0, 0, 0, n + 1]
    torch.cuda.synchronize()
    assert bool(torch.all(dd == 7.0)) and others(L) == o0 and p.unchanged()
    L.ns_hip_reset_error()


def test_captured_step_replayed_on_other_contents(L, pkg, nso):
    """The entry captured ONCE on a side stream — no tmp, no scratch, no eager call of it in front — then replayed after the CONTENTS of dQStart, dKvLens,
    the table, Q and the pools changed.  Every replay equals the same step run eagerly, bit for bit; the last one meets the reference."""
    import torch
    hn, hkv, hs, cap, bk = 4, 2, 256, 256, 16
    steps = [Step8(None, hn, hkv, hs, cap, [130, 1], [130, 77], seed=41), Step8(nso, hn, hkv, hs, cap, [1, 70], [131, 200], seed=42)]
    pools = [Pools8(2, hkv, hs, cap, bk, PM, 50 + n).fill(s.kc, s.vc, s.kvlens) for n, s in enumerate(steps)]
    rows, side = max(s.rows for s in steps), torch.cuda.Stream()
    with torch.cuda.stream(side):
        p = pools[0].upload()  # the device buffers of the graph; their contents move to step n's below
        q, dst = torch.zeros((rows, hn, hs), device="cuda"), torch.full((rows, hn, hs), 7.0, device="cuda")
        start, lens = torch.zeros(3, dtype=torch.int32, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda")
        a = block_args(pkg, steps[0], p, q.data_ptr(), dst.data_ptr(), 130, hs)

        def move_to(n):
            s = steps[n]
            q.zero_(), dst.fill_(7.0)
            q[:s.rows].copy_(torch.from_numpy(s.q.copy()))
            start.copy_(torch.tensor(s.start, dtype=torch.int32)), lens.copy_(torch.tensor(s.kvlens, dtype=torch.int32))
            p.dk.copy_(torch.from_numpy(pools[n].k)), p.dv.copy_(torch.from_numpy(pools[n].v)), p.dt.copy_(torch.from_numpy(pools[n].table))

        def call():
            pkg.check(L.ns_hip_attn_prefill_paged_wide_f8(C.byref(a), C.c_void_p(start.data_ptr()), C.c_void_p(lens.data_ptr()), 0, *p.table_args(), None, stream_ptr()))

        move_to(0)
        side.synchronize()
        s0, g = wide8_stats(L), torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            call()
        assert delta(s0, wide8_stats(L)) == [1, 0, 0, 0]
        for n, s in enumerate(steps):
            move_to(n)
            g.replay()
            side.synchronize()
            got = dst.cpu().numpy()
            move_to(n)
            call()
            side.synchronize()
            assert same(got, dst.cpu().numpy()), n
        check_rag(nso, "f8 wide, replayed step 2", s, got[:s.rows])
    torch.cuda.synchronize()


def test_far_pool_is_bit_equal_to_the_compact_twin(L, pkg, nso):
    """FarPools8: untouched pools of 2^19 + 64 blocks of 8192 bytes, the live blocks at their top — above 2^32 bytes — plus block 2, 0x7f bytes in the
    first 64 blocks (where an offset truncated to 32 bits lands) and around the live ones.  The far run holds the bits of the compact twin, which meets
    the reference; no 0x7f byte is consumed or overwritten."""
    from test_gpu_attn_far_addresses import FL, need, release, same_bits
    hs, bk = 256, 16
    c = Step8(nso, FL.HN, FL.HKV, hs, FL.PAGED_CAP[bk], [5, 40], [70, 120], seed=31)
    live, outs, p, s0 = [-(-n // bk) for n in c.kvlens], [], None, wide8_stats(L)
    need(2 * ((1 << 32) + (1 << 20)))
    try:
        for blocks in (FL.pool_blocks("near", bk * c.hkv * hs, sum(live)) + 128, (1 << 19) + 64):
            p = FarPools8(blocks, c, bk, live)
            assert blocks < 1 << 19 or all(i == 2 or i * p.block_step >= 1 << 32 for i in p.ids.values())
            for b, n in enumerate(c.kvlens):
                p.put(b, c.kc[b, :n], c.vc[b, :n])
            outs.append(run_wide(F8Wide(L), pkg, c, p)[0])
            assert p.live()[1] and np.all(np.isfinite(outs[-1])), blocks
            p = None
            release()
        assert delta(s0, wide8_stats(L)) == [2, 0, 0, 0]
        check_rag(nso, "f8 wide, far addresses, near twin", c, outs[0])
        assert same_bits(outs[1], outs[0])
    finally:
        p = None
        release()

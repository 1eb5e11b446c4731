"""Prompt-sized query blocks over the paged KV cache at head sizes 136 .. 256: ns_hip_attn_prefill_paged_wide (attn_wide_paged_kernel: the 128-row
kernel's arithmetic, K / V tiles moved pool -> LDS by DMA through one buffer descriptor per page and wave).  docs/kernels/attention.md, "Head sizes
136 .. 256 over a paged cache".

Pools, their NaN fill and guards, the packed Q / dst with lead and tail rows, dst preset to 7.0 and the per-request check are those of
tests/test_gpu_attn_block_paged.py (by import); reference and bounds are the project's: every request against nso.attn_ref through check() of
tests/test_gpu_attention_paths.py — rel_l2 < 1e-3 and, per row, max(2^-11, 4 d), d the row's distance between the fp64 rounding model and the
reference.  The padded head sizes run on pools with TWICE the kv heads, the call's heads being the even ones and the odd ones NaN: what follows a
head's dims in a position-major row is NaN, so a chunk read past head_size shows.  Largest row error / bound on an MI355X: 0.376 (docs/kernels/attention.md)."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_attention_paths import check, rounding_model
from test_gpu_attn_block_paged import LEAD, Rag, block_args, block_stats, check_rag, rag_pools
from test_gpu_attn_paged import NAN16, Pools, delta, paged_stats
from test_gpu_attn_prefill_paged import prefill_stats
from test_gpu_attn_rows import ALIBI, CAUSAL, HM, PM, TANH, attn_stats, stream_ptr

pytestmark = pytest.mark.gpu


def wide_stats(L):
    out = (C.c_ulonglong * 4)()
    L.ns_hip_attn_prefill_paged_wide_stats(out)
    return list(out)


def spaced_pools(c, bk, layout):
    """pools of 2 * hkv heads: head 2 j holds the call's kv head j, head 2 j + 1 NaN; the call steps two heads at a time"""
    p = Pools(c.bs, 2 * c.hkv, c.hs, c.cap, bk, layout, 5)
    wide = lambda x: np.stack([x.view(np.uint16), np.full(x.shape, NAN16, np.uint16)], axis=3).reshape(c.bs, c.cap, 2 * c.hkv, c.hs)
    p.fill(wide(c.k), wide(c.v), c.kvlens)
    p.step_head *= 2
    return p


def run_wide(L, pkg, c, p, dst16=False, dst_pad=0, expect=0):
    """the entry on step c over the uploaded pools p: (dst [rows][hn][hs], the fp16 shadow or None, the whole dst buffer); dst starts as 7.0; dst_pad >
    0: rows of hs + dst_pad floats and a dst pointer one float behind a 16-byte boundary"""
    import torch
    dq = torch.from_numpy(c.q.copy()).cuda()
    row, skew = c.hs + dst_pad, 1 if dst_pad else 0
    buf = torch.full((c.rows * c.hn * row + skew,), 7.0, device="cuda")
    b16 = torch.full((c.rows * c.hn * row,), 7.0, device="cuda", dtype=torch.float16) if dst16 else None
    ds = torch.tensor(c.start, dtype=torch.int32, device="cuda")
    dl = torch.tensor(c.kvlens, dtype=torch.int32, device="cuda")
    a = block_args(pkg, c, p, dq.data_ptr(), buf.data_ptr() + 4 * skew, max(c.qlens), row)
    rc = L.ns_hip_attn_prefill_paged_wide(C.byref(a), C.c_void_p(ds.data_ptr()), C.c_void_p(dl.data_ptr()), 0, *p.table_args(),
                                          C.c_void_p(b16.data_ptr()) if dst16 else None, stream_ptr())
    assert rc == expect, pkg.last_error()
    torch.cuda.synchronize()
    whole = buf[skew:].cpu().numpy().reshape(c.rows, c.hn, row)
    return np.ascontiguousarray(whole[..., :c.hs]), (b16.cpu().numpy().reshape(c.rows, c.hn, row) if dst16 else None), whole


# name: ((heads, kv heads, head size, capacity, q lens, kv lens, flags), Rag's keywords, block_keys, layout, padded)
BOUNDARY = (4, 2, 256, 512, [130, 1, 0, 17], [300, 17, 0, 64], CAUSAL)  # two query blocks with a last wave of two rows, a decode row, an idle request, a chunk that ends on a tile
PADDED = lambda hs: (4, 2, hs, 256, [33, 130], [100, 200], CAUSAL)
CASES = {
    "a_query_block_boundary_bk16": (BOUNDARY, {}, 16, PM, 0),    # four pages per tile
    "a_query_block_boundary_bk256": (BOUNDARY, {}, 256, PM, 0),  # four tiles per page
    "b_chunk_from_position_0": ((2, 2, 256, 256, [129], [129], CAUSAL), {}, 16, PM, 0),
    "c_more_rows_than_keys": ((4, 2, 256, 256, [10, 5, 3, 140], [4, 5, 0, 130], CAUSAL), dict(seed=1), 16, PM, 0),
    "d_gemma_8_on_1_not_causal_head_major": ((8, 1, 256, 1024, [150, 3], [1000, 65], 0), {}, 128, HM, 0),
    "e_head_size_136": (PADDED(136), {}, 16, PM, 1),
    "e_head_size_160": (PADDED(160), {}, 32, HM, 1),
    "e_head_size_248": (PADDED(248), {}, 64, PM, 1),
    "i_tensor_scales": ((4, 2, 256, 256, [129, 16], [200, 16], CAUSAL), dict(scales=(0.5, 2.0, 0.25, 4.0), seed=3), 16, PM, 0),
}
_steps = {}


def step(nso, name):
    """inputs and references of a case, made once and shared (Rag keeps them read-only)"""
    key = repr((CASES[name][0], sorted(CASES[name][1].items())))
    if key not in _steps:
        _steps[key] = Rag(nso, *CASES[name][0], **CASES[name][1])
    return _steps[key]


@pytest.mark.parametrize("name", list(CASES))
def test_prompt_blocks_against_the_reference(L, pkg, nso, name):
    """... with the instantiation asserted through the stats, and what the call must leave alone: dst rows outside every request keep their 7.0
    (check_rag), the guards and every pool byte are unchanged, the output is NaN-free although every cell behind a live length, every spare block and
    (padded cases) every neighbouring head is NaN.  One launch: no counter of any other attention entry moves."""
    _, _, bk, layout, padded = CASES[name]
    c = step(nso, name)
    p = (spaced_pools(c, bk, layout) if padded else rag_pools(c, bk, layout)).upload()
    s0, others = wide_stats(L), (attn_stats(L), block_stats(L), paged_stats(L), prefill_stats(L))
    out = run_wide(L, pkg, c, p)[0]
    assert delta(s0, wide_stats(L)) == [1 - padded, padded, 0, 0]
    assert (attn_stats(L), block_stats(L), paged_stats(L), prefill_stats(L)) == others
    assert np.all(np.isfinite(out)), name
    check_rag(nso, name, c, out)
    assert p.guards_intact()
    pk, pv = p.download()
    assert np.array_equal(pk, p.k) and np.array_equal(pv, p.v)  # the attention writes no cache byte


@pytest.mark.parametrize("edit", ["junk_behind", "minus_one", "pool_blocks"])
def test_table_entries_that_are_no_block_never_become_an_address(L, pkg, nso, edit):
    """junk_behind: every entry at or behind ceil(kv_len / 16) holds -1 / pool_blocks — the bits of the clean table.  The others: request 0's second
    block (300 live keys) is no block of the pool — every other request holds the clean run's bits, request 0 is finite (those keys read as zeros)."""
    c = step(nso, "a_query_block_boundary_bk16")
    good = run_wide(L, pkg, c, rag_pools(c, 16, PM).upload())[0]

    def change(p):
        if edit != "junk_behind":
            p.table[0, 1] = -1 if edit == "minus_one" else p.pool_blocks
            return
        for b, n in enumerate(c.kvlens):
            first = -(-n // 16)
            p.table[b, first:] = [(-1 if j % 2 else p.pool_blocks) for j in range(p.ts - first)]

    p = rag_pools(c, 16, PM, table_edit=change).upload()
    out = run_wide(L, pkg, c, p)[0]
    same = slice(None) if edit == "junk_behind" else slice(c.start[1], None)
    assert np.all(np.isfinite(out)) and np.array_equal(out[same].view(np.uint32), good[same].view(np.uint32))
    assert np.all(out[:LEAD] == 7.0) and p.guards_intact()


def test_strided_unaligned_dst_with_the_fp16_shadow(L, pkg, nso):
    """dst rows of hs + 3 floats from a pointer one float behind a 16-byte boundary, dst16 with the same strides: the scalar stores give the bits of
    the 16-byte ones, the shadow is the rounded output, the padding of every row and the rows of no request keep their 7.0"""
    c = step(nso, "i_tensor_scales")
    p = rag_pools(c, 16, PM).upload()
    plain, p16, _ = run_wide(L, pkg, c, p, dst16=True)
    out, o16, whole = run_wide(L, pkg, c, p, dst16=True, dst_pad=3)
    assert np.array_equal(out.view(np.uint32), plain.view(np.uint32))
    assert np.all(whole[..., c.hs:] == 7.0) and np.all(o16[..., c.hs:] == 7.0)
    live = slice(c.start[0], c.start[-1])
    assert np.array_equal(o16[live, :, :c.hs], out[live].astype(np.float16)) and np.array_equal(p16[live], plain[live].astype(np.float16))
    for x in (o16, p16):
        assert np.all(x[:LEAD] == 7.0) and np.all(x[c.start[-1]:] == 7.0)
    check_rag(nso, "strided dst", c, out)


def test_refusals_are_counted_and_write_nothing(L, pkg, nso):
    import torch
    c = step(nso, "a_query_block_boundary_bk16")
    p = rag_pools(c, 16, PM).upload()
    dq = torch.from_numpy(c.q.copy()).cuda()
    dd = torch.full((c.rows, c.hn, c.hs), 7.0, device="cuda")
    ds = torch.tensor(c.start, dtype=torch.int32, device="cuda")
    dl = torch.tensor(c.kvlens, dtype=torch.int32, device="cuda")

    def call(table=True, ts=p.ts, bk=16, blocks=p.pool_blocks, step=p.block_step, lens=True, start=True, max_q=130, hs=c.hs, flags=CAUSAL, hn=c.hn, hkv=c.hkv,
             layout=0, k_hs=1, bs=c.bs, scale=c.scale):
        a = block_args(pkg, c, p, dq.data_ptr(), dd.data_ptr(), max_q, c.hs)
        a.head_size, a.attn_flags, a.head_num, a.heads_kv, a.K_layout, a.step_k_head_size, a.batch_size, a.QK_scale = hs, flags, hn, hkv, layout, k_hs, bs, scale
        return L.ns_hip_attn_prefill_paged_wide(C.byref(a), C.c_void_p(ds.data_ptr()) if start else None, C.c_void_p(dl.data_ptr()) if lens else None, 0,
                                                C.c_void_p(p.dt.data_ptr()) if table else None, ts, bk, blocks, step, None, stream_ptr())

    width = "not built at this width"
    calls = [("block table is null", dict(table=False)), ("power of two from 16 to 256", dict(bk=48)), ("pool_blocks must be at least 1", dict(blocks=0)),
             ("must equal table_stride * block_keys", dict(ts=p.ts - 1)), ("do not fit inside block_step", dict(step=p.block_step - 8)),
             ("dKvLens is null", dict(lens=False)), ("dQStart is null", dict(start=False)), ("only ATTN_FWD_LAYOUT_PLAIN tensors are supported", dict(layout=1)),
             ("batch_size (the requests) must be at least 1", dict(bs=0)), ("multiple of 8 from 136 to 256", dict(hs=252)),
             ("multiple of 8 from 136 to 256", dict(hs=264)), ("served by ns_hip_attn_prefill_paged", dict(hs=128)),
             ("served by ns_hip_attn_prefill_paged", dict(hs=64)), ("head_num must be a multiple of heads_kv", dict(hn=5, hkv=2)), ("sl_q is max_q", dict(max_q=0)),
             ("contiguous in the head dimension and 16-byte aligned", dict(k_hs=2)), (width, dict(flags=CAUSAL | ALIBI)), (width, dict(flags=CAUSAL | TANH)),
             (width, dict(scale=0.0)), (width, dict(scale=-0.0625)), (width, dict(scale=float("inf")))]
    s0, others = wide_stats(L), (prefill_stats(L), paged_stats(L), block_stats(L), attn_stats(L))
    for n, (text, kw) in enumerate(calls):
        L.ns_hip_reset_error()
        assert call(**kw) == -1, text
        assert text in pkg.last_error(), (text, pkg.last_error())
        assert delta(s0, wide_stats(L)) == [0, 0, 0, n + 1]
    L.ns_hip_reset_error()
    assert L.ns_hip_attn_prefill_paged_wide(None, None, None, 0, None, 0, 0, 0, 0, None, stream_ptr()) == -1 and "null arguments" in pkg.last_error()
    torch.cuda.synchronize()
    assert bool(torch.all(dd == 7.0)) and (prefill_stats(L), paged_stats(L), block_stats(L), attn_stats(L)) == others
    pk, pv = p.download()
    assert np.array_equal(pk, p.k) and np.array_equal(pv, p.v)
    L.ns_hip_reset_error()


def test_captured_step_replayed_on_new_contents(L, pkg, nso):
    """The entry captured ONCE on a side stream — no tmp, no scratch, no eager call of it in front — then replayed after the CONTENTS of dQStart, dKvLens,
    the table, Q and the pools changed: step 1 is a chunk of 130 rows from position 0 beside a decode row, step 2 a decode row beside a chunk of 70
    over 200 keys, on another permutation of the blocks.  Every replay equals the same step run eagerly, bit for bit; the last one meets the reference."""
    import torch
    hn, hkv, hs, cap, bk, max_q = 4, 2, 256, 256, 16, 130
    steps = [Rag(None, hn, hkv, hs, cap, [130, 1], [130, 77], seed=41), Rag(None, hn, hkv, hs, cap, [1, 70], [131, 200], seed=42)]
    pools = [rag_pools(s, bk, PM, seed=50 + n) for n, s in enumerate(steps)]
    rows = max(s.rows for s in steps)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        p = pools[0].upload()  # the device buffers of the graph; their contents move to step n's below
        q = torch.zeros((rows, hn, hs), device="cuda")
        dst = torch.full((rows, hn, hs), 7.0, device="cuda")
        start = torch.zeros(3, dtype=torch.int32, device="cuda")
        lens = torch.zeros(2, dtype=torch.int32, device="cuda")
        a = block_args(pkg, steps[0], p, q.data_ptr(), dst.data_ptr(), max_q, hs)

        def move_to(n):
            s = steps[n]
            q.zero_()
            q[:s.rows].copy_(torch.from_numpy(s.q.copy()))
            dst.fill_(7.0)
            start.copy_(torch.tensor(s.start, dtype=torch.int32))
            lens.copy_(torch.tensor(s.kvlens, dtype=torch.int32))
            p.dk.copy_(torch.from_numpy(pools[n].k.view(np.int16)))
            p.dv.copy_(torch.from_numpy(pools[n].v.view(np.int16)))
            p.dt.copy_(torch.from_numpy(pools[n].table))

        def call():
            pkg.check(L.ns_hip_attn_prefill_paged_wide(C.byref(a), C.c_void_p(start.data_ptr()), C.c_void_p(lens.data_ptr()), 0, *p.table_args(), None, stream_ptr()))

        move_to(0)
        side.synchronize()
        s0 = wide_stats(L)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            call()
        assert delta(s0, wide_stats(L)) == [1, 0, 0, 0]
        for n, s in enumerate(steps):
            move_to(n)
            g.replay()
            side.synchronize()
            got = dst.cpu().numpy()
            move_to(n)
            call()
            side.synchronize()
            assert np.array_equal(got.view(np.uint32), dst.cpu().numpy().view(np.uint32)), n
            live = got[s.start[0]:s.start[-1]]
            assert np.all(np.isfinite(live)) and not np.any(live == 7.0), n
            assert np.all(got[:LEAD] == 7.0) and np.all(got[s.start[-1]:] == 7.0), n
        for b in range(2):
            qb = s.q[s.start[b]:s.start[b + 1]][None]
            kb, vb = s.k[b:b + 1, :s.kvlens[b]], s.v[b:b + 1, :s.kvlens[b]]
            check(nso, "replayed step 2 request %d" % b, got[s.start[b]:s.start[b + 1]][None], nso.attn_ref(qb, kb, vb, s.scale, CAUSAL),
                  rounding_model(qb, kb, vb, s.scale, CAUSAL))
    torch.cuda.synchronize()

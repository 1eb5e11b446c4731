"""Ragged query blocks over the paged KV cache: ns_hip_attn_block_paged (every request brings its own number of query rows; the PAGED instantiation of
the context-split 64-slot kernel and its merge) and ns_hip_rope_qkv_append_paged_seq (the paged append with a row -> request map).
docs/kernels/attention.md, "Ragged query blocks over a paged cache".

Reference and bounds are the project's: every request on its own against nso.attn_ref through check() / rounding_model() of
tests/test_gpu_attention_paths.py (rel_l2 < 1e-3 over the tensor and, per row, max(2^-11, 4 d)).  No case and no row is left out.

The pools, their NaN fill and their guards are those of tests/test_gpu_attn_paged.py (Pools): every spare block, every block of a request past its
live length and every cell of its last block from the live length on holds 0xFFFF (fp16 NaN).  Q and dst are packed: request b's rows are rows
start[b] .. start[b + 1] - 1; two rows in front of the first request and three behind the last belong to no request, and dst starts as 7.0."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from test_gpu_attention_paths import check, rounding_model
from test_gpu_attn_paged import GUARD, NAN16, Pools, delta, paged_stats
from test_gpu_attn_rows import CAUSAL, HM, PM, stream_ptr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "tools", "attn_block_paged_worker.py")
LEAD, TAIL = 2, 3


def block_stats(L):
    out = (C.c_ulonglong * 4)()
    L.ns_hip_attn_block_paged_stats(out)
    return list(out)


class Rag:
    """inputs of one ragged step, made once: q fp32 [rows][hn][hs] packed, k / v fp16 [bs][cap][hkv][hs], start[bs + 1]; with nso, the reference and
    the rounding model of every request that has a row which sees a key.  Causal with more rows than keys: the first q_len - kv_len rows see
    nothing (zeros), the others are the rows of a request of kv_len rows over kv_len keys."""

    def __init__(self, nso, hn, hkv, hs, cap, qlens, kvlens, flags=CAUSAL, scales=(1.0, 1.0, 1.0, 1.0), seed=0):
        self.bs, self.hn, self.hkv, self.hs, self.cap, self.flags, self.scales = len(qlens), hn, hkv, hs, cap, flags, scales
        self.qlens, self.kvlens = list(qlens), list(kvlens)
        self.start = [LEAD + sum(qlens[:b]) for b in range(self.bs + 1)]
        self.rows = self.start[-1] + TAIL
        rng = np.random.default_rng(hs * 7 + cap + self.bs + seed)
        self.q = rng.standard_normal((self.rows, hn, hs)).astype(np.float32)
        self.k = rng.standard_normal((self.bs, cap, hkv, hs)).astype(np.float16)
        self.v = rng.standard_normal((self.bs, cap, hkv, hs)).astype(np.float16)
        self.scale = float(1.0 / np.sqrt(hs))
        self.ref, self.model = {}, {}
        for b in range(self.bs):
            see = self.seeing(b)
            if nso is None or see == 0:
                continue
            end = self.start[b] + self.qlens[b]
            qb, kb, vb = self.q[end - see:end][None], self.k[b:b + 1, :self.kvlens[b]], self.v[b:b + 1, :self.kvlens[b]]
            self.ref[b] = nso.attn_ref(qb, kb, vb, self.scale, flags, scales=scales)
            self.model[b] = rounding_model(qb, kb, vb, self.scale, flags, scales)
        for x in (self.q, self.k, self.v):
            x.setflags(write=False)

    def seeing(self, b):
        """rows of request b that see a key (its last ones)"""
        if self.kvlens[b] == 0:
            return 0
        return min(self.qlens[b], self.kvlens[b]) if self.flags & CAUSAL else self.qlens[b]


def rag_pools(c, bk, layout, seed=5, table_edit=None):
    p = Pools(c.bs, c.hkv, c.hs, c.cap, bk, layout, seed)
    if table_edit:
        table_edit(p)
    return p.fill(c.k, c.v, c.kvlens)


def block_args(pkg, c, p, q_ptr, dst_ptr, max_q, row):
    a = pkg.attn_args(q_ptr, p.kp, p.vp, dst_ptr, c.bs, c.hn, c.hkv, c.hs, max_q, c.cap, c.scale, c.flags)
    a.Q_sc, a.K_sc, a.V_sc, a.dst_sc = c.scales
    a.step_q_bs = a.step_dst_bs = a.step_k_bs = a.step_v_bs = 12345  # (not used: must not matter)
    a.step_k_sl = a.step_v_sl = p.step_sl
    a.step_k_head_num = a.step_v_head_num = p.step_head
    a.step_dst_head_num, a.step_dst_sl = row, c.hn * row
    return a


def run_block(L, pkg, c, p, bias=0, dst16=False, dst_pad=0, tmp=None, expect=0, max_q=None):
    """ns_hip_attn_block_paged of step c over the uploaded pools p.  Returns (dst [rows][hn][hs], the fp16 shadow or None, the whole dst buffer); dst
    starts as 7.0; dst_pad > 0: rows of hs + dst_pad floats and a dst pointer one float behind a 16-byte boundary."""
    import torch
    dq = torch.from_numpy(c.q.copy()).cuda()
    row = c.hs + dst_pad
    skew = 1 if dst_pad else 0
    buf = torch.full((c.rows * c.hn * row + skew,), 7.0, device="cuda")
    b16 = torch.full((c.rows * c.hn * row,), 7.0, device="cuda", dtype=torch.float16) if dst16 else None
    ds = torch.tensor(c.start, dtype=torch.int32, device="cuda")
    dl = torch.tensor([n - bias for n in c.kvlens], dtype=torch.int32, device="cuda")
    a = block_args(pkg, c, p, dq.data_ptr(), buf.data_ptr() + 4 * skew, max(c.qlens) if max_q is None else max_q, row)
    if tmp is not None:
        a.tmp = tmp.data_ptr()
    rc = L.ns_hip_attn_block_paged(C.byref(a), C.c_void_p(ds.data_ptr()), C.c_void_p(dl.data_ptr()), bias, *p.table_args(),
                                   C.c_void_p(b16.data_ptr()) if dst16 else None, stream_ptr())
    assert rc == expect, pkg.last_error()
    torch.cuda.synchronize()
    whole = buf[skew:].cpu().numpy().reshape(c.rows, c.hn, row)
    return np.ascontiguousarray(whole[..., :c.hs]), (b16.cpu().numpy().reshape(c.rows, c.hn, row) if dst16 else None), whole


def check_rag(nso, tag, c, out, qlens=None):
    """every request on its own; the rows of no request keep their 7.0"""
    qlens = c.qlens if qlens is None else qlens
    assert np.all(out[:LEAD] == 7.0) and np.all(out[c.start[-1]:] == 7.0), tag
    for b in range(c.bs):
        rows = out[c.start[b]:c.start[b] + qlens[b]]
        see = c.seeing(b)
        assert np.all(rows[:qlens[b] - see] == 0.0), (tag, b)  # a row that sees no key is written as zeros
        if see:
            check(nso, "%s request %d (%d rows, %d keys)" % (tag, b, qlens[b], c.kvlens[b]), rows[qlens[b] - see:][None], c.ref[b], c.model[b])


# ---- 1. the shapes that reach each way to go wrong -----------------------------------------------------------------------------------------------
CASES = {  # name: (heads, kv heads, head size, capacity, q lens, kv lens, flags, block_keys, layout)
    "a_decode_row_beside_blocks": (4, 4, 128, 512, [16, 1, 5], [512, 17, 300], CAUSAL, 16, PM),
    "b_idle_request_three_slot_blocks_bk32": (8, 2, 64, 1024, [2, 33, 0, 7], [333, 1024, 0, 64], CAUSAL, 32, PM),
    "b_idle_request_three_slot_blocks_bk64": (8, 2, 64, 1024, [2, 33, 0, 7], [333, 1024, 0, 64], CAUSAL, 64, PM),
    "c_72_slots_last_range_of_one_key": (8, 1, 128, 512, [9], [257], CAUSAL, 256, PM),
    "d_chunk_from_position_0": (2, 2, 64, 512, [100, 64], [100, 64], CAUSAL, 16, PM),
    "e_not_causal_head_major": (4, 2, 128, 1024, [127], [1000], 0, 128, HM),
    "f_many_ranges_short_neighbour": (4, 4, 128, 4096, [33, 3], [2065, 130], CAUSAL, 64, PM),
}
_rags = {}


def rag(nso, name):
    """inputs and references of a case, made once and shared (Rag keeps them read-only)"""
    key = repr(CASES[name][:7])
    if key not in _rags:
        _rags[key] = Rag(nso, *CASES[name][:7])
    return _rags[key]


@pytest.mark.parametrize("name", list(CASES))
def test_ragged_blocks_against_the_reference(L, pkg, nso, name):
    """... and what the call must leave alone: dst rows outside every request keep their 7.0 (check_rag), the guards are unchanged, and the output is
    NaN-free although every cell behind a live length and every spare block is NaN"""
    bk, layout = CASES[name][7:]
    c = rag(nso, name)
    p = rag_pools(c, bk, layout).upload()
    s0 = block_stats(L)
    out = run_block(L, pkg, c, p)[0]
    assert delta(s0, block_stats(L)) == ([1, 0, 1, 0] if c.hs == 64 else [0, 1, 1, 0])
    assert np.all(np.isfinite(out)), name
    check_rag(nso, name, c, out)
    assert p.guards_intact()
    pk, pv = p.download()
    assert np.array_equal(pk, p.k) and np.array_equal(pv, p.v)  # the attention writes no cache byte


def test_the_position_array_drives_the_lengths_through_the_bias(L, pkg, nso):
    """dKvLens holding kv_len - 3 with kv_len_bias = 3 gives the bits of dKvLens holding kv_len"""
    c = rag(nso, "a_decode_row_beside_blocks")
    p = rag_pools(c, 16, PM).upload()
    assert np.array_equal(run_block(L, pkg, c, p, bias=3)[0].view(np.uint32), run_block(L, pkg, c, p)[0].view(np.uint32))


# ---- 2. more rows than keys ------------------------------------------------------------------------------------------------------------------------
def test_rows_that_see_no_key_are_zeros(L, pkg, nso):
    """causal, q lens [10, 5, 3] over kv lens [4, 5, 0]: request 0's first six rows and all of request 2's see no key and are zeros, the others are
    right (check_rag); max_q 10 with 4 / 2 heads: 20 slots"""
    c = Rag(nso, 4, 2, 64, 128, [10, 5, 3], [4, 5, 0], seed=1)
    assert [c.seeing(b) for b in range(3)] == [4, 5, 0]
    p = rag_pools(c, 16, PM).upload()
    out = run_block(L, pkg, c, p)[0]
    assert np.all(np.isfinite(out))
    check_rag(nso, "more rows than keys", c, out)


def test_max_q_clamps_a_requests_rows(L, pkg, nso):
    """max_q = 5 under q lens [16, 1, 5]: request 0 is served as its first five rows (which then see kv_len - 5 + i + 1 keys), its other rows keep
    their 7.0; the other requests are what they are under max_q = 16"""
    c = rag(nso, "a_decode_row_beside_blocks")
    p = rag_pools(c, 16, PM).upload()
    full = run_block(L, pkg, c, p)[0]
    out = run_block(L, pkg, c, p, max_q=5)[0]
    assert np.all(out[c.start[0] + 5:c.start[1]] == 7.0)
    assert np.array_equal(out[c.start[1]:].view(np.uint32), full[c.start[1]:].view(np.uint32))
    qb = c.q[c.start[0]:c.start[0] + 5][None]
    kb, vb = c.k[0:1, :c.kvlens[0]], c.v[0:1, :c.kvlens[0]]
    check(nso, "max_q 5", out[c.start[0]:c.start[0] + 5][None], nso.attn_ref(qb, kb, vb, c.scale, CAUSAL), rounding_model(qb, kb, vb, c.scale, CAUSAL))


# ---- 3. table entries ------------------------------------------------------------------------------------------------------------------------------
def test_table_entries_behind_the_live_blocks_may_hold_anything(L, pkg, nso):
    c = rag(nso, "a_decode_row_beside_blocks")
    good = run_block(L, pkg, c, rag_pools(c, 16, PM).upload())[0]

    def junk(p):
        for b, n in enumerate(c.kvlens):
            first = -(-n // 16)
            p.table[b, first:] = [(-1 if j % 2 else p.pool_blocks) for j in range(p.ts - first)]

    p = rag_pools(c, 16, PM, table_edit=junk).upload()
    assert p.table[1, 2] in (-1, p.pool_blocks) and 0 <= p.table[1, 1] < p.pool_blocks
    out = run_block(L, pkg, c, p)[0]
    assert np.array_equal(out.view(np.uint32), good.view(np.uint32))
    assert p.guards_intact()


@pytest.mark.parametrize("bad", ["minus_one", "pool_blocks"])
def test_a_bad_entry_inside_a_live_length_leaves_the_other_requests_alone(L, pkg, nso, bad):
    """request 2's second block (300 live keys, blocks of 16) gets an id that is no block of the pool: every other request's rows hold the bits of the
    run with the valid table and nothing is NaN there; the guards are unchanged"""
    c = rag(nso, "a_decode_row_beside_blocks")
    good = run_block(L, pkg, c, rag_pools(c, 16, PM).upload())[0]

    def poison(p):
        p.table[2, 1] = -1 if bad == "minus_one" else p.pool_blocks

    p = rag_pools(c, 16, PM, table_edit=poison).upload()
    out = run_block(L, pkg, c, p)[0]
    others = slice(0, c.start[2])
    assert np.all(np.isfinite(out[others]))
    assert np.array_equal(out[others].view(np.uint32), good[others].view(np.uint32))
    assert np.all(out[c.start[3]:] == 7.0) and p.guards_intact()


# ---- 4. strides and workspace ----------------------------------------------------------------------------------------------------------------------
def test_strided_unaligned_dst_with_the_fp16_shadow_and_the_callers_workspace(L, pkg, nso):
    """dst rows of hs + 3 floats from a pointer one float behind a 16-byte boundary, dst16 with the same element strides; tmp of exactly the size
    function's bytes, with 256 bytes behind it that must stay as they were — and the tmp is what the partials went to."""
    import torch
    c = rag(nso, "f_many_ranges_short_neighbour")
    p = rag_pools(c, 64, PM).upload()
    plain = run_block(L, pkg, c, p)[0]
    size = L.ns_hip_attn_block_paged_workspace_size(c.bs, c.hn, c.hkv, c.hs, max(c.qlens), c.cap)
    assert size > 0 and size % 4 == 0
    tmp = torch.full((size + 256,), 0x5A, dtype=torch.uint8, device="cuda")
    out, o16, whole = run_block(L, pkg, c, p, dst16=True, dst_pad=3, tmp=tmp)
    assert np.array_equal(out.view(np.uint32), plain.view(np.uint32))
    assert np.all(whole[..., c.hs:] == 7.0) and np.all(o16[..., c.hs:] == 7.0)  # the padding of every row
    live = slice(c.start[0], c.start[-1])
    assert np.array_equal(o16[live, :, :c.hs], out[live].astype(np.float16))
    assert np.all(o16[:LEAD] == 7.0) and np.all(o16[c.start[-1]:] == 7.0)
    check_rag(nso, "strided dst", c, out)
    t = tmp.cpu().numpy()
    assert np.all(t[size:] == 0x5A) and not np.all(t[:size] == 0x5A)


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_are_counted_and_write_nothing(L, pkg, nso):
    import torch
    c = rag(nso, "a_decode_row_beside_blocks")
    p = rag_pools(c, 16, PM).upload()
    dq = torch.from_numpy(c.q.copy()).cuda()
    dd = torch.full((c.rows, c.hn, c.hs), 7.0, device="cuda")
    ds = torch.tensor(c.start, dtype=torch.int32, device="cuda")
    dl = torch.tensor(c.kvlens, dtype=torch.int32, device="cuda")

    def call(table=True, ts=p.ts, bk=16, blocks=p.pool_blocks, step=p.block_step, lens=True, start=True, max_q=16, hs=c.hs, flags=CAUSAL, hn=c.hn, hkv=c.hkv):
        a = block_args(pkg, c, p, dq.data_ptr(), dd.data_ptr(), max_q, c.hs)
        a.head_size, a.attn_flags, a.head_num, a.heads_kv = hs, flags, hn, hkv
        return L.ns_hip_attn_block_paged(C.byref(a), C.c_void_p(ds.data_ptr()) if start else None, C.c_void_p(dl.data_ptr()) if lens else None, 0,
                                         C.c_void_p(p.dt.data_ptr()) if table else None, ts, bk, blocks, step, None, stream_ptr())

    calls = [("block table is null", dict(table=False)), ("power of two from 16 to 256", dict(bk=48)), ("power of two from 16 to 256", dict(bk=8)),
             ("pool_blocks must be at least 1", dict(blocks=0)), ("must equal table_stride * block_keys", dict(ts=p.ts - 1)),
             ("do not fit inside block_step", dict(step=p.block_step - 8)), ("dKvLens is null", dict(lens=False)), ("dQStart is null", dict(start=False)),
             ("head_size must be 64 or 128", dict(hs=80)), ("ALiBi and the tanh cap are not served", dict(flags=CAUSAL | 2)),
             ("ALiBi and the tanh cap are not served", dict(flags=CAUSAL | 8)), ("sl_q is max_q", dict(max_q=0)),
             ("above the grid limit of 65535", dict(hn=4096, hkv=1, max_q=1024))]
    s0, g0 = block_stats(L), paged_stats(L)
    for n, (text, kw) in enumerate(calls):
        L.ns_hip_reset_error()
        assert call(**kw) == -1, text
        assert text in pkg.last_error(), (text, pkg.last_error())
        assert delta(s0, block_stats(L)) == [0, 0, 0, n + 1]
    torch.cuda.synchronize()
    assert bool(torch.all(dd == 7.0)) and paged_stats(L) == g0
    pk, pv = p.download()
    assert np.array_equal(pk, p.k) and np.array_equal(pv, p.v)
    assert L.ns_hip_attn_block_paged_workspace_size(c.bs, c.hn, c.hkv, 80, 16, c.cap) == 0
    L.ns_hip_reset_error()


# ---- 6. against the form the library had: every query row a request of the paged decode entry ------------------------------------------------------
def test_rows_as_requests_of_the_decode_entry(L, pkg, nso):
    """Every query row of case (a) as one request of ns_hip_attn_decode_paged, with its request's table row duplicated and its own length
    kv_len - q_len + i + 1.  Two kernels with different operand rounding: both outputs pass check() against the oracle; the rel_l2 between the two
    is printed (docs/kernels/attention.md records it) and has no bound of its own."""
    import torch
    c = rag(nso, "a_decode_row_beside_blocks")
    p = rag_pools(c, 16, PM).upload()
    out = run_block(L, pkg, c, p)[0]
    check_rag(nso, "block entry", c, out)
    req = [b for b in range(c.bs) for _ in range(c.qlens[b])]
    lens = [c.kvlens[b] - c.qlens[b] + i + 1 for b in range(c.bs) for i in range(c.qlens[b])]
    n = len(req)
    table = torch.from_numpy(p.table[req].copy()).cuda()
    dq = torch.from_numpy(c.q[LEAD:LEAD + n].copy()).cuda()
    dd = torch.full((n, 1, c.hn, c.hs), 7.0, device="cuda")
    dl = torch.tensor(lens, dtype=torch.int32, device="cuda")
    a = pkg.attn_args(dq.data_ptr(), p.kp, p.vp, dd.data_ptr(), n, c.hn, c.hkv, c.hs, 1, c.cap, c.scale, c.flags)
    a.step_k_sl = a.step_v_sl = p.step_sl
    a.step_k_head_num = a.step_v_head_num = p.step_head
    pkg.check(L.ns_hip_attn_decode_paged(C.byref(a), C.c_void_p(dl.data_ptr()), 0, C.c_void_p(table.data_ptr()), p.ts, p.bk, p.pool_blocks, p.block_step, None,
                                         stream_ptr()))
    torch.cuda.synchronize()
    rows = np.full_like(out, 7.0)
    rows[LEAD:LEAD + n] = dd.cpu().numpy()[:, 0]
    check_rag(nso, "rows as requests", c, rows)
    print("ATTN_BLOCK_PAGED rows-as-requests against the block entry: rel_l2 %.3g" % nso.rel_l2(out[LEAD:LEAD + n], rows[LEAD:LEAD + n]))


# ---- 7. the append with a row -> request map ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [PM, HM])
@pytest.mark.parametrize("mode,n_dims", [(0, 64), (2, 32)])
def test_append_seq_is_bit_equal_to_the_paged_append_on_the_expanded_table(L, pkg, mode, n_dims, layout):
    """9 rows of 3 requests (a chunk of four, one decode row, a chunk of two; one row idle by position, one by a request id of 3 and one by -1), 4 / 2
    heads of size 64, blocks of 16, capacity 256.  ns_hip_rope_qkv_append_paged takes the table with one row per query row (row r: a copy of request
    row_req[r]'s; the two idle-by-id rows: position -1).  Q and both pools hold the same bits, guards included; the idle rows' Q is untouched."""
    import torch
    heads, hkv, hs, cap, bk, requests = 4, 2, 64, 256, 16, 3
    row_req = [0, 0, 0, 0, 1, 2, 2, 3, -1]
    pos = [14, 15, 16, 17, 200, 255, 256, 5, 6]  # (256: at the capacity, idle)
    rows = len(pos)
    rng = np.random.default_rng(mode * 100 + n_dims)
    q = rng.standard_normal((rows, heads, hs)).astype(np.float32)
    k = rng.standard_normal((rows, hkv, hs)).astype(np.float32)
    v = rng.standard_normal((rows, hkv, hs)).astype(np.float32)
    dk, dv = torch.from_numpy(k).cuda(), torch.from_numpy(v).cuda()
    st = stream_ptr()
    res = []
    for form in ("seq", "expanded"):
        p = Pools(requests, hkv, hs, cap, bk, layout, seed=9, fill=0x5A5B).upload()
        dq = torch.from_numpy(q).cuda()
        if form == "seq":
            dpos = torch.tensor(pos, dtype=torch.int32, device="cuda")
            dreq = torch.tensor(row_req, dtype=torch.int32, device="cuda")
            pkg.check(L.ns_hip_rope_qkv_append_paged_seq(dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), p.kp, p.vp, rows, heads, hkv, hs, dpos.data_ptr(), 4096, n_dims,
                                                         mode, 10000.0, 0.75, 0.0, 1.1, dreq.data_ptr(), requests, *p.table_args(), p.step_sl, p.step_head, st))
        else:
            ok = [0 <= r < requests for r in row_req]
            table = torch.from_numpy(np.stack([p.table[r if o else 0] for r, o in zip(row_req, ok)])).cuda()
            dpos = torch.tensor([n if o else -1 for n, o in zip(pos, ok)], dtype=torch.int32, device="cuda")
            pkg.check(L.ns_hip_rope_qkv_append_paged(dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), p.kp, p.vp, rows, heads, hkv, hs, dpos.data_ptr(), 4096, n_dims,
                                                     mode, 10000.0, 0.75, 0.0, 1.1, C.c_void_p(table.data_ptr()), p.ts, bk, p.pool_blocks, p.block_step, p.step_sl,
                                                     p.step_head, st))
        torch.cuda.synchronize()
        res.append((dq.cpu().numpy(), p.download(), p))
    (q_seq, (k_seq, v_seq), p), (q_exp, (k_exp, v_exp), _) = res
    assert np.array_equal(q_seq.view(np.uint32), q_exp.view(np.uint32))
    assert np.array_equal(k_seq, k_exp) and np.array_equal(v_seq, v_exp)
    for r in (6, 7, 8):
        assert np.array_equal(q_seq[r], q[r])
    for r in range(6):
        assert not np.array_equal(q_seq[r], q[r])
        assert np.all(p.cells(k_seq, p.table[row_req[r], pos[r] // bk], pos[r] % bk, 1) != 0x5A5B)
    assert int((k_seq != p.k).reshape(k_seq.shape[0], -1).any(axis=1).sum()) == 4  # blocks 0 and 1 of request 0, one of request 1, one of request 2
    assert p.guards_intact()


# ---- 8. a prompt in chunks, end to end ---------------------------------------------------------------------------------------------------------------
def test_chunked_prefill_on_pages(L, pkg, nso):
    """A 150-token prompt goes in as chunks of 64 / 64 / 22 through append + attention on pages (4 / 2 heads of size 128, blocks of 16, capacity 256),
    beside a second request that stays idle.  Every chunk's rows lie within the check() bounds of the whole-prompt reference: the causal attention of
    the rotated Q rows over the keys as the pool holds them after the last chunk."""
    import torch
    hn, hkv, hs, cap, bk, n_tok = 4, 2, 128, 256, 16, 150
    rng = np.random.default_rng(150)
    q = rng.standard_normal((n_tok, hn, hs)).astype(np.float32)
    k = rng.standard_normal((n_tok, hkv, hs)).astype(np.float32)
    v = rng.standard_normal((n_tok, hkv, hs)).astype(np.float32)
    p = Pools(2, hkv, hs, cap, bk, PM, seed=21).upload()
    dq, dk, dv = torch.from_numpy(q).cuda(), torch.from_numpy(k).cuda(), torch.from_numpy(v).cuda()
    dst = torch.full((n_tok, hn, hs), 7.0, device="cuda")
    scale = float(1.0 / np.sqrt(hs))
    c = Rag.__new__(Rag)
    c.bs, c.hn, c.hkv, c.hs, c.cap, c.scale, c.flags, c.scales = 2, hn, hkv, hs, cap, scale, CAUSAL, (1.0, 1.0, 1.0, 1.0)
    st, done = stream_ptr(), 0
    for chunk in (64, 64, 22):
        dpos = torch.arange(done, done + chunk, dtype=torch.int32, device="cuda")
        dreq = torch.zeros(chunk, dtype=torch.int32, device="cuda")
        qc = dq[done:done + chunk]
        pkg.check(L.ns_hip_rope_qkv_append_paged_seq(qc.data_ptr(), dk[done:].data_ptr(), dv[done:].data_ptr(), p.kp, p.vp, chunk, hn, hkv, hs, dpos.data_ptr(), cap,
                                                     hs, 0, 10000.0, 1.0, 0.0, 1.0, dreq.data_ptr(), 2, *p.table_args(), p.step_sl, p.step_head, st))
        ds = torch.tensor([0, chunk, chunk], dtype=torch.int32, device="cuda")
        dl = torch.tensor([done + chunk, 0], dtype=torch.int32, device="cuda")
        a = block_args(pkg, c, p, qc.data_ptr(), dst[done:].data_ptr(), 64, hs)
        pkg.check(L.ns_hip_attn_block_paged(C.byref(a), C.c_void_p(ds.data_ptr()), C.c_void_p(dl.data_ptr()), 0, *p.table_args(), None, st))
        done += chunk
    torch.cuda.synchronize()
    pk, pv = p.download()
    kb = np.concatenate([p.cells(pk, p.table[0, j], 0, bk) for j in range(-(-n_tok // bk))])[:n_tok].view(np.float16)[None]
    vb = np.concatenate([p.cells(pv, p.table[0, j], 0, bk) for j in range(-(-n_tok // bk))])[:n_tok].view(np.float16)[None]
    assert np.all(np.isfinite(kb.astype(np.float32))) and np.all(np.isfinite(vb.astype(np.float32)))
    assert np.array_equal(vb[0], v.astype(np.float16))
    qr = dq.cpu().numpy()[None]
    ref, model = nso.attn_ref(qr, kb, vb, scale, CAUSAL), rounding_model(qr, kb, vb, scale, CAUSAL)
    out = dst.cpu().numpy()[None]
    for lo, hi in ((0, 64), (64, 128), (128, 150)):
        check(nso, "chunk rows %d..%d of the prompt" % (lo, hi - 1), out[:, lo:hi], ref[:, lo:hi], model[:, lo:hi])
    assert p.guards_intact()


# ---- 9. one captured step, replayed on other contents ---------------------------------------------------------------------------------------------
def test_captured_step_replayed_on_new_contents(L, pkg, nso):
    """{append; attention} captured ONCE on a side stream with `tmp` given (after one eager call), then replayed after the CONTENTS of dPos, dRowReq,
    dQStart, dKvLens and the table changed: step 1 is a chunk of five rows for request 0 (positions 32 .. 36) beside a decode row of request 1
    (position 13); step 2 is a decode row of request 0 (37) beside a chunk of eight of request 1 (14 .. 21), which enters block 1 — its table entry
    holds -1 until then.  Every replay equals the same step run eagerly on a twin, bit for bit (dst, Q, both pools)."""
    import torch
    bs, hn, hkv, hs, cap, bk, max_q, rows = 2, 4, 2, 128, 256, 16, 8, 9
    first = [32, 13]
    steps = [dict(pos=[32, 33, 34, 35, 36, 13, -1, -1, -1], req=[0, 0, 0, 0, 0, 1, -1, -1, -1], start=[0, 5, 6], lens=[37, 14]),
             dict(pos=[37, 14, 15, 16, 17, 18, 19, 20, 21], req=[0, 1, 1, 1, 1, 1, 1, 1, 1], start=[0, 1, 9], lens=[38, 22])]
    rng = np.random.default_rng(91)
    k0 = rng.standard_normal((bs, cap, hkv, hs)).astype(np.float16)
    v0 = rng.standard_normal((bs, cap, hkv, hs)).astype(np.float16)
    scale = float(1.0 / np.sqrt(hs))
    ws_bytes = L.ns_hip_attn_block_paged_workspace_size(bs, hn, hkv, hs, max_q, cap)
    side = torch.cuda.Stream()
    c = Rag.__new__(Rag)
    c.bs, c.hn, c.hkv, c.hs, c.cap, c.scale, c.flags, c.scales = bs, hn, hkv, hs, cap, scale, CAUSAL, (1.0, 1.0, 1.0, 1.0)
    with torch.cuda.stream(side):
        qin = torch.zeros((rows, hn, hs), device="cuda")
        kin, vin = torch.zeros((rows, hkv, hs), device="cuda"), torch.zeros((rows, hkv, hs), device="cuda")

        class State:
            def __init__(self):
                self.p = Pools(bs, hkv, hs, cap, bk, PM, seed=11).fill(k0, v0, first)
                self.full_table = self.p.table.copy()
                for b, n in enumerate(first):  # blocks the request has not entered yet: no id
                    self.p.table[b, n // bk + 1:] = -1
                self.p.upload()
                self.pos = torch.zeros(rows, dtype=torch.int32, device="cuda")
                self.req = torch.zeros(rows, dtype=torch.int32, device="cuda")
                self.start = torch.zeros(bs + 1, dtype=torch.int32, device="cuda")
                self.lens = torch.zeros(bs, dtype=torch.int32, device="cuda")
                self.q = torch.zeros_like(qin)
                self.dst = torch.full((rows, hn, hs), 7.0, device="cuda")
                self.ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
                self.a = block_args(pkg, c, self.p, self.q.data_ptr(), self.dst.data_ptr(), max_q, hs)
                self.a.tmp = self.ws.data_ptr()

            def move_to(self, s):
                """what the serving loop does between steps: the four arrays, and the id of a block a request enters"""
                self.pos.copy_(torch.tensor(s["pos"], dtype=torch.int32))
                self.req.copy_(torch.tensor(s["req"], dtype=torch.int32))
                self.start.copy_(torch.tensor(s["start"], dtype=torch.int32))
                self.lens.copy_(torch.tensor(s["lens"], dtype=torch.int32))
                for b, n in enumerate(s["lens"]):
                    self.p.dt[b, (n - 1) // bk] = int(self.full_table[b, (n - 1) // bk])

            def step(self):
                st = stream_ptr()
                self.q.copy_(qin)
                pkg.check(L.ns_hip_rope_qkv_append_paged_seq(self.q.data_ptr(), kin.data_ptr(), vin.data_ptr(), self.p.kp, self.p.vp, rows, hn, hkv, hs,
                                                             self.pos.data_ptr(), cap, hs, 0, 10000.0, 1.0, 0.0, 1.0, self.req.data_ptr(), bs,
                                                             *self.p.table_args(), self.p.step_sl, self.p.step_head, st))
                pkg.check(L.ns_hip_attn_block_paged(C.byref(self.a), C.c_void_p(self.start.data_ptr()), C.c_void_p(self.lens.data_ptr()), 0,
                                                    *self.p.table_args(), None, st))

        warm = State()
        warm.move_to(steps[0])
        warm.step()  # (one eager call in front of the capture: the kernels' code objects are in place)
        graphed, eager = State(), State()
        graphed.move_to(steps[0])
        side.synchronize()
        s0 = block_stats(L)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            graphed.step()
        assert delta(s0, block_stats(L)) == [0, 1, 1, 0]  # (captured: the head-size-128 kernel and its merge; nothing has run)
        for n, s in enumerate(steps):
            step_rng = np.random.default_rng(2000 + n)
            for t in (qin, kin, vin):
                t.copy_(torch.from_numpy(step_rng.standard_normal(tuple(t.shape)).astype(np.float32)))
            graphed.move_to(s)
            eager.move_to(s)
            g.replay()
            eager.step()
            side.synchronize()
            assert torch.equal(graphed.dst, eager.dst) and torch.equal(graphed.q, eager.q), n
            assert torch.equal(graphed.p.dk, eager.p.dk) and torch.equal(graphed.p.dv, eager.p.dv), n
            live = graphed.dst[:s["start"][-1]]
            assert bool(torch.all(torch.isfinite(live))) and not bool(torch.any(live == 7.0)), n
        assert graphed.p.guards_intact()
        # the last step against the reference, over the keys as the pool now holds them
        out, q = graphed.dst.cpu().numpy(), graphed.q.cpu().numpy()
        pk, pv = graphed.p.download()
        s = steps[-1]
        for b, n in enumerate(s["lens"]):
            kb = np.concatenate([graphed.p.cells(pk, graphed.full_table[b, j], 0, bk) for j in range(-(-n // bk))])[:n].view(np.float16)[None]
            vb = np.concatenate([graphed.p.cells(pv, graphed.full_table[b, j], 0, bk) for j in range(-(-n // bk))])[:n].view(np.float16)[None]
            assert np.all(np.isfinite(kb.astype(np.float32)))
            qb = q[s["start"][b]:s["start"][b + 1]][None]
            check(nso, "replayed step 2 request %d (%d rows, %d keys)" % (b, qb.shape[1], n), out[s["start"][b]:s["start"][b + 1]][None],
                  nso.attn_ref(qb, kb, vb, scale, CAUSAL), rounding_model(qb, kb, vb, scale, CAUSAL))
    torch.cuda.synchronize()


# ---- 10. the ranges as laid out --------------------------------------------------------------------------------------------------------------------
def test_ranges_as_laid_out_stay_within_the_bounds(L, pkg, nso):
    """NS_ATTN_DYN_RANGES=0 is read once per process: a child runs case (f) — a request of 130 keys under a layout of many ranges for 4096 — with the
    ranges as laid out; its output passes the same check"""
    name = "f_many_ranges_short_neighbour"
    c = rag(nso, name)
    env = dict(os.environ)
    env["NS_ATTN_DYN_RANGES"] = "0"
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "out.npz")
        r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, WORKER, name, path], env=env, capture_output=True, text=True, cwd=ROOT)
        assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
        out = np.load(path)["out"]
    assert np.all(np.isfinite(out))
    check_rag(nso, "ranges as laid out", c, out)

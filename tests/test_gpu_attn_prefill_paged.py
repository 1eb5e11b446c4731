"""Prompt-sized query blocks over the paged KV cache: ns_hip_attn_prefill_paged (the PAGED instantiations of the 128-row matrix-core kernel: one launch,
no partials, every staged K / V row fetched through its own table entry).  docs/kernels/attention.md, "Prompt-sized query blocks over a paged cache".

Pools, their NaN fill and guards, the packed Q / dst with two lead and three tail rows, dst preset to 7.0 and the per-request check are those of
tests/test_gpu_attn_block_paged.py (Pools, Rag, block_args, check_rag, by import).  Reference and bounds are the project's: every request on its own
against nso.attn_ref through check() of tests/test_gpu_attention_paths.py — rel_l2 < 1e-3 over the tensor and, per row, max(2^-11, 4 d), d being the
row's distance between the fp64 rounding model and the reference.  No case and no row is left out.

rounding_model() of that file takes flags 0 / 1 only; model64_rows() below is the same fp64 attention with the same two operand roundings (Q to fp16,
every unnormalised weight to fp16 in front of P.V) plus the tanh cap, `+ key position x slope` and the head partition.  The reference of a tanh-capped
case is that model without the roundings, as tests/test_gpu_attn_rows.py does (the oracle has no tanh cap); ALiBi under a head partition is the oracle
on the full model's heads, of which the call's heads are a slice.

Largest row error / bound seen on an MI355X: see docs/kernels/attention.md."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_attention_paths import check, rounding_model
from test_gpu_attn_block_paged import LEAD, Rag, block_args, block_stats, check_rag, rag_pools
from test_gpu_attn_paged import delta, paged_stats
from test_gpu_attn_rows import ALIBI, CAUSAL, HM, PM, TANH, attn_stats, stream_ptr

pytestmark = pytest.mark.gpu
AP_ROWS128 = 5  # slot of ns_hip_attn_stats: attn_mfma2_kernel (AttnPath, ns_attn.h)
ONES = (1.0, 1.0, 1.0, 1.0)


def prefill_stats(L):
    out = (C.c_ulonglong * 6)()
    L.ns_hip_attn_prefill_paged_stats(out)
    return list(out)


def model64_rows(q, k, v, qk_scale, flags, scales=ONES, rounded=True, all_heads=None, head_off=0):
    """fp64 attention of ONE request, q fp32 [1][sl_q][hn][hs], k / v fp16 [1][sl_kv][hkv][hs]: scores (q . k) * scale, the tanh cap, + key position x
    the slope of head head_off + h among all_heads, the causal mask, softmax.  rounded: Q to fp16 and each unnormalised weight exp(s - rowmax) to fp16
    in front of P.V (the row sum keeps the unrounded weights) — rounding_model()'s roundings."""
    _, sl_q, hn, hs = q.shape
    sl_kv, hkv = k.shape[1], k.shape[2]
    q_sc, k_sc, v_sc, dst_sc = scales
    sc = float(np.float32(qk_scale)) * q_sc * k_sc
    heads = all_heads or hn
    lf = 1 << int(np.floor(np.log2(heads)))
    m0, m1 = 2.0 ** (-8.0 / lf), 2.0 ** (-4.0 / lf)
    qq = q.astype(np.float16).astype(np.float64) if rounded else q.astype(np.float64)
    out = np.zeros(q.shape, np.float64)
    hidden = np.arange(sl_kv)[None, :] > (np.arange(sl_q)[:, None] + (sl_kv - sl_q)) if flags & CAUSAL else None
    for h in range(hn):
        kk, vv = k[0, :, h // (hn // hkv)].astype(np.float64), v[0, :, h // (hn // hkv)].astype(np.float64)
        s = (qq[0, :, h] @ kk.T) * sc
        if flags & TANH:
            s = 30.0 * np.tanh(s / 30.0)
        if flags & ALIBI:
            gh = h + head_off
            s = s + np.arange(sl_kv)[None, :] * (m0 ** (gh + 1) if gh < lf else m1 ** (2 * (gh - lf) + 1))
        if hidden is not None:
            s[hidden] = -np.inf
        p = np.exp(s - s.max(axis=1, keepdims=True))
        pv = p.astype(np.float16).astype(np.float64) if rounded else p
        out[0, :, h] = (pv @ vv) / p.sum(axis=1, keepdims=True) * (v_sc / dst_sc)
    return out


class Step(Rag):
    """Rag with any flags, score scale and head partition: the inputs are Rag's (same generator), references and models are made here, once."""

    def __init__(self, nso, hn, hkv, hs, cap, qlens, kvlens, flags=CAUSAL, scales=ONES, seed=0, scale=None, partition=None):
        Rag.__init__(self, None, hn, hkv, hs, cap, qlens, kvlens, flags, scales, seed)
        if scale is not None:
            self.scale = float(scale)
        self.partition = partition  # (heads of the full model, this call's first head) or None
        all_heads, off = partition if partition else (hn, 0)
        for b in range(self.bs):
            see = self.seeing(b)
            if see == 0:
                continue
            end = self.start[b] + self.qlens[b]
            qb, kb, vb = self.q[end - see:end][None], self.k[b:b + 1, :self.kvlens[b]], self.v[b:b + 1, :self.kvlens[b]]
            if not flags & (ALIBI | TANH):
                self.ref[b] = nso.attn_ref(qb, kb, vb, self.scale, flags, scales=scales)
                self.model[b] = rounding_model(qb, kb, vb, self.scale, flags, scales)
                continue
            self.model[b] = model64_rows(qb, kb, vb, self.scale, flags, scales, True, all_heads, off)
            if flags & TANH:
                self.ref[b] = model64_rows(qb, kb, vb, self.scale, flags, scales, False, all_heads, off)
            elif partition:  # the oracle on the full model's heads: this call's are heads off .. off + hn - 1, on kv heads off / g ..
                g, reps = hn // hkv, all_heads // hn
                assert all_heads == reps * hn and off % hn == 0
                full = nso.attn_ref(np.concatenate([qb] * reps, axis=2), np.concatenate([kb] * reps, axis=2), np.concatenate([vb] * reps, axis=2),
                                    self.scale, flags, scales=scales)
                self.ref[b] = full[:, :, off:off + hn]
                assert g * hkv == hn
            else:
                self.ref[b] = nso.attn_ref(qb, kb, vb, self.scale, flags, scales=scales)


def run_prefill(L, pkg, c, p, bias=0, dst16=False, dst_pad=0, expect=0, max_q=None):
    """ns_hip_attn_prefill_paged of step c over the uploaded pools p, as run_block runs the block entry: returns (dst [rows][hn][hs], the fp16 shadow or
    None, the whole dst buffer); dst starts as 7.0; dst_pad > 0: rows of hs + dst_pad floats and a dst pointer one float behind a 16-byte boundary."""
    import torch
    dq = torch.from_numpy(c.q.copy()).cuda()
    row = c.hs + dst_pad
    skew = 1 if dst_pad else 0
    buf = torch.full((c.rows * c.hn * row + skew,), 7.0, device="cuda")
    b16 = torch.full((c.rows * c.hn * row,), 7.0, device="cuda", dtype=torch.float16) if dst16 else None
    ds = torch.tensor(c.start, dtype=torch.int32, device="cuda")
    dl = torch.tensor([n - bias for n in c.kvlens], dtype=torch.int32, device="cuda")
    a = block_args(pkg, c, p, dq.data_ptr(), buf.data_ptr() + 4 * skew, max(c.qlens) if max_q is None else max_q, row)
    part = getattr(c, "partition", None)
    if part:
        assert L.ns_hip_attn_set_head_partition(*part) == 0
    try:
        rc = L.ns_hip_attn_prefill_paged(C.byref(a), C.c_void_p(ds.data_ptr()), C.c_void_p(dl.data_ptr()), bias, *p.table_args(),
                                         C.c_void_p(b16.data_ptr()) if dst16 else None, stream_ptr())
    finally:
        if part:
            assert L.ns_hip_attn_set_head_partition(0, 0) == 0
    assert rc == expect, pkg.last_error()
    torch.cuda.synchronize()
    whole = buf[skew:].cpu().numpy().reshape(c.rows, c.hn, row)
    return np.ascontiguousarray(whole[..., :c.hs]), (b16.cpu().numpy().reshape(c.rows, c.hn, row) if dst16 else None), whole


# ---- 1. the shapes that reach each way to go wrong ---------------------------------------------------------------------------------------------------
# name: ((heads, kv heads, head size, capacity, q lens, kv lens, flags), Step's keywords, block_keys, layout, stats delta [64, 128, 256, biased, padded, refused])
BOUNDARY = (4, 2, 64, 512, [130, 1, 0, 17], [300, 17, 0, 64], CAUSAL)  # two query blocks with a last wave of two rows, a decode row, an idle request, a chunk that ends on a tile
CASES = {
    "a_query_block_boundary_bk16": (BOUNDARY, {}, 16, PM, [1, 0, 0, 0, 0, 0]),
    "a_query_block_boundary_bk256": (BOUNDARY, {}, 256, PM, [1, 0, 0, 0, 0, 0]),
    "b_chunk_from_position_0": ((2, 2, 128, 256, [129], [129], CAUSAL), {}, 16, PM, [0, 1, 0, 0, 0, 0]),
    "c_more_rows_than_keys": ((4, 2, 64, 256, [10, 5, 3, 140], [4, 5, 0, 130], CAUSAL), dict(seed=1), 16, PM, [1, 0, 0, 0, 0, 0]),
    "d_not_causal_head_major": ((4, 2, 128, 1024, [150, 3], [1000, 65], 0), {}, 128, HM, [0, 1, 0, 0, 0, 0]),
    "e_head_size_40": ((4, 2, 40, 256, [33, 130], [100, 200], CAUSAL), {}, 16, PM, [1, 0, 0, 0, 1, 0]),
    "e_head_size_80": ((4, 2, 80, 256, [33, 130], [100, 200], CAUSAL), {}, 32, HM, [0, 1, 0, 0, 1, 0]),
    "f_alibi_head_partition": ((8, 2, 64, 256, [130, 3], [200, 70], CAUSAL | ALIBI), dict(partition=(16, 8)), 16, PM, [1, 0, 0, 1, 0, 0]),
    "f_alibi_head_size_96": ((8, 2, 96, 256, [40], [129], CAUSAL | ALIBI), {}, 64, PM, [0, 1, 0, 1, 1, 0]),
    "g_tanh_cap": ((4, 4, 128, 256, [131, 2], [256, 2], CAUSAL | TANH), dict(scale=3.0 / np.sqrt(128.0)), 16, PM, [0, 1, 0, 1, 0, 0]),  # (scores large enough for the cap to matter)
    "h_negative_score_scale": ((4, 2, 64, 256, [70, 1], [130, 64], CAUSAL), dict(scale=-0.125), 16, PM, [1, 0, 0, 1, 0, 0]),
    "h_zero_score_scale": ((4, 2, 128, 256, [70, 1], [130, 64], CAUSAL), dict(scale=0.0), 16, PM, [0, 1, 0, 1, 0, 0]),
    "i_tensor_scales": ((4, 2, 128, 256, [129, 16], [200, 16], CAUSAL), dict(scales=(0.5, 2.0, 0.25, 4.0), seed=3), 16, PM, [0, 1, 0, 0, 0, 0]),
}
_steps = {}


def step(nso, name):
    """inputs and references of a case, made once and shared (Rag keeps them read-only)"""
    key = repr((CASES[name][0], sorted(CASES[name][1].items())))
    if key not in _steps:
        _steps[key] = Step(nso, *CASES[name][0], **CASES[name][1])
    return _steps[key]


@pytest.mark.parametrize("name", list(CASES))
def test_prompt_blocks_against_the_reference(L, pkg, nso, name):
    """... with the instantiation asserted through the stats, and what the call must leave alone: dst rows outside every request keep their 7.0
    (check_rag), the guards and every pool byte are unchanged, and the output is NaN-free although every cell behind a live length and every spare
    block is NaN.  One launch: no counter of any other attention entry moves."""
    _, _, bk, layout, want = CASES[name]
    c = step(nso, name)
    p = rag_pools(c, bk, layout).upload()
    s0, others = prefill_stats(L), (attn_stats(L), block_stats(L), paged_stats(L))
    out = run_prefill(L, pkg, c, p)[0]
    assert delta(s0, prefill_stats(L)) == want
    assert (attn_stats(L), block_stats(L), paged_stats(L)) == others
    assert np.all(np.isfinite(out)), name
    check_rag(nso, name, c, out)
    assert p.guards_intact()
    pk, pv = p.download()
    assert np.array_equal(pk, p.k) and np.array_equal(pv, p.v)  # the attention writes no cache byte


def test_the_position_array_drives_the_lengths_through_the_bias(L, pkg, nso):
    c = step(nso, "a_query_block_boundary_bk16")
    p = rag_pools(c, 16, PM).upload()
    assert np.array_equal(run_prefill(L, pkg, c, p, bias=3)[0].view(np.uint32), run_prefill(L, pkg, c, p)[0].view(np.uint32))


def test_max_q_clamps_a_requests_rows(L, pkg, nso):
    """max_q = 5 under q lens [130, 1, 0, 17]: requests 0 and 3 are served as their first five rows (which then see kv_len - 5 + i + 1 keys), their
    other rows keep their 7.0; request 1 is what it is under max_q = 130"""
    c = step(nso, "a_query_block_boundary_bk16")
    p = rag_pools(c, 16, PM).upload()
    full = run_prefill(L, pkg, c, p)[0]
    out = run_prefill(L, pkg, c, p, max_q=5)[0]
    assert np.all(out[:LEAD] == 7.0) and np.all(out[c.start[-1]:] == 7.0)
    assert np.array_equal(out[c.start[1]:c.start[2]].view(np.uint32), full[c.start[1]:c.start[2]].view(np.uint32))
    for b in (0, 3):
        assert np.all(out[c.start[b] + 5:c.start[b + 1]] == 7.0)
        qb = c.q[c.start[b]:c.start[b] + 5][None]
        kb, vb = c.k[b:b + 1, :c.kvlens[b]], c.v[b:b + 1, :c.kvlens[b]]
        check(nso, "max_q 5, request %d" % b, out[c.start[b]:c.start[b] + 5][None], nso.attn_ref(qb, kb, vb, c.scale, CAUSAL),
              rounding_model(qb, kb, vb, c.scale, CAUSAL))


# ---- 2. table entries ----------------------------------------------------------------------------------------------------------------------------------
def test_table_entries_behind_the_live_blocks_may_hold_anything(L, pkg, nso):
    c = step(nso, "a_query_block_boundary_bk16")
    good = run_prefill(L, pkg, c, rag_pools(c, 16, PM).upload())[0]

    def junk(p):
        for b, n in enumerate(c.kvlens):
            first = -(-n // 16)
            p.table[b, first:] = [(-1 if j % 2 else p.pool_blocks) for j in range(p.ts - first)]

    p = rag_pools(c, 16, PM, table_edit=junk).upload()
    assert p.table[1, 2] in (-1, p.pool_blocks) and 0 <= p.table[1, 1] < p.pool_blocks and p.table[2, 0] in (-1, p.pool_blocks)
    out = run_prefill(L, pkg, c, p)[0]
    assert np.array_equal(out.view(np.uint32), good.view(np.uint32))
    assert p.guards_intact()


@pytest.mark.parametrize("bad", ["minus_one", "pool_blocks"])
def test_a_bad_entry_inside_a_live_length_leaves_the_other_requests_alone(L, pkg, nso, bad):
    """request 0's second block (300 live keys, blocks of 16) gets an id that is no block of the pool: every other request's rows hold the bits of the
    run with the valid table and nothing is NaN there; request 0's rows are finite too (the keys read as zeros); the guards are unchanged"""
    c = step(nso, "a_query_block_boundary_bk16")
    good = run_prefill(L, pkg, c, rag_pools(c, 16, PM).upload())[0]

    def poison(p):
        p.table[0, 1] = -1 if bad == "minus_one" else p.pool_blocks

    p = rag_pools(c, 16, PM, table_edit=poison).upload()
    out = run_prefill(L, pkg, c, p)[0]
    others = slice(c.start[1], None)
    assert np.all(np.isfinite(out))
    assert np.array_equal(out[others].view(np.uint32), good[others].view(np.uint32))
    assert np.all(out[:LEAD] == 7.0) and p.guards_intact()


# ---- 3. strides ------------------------------------------------------------------------------------------------------------------------------------------
def test_strided_unaligned_dst_with_the_fp16_shadow(L, pkg, nso):
    """dst rows of hs + 3 floats from a pointer one float behind a 16-byte boundary, dst16 with the same element strides: the scalar stores give the
    bits of the 16-byte ones, the shadow is the rounded output, the padding of every row and the rows of no request keep their 7.0"""
    c = step(nso, "i_tensor_scales")
    p = rag_pools(c, 16, PM).upload()
    plain, p16, _ = run_prefill(L, pkg, c, p, dst16=True)
    out, o16, whole = run_prefill(L, pkg, c, p, dst16=True, dst_pad=3)
    assert np.array_equal(out.view(np.uint32), plain.view(np.uint32))
    assert np.all(whole[..., c.hs:] == 7.0) and np.all(o16[..., c.hs:] == 7.0)
    live = slice(c.start[0], c.start[-1])
    assert np.array_equal(o16[live, :, :c.hs], out[live].astype(np.float16)) and np.array_equal(p16[live], plain[live].astype(np.float16))
    for x in (o16, p16):
        assert np.all(x[:LEAD] == 7.0) and np.all(x[c.start[-1]:] == 7.0)
    check_rag(nso, "strided dst", c, out)


# ---- 4. refusals -----------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_are_counted_and_write_nothing(L, pkg, nso):
    import torch
    c = step(nso, "a_query_block_boundary_bk16")
    p = rag_pools(c, 16, PM).upload()
    dq = torch.from_numpy(c.q.copy()).cuda()
    dd = torch.full((c.rows, c.hn, c.hs), 7.0, device="cuda")
    ds = torch.tensor(c.start, dtype=torch.int32, device="cuda")
    dl = torch.tensor(c.kvlens, dtype=torch.int32, device="cuda")

    def call(table=True, ts=p.ts, bk=16, blocks=p.pool_blocks, step=p.block_step, lens=True, start=True, max_q=130, hs=c.hs, flags=CAUSAL, hn=c.hn, hkv=c.hkv,
             layout=0, k_hs=1, bs=c.bs, part=None):
        a = block_args(pkg, c, p, dq.data_ptr(), dd.data_ptr(), max_q, c.hs)
        a.head_size, a.attn_flags, a.head_num, a.heads_kv, a.K_layout, a.step_k_head_size, a.batch_size = hs, flags, hn, hkv, layout, k_hs, bs
        if part:
            assert L.ns_hip_attn_set_head_partition(*part) == 0
        try:
            return L.ns_hip_attn_prefill_paged(C.byref(a), C.c_void_p(ds.data_ptr()) if start else None, C.c_void_p(dl.data_ptr()) if lens else None, 0,
                                               C.c_void_p(p.dt.data_ptr()) if table else None, ts, bk, blocks, step, None, stream_ptr())
        finally:
            assert L.ns_hip_attn_set_head_partition(0, 0) == 0

    calls = [("block table is null", dict(table=False)), ("power of two from 16 to 256", dict(bk=48)), ("power of two from 16 to 256", dict(bk=8)),
             ("pool_blocks must be at least 1", dict(blocks=0)), ("must equal table_stride * block_keys", dict(ts=p.ts - 1)),
             ("do not fit inside block_step", dict(step=p.block_step - 8)), ("dKvLens is null", dict(lens=False)), ("dQStart is null", dict(start=False)),
             ("only ATTN_FWD_LAYOUT_PLAIN tensors are supported", dict(layout=1)), ("batch_size (the requests) must be at least 1", dict(bs=0)),
             ("head_size must be a multiple of 8, at most 256", dict(hs=60)), ("head_size must be a multiple of 8, at most 256", dict(hs=264)),
             ("head sizes above 128 are not served", dict(hs=256)), ("head sizes above 128 are not served", dict(hs=136)),
             ("head_num must be a multiple of heads_kv", dict(hn=5, hkv=2)), ("sl_q is max_q", dict(max_q=0)),
             ("contiguous in the head dimension and 16-byte aligned", dict(k_hs=2)),
             ("head partition (ns_hip_attn_set_head_partition) does not contain this call's heads", dict(flags=CAUSAL | ALIBI, part=(6, 4)))]
    s0, g0, b0, a0 = prefill_stats(L), paged_stats(L), block_stats(L), attn_stats(L)
    for n, (text, kw) in enumerate(calls):
        L.ns_hip_reset_error()
        assert call(**kw) == -1, text
        assert text in pkg.last_error(), (text, pkg.last_error())
        assert delta(s0, prefill_stats(L)) == [0, 0, 0, 0, 0, n + 1]
    L.ns_hip_reset_error()
    assert L.ns_hip_attn_prefill_paged(None, None, None, 0, None, 0, 0, 0, 0, None, stream_ptr()) == -1 and "null arguments" in pkg.last_error()
    torch.cuda.synchronize()
    assert bool(torch.all(dd == 7.0)) and (paged_stats(L), block_stats(L), attn_stats(L)) == (g0, b0, a0)
    pk, pv = p.download()
    assert np.array_equal(pk, p.k) and np.array_equal(pv, p.v)
    L.ns_hip_reset_error()


# ---- 5. the bits of the uniform 128-row kernel -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hs,flags", [(80, CAUSAL), (64, CAUSAL | ALIBI)], ids=["padded_80", "alibi"])
def test_bit_equal_to_the_uniform_kernel_on_a_contiguous_copy(L, pkg, nso, hs, flags):
    """Two requests of q_len 130 over kv_len 300 on pages of 16 in a random permutation against ns_hip_attn_fp32_fp16_fp16_fp32_forward_h on the
    contiguous copy of the same keys, which attn_mfma2_kernel serves (a padded or a biased shape from 16 rows on; asserted through
    ns_hip_attn_stats): the arithmetic is the same, operation for operation, so the bits are."""
    import torch
    hn, hkv, n_q, n_kv = 8, 2, 130, 300
    c = Rag(None, hn, hkv, hs, 512, [n_q, n_q], [n_kv, n_kv], flags, seed=17)  # (inputs only: the other run is the reference here)
    p = rag_pools(c, 16, PM).upload()
    s0 = prefill_stats(L)
    out = run_prefill(L, pkg, c, p)[0]
    assert delta(s0, prefill_stats(L)) == [int(hs <= 64), int(hs > 64), 0, int(bool(flags & ALIBI)), int(hs not in (64, 128)), 0]
    dq = torch.from_numpy(np.stack([c.q[c.start[b]:c.start[b] + n_q] for b in range(2)])).cuda()
    dk, dv = torch.from_numpy(c.k[:, :n_kv].copy()).cuda(), torch.from_numpy(c.v[:, :n_kv].copy()).cuda()
    dd = torch.full((2, n_q, hn, hs), 7.0, device="cuda")
    a = pkg.attn_args(dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), dd.data_ptr(), 2, hn, hkv, hs, n_q, n_kv, c.scale, flags)
    a0 = attn_stats(L)
    pkg.check(L.ns_hip_attn_fp32_fp16_fp16_fp32_forward_h(C.byref(a), None, stream_ptr()))
    torch.cuda.synchronize()
    d = delta(a0, attn_stats(L))
    assert d[AP_ROWS128] == 1 and sum(d) == 1, d
    uni = dd.cpu().numpy()
    assert np.all(np.isfinite(uni))
    for b in range(2):
        assert np.array_equal(out[c.start[b]:c.start[b] + n_q].view(np.uint32), uni[b].view(np.uint32)), b


# ---- 6. one captured step, replayed on other contents -------------------------------------------------------------------------------------------------------
def test_captured_step_replayed_on_new_contents(L, pkg, nso):
    """The entry captured ONCE on a side stream — no tmp, no scratch, no eager call of it on that stream in front — then replayed after the CONTENTS of
    dQStart, dKvLens, the table, Q and the pools changed: step 1 is a chunk of 130 rows from position 0 beside a decode row, step 2 a decode row
    beside a chunk of 70 over 200 keys, on another permutation of the blocks.  Every replay equals the same step run eagerly, bit for bit."""
    import torch
    hn, hkv, hs, cap, bk, max_q = 4, 2, 64, 256, 16, 130
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
            pkg.check(L.ns_hip_attn_prefill_paged(C.byref(a), C.c_void_p(start.data_ptr()), C.c_void_p(lens.data_ptr()), 0, *p.table_args(), None, stream_ptr()))

        move_to(0)
        side.synchronize()
        s0 = prefill_stats(L)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            call()
        assert delta(s0, prefill_stats(L)) == [1, 0, 0, 0, 0, 0]
        for n, s in enumerate(steps):
            move_to(n)
            g.replay()
            side.synchronize()
            got = dst.cpu().numpy()
            move_to(n)
            call()
            side.synchronize()
            eager = dst.cpu().numpy()
            assert np.array_equal(got.view(np.uint32), eager.view(np.uint32)), n
            live = got[s.start[0]:s.start[-1]]
            assert np.all(np.isfinite(live)) and not np.any(live == 7.0), n
            assert np.all(got[:LEAD] == 7.0) and np.all(got[s.start[-1]:] == 7.0), n
        # the last step against the reference
        s = steps[-1]
        for b in range(2):
            qb = s.q[s.start[b]:s.start[b + 1]][None]
            kb, vb = s.k[b:b + 1, :s.kvlens[b]], s.v[b:b + 1, :s.kvlens[b]]
            check(nso, "replayed step 2 request %d" % b, got[s.start[b]:s.start[b + 1]][None], nso.attn_ref(qb, kb, vb, s.scale, CAUSAL),
                  rounding_model(qb, kb, vb, s.scale, CAUSAL))
    torch.cuda.synchronize()


# ---- 7. a pool above 2^31 elements ----------------------------------------------------------------------------------------------------------------------------
def test_far_pool_is_bit_equal_to_the_compact_twin(L, pkg, nso):
    """The helpers of tests/test_gpu_attn_far_addresses.py by import: a pool of 1.4 * 2^31 elements with the live blocks at its top and block 2, traps
    at every alias of a truncated address; q lens [1, 130, 40] over kv lens [70, 200, 120], head size 128, blocks of 16.  The far run holds the bits of
    the compact twin, which passes the check against the reference; no trap is read (no NaN) or written."""
    from test_gpu_attn_far_addresses import FL, HKV, HN, Pages, live_blocks, release, same_bits
    hs, bk = 128, 16
    c = Step(nso, HN, HKV, hs, FL.PAGED_CAP[bk], [1, 130, 40], FL.BLOCK_KV[bk], seed=31)
    near = far = None
    try:
        near = Pages("near", hs, bk, live_blocks(c.kvlens, bk)).fill_keys(c.k, c.v, c.kvlens)
        far = Pages("over", hs, bk, live_blocks(c.kvlens, bk)).fill_keys(c.k, c.v, c.kvlens)
        s0 = prefill_stats(L)
        out_n = run_prefill(L, pkg, c, near)[0]
        out_f = run_prefill(L, pkg, c, far)[0]
        assert delta(s0, prefill_stats(L)) == [0, 2, 0, 0, 0, 0]
        check_rag(nso, "far addresses, near twin: prefill_paged hs %d bk %d" % (hs, bk), c, out_n)
        assert np.all(np.isfinite(out_f)), "a trap or a dead cell was consumed"
        assert same_bits(out_f, out_n)
        assert far.traps_intact()
    finally:
        near = far = None
        release()

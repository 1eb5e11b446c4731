"""Ragged query blocks over an FP8 (E4M3) paged KV cache: ns_hip_attn_block_paged_f8 (attn_block_split8_kernel and the fp16 entry's merge) and
ns_hip_rope_qkv_append_paged_seq_f8.  docs/kernels/attention.md, "Ragged query blocks over an FP8 paged cache".

Inputs as in tests/test_gpu_attn_paged_f8.py: K / V are drawn, then rounded to E4M3 of x / scale with a power-of-two scale, so a case's fp16 arrays hold
code * scale exactly.  The uint8 pools (Pools8) hold 0x7f — NaN — behind every live length and in spare blocks, with a guard block on either side.
Every attention case is checked (1) per request against nso.attn_ref over the decoded values through check_rag / rounding_model, the fp16 module's
per-row bound, and (2) against ns_hip_attn_block_paged over fp16 pools of the decoded values under the same table: rel_l2 < 2e-4.  The two kernels
share their operand rounding (the decode is exact) and differ in the k-slot order of the K.Q^T sums; 2e-4 is the lower end of what this project
measured between two kernels with DIFFERENT operand rounding, so they must lie far inside it."""
import copy
import ctypes as C

import numpy as np
import pytest

from test_gpu_attention_paths import check, rounding_model
from test_gpu_attn_block_paged import CASES, LEAD, Rag, block_args, check_rag, run_block
from test_gpu_attn_paged import Pools, delta
from test_gpu_attn_paged_f8 import NAN8, Pools8, decoded, pools_pair, to_codes
from test_gpu_attn_rows import CAUSAL, HM, PM, attn_stats, stream_ptr

pytestmark = pytest.mark.gpu
BLOCK_SPLIT = 7  # AttnPath AP_BLOCK_SPLIT: the family the launches count under in ns_hip_attn_stats


def block8_stats(L):
    out = (C.c_ulonglong * 4)()
    L.ns_hip_attn_block_paged_f8_stats(out)
    return list(out)


class Rag8(Rag):
    """Rag over E4M3-representable K / V: kc / vc the codes, k / v = code * scale in fp16; scales is what the FP16 entry gets (the pools' scales are
    in its values), f8_scales what the FP8 entry gets.  codes: (kc, vc) given instead of drawn."""

    def __init__(self, nso, hn, hkv, hs, cap, qlens, kvlens, flags=CAUSAL, scales=(1.0, 0.125, 0.125, 1.0), codes=None):
        Rag.__init__(self, None, hn, hkv, hs, cap, qlens, kvlens, flags)
        qs, ks, vs, ds = scales
        self.f8_scales, self.scales, self.lens = scales, (qs, 1.0, 1.0, ds), self.kvlens  # (lens: pools_pair's name for the live lengths)
        self.kc, self.vc = codes(self.k.shape) if codes else (to_codes(self.k.astype(np.float32), ks), to_codes(self.v.astype(np.float32), vs))
        self.k, self.v = decoded(self.kc, ks), decoded(self.vc, vs)
        assert np.array_equal(to_codes(self.k, ks), self.kc) and np.array_equal(to_codes(self.v, vs), self.vc)  # the fp16 copy is exact
        for b in range(self.bs):
            see, end = self.seeing(b), self.start[b] + self.qlens[b]
            if see:
                qb, kb, vb = self.q[end - see:end][None], self.k[b:b + 1, :self.kvlens[b]], self.v[b:b + 1, :self.kvlens[b]]
                self.ref[b] = nso.attn_ref(qb, kb, vb, self.scale, flags, scales=self.scales)
                self.model[b] = rounding_model(qb, kb, vb, self.scale, flags, self.scales)


def all_codes(shape):
    """K and V cycle through the 254 finite codes (254 is no multiple of the head size: every byte of a load sees every code), V half a cycle behind"""
    finite = np.array([c for c in range(256) if c & 0x7f != NAN8], np.uint8)
    n = int(np.prod(shape))
    return finite[np.arange(n) % 254].reshape(shape), finite[(np.arange(n) + 127) % 254].reshape(shape)


class AsFp16Entry:
    """run_block's library handle with the FP8 entry in the fp16 entry's place"""

    def __init__(self, L):
        self.ns_hip_attn_block_paged = L.ns_hip_attn_block_paged_f8


def run_block8(L, pkg, c, p, **kw):
    c8 = copy.copy(c)
    c8.scales = c.f8_scales
    return run_block(AsFp16Entry(L), pkg, c8, p, **kw)


# the fp16 module's cases (a) .. (e), its case (f) cut to capacity 1024, and every finite code (Q_sc 2^-6 keeps the softmax wide: every V code counts)
CASES8 = {name: CASES[name] for name in CASES if name[0] in "abcde"}
CASES8["f_several_ranges_short_neighbour"] = (4, 4, 128, 1024, [33, 3], [1000, 130], CAUSAL, 64, PM)
CASES8["g_all_codes"] = (4, 2, 64, 256, [16], [256], CAUSAL, 16, PM)
_rags = {}


def rag8(nso, name):
    key = repr(CASES8[name][:7])
    if key not in _rags:
        extra = dict(scales=(2.0 ** -6, 0.25, 2.0, 4.0), codes=all_codes) if name == "g_all_codes" else {}
        _rags[key] = Rag8(nso, *CASES8[name][:7], **extra)
    return _rags[key]


# ---- 1. against the reference and against the fp16 entry on the decoded pools ------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES8))
def test_f8_blocks_against_the_reference_and_the_fp16_entry(L, pkg, nso, name):
    bk, layout = CASES8[name][7:]
    c = rag8(nso, name)
    p8, p16 = pools_pair(c, bk, layout)
    s0, a0 = block8_stats(L), attn_stats(L)
    out = run_block8(L, pkg, c, p8)[0]
    assert delta(s0, block8_stats(L)) == ([1, 0, 1, 0] if c.hs == 64 else [0, 1, 1, 0])
    assert delta(a0, attn_stats(L))[BLOCK_SPLIT] == 1 and sum(delta(a0, attn_stats(L))) == 1
    assert np.all(np.isfinite(out)), name  # no byte behind a live length, no spare block was consumed
    check_rag(nso, "f8 " + name, c, out)
    assert p8.guards_intact() and p8.unchanged()
    half = run_block(L, pkg, c, p16)[0]
    live = slice(c.start[0], c.start[-1])
    e = nso.rel_l2(out[live], half[live])
    print("ATTN_BLOCK_PAGED_F8 %s: rel_l2 against ns_hip_attn_block_paged %.3g" % (name, e))
    assert e < 2e-4, (name, e)


# ---- 2. contract edges -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("edge", ["junk_behind_the_live_blocks", "bad_id_minus_one", "bad_id_pool_blocks", "bias", "dst16_and_tmp"])
def test_contract_edges(L, pkg, nso, edge):
    """case (a), blocks of 16.  junk: every entry behind a request's live blocks holds -1, pool_blocks or the id of a NaN block — the same bits.  bad id:
    request 2's second block (live) is no block of the pool — the other requests' rows hold the same bits.  bias: dKvLens - 3 with kv_len_bias 3 — the
    same bits.  dst16 and tmp: the fp16 shadow is the rounded output, the partials went to the caller's tmp and not a byte behind its size."""
    import torch
    c = rag8(nso, "a_decode_row_beside_blocks")
    good = run_block8(L, pkg, c, pools_pair(c, 16, PM)[0])[0]

    def junk(p):
        spare = min(set(range(p.pool_blocks)) - set(p.table.ravel().tolist()))  # a block no request names: NaN codes throughout
        for b, n in enumerate(c.kvlens):
            first = -(-n // 16)
            p.table[b, first:] = [(-1, p.pool_blocks, spare)[j % 3] for j in range(p.ts - first)]

    def poison(p):
        p.table[2, 1] = -1 if edge == "bad_id_minus_one" else p.pool_blocks

    same = lambda x, y: np.array_equal(x.view(np.uint32), y.view(np.uint32))
    if edge == "junk_behind_the_live_blocks":
        p = pools_pair(c, 16, PM, table_edit=junk)[0]
        assert same(run_block8(L, pkg, c, p)[0], good) and p.guards_intact()
    elif edge.startswith("bad_id"):
        p = pools_pair(c, 16, PM, table_edit=poison)[0]
        out = run_block8(L, pkg, c, p)[0]
        assert same(out[:c.start[2]], good[:c.start[2]]) and np.all(out[c.start[3]:] == 7.0) and p.guards_intact()
    elif edge == "bias":
        assert same(run_block8(L, pkg, c, pools_pair(c, 16, PM)[0], bias=3)[0], good)
    else:
        size = L.ns_hip_attn_block_paged_workspace_size(c.bs, c.hn, c.hkv, c.hs, max(c.qlens), c.cap)
        tmp = torch.full((size + 256,), 0x5A, dtype=torch.uint8, device="cuda")
        out, o16, _ = run_block8(L, pkg, c, pools_pair(c, 16, PM)[0], dst16=True, tmp=tmp)
        live = slice(c.start[0], c.start[-1])
        assert same(out, good) and np.array_equal(o16[live], out[live].astype(np.float16)) and np.all(o16[:LEAD] == 7.0) and np.all(o16[c.start[-1]:] == 7.0)
        t = tmp.cpu().numpy()
        assert np.all(t[size:] == 0x5A) and not np.all(t[:size] == 0x5A)


def test_refusals_are_counted_and_write_nothing(L, pkg, nso):
    """the fp16 entry's refusals and the FP8 pool's: -1, the reason, stats [3], no launch, dst and pools as they were"""
    import torch
    c = rag8(nso, "a_decode_row_beside_blocks")
    p = pools_pair(c, 16, PM)[0]
    dq = torch.from_numpy(c.q.copy()).cuda()
    dd = torch.full((c.rows, c.hn, c.hs), 7.0, device="cuda")
    ds = torch.tensor(c.start, dtype=torch.int32, device="cuda")
    dl = torch.tensor(c.kvlens, dtype=torch.int32, device="cuda")

    def call(table=True, ts=p.ts, bk=16, blocks=p.pool_blocks, step=p.block_step, lens=True, start=True, **fields):
        a = block_args(pkg, c, p, dq.data_ptr(), dd.data_ptr(), 16, c.hs)
        a.Q_sc, a.K_sc, a.V_sc, a.dst_sc = c.f8_scales
        for k, v in fields.items():
            setattr(a, k, v)
        return L.ns_hip_attn_block_paged_f8(C.byref(a), C.c_void_p(ds.data_ptr()) if start else None, C.c_void_p(dl.data_ptr()) if lens else None, 0,
                                            C.c_void_p(p.dt.data_ptr()) if table else None, ts, bk, blocks, step, None, stream_ptr())

    calls = [("block table is null", dict(table=False)), ("power of two from 16 to 256", dict(bk=48)), ("pool_blocks must be at least 1", dict(blocks=0)),
             ("must equal table_stride * block_keys", dict(ts=p.ts - 1)), ("do not fit inside block_step", dict(step=p.block_step - 16)),
             ("dKvLens is null", dict(lens=False)), ("dQStart is null", dict(start=False)), ("head_size must be 64 or 128", dict(head_size=80)),
             ("ALiBi and the tanh cap are not served", dict(attn_flags=CAUSAL | 2)), ("sl_q is max_q", dict(sl_q=0)),
             ("above the grid limit of 65535", dict(head_num=4096, heads_kv=1, sl_q=1024)),
             ("head_size must be a multiple of 16", dict(head_size=72)), ("block_step must be a multiple of 16", dict(step=p.block_step + 8)),
             ("pool bases must be 16-byte aligned", dict(K=p.kp + 8)), ("strides must be multiples of 16", dict(step_v_sl=p.step_sl + 8)),
             ("strides must be multiples of 16", dict(step_k_head_num=p.step_head + 8)), ("must be positive and finite", dict(K_sc=0.0)),
             ("must be positive and finite", dict(V_sc=float("inf"))), ("must be positive and finite", dict(V_sc=float("nan")))]
    s0, a0 = block8_stats(L), attn_stats(L)
    for n, (text, kw) in enumerate(calls):
        L.ns_hip_reset_error()
        assert call(**kw) == -1, text
        assert text in pkg.last_error(), (text, pkg.last_error())
        assert delta(s0, block8_stats(L)) == [0, 0, 0, n + 1]
    torch.cuda.synchronize()
    assert bool(torch.all(dd == 7.0)) and attn_stats(L) == a0 and p.unchanged()
    L.ns_hip_reset_error()


# ---- 3. the append with a row -> request map -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [PM, HM])
@pytest.mark.parametrize("mode,n_dims", [(0, 64), (2, 32)])
def test_append_seq_f8_is_bit_equal_to_the_f8_append_on_the_expanded_table(L, pkg, mode, n_dims, layout):
    """The fp16 module's set-up: 9 rows of 3 requests (a chunk of four, one decode row, a chunk of two; one row idle by position, one by a request id
    of 3 and one by -1), 4 / 2 heads of 64, blocks of 16, capacity 256.  ns_hip_rope_qkv_append_paged_f8 takes the table with one row per query row.
    Q and both pools hold the same bytes, guards and untouched cells included; the idle rows' Q is untouched and six rows were written."""
    import torch
    heads, hkv, hs, cap, bk, requests, ks, vs = 4, 2, 64, 256, 16, 3, 0.25, 2.0
    row_req = [0, 0, 0, 0, 1, 2, 2, 3, -1]
    pos = [14, 15, 16, 17, 200, 255, 256, 5, 6]  # (256: at the capacity, idle)
    rows = len(pos)
    rng = np.random.default_rng(mode * 100 + n_dims)
    q, k, v = (rng.standard_normal((rows, h, hs)).astype(np.float32) for h in (heads, hkv, hkv))
    dk, dv, st = torch.from_numpy(k).cuda(), torch.from_numpy(v).cuda(), stream_ptr()
    ok = [0 <= r < requests for r in row_req]
    res = []
    for form in ("seq", "expanded"):
        p = Pools8(requests, hkv, hs, cap, bk, layout, seed=9).upload()
        dq = torch.from_numpy(q).cuda()
        rope = (n_dims, mode, 10000.0, 0.75, 0.0, 1.1)
        if form == "seq":
            dpos, dreq = (torch.tensor(x, dtype=torch.int32, device="cuda") for x in (pos, row_req))
            pkg.check(L.ns_hip_rope_qkv_append_paged_seq_f8(dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), p.kp, p.vp, rows, heads, hkv, hs, dpos.data_ptr(), 4096,
                                                            *rope, dreq.data_ptr(), requests, *p.table_args(), p.step_sl, p.step_head, ks, vs, st))
        else:
            table = torch.from_numpy(np.stack([p.table[r if o else 0] for r, o in zip(row_req, ok)])).cuda()
            dpos = torch.tensor([n if o else -1 for n, o in zip(pos, ok)], dtype=torch.int32, device="cuda")
            pkg.check(L.ns_hip_rope_qkv_append_paged_f8(dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), p.kp, p.vp, rows, heads, hkv, hs, dpos.data_ptr(), 4096, *rope,
                                                        C.c_void_p(table.data_ptr()), p.ts, bk, p.pool_blocks, p.block_step, p.step_sl, p.step_head, ks, vs, st))
        torch.cuda.synchronize()
        res.append((dq.cpu().numpy(), p.download(), p))
    (q_seq, (k_seq, v_seq), p), (q_exp, (k_exp, v_exp), _) = res
    assert np.array_equal(q_seq.view(np.uint32), q_exp.view(np.uint32)) and np.array_equal(k_seq, k_exp) and np.array_equal(v_seq, v_exp)
    assert all(np.array_equal(q_seq[r], q[r]) for r in (6, 7, 8)) and not any(np.array_equal(q_seq[r], q[r]) for r in range(6))
    assert int((k_seq != p.k).reshape(k_seq.shape[0], -1).any(axis=1).sum()) == 4 and p.guards_intact()  # blocks 0 and 1 of request 0, one each of 1 and 2


# ---- 4. a prompt in chunks on an FP8 pool, through the two new entries alone ---------------------------------------------------------------------------
def test_chunked_prefill_on_an_f8_pool(L, pkg, nso):
    """A 150-token prompt goes in as chunks of 64 / 64 / 22 (4 / 2 heads of 128, blocks of 16, capacity 256) beside a second request that stays idle.
    Every chunk's rows lie within the check() bounds of the causal attention of the rotated Q rows over the DECODED pool contents; the pools' bytes are
    those ns_hip_kv_paged_store_f8 makes of the slab the fp16 append wrote for the same tokens."""
    import torch
    hn, hkv, hs, cap, bk, n_tok, ks, vs = 4, 2, 128, 256, 16, 150, 0.0625, 0.125
    rng = np.random.default_rng(150)
    dq, dk, dv = (torch.from_numpy(rng.standard_normal((n_tok, h, hs)).astype(np.float32)).cuda() for h in (hn, hkv, hkv))
    p, stored, p16 = Pools8(2, hkv, hs, cap, bk, PM, seed=21).upload(), Pools8(2, hkv, hs, cap, bk, PM, seed=21).upload(), Pools(2, hkv, hs, cap, bk, PM, seed=21).upload()
    q16, dst, scale = dq.clone(), torch.full((n_tok, hn, hs), 7.0, device="cuda"), float(1.0 / np.sqrt(hs))
    c = Rag.__new__(Rag)
    c.bs, c.hn, c.hkv, c.hs, c.cap, c.scale, c.flags, c.scales = 2, hn, hkv, hs, cap, scale, CAUSAL, (1.0, ks, vs, 1.0)
    st, done = stream_ptr(), 0
    for chunk in (64, 64, 22):
        dpos = torch.arange(done, done + chunk, dtype=torch.int32, device="cuda")
        dreq = torch.zeros(chunk, dtype=torch.int32, device="cuda")
        rope = (chunk, hn, hkv, hs, dpos.data_ptr(), cap, hs, 0, 10000.0, 1.0, 0.0, 1.0, dreq.data_ptr(), 2)
        qc = dq[done:done + chunk]
        pkg.check(L.ns_hip_rope_qkv_append_paged_seq_f8(qc.data_ptr(), dk[done:].data_ptr(), dv[done:].data_ptr(), p.kp, p.vp, *rope, *p.table_args(), p.step_sl,
                                                        p.step_head, ks, vs, st))
        pkg.check(L.ns_hip_rope_qkv_append_paged_seq(q16[done:].data_ptr(), dk[done:].data_ptr(), dv[done:].data_ptr(), p16.kp, p16.vp, *rope, *p16.table_args(),
                                                     p16.step_sl, p16.step_head, st))
        ds = torch.tensor([0, chunk, chunk], dtype=torch.int32, device="cuda")
        dl = torch.tensor([done + chunk, 0], dtype=torch.int32, device="cuda")
        a = block_args(pkg, c, p, qc.data_ptr(), dst[done:].data_ptr(), 64, hs)
        pkg.check(L.ns_hip_attn_block_paged_f8(C.byref(a), C.c_void_p(ds.data_ptr()), C.c_void_p(dl.data_ptr()), 0, *p.table_args(), None, st))
        done += chunk
    blocks = -(-n_tok // bk)
    for j in range(blocks):  # the fp16 pool, block by block, is the prompt's slab: store it through the same table
        off = 2 * int(p16.table[0, j]) * p16.block_step
        pkg.check(L.ns_hip_kv_paged_store_f8(p16.kp + off, p16.vp + off, hkv * hs, hs, 0, min(bk, n_tok - j * bk), hkv, hs, stored.kp, stored.vp,
                                             C.c_void_p(stored.dt.data_ptr() + 4 * j), 1, bk, stored.pool_blocks, stored.block_step, stored.step_sl,
                                             stored.step_head, ks, vs, st))
    torch.cuda.synchronize()
    assert torch.equal(p.dk, stored.dk) and torch.equal(p.dv, stored.dv) and torch.equal(dq, q16) and p.guards_intact()
    kb, vb = (decoded(np.concatenate([p.cells(x, p.table[0, j], 0, bk) for j in range(blocks)])[:n_tok], s)[None] for x, s in zip(p.download(), (ks, vs)))
    assert np.all(np.isfinite(kb.astype(np.float32))) and np.all(np.isfinite(vb.astype(np.float32)))
    qr, out = dq.cpu().numpy()[None], dst.cpu().numpy()[None]
    ref, model = nso.attn_ref(qr, kb, vb, scale, CAUSAL), rounding_model(qr, kb, vb, scale, CAUSAL)
    for lo, hi in ((0, 64), (64, 128), (128, 150)):
        check(nso, "chunk rows %d..%d of the prompt on an FP8 pool" % (lo, hi - 1), out[:, lo:hi], ref[:, lo:hi], model[:, lo:hi])


# ---- 5. a pool just over 2^32 bytes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,n_dims", [(0, 128), (2, 64)])
def test_far_pool_is_bit_equal_to_the_compact_twin(L, pkg, nso, mode, n_dims):
    """The ragged step of tests/test_gpu_attn_far_addresses.py (q lens 1 / 5 / 40 over kv lens 70 / 200 / 120, 4 / 2 heads of 128, blocks of 16 = 4096
    bytes, partials in the caller's workspace) on FarPools8 of tests/test_gpu_attn_paged_f8.py: an untouched pool of 2^20 + 64 blocks, every live block
    but block 2 above 2^32 bytes.  Request 0's last key is written by ns_hip_rope_qkv_append_paged_seq_f8 in both twins (mode 0; NeoX pairs over half
    the head).  The compact twin meets the reference over the pool's decoded contents and the fp16 entry; the far run holds its bits — the output,
    the rotated Q and every live block — consumes no 0x7f byte and changes none."""
    import torch
    from test_gpu_attn_far_addresses import FL, need, release, same_bits
    from test_gpu_attn_paged_f8 import FarPools8
    hs, bk, (qs, ks, vs, ds) = 128, 16, (1.0, 0.125, 0.125, 1.0)
    c = Rag8(nso, FL.HN, FL.HKV, hs, FL.PAGED_CAP[bk], FL.BLOCK_Q, FL.BLOCK_KV[bk])
    live, n0 = [-(-n // bk) for n in c.kvlens], c.kvlens[0]
    rng = np.random.default_rng(500 + mode)
    q1, k1, v1 = (torch.from_numpy(rng.standard_normal((1, h, hs)).astype(np.float32)).cuda() for h in (c.hn, c.hkv, c.hkv))
    dpos, dreq = torch.tensor([n0 - 1], dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    ws = L.ns_hip_attn_block_paged_workspace_size(c.bs, c.hn, c.hkv, hs, max(c.qlens), c.cap)
    assert ws > 0
    need(2 * FL.F8_BLOCKS * FL.block_step(hs, bk))
    got, p, tmp = [], None, None
    try:
        tmp = torch.empty(ws, dtype=torch.uint8, device="cuda")
        for blocks in (FL.pool_blocks("near", FL.block_step(hs, bk), sum(live)) + 128, FL.F8_BLOCKS):
            p = FarPools8(blocks, c, bk, live)
            assert blocks < 1 << 20 or all(i == 2 or i * p.block_step >= 1 << 32 for i in p.ids.values())
            for b, n in enumerate(c.kvlens):
                p.put(b, c.kc[b, :n - (b == 0)], c.vc[b, :n - (b == 0)])
            dq = q1.clone()
            pkg.check(L.ns_hip_rope_qkv_append_paged_seq_f8(dq.data_ptr(), k1.data_ptr(), v1.data_ptr(), p.kp, p.vp, 1, c.hn, c.hkv, hs, dpos.data_ptr(), c.cap, n_dims,
                                                            mode, 10000.0, 0.75, 0.0, 1.1, dreq.data_ptr(), c.bs, *p.table_args(), p.step_sl, p.step_head, ks, vs,
                                                            stream_ptr()))
            s0 = block8_stats(L)
            out = run_block8(L, pkg, c, p, tmp=tmp)[0]
            assert delta(s0, block8_stats(L)) == [0, 1, 1, 0], blocks
            cells, clean = p.live()
            assert clean and np.all(np.isfinite(out)), blocks
            got.append((out, dq.cpu().numpy(), cells))
            p = None
            release()
        (on, qn, cn), (of, qf, cf) = got
        # the near twin against the reference and the fp16 entry: the step with request 0's last key as the pool holds it
        last = [x.reshape(bk, c.hkv, hs)[(n0 - 1) % bk] for x in cn[(0, (n0 - 1) // bk)]]
        assert all(NAN8 not in x for x in last)
        kc, vc = c.kc.copy(), c.vc.copy()
        kc[0, n0 - 1], vc[0, n0 - 1] = last
        c2 = Rag8(nso, FL.HN, FL.HKV, hs, FL.PAGED_CAP[bk], FL.BLOCK_Q, FL.BLOCK_KV[bk], codes=lambda shape: (kc, vc))
        assert np.array_equal(c2.q, c.q)
        check_rag(nso, "far addresses, near twin: block_paged_f8 after append_paged_seq_f8 mode %d" % mode, c2, on)
        half = run_block(L, pkg, c2, pools_pair(c2, bk, PM)[1])[0]
        rows = slice(c.start[0], c.start[-1])
        e = nso.rel_l2(on[rows], half[rows])
        assert e < 2e-4, e
        assert same_bits(on, of) and same_bits(qn, qf) and not same_bits(qn, q1.cpu().numpy())
        assert all(same_bits(cn[key][x], cf[key][x]) for key in cn for x in (0, 1))
    finally:
        p = tmp = None
        release()

"""Prompt-sized query blocks over an FP8 (E4M3) paged KV cache: ns_hip_attn_prefill_paged_f8 (the F8 instantiations of the 128-row matrix-core kernel).
docs/kernels/attention.md, "Prompt-sized query blocks over an FP8 paged cache".

Inputs: K / V are drawn, then rounded to E4M3 of x / scale with a power-of-two scale; c.kc / c.vc are the codes and c.k / c.v the CODES' VALUES in fp16 (no
scale baked in), so the fp16 entry takes the same argument block — K_sc, V_sc and every stride number — with only the pool pointers changed.  The uint8
pools (Pools8) hold 0x7f — NaN — behind every live length and in spare blocks, with a guard block on either side; dst is preset to 7.0 with lead and tail
rows.  Every case is checked (1) per request and per row against the fp64 attention over the decoded values (model64_rows without its roundings) through
check_rag, the fp16 module's bound — rel_l2 < 1e-3 and per row max(2^-11, 4 d), d the distance between the rounding model and the reference — and (2) BIT
FOR BIT against ns_hip_attn_prefill_paged over fp16 pools of the codes' values under the same table: the decode is exact, the LDS images coincide and the
argument blocks coincide, so equality is derived, not measured."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_attn_block_paged import LEAD, Rag, block_args, check_rag
from test_gpu_attn_block_paged_f8 import all_codes
from test_gpu_attn_paged import delta
from test_gpu_attn_paged_f8 import FarPools8, Pools8, decoded, pools_pair, to_codes
from test_gpu_attn_prefill_paged import Step, model64_rows, prefill_stats, run_prefill
from test_gpu_attn_rows import ALIBI, CAUSAL, HM, PM, TANH, attn_stats, stream_ptr

pytestmark = pytest.mark.gpu
SCALES = (1.0, 0.125, 0.125, 1.0)


def prefill8_stats(L):
    out = (C.c_ulonglong * 6)()
    L.ns_hip_attn_prefill_paged_f8_stats(out)
    return list(out)


class Step8(Step):
    """Step over E4M3 codes (drawn and rounded, or given by `codes`); reference and rounding model of every request: model64_rows over the codes' values
    with the pools' scales in `scales`.  nso None: inputs only."""

    def __init__(self, nso, hn, hkv, hs, cap, qlens, kvlens, flags=CAUSAL, scales=SCALES, seed=0, scale=None, partition=None, codes=None):
        Rag.__init__(self, None, hn, hkv, hs, cap, qlens, kvlens, flags, scales, seed)
        self.scale, self.partition, self.lens = float(scale) if scale is not None else self.scale, partition, self.kvlens
        self.kc, self.vc = codes(self.k.shape) if codes else (to_codes(self.k.astype(np.float32), scales[1]), to_codes(self.v.astype(np.float32), scales[2]))
        self.k, self.v = decoded(self.kc, 1.0), decoded(self.vc, 1.0)
        assert np.array_equal(to_codes(self.k, 1.0), self.kc) and np.array_equal(to_codes(self.v, 1.0), self.vc)  # the fp16 copy is exact
        all_heads, off = partition if partition else (hn, 0)
        for b in range(self.bs if nso else 0):
            see, end = self.seeing(b), self.start[b] + self.qlens[b]
            if see:
                x = (self.q[end - see:end][None], self.k[b:b + 1, :self.kvlens[b]], self.v[b:b + 1, :self.kvlens[b]], self.scale, flags, scales)
                self.ref[b], self.model[b] = model64_rows(*x, False, all_heads, off), model64_rows(*x, True, all_heads, off)


class F8Entry:
    """run_prefill's library handle with the FP8 entry in the fp16 entry's place"""

    def __init__(self, L):
        self.ns_hip_attn_prefill_paged, self.ns_hip_attn_set_head_partition = L.ns_hip_attn_prefill_paged_f8, L.ns_hip_attn_set_head_partition


def run8(L, pkg, c, p, **kw):
    return run_prefill(F8Entry(L), pkg, c, p, **kw)


def same(x, y):
    return np.array_equal(x.view(np.uint32), y.view(np.uint32))


# name: ((heads, kv heads, head size, capacity, q lens, kv lens, flags), Step8's keywords, block_keys, layout, stats delta [64, 128, 256, biased, padded, refused])
BOUNDARY = (4, 2, 64, 512, [130, 1, 0, 17], [300, 17, 0, 64], CAUSAL)  # two query blocks, whole tiles and last tiles, a decode row, an idle request
CASES = {
    "a_query_block_boundary_bk16": (BOUNDARY, {}, 16, PM, [1, 0, 0, 0, 0, 0]),    # four pages per tile: the 16-row group fills a page
    "a_query_block_boundary_bk256": (BOUNDARY, {}, 256, PM, [1, 0, 0, 0, 0, 0]),
    "b_head_size_128_from_position_0": ((2, 2, 128, 256, [129], [129], CAUSAL), {}, 64, PM, [0, 1, 0, 0, 0, 0]),
    "c_more_rows_than_keys": ((4, 2, 64, 256, [10, 5, 3, 140], [4, 5, 0, 130], CAUSAL), dict(seed=1), 16, PM, [1, 0, 0, 0, 0, 0]),
    "d_not_causal_head_major": ((4, 2, 128, 1024, [150, 3], [1000, 65], 0), {}, 128, HM, [0, 1, 0, 0, 0, 0]),
    "e_head_size_48": ((4, 2, 48, 256, [33, 130], [100, 200], CAUSAL), {}, 16, PM, [1, 0, 0, 0, 1, 0]),
    "e_head_size_80": ((4, 2, 80, 256, [33, 130], [100, 200], CAUSAL), {}, 32, HM, [0, 1, 0, 0, 1, 0]),
    "e_head_size_96_alibi_partition": ((8, 2, 96, 256, [40], [129], CAUSAL | ALIBI), dict(partition=(16, 8)), 64, PM, [0, 1, 0, 1, 1, 0]),
    "f_tanh_cap": ((4, 4, 128, 256, [131, 2], [256, 2], CAUSAL | TANH), dict(scale=3.0 / np.sqrt(128.0)), 16, PM, [0, 1, 0, 1, 0, 0]),  # (scores large enough to move the output)
    "f_negative_score_scale": ((4, 2, 64, 256, [70, 1], [130, 64], CAUSAL), dict(scale=-0.125), 16, PM, [1, 0, 0, 1, 0, 0]),
    "g_all_254_finite_codes": ((4, 2, 64, 256, [16], [100], CAUSAL), dict(scales=(2.0 ** -6, 0.25, 2.0, 4.0), codes=all_codes), 16, PM, [1, 0, 0, 0, 0, 0]),
}
_steps = {}


def step8(nso, name):
    key = repr((CASES[name][0], sorted((k, repr(v)) for k, v in CASES[name][1].items())))
    if key not in _steps:
        _steps[key] = Step8(nso, *CASES[name][0], **CASES[name][1])
    return _steps[key]


def good_run(L, pkg, c, bk, layout, **kw):
    """the FP8 entry and the fp16 entry over one table: (FP8 output, fp16 output, FP8 pools); the housekeeping every case shares is asserted here"""
    p8, p16 = pools_pair(c, bk, layout, **kw)
    f0, others = prefill_stats(L), attn_stats(L)
    out = run8(L, pkg, c, p8)[0]
    assert prefill_stats(L) == f0 and attn_stats(L) == others  # the fp16 entry's counters do not move on the FP8 call
    assert p8.guards_intact() and p8.unchanged()
    return out, run_prefill(L, pkg, c, p16)[0], p8


@pytest.mark.parametrize("name", list(CASES))
def test_f8_prompt_blocks_against_the_reference_and_the_bits_of_the_fp16_entry(L, pkg, nso, name):
    _, _, bk, layout, want = CASES[name]
    c = step8(nso, name)
    s0 = prefill8_stats(L)
    out, half, _ = good_run(L, pkg, c, bk, layout)
    assert delta(s0, prefill8_stats(L)) == want
    assert np.all(np.isfinite(out)), name  # no byte behind a live length, no spare block was consumed
    check_rag(nso, "f8 " + name, c, out)
    assert same(out, half), name


@pytest.mark.parametrize("edge", ["junk_behind_the_live_blocks", "bad_id_minus_one", "bad_id_pool_blocks", "strided_unaligned_dst_with_dst16"])
def test_contract_edges(L, pkg, nso, edge):
    """case (a), blocks of 16.  junk: every entry behind a request's live blocks holds -1, pool_blocks or the id of a NaN block — the same bits.  bad id:
    request 0's second block (live) is no block of the pool — the other requests' rows hold the same bits and everything is finite.  strided dst: rows of
    hs + 3 floats from a pointer one float behind a 16-byte boundary give the bits of the 16-byte stores, dst16 is the rounded output, the padding of
    every row and the rows of no request keep their 7.0.  Each run also holds the fp16 entry's bits under the same table."""
    c = step8(nso, "a_query_block_boundary_bk16")
    good = good_run(L, pkg, c, 16, PM)[0]

    def junk(p):
        spare = min(set(range(p.pool_blocks)) - set(p.table.ravel().tolist()))  # a block no request names: NaN codes throughout
        for b, n in enumerate(c.kvlens):
            first = -(-n // 16)
            p.table[b, first:] = [(-1, p.pool_blocks, spare)[j % 3] for j in range(p.ts - first)]

    def poison(p):
        p.table[0, 1] = -1 if edge == "bad_id_minus_one" else p.pool_blocks

    if edge == "junk_behind_the_live_blocks":
        out, half, p = good_run(L, pkg, c, 16, PM, table_edit=junk)
        assert p.table[2, 0] in (-1, p.pool_blocks) and same(out, good) and same(out, half)
    elif edge.startswith("bad_id"):
        out, half, _ = good_run(L, pkg, c, 16, PM, table_edit=poison)
        others = slice(c.start[1], None)
        assert np.all(np.isfinite(out)) and same(out[others], good[others]) and np.all(out[:LEAD] == 7.0) and same(out, half)
    else:
        p8 = pools_pair(c, 16, PM)[0]
        plain, p16, _ = run8(L, pkg, c, p8, dst16=True)
        out, o16, whole = run8(L, pkg, c, p8, dst16=True, dst_pad=3)
        live = slice(c.start[0], c.start[-1])
        assert same(plain, good) and same(out, good) and np.all(whole[..., c.hs:] == 7.0) and np.all(o16[..., c.hs:] == 7.0)
        assert np.array_equal(o16[live, :, :c.hs], out[live].astype(np.float16)) and np.array_equal(p16[live], plain[live].astype(np.float16))
        assert all(np.all(x[:LEAD] == 7.0) and np.all(x[c.start[-1]:] == 7.0) for x in (o16, p16))


def test_refusals_are_counted_and_write_nothing(L, pkg, nso):
    """the FP8 pool's refusals first (head size 40 in the pool's words), then the fp16 plan's: -1, the reason, stats [5], no launch, dst and pools as they were"""
    import torch
    c = step8(nso, "a_query_block_boundary_bk16")
    p = pools_pair(c, 16, PM)[0]
    dq = torch.from_numpy(c.q.copy()).cuda()
    dd = torch.full((c.rows, c.hn, c.hs), 7.0, device="cuda")
    ds = torch.tensor(c.start, dtype=torch.int32, device="cuda")
    dl = torch.tensor(c.kvlens, dtype=torch.int32, device="cuda")

    def call(step=p.block_step, start=True, **fields):
        a = block_args(pkg, c, p, dq.data_ptr(), dd.data_ptr(), 130, c.hs)
        for k, v in fields.items():
            setattr(a, k, v)
        return L.ns_hip_attn_prefill_paged_f8(C.byref(a), C.c_void_p(ds.data_ptr()) if start else None, C.c_void_p(dl.data_ptr()), 0, C.c_void_p(p.dt.data_ptr()),
                                              p.ts, 16, p.pool_blocks, step, None, stream_ptr())

    calls = [("FP8 paged cache: head_size must be a multiple of 16", dict(head_size=40)), ("head sizes above 128 are not served", dict(head_size=144)),
             ("strides must be multiples of 16", dict(step_k_sl=p.step_sl + 8)), ("block_step must be a multiple of 16", dict(step=p.block_step + 8)),
             ("pool bases must be 16-byte aligned", dict(K=p.kp + 8)), ("must be positive and finite", dict(K_sc=0.0)),
             ("must be positive and finite", dict(V_sc=float("inf"))), ("dQStart is null", dict(start=False))]
    s0, f0, a0 = prefill8_stats(L), prefill_stats(L), attn_stats(L)
    for n, (text, kw) in enumerate(calls):
        L.ns_hip_reset_error()
        assert call(**kw) == -1, text
        assert text in pkg.last_error(), (text, pkg.last_error())
        assert delta(s0, prefill8_stats(L)) == [0, 0, 0, 0, 0, n + 1]
    torch.cuda.synchronize()
    assert bool(torch.all(dd == 7.0)) and (prefill_stats(L), attn_stats(L)) == (f0, a0) and p.unchanged()
    L.ns_hip_reset_error()


def test_captured_step_replayed_on_new_contents(L, pkg, nso):
    """The entry captured ONCE on a side stream — no tmp, no scratch, no eager call of it on that stream in front — then replayed after the CONTENTS of
    dQStart, dKvLens, the table, Q and the pools changed (a chunk of 130 rows from position 0 beside a decode row; a decode row beside a chunk of 70 over
    200 keys, on another permutation of the blocks).  Every replay equals the same step run eagerly, bit for bit."""
    import torch
    hn, hkv, hs, cap, bk, max_q = 4, 2, 64, 256, 16, 130
    steps = [Step8(None, hn, hkv, hs, cap, [130, 1], [130, 77], seed=41), Step8(None, hn, hkv, hs, cap, [1, 70], [131, 200], seed=42)]
    pools = [Pools8(2, hkv, hs, cap, bk, PM, 50 + n).fill(s.kc, s.vc, s.kvlens) for n, s in enumerate(steps)]
    rows = max(s.rows for s in steps)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        p = pools[0].upload()  # the device buffers of the graph; their contents move to step n's below
        q = torch.zeros((rows, hn, hs), device="cuda")
        dst = torch.full((rows, hn, hs), 7.0, device="cuda")
        start, lens = torch.zeros(3, dtype=torch.int32, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda")
        a = block_args(pkg, steps[0], p, q.data_ptr(), dst.data_ptr(), max_q, hs)

        def move_to(n):
            s = steps[n]
            q.zero_()
            q[:s.rows].copy_(torch.from_numpy(s.q.copy()))
            dst.fill_(7.0)
            start.copy_(torch.tensor(s.start, dtype=torch.int32))
            lens.copy_(torch.tensor(s.kvlens, dtype=torch.int32))
            p.dk.copy_(torch.from_numpy(pools[n].k)), p.dv.copy_(torch.from_numpy(pools[n].v)), p.dt.copy_(torch.from_numpy(pools[n].table))

        def call():
            pkg.check(L.ns_hip_attn_prefill_paged_f8(C.byref(a), C.c_void_p(start.data_ptr()), C.c_void_p(lens.data_ptr()), 0, *p.table_args(), None, stream_ptr()))

        move_to(0)
        side.synchronize()
        s0 = prefill8_stats(L)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            call()
        assert delta(s0, prefill8_stats(L)) == [1, 0, 0, 0, 0, 0]
        for n, s in enumerate(steps):
            move_to(n)
            g.replay()
            side.synchronize()
            got = dst.cpu().numpy()
            move_to(n)
            call()
            side.synchronize()
            assert same(got, dst.cpu().numpy()), n
            live = got[s.start[0]:s.start[-1]]
            assert np.all(np.isfinite(live)) and not np.any(live == 7.0) and np.all(got[:LEAD] == 7.0) and np.all(got[s.start[-1]:] == 7.0), n
    torch.cuda.synchronize()


def test_far_pool_is_bit_equal_to_the_compact_twin(L, pkg, nso):
    """After the FP8 decode module's far test (FarPools8, placed by tests/tools/attn_far_layout.py): untouched pools of 2^20 + 40 blocks of 4096 bytes, the
    live blocks at their top plus block 2, 0x7f bytes in the first 64 blocks — where an offset truncated to 32 bits lands — and around the live ones.
    q lens [5, 40] over kv lens [70, 120], head size 128, blocks of 16: each request has one whole tile and one partial tile, so both address forms run
    far.  The far run holds the bits of the compact twin, which passes the check against the reference; no 0x7f byte is consumed or overwritten."""
    from test_gpu_attn_far_addresses import FL, need, release, same_bits
    hs, bk = 128, 16
    c = Step8(nso, FL.HN, FL.HKV, hs, FL.PAGED_CAP[bk], [5, 40], [70, 120], seed=31)
    live = [-(-n // bk) for n in c.kvlens]
    need(2 * ((1 << 32) + (1 << 20)))
    outs, p = [], None
    try:
        s0 = prefill8_stats(L)
        for blocks in (FL.pool_blocks("near", bk * c.hkv * hs, sum(live)) + 128, (1 << 20) + 40):
            p = FarPools8(blocks, c, bk, live)
            assert blocks < 1 << 20 or all(i == 2 or i * p.block_step >= 1 << 32 for i in p.ids.values())
            for b, n in enumerate(c.kvlens):
                p.put(b, c.kc[b, :n], c.vc[b, :n])
            outs.append(run8(L, pkg, c, p)[0])
            assert p.live()[1] and np.all(np.isfinite(outs[-1])), blocks
            p = None
            release()
        assert delta(s0, prefill8_stats(L)) == [0, 2, 0, 0, 0, 0]
        check_rag(nso, "far addresses, near twin: prefill_paged_f8", c, outs[0])
        assert same_bits(outs[1], outs[0])
    finally:
        p = None
        release()

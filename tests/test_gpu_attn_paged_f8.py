"""Decode over an FP8 (E4M3) paged KV cache: ns_hip_attn_decode_paged_f8, ns_hip_rope_qkv_append_paged_f8, ns_hip_kv_paged_store_f8
(docs/kernels/attention.md, "Decode over an FP8 paged cache").

Inputs: K / V are drawn as usual, then rounded to E4M3 of x / scale, scale a power of two — a case's fp16 arrays hold exactly code * scale, so the fp16
pools of ns_hip_attn_decode_paged hold the FP8 pools' values exactly.  Each attention case is checked (1) against the oracle per request through
check_case (the existing bound) and (2) against ns_hip_attn_decode_paged over those fp16 pools with the same table: rel_l2 < 2e-6, this project's figure
for two one-row kernels that split or order a context differently.  The uint8 pools hold 0x7f (NaN) in spare blocks, behind every live length and in
the rest of a last block; a guard block (0xA5) lies on either side.  The writers are checked bit for bit against torch's cast of the fp16 cells that
ns_hip_rope_qkv_append_paged / ns_hip_kv_paged_store write for the same inputs."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_attention_paths import rounding_model
from test_gpu_attn_far_addresses import FL, need, release, same_bits, tuning
from test_gpu_attn_paged import Pools, delta, family, run_paged
from test_gpu_attn_rows import ALIBI, CAUSAL, HM, PM, TANH, Case, attn_stats, check_case, model64, stream_ptr, strides, to_slabs

pytestmark = pytest.mark.gpu
GUARD8, NAN8 = 0xA5, 0x7F


def f8_stats(L):
    out = (C.c_ulonglong * 4)()
    L.ns_hip_attn_paged_f8_stats(out)
    return list(out)


def to_codes(x, scale):
    """numpy fp16 / fp32 -> E4M3 codes of x / scale by the stated rule (torch's cast: round to nearest even, subnormals, NaN -> 0x7f)"""
    import torch
    t = torch.clamp(torch.from_numpy(np.ascontiguousarray(x)).float() * (1.0 / np.float32(scale)), -448, 448)
    codes = t.to(torch.float8_e4m3fn).view(torch.uint8).numpy().copy()
    codes[np.isnan(np.asarray(x, np.float32))] = NAN8
    return codes


def decoded(codes, scale):
    import torch
    return (torch.from_numpy(codes.copy()).view(torch.float8_e4m3fn).float() * scale).numpy().astype(np.float16)


class Pools8(Pools):
    """Pools with one byte per element: self.k / self.v hold codes, NaN codes where the fp16 pools hold NaN"""

    def __init__(self, *a, **kw):
        Pools.__init__(self, *a, **kw)
        self.k, self.v = (np.full(x.shape, NAN8, np.uint8) for x in (self.k, self.v))
        for x in (self.k, self.v):
            x[0], x[-1] = GUARD8, GUARD8

    def fill(self, kc, vc, lens):
        for b, n in enumerate(lens):
            for j in range(-(-n // self.bk)):
                cnt = min(self.bk, n - j * self.bk)
                if 0 <= self.table[b, j] < self.pool_blocks:
                    self.cells(self.k, self.table[b, j], 0, cnt)[...] = kc[b, j * self.bk:j * self.bk + cnt]
                    self.cells(self.v, self.table[b, j], 0, cnt)[...] = vc[b, j * self.bk:j * self.bk + cnt]
        return self

    def upload(self):
        import torch
        self.dk, self.dv, self.dt = torch.from_numpy(self.k).cuda(), torch.from_numpy(self.v).cuda(), torch.from_numpy(self.table).cuda()
        self.kp, self.vp = self.dk.data_ptr() + self.block_step, self.dv.data_ptr() + self.block_step  # (behind the front guard)
        return self

    def download(self):
        return self.dk.cpu().numpy(), self.dv.cpu().numpy()

    def guards_intact(self):
        return all(np.all(x[0] == GUARD8) and np.all(x[-1] == GUARD8) for x in self.download())

    def unchanged(self):
        return all(np.array_equal(x, y) for x, y in zip(self.download(), (self.k, self.v)))


# name: (batch, heads, kv heads, head size, capacity, lengths, flags, block layout, block_keys, family, (Q_sc, K scale, V scale, dst_sc))
ONE = (1.0, 0.125, 0.125, 1.0)
CASES = {
    "ring_8key_requests": (4, 4, 4, 128, 512, [1, 17, 300, 512], CAUSAL, PM, 16, "ring", ONE),  # the last request of a range partly live
    "ring_16key_block16": (4, 8, 2, 64, 1024, [31, 33, 129, 1024], CAUSAL, PM, 16, "ring", ONE),  # a request straddles two blocks
    "ring_16key_block64": (4, 8, 2, 64, 1024, [31, 33, 129, 1024], CAUSAL, PM, 64, "ring", ONE),
    "ring_hs80_idle_lanes": (4, 4, 4, 80, 512, [1, 17, 300, 512], CAUSAL, PM, 16, "ring", ONE),
    "ring_hs48_idle_lanes": (2, 4, 2, 48, 256, [33, 256], CAUSAL, PM, 32, "ring", ONE),
    "alibi_and_idle_slot": (3, 8, 1, 128, 256, [200, 0, 65], CAUSAL | ALIBI, PM, 16, "ring", ONE),
    "head_major": (4, 4, 4, 128, 512, [1, 17, 300, 512], CAUSAL, HM, 16, "ring", ONE),
    "regs_32": (4, 4, 4, 32, 256, [1, 32, 33, 256], CAUSAL, PM, 32, "registers", ONE),
    "regs_256": (4, 4, 4, 256, 256, [1, 32, 33, 256], CAUSAL, HM, 32, "registers", ONE),
    "many_ranges": (8, 8, 2, 128, 4096, [1, 4096, 2048, 17, 3000, 129, 1024, 700], CAUSAL, PM, 128, "ring", ONE),
    "many_ranges_inlaunch": (8, 8, 2, 128, 4096, [1, 4096, 2048, 17, 3000, 129, 1024, 700], CAUSAL, PM, 128, "ring", ONE),
    "tanh_cap": (4, 4, 4, 128, 512, [1, 17, 300, 512], CAUSAL | TANH, PM, 16, "ring", ONE),
    "far_shape": (2, FL.HN, FL.HKV, 128, FL.PAGED_CAP[16], FL.PAGED_LENS[16], CAUSAL, PM, 16, "ring", ONE),  # (section 7's inputs, compact)
    "scales": (4, 4, 4, 128, 512, [1, 17, 300, 512], CAUSAL, PM, 16, "ring", (0.5, 0.25, 2.0, 4.0)),
}
_cases = {}


def f8_case(nso, name):
    """Case of tests/test_gpu_attn_rows.py over E4M3-representable K / V (c.k / c.v = code * scale in fp16, c.kc / c.vc the codes), made once per
    shape; c.scales is what the FP16 entry gets (the pools' scales are in its values), c.f8_scales what the FP8 entry gets."""
    bs, hn, hkv, hs, cap, lens, flags = CASES[name][:7]
    qs, ks, vs, ds = CASES[name][10]
    key = (bs, hn, hkv, hs, cap, tuple(lens), flags, qs, ks, vs, ds)
    if key in _cases:
        return _cases[key]
    c = Case.__new__(Case)
    c.bs, c.hn, c.hkv, c.hs, c.cap, c.lens, c.flags, c.scales, c.f8_scales = bs, hn, hkv, hs, cap, list(lens), flags, (qs, 1.0, 1.0, ds), (qs, ks, vs, ds)
    rng = np.random.default_rng(hs * 7 + cap + bs)
    c.q = rng.standard_normal((bs, 1, hn, hs)).astype(np.float32)
    c.kc, c.vc = to_codes(rng.standard_normal((bs, cap, hkv, hs)), ks), to_codes(rng.standard_normal((bs, cap, hkv, hs)), vs)
    c.k, c.v = decoded(c.kc, ks), decoded(c.vc, vs)
    assert np.array_equal(to_codes(c.k, ks), c.kc) and np.array_equal(to_codes(c.v, vs), c.vc)  # the fp16 copy is exact
    c.scale = float(1.0 / np.sqrt(hs))
    c.ref, c.model = {}, {}
    for b, n in enumerate(lens):
        if n:
            qb, kb, vb = c.q[b:b + 1], c.k[b:b + 1, :n], c.v[b:b + 1, :n]
            if flags & (ALIBI | TANH):
                c.model[b] = model64(qb, kb, vb, c.scale * qs, flags, True) / ds
                c.ref[b] = model64(qb, kb, vb, c.scale * qs, flags, False) / ds if flags & TANH else nso.attn_ref(qb, kb, vb, c.scale, flags, scales=c.scales)
            else:
                c.ref[b], c.model[b] = nso.attn_ref(qb, kb, vb, c.scale, flags, scales=c.scales), rounding_model(qb, kb, vb, c.scale, flags, c.scales)
    _cases[key] = c
    return c


def pools_pair(c, bk, layout, table_edit=None, seed=5):
    """the FP8 pools and the fp16 pools of the decoded values under one table"""
    p8, p16 = Pools8(c.bs, c.hkv, c.hs, c.cap, bk, layout, seed), Pools(c.bs, c.hkv, c.hs, c.cap, bk, layout, seed)
    if table_edit:
        table_edit(p8), table_edit(p16)
    assert np.array_equal(p8.table, p16.table)
    return p8.fill(c.kc, c.vc, c.lens).upload(), p16.fill(c.k, c.v, c.lens).upload()


def run_f8(L, pkg, c, p, bias=1, expect=0, q=None, **edit):
    """ns_hip_attn_decode_paged_f8 of case c over the uploaded pools p; returns dst [bs][1][hn][hs] (started as 7.0)"""
    import torch
    dq = torch.from_numpy((c.q if q is None else q).copy()).cuda()
    dd = torch.full((c.bs, 1, c.hn, c.hs), 7.0, device="cuda")
    dl = torch.tensor([n - bias for n in c.lens], dtype=torch.int32, device="cuda")
    a = pkg.attn_args(dq.data_ptr(), p.kp, p.vp, dd.data_ptr(), c.bs, c.hn, c.hkv, c.hs, 1, c.cap, c.scale, c.flags)
    a.Q_sc, a.K_sc, a.V_sc, a.dst_sc = c.f8_scales
    a.step_k_sl = a.step_v_sl = p.step_sl
    a.step_k_head_num = a.step_v_head_num = p.step_head
    table = [C.c_void_p(p.dt.data_ptr()), p.ts, p.bk, p.pool_blocks, p.block_step]
    for k, v in edit.items():
        if k in ("kp", "K_sc", "step_k_sl"):
            setattr(a, {"kp": "K"}.get(k, k), v)
        else:
            table[("table", "ts", "bk", "blocks", "step").index(k)] = v
    rc = L.ns_hip_attn_decode_paged_f8(C.byref(a), C.c_void_p(dl.data_ptr()), bias, *table, None, stream_ptr())
    assert rc == expect, pkg.last_error()
    torch.cuda.synchronize()
    return dd.cpu().numpy()


# ---- 1. attention: against the oracle and against the fp16 entry on the decoded pools ---------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_f8_attention_against_the_reference_and_the_fp16_entry(L, pkg, nso, name):
    layout, bk, want = CASES[name][7:10]
    c = f8_case(nso, name)
    p8, p16 = pools_pair(c, bk, layout)
    L.ns_hip_set_tuning(b"attn_inlaunch", int(name.endswith("inlaunch")))
    try:
        g0, a0 = f8_stats(L), attn_stats(L)
        out = run_f8(L, pkg, c, p8)
        g1, a1 = f8_stats(L), attn_stats(L)
        half = run_paged(L, pkg, c, p16)
    finally:
        L.ns_hip_set_tuning(b"attn_inlaunch", 0)
    assert family(delta(g0, g1)) == want and sum(delta(a0, a1)) == 1, (delta(g0, g1), delta(a0, a1))
    if name.startswith("many_ranges"):
        assert delta(g0, g1)[2] == (0 if name.endswith("inlaunch") else 1)  # attn_merge_kernel<true>, or the tickets
    assert np.all(np.isfinite(out)), name  # no byte behind a live length, no spare block was consumed
    check_case(nso, "f8 %s" % name, c, out)
    e = nso.rel_l2(out, half)
    print("ATTN_PAGED_F8 %s: rel_l2 against ns_hip_attn_decode_paged %.3g" % (name, e))
    assert e < 2e-6, (name, e)
    assert p8.guards_intact() and p8.unchanged()


# ---- 2. table entries that are not blocks of the pool, and junk behind the live blocks ---------------------------------------------------------------
@pytest.mark.parametrize("name", ["ring_8key_requests", "ring_16key_block16", "regs_256"])
def test_bad_and_junk_table_entries(L, pkg, nso, name):
    """request 2's second block — live — gets an id outside the pool: every other request's row holds the bits of the clean run; then every entry
    behind a request's live blocks gets junk (ids outside the pool and the id of a NaN block): all rows hold them."""
    layout, bk = CASES[name][7:9]
    c = f8_case(nso, name)
    good = run_f8(L, pkg, c, pools_pair(c, bk, layout)[0])

    def poison(p):
        p.table[2, 1] = p.pool_blocks

    def junk(p):
        for b, n in enumerate(c.lens):
            p.table[b, -(-n // bk):] = [(-1, p.pool_blocks, int(p.table[0, 0]), 0x7fffffff)[j % 4] for j in range(p.ts - -(-n // bk))]

    p = pools_pair(c, bk, layout, table_edit=poison)[0]
    out = run_f8(L, pkg, c, p)
    assert c.lens[2] > bk and np.array_equal(out[[0, 1, 3]].view(np.uint32), good[[0, 1, 3]].view(np.uint32)) and p.guards_intact()
    assert np.array_equal(run_f8(L, pkg, c, pools_pair(c, bk, layout, table_edit=junk)[0]).view(np.uint32), good.view(np.uint32))


# ---- 3. the writers: bit for bit the cast of what the fp16 writers write ------------------------------------------------------------------------------
def special(x, scale):
    """values above 448 * scale, below the smallest subnormal, at a rounding tie, and a NaN"""
    x.reshape(-1)[:6] = np.array([500.0, -1000.0, 2.0 ** -11, 2.0 ** -10, 3 * 2.0 ** -10, np.nan], np.float32) * scale
    return x


@pytest.mark.parametrize("layout", [PM, HM])
@pytest.mark.parametrize("mode,n_dims", [(0, 64), (2, 32)])
def test_append_and_store_write_the_cast_of_the_fp16_cells(L, pkg, mode, n_dims, layout):
    """5 rows (one idle, one through an id outside the pool), 4 / 2 heads of 64, block 16.  The FP8 append's cells are the cast of the fp16 append's, Q
    holds the same bits, nothing else changes; the FP8 store of a slab holding the fp16 append's rows (aligned, then one element off: the element form)
    gives the same pool."""
    import torch
    rows, heads, hkv, hs, cap, bk, ks, vs = 5, 4, 2, 64, 256, 16, 0.25, 2.0
    pos = [0, 15, 16, 255, -1]
    rng = np.random.default_rng(mode * 100 + n_dims)
    q, k = rng.standard_normal((rows, heads, hs)).astype(np.float32), special(rng.standard_normal((rows, hkv, hs)).astype(np.float32), ks)
    v = special(rng.standard_normal((rows, hkv, hs)).astype(np.float32), vs)
    dk, dv, dpos, st = torch.from_numpy(k).cuda(), torch.from_numpy(v).cuda(), torch.tensor(pos, dtype=torch.int32, device="cuda"), stream_ptr()
    p16, p8 = Pools(rows, hkv, hs, cap, bk, layout, seed=9), Pools8(rows, hkv, hs, cap, bk, layout, seed=9)
    for p in (p16, p8):
        p.table[2, 1] = -1  # row 2 (position 16) has no block
        p.upload()
    q16, q8 = torch.from_numpy(q).cuda(), torch.from_numpy(q).cuda()
    rope = (dpos.data_ptr(), cap, n_dims, mode, 10000.0, 0.75, 0.0, 1.1)
    pkg.check(L.ns_hip_rope_qkv_append_paged(q16.data_ptr(), dk.data_ptr(), dv.data_ptr(), p16.kp, p16.vp, rows, heads, hkv, hs, *rope, *p16.table_args(),
                                             p16.step_sl, p16.step_head, st))
    pkg.check(L.ns_hip_rope_qkv_append_paged_f8(q8.data_ptr(), dk.data_ptr(), dv.data_ptr(), p8.kp, p8.vp, rows, heads, hkv, hs, *rope, *p8.table_args(),
                                                p8.step_sl, p8.step_head, ks, vs, st))
    torch.cuda.synchronize()
    assert torch.equal(q8.view(torch.int32), q16.view(torch.int32)) and torch.equal(q8[[2, 4]], torch.from_numpy(q[[2, 4]]).cuda())
    h = [x.view(np.float16) for x in p16.download()]
    want = [p8.k.copy(), p8.v.copy()]
    slab = [np.zeros((1, cap, hkv, hs), np.float16) for _ in range(2)]
    for r, n in ((0, 0), (1, 15), (3, 255)):
        for x, w, s, sc in zip(h, want, slab, (ks, vs)):
            cell = p16.cells(x, p16.table[r, n // bk], n % bk, 1)
            p8.cells(w, p8.table[r, n // bk], n % bk, 1)[...] = to_codes(cell, sc)
            s[0, n] = cell[0]
    got = p8.download()
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])  # (guards and every idle cell included)
    assert NAN8 in p8.cells(got[1], p8.table[0, 0], 0, 1) and 0x7E in p8.cells(got[1], p8.table[0, 0], 0, 1)
    # the store: request r's row of the table, the slab row its position — the same tokens, the same pools
    for pad in (8, 7):  # the slab 16-byte aligned (vector form), then 14 bytes into an allocation (element form)
        s8 = Pools8(rows, hkv, hs, cap, bk, layout, seed=9).upload()
        _, s_sl, s_head = strides(layout, cap, hkv, hs)
        dsl = [torch.cat([torch.zeros(pad, dtype=torch.float16), to_slabs(x, layout).cpu().reshape(-1)]).cuda() for x in slab]
        for r, n in ((0, 0), (1, 15), (3, 255)):
            pkg.check(L.ns_hip_kv_paged_store_f8(dsl[0].data_ptr() + 2 * pad, dsl[1].data_ptr() + 2 * pad, s_sl, s_head, n, 1, hkv, hs, s8.kp, s8.vp,
                                                 C.c_void_p(s8.dt.data_ptr() + 4 * r * s8.ts), s8.ts, bk, s8.pool_blocks, s8.block_step, s8.step_sl,
                                                 s8.step_head, ks, vs, st))
        torch.cuda.synchronize()
        assert all(np.array_equal(x, y) for x, y in zip(s8.download(), got)), pad


# ---- 4. end to end: token by token against one store -----------------------------------------------------------------------------------------------
def test_forty_appended_tokens_equal_one_stored_prompt(L, pkg, nso):
    """one request, 4 / 2 heads of 128, block 16: 40 tokens appended one by one with attention after each; at the last step the output equals one call over
    a pool that the store filled from the fp16 slab ns_hip_rope_qkv_append_paged wrote for the same tokens — bit for bit, the pools as well."""
    import torch
    hn, hkv, hs, cap, bk, n, ks, vs = 4, 2, 128, 64, 16, 40, 0.0625, 0.125
    rng = np.random.default_rng(40)
    q, k, v = (torch.from_numpy(rng.standard_normal((n, h, hs)).astype(np.float32)).cuda() for h in (hn, hkv, hkv))
    pa, ps, p16 = Pools8(1, hkv, hs, cap, bk, PM, seed=2).upload(), Pools8(1, hkv, hs, cap, bk, PM, seed=2).upload(), Pools(1, hkv, hs, cap, bk, PM, seed=2).upload()
    st, dd, ds = stream_ptr(), torch.zeros((1, 1, hn, hs), device="cuda"), torch.zeros((1, 1, hn, hs), device="cuda")

    def attend(p, qrow, dst, length):
        a = pkg.attn_args(qrow.data_ptr(), p.kp, p.vp, dst.data_ptr(), 1, hn, hkv, hs, 1, cap, float(hs ** -0.5), CAUSAL)
        a.K_sc, a.V_sc, a.step_k_sl, a.step_v_sl, a.step_k_head_num, a.step_v_head_num = ks, vs, p.step_sl, p.step_sl, p.step_head, p.step_head
        pkg.check(L.ns_hip_attn_decode_paged_f8(C.byref(a), C.c_void_p(length.data_ptr()), 0, *p.table_args(), None, st))

    for t in range(n):
        pos, qa, q16 = torch.tensor([t], dtype=torch.int32, device="cuda"), q[t:t + 1].clone(), q[t:t + 1].clone()
        rope = (pos.data_ptr(), cap, hs, 0, 10000.0, 1.0, 0.0, 1.0)
        pkg.check(L.ns_hip_rope_qkv_append_paged_f8(qa.data_ptr(), k[t].data_ptr(), v[t].data_ptr(), pa.kp, pa.vp, 1, hn, hkv, hs, *rope, *pa.table_args(),
                                                    pa.step_sl, pa.step_head, ks, vs, st))
        pkg.check(L.ns_hip_rope_qkv_append_paged(q16.data_ptr(), k[t].data_ptr(), v[t].data_ptr(), p16.kp, p16.vp, 1, hn, hkv, hs, *rope, *p16.table_args(),
                                                 p16.step_sl, p16.step_head, st))
        attend(pa, qa, dd, pos + 1)
    # the fp16 pool, block by block, is the prompt's slab: store it through the same table
    for j in range(-(-n // bk)):
        off = 2 * int(p16.table[0, j]) * p16.block_step
        pkg.check(L.ns_hip_kv_paged_store_f8(p16.kp + off, p16.vp + off, hkv * hs, hs, 0, min(bk, n - j * bk), hkv, hs, ps.kp, ps.vp,
                                             C.c_void_p(ps.dt.data_ptr() + 4 * j), 1, bk, ps.pool_blocks, ps.block_step, ps.step_sl, ps.step_head, ks, vs, st))
    attend(ps, qa, ds, pos + 1)
    torch.cuda.synchronize()
    assert torch.equal(pa.dk, ps.dk) and torch.equal(pa.dv, ps.dv) and torch.equal(dd, ds) and bool(torch.all(torch.isfinite(dd)))


# ---- 5. one captured step replayed on other contents ---------------------------------------------------------------------------------------------
def test_captured_step_replayed_on_other_contents(L, pkg, nso):
    """{append; attention} captured once on a side stream (after one eager call, tmp given), replayed on other lengths, table, Q and pools: each replay
    equals the same step run eagerly on a twin, bit for bit (output, Q, pools)."""
    import torch
    bs, hn, hkv, hs, cap, bk, ks, vs = 2, 8, 8, 128, 512, 16, 0.125, 0.125
    side = torch.cuda.Stream()
    ws_bytes = L.bestla_fusion_attn_workspace_size(C.byref(pkg.AttnShape(bs, hn, hkv, hs, 1, cap)))
    with torch.cuda.stream(side):
        qin, kin, vin = (torch.zeros((bs, h, hs), device="cuda") for h in (hn, hkv, hkv))

        class State:
            def __init__(self):
                self.p = Pools8(bs, hkv, hs, cap, bk, PM, seed=11).upload()
                self.pos, self.q = torch.zeros(bs, dtype=torch.int32, device="cuda"), torch.zeros_like(qin)
                self.dst, self.ws = torch.full((bs, 1, hn, hs), 7.0, device="cuda"), torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
                self.a = pkg.attn_args(self.q.data_ptr(), self.p.kp, self.p.vp, self.dst.data_ptr(), bs, hn, hkv, hs, 1, cap, float(hs ** -0.5), CAUSAL)
                self.a.K_sc, self.a.V_sc, self.a.tmp = ks, vs, self.ws.data_ptr()
                self.a.step_k_sl = self.a.step_v_sl = self.p.step_sl
                self.a.step_k_head_num = self.a.step_v_head_num = self.p.step_head

            def load(self, codes, table, pos):
                """other contents: every cell of the pools a valid code, a new table, new positions"""
                self.p.dk.view(-1)[self.p.block_step:-self.p.block_step] = codes[0]
                self.p.dv.view(-1)[self.p.block_step:-self.p.block_step] = codes[1]
                self.p.dt.copy_(table)
                self.pos.copy_(pos)

            def step(self):
                st, p = stream_ptr(), self.p
                self.q.copy_(qin)
                pkg.check(L.ns_hip_rope_qkv_append_paged_f8(self.q.data_ptr(), kin.data_ptr(), vin.data_ptr(), p.kp, p.vp, bs, hn, hkv, hs, self.pos.data_ptr(), cap,
                                                            hs, 0, 10000.0, 1.0, 0.0, 1.0, *p.table_args(), p.step_sl, p.step_head, ks, vs, st))
                pkg.check(L.ns_hip_attn_decode_paged_f8(C.byref(self.a), C.c_void_p(self.pos.data_ptr()), 1, *p.table_args(), None, st))

        State().step()
        graphed, eager = State(), State()
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            graphed.step()
        for s, pos in enumerate(([0, 130], [511, 47], [300, 301])):
            gen = torch.Generator(device="cuda").manual_seed(s)
            for x in (qin, kin, vin):
                x.copy_(torch.randn(x.shape, device="cuda", generator=gen))
            n = graphed.p.pool_blocks * graphed.p.block_step
            codes = [torch.randint(0, 0x78, (n,), device="cuda", generator=gen, dtype=torch.uint8) | (torch.randint(0, 2, (n,), device="cuda", generator=gen, dtype=torch.uint8) << 7) for _ in range(2)]
            table = torch.randperm(graphed.p.pool_blocks, device="cuda", generator=gen)[:bs * graphed.p.ts].reshape(bs, -1).int()
            for x in (graphed, eager):
                x.load(codes, table, torch.tensor(pos, dtype=torch.int32))
            g.replay()
            eager.step()
            side.synchronize()
            assert torch.equal(graphed.dst, eager.dst) and torch.equal(graphed.q, eager.q) and torch.equal(graphed.p.dk, eager.p.dk), s
            assert torch.equal(graphed.p.dv, eager.p.dv) and bool(torch.all(torch.isfinite(graphed.dst))) and graphed.p.guards_intact(), s
    torch.cuda.synchronize()


# ---- 6. refusals: counted, nothing written ---------------------------------------------------------------------------------------------------------------
def test_refusals_are_counted_and_write_nothing(L, pkg, nso):
    import torch
    c = f8_case(nso, "ring_8key_requests")
    p = pools_pair(c, 16, PM)[0]
    calls = [("block table is null", dict(table=None)), ("power of two from 16 to 256", dict(bk=48)), ("pool_blocks must be at least 1", dict(blocks=0)),
             ("must equal table_stride * block_keys", dict(ts=p.ts - 1)), ("do not fit inside block_step", dict(step=p.block_step - 16)),
             ("block_step must be a multiple of 16", dict(step=p.block_step + 8)), ("pool bases must be 16-byte aligned", dict(kp=p.kp + 8)),
             ("strides must be multiples of 16", dict(step_k_sl=p.step_sl + 8)), ("must be positive and finite", dict(K_sc=0.0)),
             ("must be positive and finite", dict(K_sc=float("inf")))]
    g0, a0 = f8_stats(L), attn_stats(L)
    for n, (text, kw) in enumerate(calls):
        L.ns_hip_reset_error()
        out = run_f8(L, pkg, c, p, expect=-1, **kw)
        assert text in pkg.last_error() and np.all(out == 7.0) and delta(g0, f8_stats(L)) == [0, 0, 0, n + 1], (text, pkg.last_error())
    t, pos = torch.zeros(8192, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda")
    for kw in (dict(ks=0.0), dict(ks=-1.0), dict(vs=float("nan")), dict(step=p.block_step + 8), dict(kp=p.kp + 4)):
        ks, vs, step, kp = kw.get("ks", 1.0), kw.get("vs", 1.0), kw.get("step", p.block_step), kw.get("kp", p.kp)
        L.ns_hip_reset_error()
        assert L.ns_hip_rope_qkv_append_paged_f8(t.data_ptr(), t.data_ptr(), t.data_ptr(), kp, p.vp, 2, c.hn, c.hkv, c.hs, pos.data_ptr(), c.cap, c.hs, 0, 10000.0,
                                                 1.0, 0.0, 1.0, C.c_void_p(p.dt.data_ptr()), p.ts, 16, p.pool_blocks, step, p.step_sl, p.step_head, ks, vs,
                                                 stream_ptr()) == -1 and "rope_qkv_append_paged_f8" in pkg.last_error()
        assert L.ns_hip_kv_paged_store_f8(t.data_ptr(), t.data_ptr(), c.hkv * c.hs, c.hs, 0, 4, c.hkv, c.hs, kp, p.vp, C.c_void_p(p.dt.data_ptr()), p.ts, 16,
                                          p.pool_blocks, step, p.step_sl, p.step_head, ks, vs, stream_ptr()) == -1 and "kv_paged_store_f8" in pkg.last_error()
    torch.cuda.synchronize()
    assert attn_stats(L) == a0 and p.unchanged() and bool(torch.all(t == 0))
    L.ns_hip_reset_error()


# ---- 7. a pool just over 2^32 bytes ---------------------------------------------------------------------------------------------------------------------
class FarPools8:
    """K / V pools of position-major blocks placed by tests/tools/attn_far_layout.py: UNTOUCHED allocations of `blocks` blocks, the live blocks at the
    top (every second one) plus block 2.  0x7f bytes: the live blocks' dead cells, their neighbours (the top 64 blocks), and the first 64 blocks —
    block 0, which entries behind a live length name, and where the offset of a block above 2^32 bytes lands when truncated to 32 bits."""

    def __init__(self, blocks, c, bk, live):
        import torch
        self.bk, self.ts, self.pool_blocks, self.block_step, self.step_sl, self.step_head = bk, c.cap // bk, blocks, bk * c.hkv * c.hs, c.hkv * c.hs, c.hs
        self.table, self.ids = FL.place(live, self.ts, blocks)
        self.dk, self.dv = (torch.empty(blocks * self.block_step, dtype=torch.uint8, device="cuda") for _ in range(2))
        for x in (self.dk, self.dv):
            x[:64 * self.block_step].fill_(NAN8), x[-64 * self.block_step:].fill_(NAN8)
        self.dt, self.kp, self.vp = torch.from_numpy(self.table).cuda(), self.dk.data_ptr(), self.dv.data_ptr()

    def table_args(self):
        return C.c_void_p(self.dt.data_ptr()), self.ts, self.bk, self.pool_blocks, self.block_step

    def put(self, b, kc, vc):
        """the codes of request b's first keys (numpy [n][hkv][hs]) to the cells its table row names"""
        import torch
        for x, codes in ((self.dk, kc), (self.dv, vc)):
            for j in range(-(-len(codes) // self.bk)):
                rows = torch.from_numpy(codes[j * self.bk:(j + 1) * self.bk].copy()).cuda().reshape(-1)
                x[self.ids[(b, j)] * self.block_step:][:rows.numel()] = rows

    def live(self):
        """{(request, logical block): the block's bytes of K and of V}; and: is every other byte of the two painted regions still 0x7f"""
        step, got, clean = self.block_step, {}, True
        for x in (self.dk, self.dv):
            low, high = x[:64 * step].clone(), x[-64 * step:].clone()
            for key, i in self.ids.items():
                got.setdefault(key, []).append(x[i * step:(i + 1) * step].cpu().numpy())
                part, at = (low, i) if i < 64 else (high, i - (self.pool_blocks - 64))
                part[at * step:(at + 1) * step] = NAN8
            clean = clean and bool((low == NAN8).all()) and bool((high == NAN8).all())
        return got, clean


def test_far_pool_takes_the_register_form_and_gives_the_compact_pools_bits(L, pkg, nso):
    """2 requests of 70 / 200 keys, 4 / 2 heads of 128, blocks of 16 (4096 bytes): a pool of 2^20 + 40 blocks, so every live block but block 2 starts
    above 2^32 bytes.  Request 0's keys but the last are put there directly, its last key by the FP8 append, request 1's by the FP8 store — all writes
    but block 2's land above 2^32 bytes.  The stats name the register form under the shipped knobs; Q, the written blocks and the output hold the bits
    of a compact pool forced to the register form by "attn_stream" 0; no 0x7f byte is consumed or overwritten."""
    import torch
    c, bk, sc = f8_case(nso, "far_shape"), 16, ONE[1]
    n0, n1 = c.lens
    rng = np.random.default_rng(232)
    q, k, v = (torch.from_numpy(rng.standard_normal((2, h, c.hs)).astype(np.float32)).cuda() for h in (c.hn, c.hkv, c.hkv))
    slab = [torch.from_numpy(x[1, :n1].copy()).cuda() for x in (c.k, c.v)]
    pos = torch.tensor([n0 - 1, -1], dtype=torch.int32, device="cuda")
    need(2 * ((1 << 32) + (1 << 20)))
    got = []
    try:
        for blocks, knobs in ((FL.pool_blocks("near", bk * c.hkv * c.hs, 18) + 128, dict(attn_stream=0)), ((1 << 20) + 40, {})):
            p = FarPools8(blocks, c, bk, [-(-n // bk) for n in c.lens])
            assert blocks < 1 << 20 or all(i == 2 or i * p.block_step >= 1 << 32 for i in p.ids.values())
            p.put(0, c.kc[0, :n0 - 1], c.vc[0, :n0 - 1])
            dq = q.clone()
            pkg.check(L.ns_hip_rope_qkv_append_paged_f8(dq.data_ptr(), k.data_ptr(), v.data_ptr(), p.kp, p.vp, 2, c.hn, c.hkv, c.hs, pos.data_ptr(), c.cap, c.hs, 0,
                                                        10000.0, 1.0, 0.0, 1.0, *p.table_args(), p.step_sl, p.step_head, sc, sc, stream_ptr()))
            pkg.check(L.ns_hip_kv_paged_store_f8(slab[0].data_ptr(), slab[1].data_ptr(), c.hkv * c.hs, c.hs, 0, n1, c.hkv, c.hs, p.kp, p.vp,
                                                 C.c_void_p(p.dt.data_ptr() + 4 * p.ts), p.ts, bk, blocks, p.block_step, p.step_sl, p.step_head, sc, sc, stream_ptr()))
            with tuning(L, **knobs):
                g0 = f8_stats(L)
                out = run_f8(L, pkg, c, p, q=dq.cpu().numpy()[:, None])
                assert family(delta(g0, f8_stats(L))) == "registers", blocks
            cells, clean = p.live()
            assert clean and np.all(np.isfinite(out)), blocks
            got.append((out, dq.cpu().numpy(), cells))
            p = None
            release()
        (on, qn, cn), (of, qf, cf) = got
        assert same_bits(on, of) and same_bits(qn, qf) and not same_bits(qn, q.cpu().numpy())
        assert all(same_bits(cn[key][x], cf[key][x]) for key in cn for x in (0, 1))
        last = cf[(0, (n0 - 1) // bk)]  # the appended key's row, and request 1's stored rows: valid codes, the store's the case's own
        assert all(NAN8 not in x.reshape(bk, -1)[(n0 - 1) % bk] for x in last)
        assert np.array_equal(np.concatenate([cf[(1, j)][0] for j in range(13)])[:n1 * c.hkv * c.hs], c.kc[1, :n1].reshape(-1))
    finally:
        p = None
        release()

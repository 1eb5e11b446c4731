"""Batched decode over a paged KV cache: ns_hip_rope_qkv_append_paged, ns_hip_attn_decode_paged and ns_hip_kv_paged_store (block tables: a K and a V
pool of blocks, a device table per request; docs/kernels/attention.md, "Decode over a paged cache").

What the results are compared with:
  (i)  ns_hip_attn_decode_rows on slabs of the same capacity holding the same keys (run_rows of tests/test_gpu_attn_rows.py).  The paged plan is that
       plan and the kernels keep the assignment of keys to lanes and the order of the softmax updates, so the outputs must be BIT-EQUAL whenever
       ns_hip_attn_paged_stats and ns_hip_attn_rows_stats name the same kernel family.  Were the families ever to differ, the bound would be the
       project's 2e-6 relative L2 for two one-row launches that split a context differently, and the test says so (same_bits_or_bound).
  (ii) the oracle per request through check() / rounding_model() of tests/test_gpu_attention_paths.py, exactly as test_gpu_attn_rows.py does.

The pools: a request's blocks lie at a random permutation of the physical blocks of a pool that has spare blocks; every spare block, every block of
a request past its live length and every cell of its last block from the live length on holds 0xFFFF (fp16 NaN), so any consumed byte that should
not be consumed shows as NaN.  A block's worth of guard memory (pattern 0x7BCD) lies in front of and behind each pool and must never change."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_attention_paths import check, rounding_model
from test_gpu_attn_rows import ALIBI, CAUSAL, HM, PM, Case, attn_stats, check_case, rows_stats, run_rows, stream_ptr, strides, to_slabs

pytestmark = pytest.mark.gpu
GUARD, NAN16 = 0x7BCD, 0xFFFF


def paged_stats(L):
    out = (C.c_ulonglong * 4)()
    L.ns_hip_attn_paged_stats(out)
    return list(out)


def delta(a, b):
    return [y - x for x, y in zip(a, b)]


class Pools:
    """K and V pools of pool_blocks blocks of bk keys with a guard block on either side, and the table [requests][cap / bk].  layout: of a block —
    PM [key][head][dim], HM [head][key][dim].  fill(k, v, lens): keys [0, len_b) of request b (numpy [bs][..][hkv][hs]) go to the cells the table names."""

    def __init__(self, bs, hkv, hs, cap, bk, layout, seed, spare=3, fill=NAN16):
        self.bs, self.hkv, self.hs, self.cap, self.bk, self.layout = bs, hkv, hs, cap, bk, layout
        self.ts = cap // bk
        assert self.ts * bk == cap
        self.pool_blocks = bs * self.ts + spare
        self.block_step = bk * hkv * hs
        self.step_sl, self.step_head = (hkv * hs, hs) if layout == PM else (hs, bk * hs)
        perm = np.random.default_rng(seed).permutation(self.pool_blocks)
        self.table = perm[:bs * self.ts].reshape(bs, self.ts).astype(np.int32)
        shape = (self.pool_blocks + 2, bk, hkv, hs) if layout == PM else (self.pool_blocks + 2, hkv, bk, hs)
        self.k = np.full(shape, fill, np.uint16)
        self.v = np.full(shape, fill, np.uint16)
        for x in (self.k, self.v):
            x[0], x[-1] = GUARD, GUARD

    def cells(self, x, blk, n0, cnt):
        """view of keys [n0, n0 + cnt) of physical block blk as [cnt][hkv][hs]"""
        return x[blk + 1, n0:n0 + cnt] if self.layout == PM else x[blk + 1, :, n0:n0 + cnt].transpose(1, 0, 2)

    def fill(self, k, v, lens):
        for b, n in enumerate(lens):
            for j in range(-(-n // self.bk)):
                cnt = min(self.bk, n - j * self.bk)
                if not 0 <= self.table[b, j] < self.pool_blocks:  # (a test's out-of-range entry: those keys have no cell)
                    continue
                self.cells(self.k, self.table[b, j], 0, cnt)[...] = k[b, j * self.bk:j * self.bk + cnt].view(np.uint16)
                self.cells(self.v, self.table[b, j], 0, cnt)[...] = v[b, j * self.bk:j * self.bk + cnt].view(np.uint16)
        return self

    def upload(self):
        import torch
        self.dk, self.dv = torch.from_numpy(self.k.view(np.int16)).cuda(), torch.from_numpy(self.v.view(np.int16)).cuda()
        self.dt = torch.from_numpy(self.table).cuda()
        self.kp, self.vp = self.dk.data_ptr() + 2 * self.block_step, self.dv.data_ptr() + 2 * self.block_step  # (behind the front guard)
        return self

    def download(self):
        return self.dk.cpu().numpy().view(np.uint16), self.dv.cpu().numpy().view(np.uint16)

    def table_args(self):
        return C.c_void_p(self.dt.data_ptr()), self.ts, self.bk, self.pool_blocks, self.block_step

    def guards_intact(self):
        k, v = self.download()
        return all(np.all(x[0] == GUARD) and np.all(x[-1] == GUARD) for x in (k, v))


def case_pools(c, bk, layout, seed=5, table_edit=None):
    p = Pools(c.bs, c.hkv, c.hs, c.cap, bk, layout, seed)
    if table_edit:
        table_edit(p)
    return p.fill(c.k, c.v, c.lens)


def run_paged(L, pkg, c, p, bias=1, tmp=None, expect=0):
    """ns_hip_attn_decode_paged of case c over the uploaded pools p; returns dst [bs][1][hn][hs] (started as 7.0)"""
    import torch
    dq = torch.from_numpy(c.q.copy()).cuda()
    dd = torch.full((c.bs, 1, c.hn, c.hs), 7.0, device="cuda")
    dl = torch.tensor([n - bias for n in c.lens], dtype=torch.int32, device="cuda")
    a = pkg.attn_args(dq.data_ptr(), p.kp, p.vp, dd.data_ptr(), c.bs, c.hn, c.hkv, c.hs, 1, c.cap, c.scale, c.flags)
    a.Q_sc, a.K_sc, a.V_sc, a.dst_sc = c.scales
    a.step_k_bs = a.step_v_bs = 12345  # (not used: must not matter)
    a.step_k_sl = a.step_v_sl = p.step_sl
    a.step_k_head_num = a.step_v_head_num = p.step_head
    if tmp is not None:
        a.tmp = tmp.data_ptr()
    rc = L.ns_hip_attn_decode_paged(C.byref(a), C.c_void_p(dl.data_ptr()), bias, *p.table_args(), None, stream_ptr())
    assert rc == expect, pkg.last_error()
    torch.cuda.synchronize()
    return dd.cpu().numpy()


def same_bits_or_bound(nso, tag, paged, rows, fam_paged, fam_rows):
    """(i) of the module's docstring"""
    if fam_paged == fam_rows:
        assert np.array_equal(paged.view(np.uint32), rows.view(np.uint32)), "%s: same kernel family (%s), bits differ: rel_l2 %.3g" % (
            tag, fam_paged, nso.rel_l2(paged, rows))
    else:
        e = nso.rel_l2(paged, rows)
        print("ATTN_PAGED %s: the families differ (paged %s, rows %s): rel_l2 %.3g against the 2e-6 bound" % (tag, fam_paged, fam_rows, e))
        assert e < 2e-6, (tag, e)


def family(d):
    """which kernel served, from the difference of a stats entry's four slots around one call"""
    assert d[0] + d[1] == 1 and d[3] == 0, d
    return "ring" if d[0] else "registers"


# ---- 1. attention: against the rows entry on slabs (bit-equal) and against the oracle ------------------------------------------------------------
ATTN_CASES = {  # name: (batch, heads, kv heads, head size, capacity, lengths, flags, block layout, block_keys, kernel family)
    "ring_step16_block16": (4, 4, 4, 128, 512, [1, 17, 300, 512], CAUSAL, PM, 16, "ring"),
    "ring_step32_block16": (4, 8, 2, 64, 1024, [31, 33, 129, 1024], CAUSAL, PM, 16, "ring"),  # a 32-key step straddles two blocks
    "ring_step32_block64": (4, 8, 2, 64, 1024, [31, 33, 129, 1024], CAUSAL, PM, 64, "ring"),
    "regs_256": (4, 4, 4, 256, 256, [1, 32, 33, 256], CAUSAL, PM, 32, "registers"),
    "regs_32": (4, 4, 4, 32, 256, [1, 32, 33, 256], CAUSAL, PM, 32, "registers"),
    "ring_head_major": (4, 4, 4, 128, 512, [1, 17, 300, 512], CAUSAL, HM, 16, "ring"),
    "regs_head_major": (4, 4, 4, 32, 256, [1, 32, 33, 256], CAUSAL, HM, 32, "registers"),
    "alibi_and_idle_slot": (3, 8, 1, 128, 256, [200, 0, 65], CAUSAL | ALIBI, PM, 16, "ring"),
    "block_256": (2, 4, 4, 128, 512, [255, 257], CAUSAL, PM, 256, "ring"),
    "block_128_many_ranges": (8, 8, 2, 128, 4096, [1, 4096, 2048, 17, 3000, 129, 1024, 700], CAUSAL, PM, 128, "ring"),
}
_cases = {}


def attn_case(nso, name):
    """the inputs and references of a case, made once and shared by the cases of the same shape (Case keeps them read-only)"""
    bs, hn, hkv, hs, cap, lens, flags = ATTN_CASES[name][:7]
    key = (bs, hn, hkv, hs, cap, tuple(lens), flags)
    if key not in _cases:
        _cases[key] = Case(nso, bs, hn, hkv, hs, cap, lens, flags)
    return _cases[key]


@pytest.mark.parametrize("name", list(ATTN_CASES))
def test_paged_attention_against_the_rows_entry_and_the_reference(L, pkg, nso, name):
    layout, bk, want = ATTN_CASES[name][7:]
    c = attn_case(nso, name)
    p = case_pools(c, bk, layout).upload()
    r0, g0, a0 = rows_stats(L), paged_stats(L), attn_stats(L)
    rows = run_rows(L, pkg, c, layout)[0]
    r1 = rows_stats(L)
    out = run_paged(L, pkg, c, p)
    g1, a1 = paged_stats(L), attn_stats(L)
    fam_rows, fam_paged = family(delta(r0, r1)), family(delta(g0, g1))
    assert fam_paged == want, (fam_paged, want)
    assert delta(g0, g1)[2] == delta(r0, r1)[2]  # the merge launch follows in both or in neither
    assert sum(delta(a0, a1)) == 2  # (ns_hip_attn_stats counts both launches by family)
    if name == "block_128_many_ranges":
        assert delta(g0, g1)[2] == 1  # nsplit > 1: attn_merge_kernel<true> ran
    assert np.all(np.isfinite(out)), name  # nothing behind a live length, no spare block was consumed
    check_case(nso, "paged %s" % name, c, out)  # (ii): per request; the idle slot's row is zeros
    same_bits_or_bound(nso, name, out, rows, fam_paged, fam_rows)  # (i)
    assert p.guards_intact()


# ---- 2. two requests sharing their first blocks ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hs,bk,lens", [(128, 16, [40, 45]), (256, 32, [70, 90])], ids=["ring", "registers"])
def test_prefix_sharing(L, pkg, nso, hs, bk, lens):
    """Both requests' first two table entries name the SAME physical blocks (request 1's own first two blocks stay spare: NaN); the tails differ.  Both
    rows equal the rows entry on slabs holding the same keys."""
    bs, hn, hkv, cap = 2, 4, 4, 256
    c = Case.__new__(Case)
    c.bs, c.hn, c.hkv, c.hs, c.cap, c.lens, c.flags, c.scales = bs, hn, hkv, hs, cap, lens, CAUSAL, (1.0, 1.0, 1.0, 1.0)
    rng = np.random.default_rng(hs + bk)
    c.q = rng.standard_normal((bs, 1, hn, hs)).astype(np.float32)
    c.k = rng.standard_normal((bs, cap + 64, hkv, hs)).astype(np.float16)
    c.v = rng.standard_normal((bs, cap + 64, hkv, hs)).astype(np.float16)
    c.k[1, :2 * bk], c.v[1, :2 * bk] = c.k[0, :2 * bk], c.v[0, :2 * bk]
    c.scale = float(1.0 / np.sqrt(hs))
    c.ref = {b: nso.attn_ref(c.q[b:b + 1], c.k[b:b + 1, :n], c.v[b:b + 1, :n], c.scale, CAUSAL) for b, n in enumerate(lens)}
    c.model = {b: rounding_model(c.q[b:b + 1], c.k[b:b + 1, :n], c.v[b:b + 1, :n], c.scale, CAUSAL, c.scales) for b, n in enumerate(lens)}

    def share(p):
        p.table[1, :2] = p.table[0, :2]

    p = case_pools(c, bk, PM, table_edit=share).upload()
    assert list(p.table[1, :2]) == list(p.table[0, :2]) and p.table[1, 2] != p.table[0, 2]
    r0, g0 = rows_stats(L), paged_stats(L)
    rows = run_rows(L, pkg, c, PM)[0]
    r1 = rows_stats(L)
    out = run_paged(L, pkg, c, p)
    assert np.all(np.isfinite(out))
    check_case(nso, "shared prefix", c, out)
    same_bits_or_bound(nso, "shared prefix", out, rows, family(delta(g0, paged_stats(L))), family(delta(r0, r1)))


# ---- 3. a table entry that is not a block of the pool -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", ["minus_one", "pool_blocks"])
@pytest.mark.parametrize("name", ["ring_step16_block16", "ring_step32_block16", "regs_256"])
def test_out_of_range_block_id(L, pkg, nso, name, bad):
    """Request 2's second block — live: its lengths are 300, 129 and 33 keys — gets the id -1 or pool_blocks.  The other requests' rows hold the bits of
    the run with the valid table and no NaN; the append and the store through that entry write nothing; the guards are unchanged after all three."""
    import torch
    layout, bk, _ = ATTN_CASES[name][7:]
    c = attn_case(nso, name)
    good = run_paged(L, pkg, c, case_pools(c, bk, layout).upload())

    def poison(p):
        p.table[2, 1] = -1 if bad == "minus_one" else p.pool_blocks

    p = case_pools(c, bk, layout, table_edit=poison).upload()
    assert c.lens[2] > bk and not 0 <= p.table[2, 1] < p.pool_blocks
    out = run_paged(L, pkg, c, p)
    others = [0, 1, 3]
    assert np.all(np.isfinite(out[others]))
    assert np.array_equal(out[others].view(np.uint32), good[others].view(np.uint32))
    assert p.guards_intact()
    before = p.download()
    # the append: request 2 at a position inside the bad block (skipped, Q untouched), request 0 idle
    pos = torch.tensor([-1, -1, bk + 3, -1], dtype=torch.int32, device="cuda")
    q = torch.randn((c.bs, c.hn, c.hs), device="cuda")
    q0 = q.clone()
    kv = torch.randn((c.bs, c.hkv, c.hs), device="cuda")
    pkg.check(L.ns_hip_rope_qkv_append_paged(q.data_ptr(), kv.data_ptr(), kv.data_ptr(), p.kp, p.vp, c.bs, c.hn, c.hkv, c.hs, pos.data_ptr(), c.cap, c.hs, 0,
                                             10000.0, 1.0, 0.0, 1.0, *p.table_args(), p.step_sl, p.step_head, stream_ptr()))
    # the store: rows [0, 3 * bk) of a slab through request 2's table row — the rows of the bad block are skipped, the others written
    slab = torch.randn((3 * bk, c.hkv, c.hs), device="cuda").half()
    pkg.check(L.ns_hip_kv_paged_store(slab.data_ptr(), slab.data_ptr(), c.hkv * c.hs, c.hs, 0, 3 * bk, c.hkv, c.hs, p.kp, p.vp,
                                      C.c_void_p(p.dt.data_ptr() + 4 * 2 * p.ts), p.ts, bk, p.pool_blocks, p.block_step, p.step_sl, p.step_head, stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(q, q0)
    after = p.download()
    assert p.guards_intact()
    s = slab.cpu().numpy().view(np.uint16)
    for x0, x1 in zip(before, after):
        changed = np.unique(np.nonzero((x0 != x1).reshape(x0.shape[0], -1).any(axis=1))[0]) - 1
        assert set(changed) <= {p.table[2, 0], p.table[2, 2]}, changed  # only the two valid blocks of the stored rows
        for j in (0, 2):
            assert np.array_equal(p.cells(x1, p.table[2, j], 0, bk), s[j * bk:(j + 1) * bk])


# ---- 4. the append ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pos,pos_cap", [([0, 15, 16, 255, -1], 256), ([0, 15, 16, 256, 300], 4096)], ids=["idle_negative", "idle_at_capacity"])
@pytest.mark.parametrize("layout", [PM, HM])
@pytest.mark.parametrize("mode,n_dims", [(0, 64), (2, 32)])
def test_append_is_bit_equal_to_the_rows_entry(L, pkg, mode, n_dims, layout, pos, pos_cap):
    """5 rows, 4 / 2 heads of size 64, block 16, capacity 256.  Against ns_hip_rope_qkv_append_rows on slabs: every Q row and every written cell hold the
    same bits; every other byte of the pools and the guards is unchanged; a position at (or behind) the capacity is idle even under a larger pos_cap."""
    import torch
    rows, heads, hkv, hs, cap, bk = 5, 4, 2, 64, 256, 16
    rng = np.random.default_rng(mode * 100 + n_dims)
    q = rng.standard_normal((rows, heads, hs)).astype(np.float32)
    k = rng.standard_normal((rows, hkv, hs)).astype(np.float32)
    v = rng.standard_normal((rows, hkv, hs)).astype(np.float32)
    dk, dv, dpos = torch.from_numpy(k).cuda(), torch.from_numpy(v).cuda(), torch.tensor(pos, dtype=torch.int32, device="cuda")
    st = stream_ptr()
    # the rows entry on slabs of `cap` rows (its own bound: pos_cap = cap)
    c_bs, c_sl, c_head = strides(PM, cap, hkv, hs)
    q_rows = torch.from_numpy(q).cuda()
    kc = torch.full((rows * c_bs,), 0x5A5B, dtype=torch.int16, device="cuda")
    vc = torch.full((rows * c_bs,), 0x5A5B, dtype=torch.int16, device="cuda")
    pkg.check(L.ns_hip_rope_qkv_append_rows(q_rows.data_ptr(), dk.data_ptr(), dv.data_ptr(), kc.data_ptr(), vc.data_ptr(), rows, heads, hkv, hs, dpos.data_ptr(),
                                            cap, n_dims, mode, 10000.0, 0.75, 0.0, 1.1, c_bs, c_sl, c_head, st))
    p = Pools(rows, hkv, hs, cap, bk, layout, seed=9, fill=0x5A5B).upload()
    q_paged = torch.from_numpy(q).cuda()
    pkg.check(L.ns_hip_rope_qkv_append_paged(q_paged.data_ptr(), dk.data_ptr(), dv.data_ptr(), p.kp, p.vp, rows, heads, hkv, hs, dpos.data_ptr(), pos_cap, n_dims,
                                             mode, 10000.0, 0.75, 0.0, 1.1, *p.table_args(), p.step_sl, p.step_head, st))
    torch.cuda.synchronize()
    assert torch.equal(q_paged.view(torch.int32), q_rows.view(torch.int32))
    slab_k = kc.cpu().numpy().view(np.uint16).reshape(rows, cap, hkv, hs)
    slab_v = vc.cpu().numpy().view(np.uint16).reshape(rows, cap, hkv, hs)
    pk, pv = p.download()
    want_k, want_v = p.k.copy(), p.v.copy()  # the pools as uploaded, plus the live rows' cells
    live = [(r, n) for r, n in enumerate(pos) if 0 <= n < cap]
    assert len(live) == (4 if pos_cap == 256 else 3)
    for r, n in live:
        p.cells(want_k, p.table[r, n // bk], n % bk, 1)[...] = slab_k[r, n:n + 1]
        p.cells(want_v, p.table[r, n // bk], n % bk, 1)[...] = slab_v[r, n:n + 1]
        assert np.all(slab_k[r, n] != 0x5A5B)
    assert np.array_equal(pk, want_k) and np.array_equal(pv, want_v)  # (guards included)
    for r, n in enumerate(pos):
        if not 0 <= n < cap:
            assert np.array_equal(q_paged[r].cpu().numpy(), q[r])


# ---- 5. the store ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slab_layout", [PM, HM])
@pytest.mark.parametrize("pos0,n", [(0, 37), (16, 32)])
def test_store_copies_slab_rows_into_pages(L, pkg, pos0, n, slab_layout):
    """rows [0, 37) and [16, 48) of a slab (position-major as ns_hip_rope_qkv_append writes it, or head-major) into block-16 pages of request 1 of 2: the
    cells hold the slab's bits, everything else — other blocks, the cells behind the rows, the guards — is unchanged; K and V in one call."""
    import torch
    hkv, hs, cap, bk, rows_alloc = 2, 64, 64, 16, 48
    rng = np.random.default_rng(pos0 + n)
    sk = rng.standard_normal((1, rows_alloc, hkv, hs)).astype(np.float16)
    sv = rng.standard_normal((1, rows_alloc, hkv, hs)).astype(np.float16)
    dsk, dsv = to_slabs(sk, slab_layout), to_slabs(sv, slab_layout)
    _, s_sl, s_head = strides(slab_layout, rows_alloc, hkv, hs)
    p = Pools(2, hkv, hs, cap, bk, HM, seed=3).upload()
    row = C.c_void_p(p.dt.data_ptr() + 4 * p.ts)  # request 1's table row
    pkg.check(L.ns_hip_kv_paged_store(dsk.data_ptr(), dsv.data_ptr(), s_sl, s_head, pos0, n, hkv, hs, p.kp, p.vp, row, p.ts, bk, p.pool_blocks, p.block_step,
                                      p.step_sl, p.step_head, stream_ptr()))
    torch.cuda.synchronize()
    want_k, want_v = p.k.copy(), p.v.copy()
    for x in range(pos0, pos0 + n):
        p.cells(want_k, p.table[1, x // bk], x % bk, 1)[...] = sk[0, x:x + 1].view(np.uint16)
        p.cells(want_v, p.table[1, x // bk], x % bk, 1)[...] = sv[0, x:x + 1].view(np.uint16)
    pk, pv = p.download()
    assert np.array_equal(pk, want_k) and np.array_equal(pv, want_v)
    assert not np.array_equal(pk, p.k)


# ---- 6. one captured step, replayed while the requests grow into new blocks ----------------------------------------------------------------------
def live_ranges(n, nsplit, min_keys, batch_keys, single_below):
    """attn_live_kps / attn_live_splits (ns_attn.h) restated"""
    if n <= single_below:
        return 1
    want = max(1, min(nsplit, -(-n // min_keys)))
    kps = -(-n // want)
    if batch_keys > 1 and want > 1:
        kps = -(-kps // batch_keys) * batch_keys
    return max(1, -(-n // kps))


def test_captured_step_replayed_across_block_boundaries(L, pkg, nso):
    """{append; attention} captured ONCE on a side stream with `tmp` given (after one eager call), replayed five times at positions 126 .. 130 (request 0) and 14 .. 18 (request
    1), block 16, capacity 256.  Between replays the test writes the new positions to the device and, when a request enters a new block (positions 128
    and 16), that block's id into the table — until then the entry holds -1.  Every replay equals the same step run eagerly on a twin, bit for bit
    (output, Q, both pools), and the last passes check() against the reference over the pool as it then stands.
    2 requests x 16 / 16 heads of size 128: 32 workgroups per range, so the shipped rule keeps up to 128 keys in one range and request 0 goes from one
    live range to three at 128 -> 129 keys — the step at which it also enters block 8."""
    import torch
    bs, hn, hkv, hs, cap, bk = 2, 16, 16, 128, 256, 16
    first = [126, 14]
    # the plan of capacity 256: 256 / 32 workgroups = 8 ranges of at least 32 keys, rounded to whole softmax updates of a one-head workgroup (64 keys): 4
    assert [live_ranges(n, 4, 32, 64, 128) for n in (127, 128, 129)] == [1, 1, 3]
    rng = np.random.default_rng(77)
    k0 = rng.standard_normal((bs, cap, hkv, hs)).astype(np.float16)
    v0 = rng.standard_normal((bs, cap, hkv, hs)).astype(np.float16)
    scale = float(1.0 / np.sqrt(hs))
    side = torch.cuda.Stream()
    shape = pkg.AttnShape(bs, hn, hkv, hs, 1, cap)
    ws_bytes = L.bestla_fusion_attn_workspace_size(C.byref(shape))
    with torch.cuda.stream(side):
        qin = torch.zeros((bs, hn, hs), device="cuda")
        kin, vin = torch.zeros((bs, hkv, hs), device="cuda"), torch.zeros((bs, hkv, hs), device="cuda")

        class State:
            def __init__(self):
                self.p = Pools(bs, hkv, hs, cap, bk, PM, seed=11).fill(k0, v0, first)
                self.full_table = self.p.table.copy()
                for b, n in enumerate(first):  # blocks the request has not entered yet: no id
                    self.p.table[b, n // bk + 1:] = -1
                self.p.upload()
                self.pos = torch.tensor(first, dtype=torch.int32, device="cuda")
                self.q = torch.zeros_like(qin)
                self.dst = torch.full((bs, 1, hn, hs), 7.0, device="cuda")
                self.ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
                self.a = pkg.attn_args(self.q.data_ptr(), self.p.kp, self.p.vp, self.dst.data_ptr(), bs, hn, hkv, hs, 1, cap, scale, CAUSAL)
                self.a.step_k_sl = self.a.step_v_sl = self.p.step_sl
                self.a.step_k_head_num = self.a.step_v_head_num = self.p.step_head
                self.a.tmp = self.ws.data_ptr()

            def move_to(self, pos):
                """what the serving loop does between steps: the positions, and the id of a block a request enters"""
                self.pos.copy_(torch.tensor(pos, dtype=torch.int32))
                for b, n in enumerate(pos):
                    self.p.dt[b, n // bk] = int(self.full_table[b, n // bk])

            def step(self):
                st = stream_ptr()
                self.q.copy_(qin)
                pkg.check(L.ns_hip_rope_qkv_append_paged(self.q.data_ptr(), kin.data_ptr(), vin.data_ptr(), self.p.kp, self.p.vp, bs, hn, hkv, hs,
                                                         self.pos.data_ptr(), cap, hs, 0, 10000.0, 1.0, 0.0, 1.0, *self.p.table_args(), self.p.step_sl,
                                                         self.p.step_head, st))
                pkg.check(L.ns_hip_attn_decode_paged(C.byref(self.a), C.c_void_p(self.pos.data_ptr()), 1, *self.p.table_args(), None, st))

        State().step()  # (one eager call in front of the capture: the kernels' code objects and attributes are in place)
        graphed, eager = State(), State()
        side.synchronize()
        g0 = paged_stats(L)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            graphed.step()
        assert delta(g0, paged_stats(L)) == [1, 0, 1, 0]  # (captured: the ring kernel and the merge launch; nothing has run)
        for s in range(5):
            pos = [n + s for n in first]
            step_rng = np.random.default_rng(1000 + s)
            qin.copy_(torch.from_numpy(step_rng.standard_normal(tuple(qin.shape)).astype(np.float32)))
            kin.copy_(torch.from_numpy(step_rng.standard_normal(tuple(kin.shape)).astype(np.float32)))
            vin.copy_(torch.from_numpy(step_rng.standard_normal(tuple(vin.shape)).astype(np.float32)))
            graphed.move_to(pos)
            eager.move_to(pos)
            g.replay()
            eager.step()
            side.synchronize()
            assert torch.equal(graphed.dst, eager.dst) and torch.equal(graphed.q, eager.q), s
            assert torch.equal(graphed.p.dk, eager.p.dk) and torch.equal(graphed.p.dv, eager.p.dv), s
            assert bool(torch.all(torch.isfinite(graphed.dst))), s
        assert graphed.p.guards_intact()
        # the last step against the reference, over the keys as the pool now holds them
        out, q = graphed.dst.cpu().numpy(), graphed.q.cpu().numpy()
        pk, pv = graphed.p.download()
        for b, n in enumerate([x + 5 for x in first]):
            kb = np.concatenate([graphed.p.cells(pk, graphed.full_table[b, j], 0, bk) for j in range(-(-n // bk))])[:n].view(np.float16)[None]
            vb = np.concatenate([graphed.p.cells(pv, graphed.full_table[b, j], 0, bk) for j in range(-(-n // bk))])[:n].view(np.float16)[None]
            assert np.all(np.isfinite(kb.astype(np.float32)))
            qb = q[b][None, None]
            check(nso, "replay 4 request %d (%d keys)" % (b, n), out[b:b + 1], nso.attn_ref(qb, kb, vb, scale, CAUSAL), rounding_model(qb, kb, vb, scale, CAUSAL))
    torch.cuda.synchronize()


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(L, pkg, nso):
    import torch
    c = attn_case(nso, "ring_step16_block16")
    p = case_pools(c, 16, PM).upload()
    dq = torch.from_numpy(c.q.copy()).cuda()
    dd = torch.full((c.bs, 1, c.hn, c.hs), 7.0, device="cuda")
    dl = torch.tensor(c.lens, dtype=torch.int32, device="cuda")

    def call(table=True, ts=p.ts, bk=16, blocks=p.pool_blocks, step=p.block_step, lens=True, sl_q=1):
        a = pkg.attn_args(dq.data_ptr(), p.kp, p.vp, dd.data_ptr(), c.bs, c.hn, c.hkv, c.hs, sl_q, c.cap, c.scale, c.flags)
        a.step_k_sl = a.step_v_sl = p.step_sl
        a.step_k_head_num = a.step_v_head_num = p.step_head
        return L.ns_hip_attn_decode_paged(C.byref(a), C.c_void_p(dl.data_ptr()) if lens else None, 0, C.c_void_p(p.dt.data_ptr()) if table else None, ts, bk,
                                          blocks, step, None, stream_ptr())

    calls = [("block table is null", dict(table=False)), ("power of two from 16 to 256", dict(bk=48)), ("power of two from 16 to 256", dict(bk=8)),
             ("power of two from 16 to 256", dict(bk=512)), ("pool_blocks must be at least 1", dict(blocks=0)),
             ("must equal table_stride * block_keys", dict(ts=p.ts - 1)), ("do not fit inside block_step", dict(step=p.block_step - 8)),
             ("dKvLens is null", dict(lens=False)), ("one query row", dict(sl_q=2))]
    g0, a0 = paged_stats(L), attn_stats(L)
    for n, (text, kw) in enumerate(calls):
        L.ns_hip_reset_error()
        assert call(**kw) == -1, text
        assert text in pkg.last_error(), (text, pkg.last_error())
        assert delta(g0, paged_stats(L)) == [0, 0, 0, n + 1]
    # the two writers
    t = torch.zeros(8192, device="cuda")
    pos = torch.zeros(4, dtype=torch.int32, device="cuda")

    def append(table=p.dt.data_ptr(), bk=16, blocks=p.pool_blocks, mode=0, ext=0.0):
        return L.ns_hip_rope_qkv_append_paged(t.data_ptr(), t.data_ptr(), t.data_ptr(), p.kp, p.vp, 2, c.hn, c.hkv, c.hs, pos.data_ptr(), c.cap, c.hs, mode, 10000.0,
                                              1.0, ext, 1.0, C.c_void_p(table) if table else None, p.ts, bk, blocks, p.block_step, p.step_sl, p.step_head, stream_ptr())

    def store(table=p.dt.data_ptr(), bk=16, blocks=p.pool_blocks, pos0=0, n=16):
        return L.ns_hip_kv_paged_store(p.kp, p.vp, c.hkv * c.hs, c.hs, pos0, n, c.hkv, c.hs, p.kp, p.vp, C.c_void_p(table) if table else None, p.ts, bk, blocks,
                                       p.block_step, p.step_sl, p.step_head, stream_ptr())

    for fn in (append, store):
        for text, kw in (("block table is null", dict(table=None)), ("power of two from 16 to 256", dict(bk=24)), ("pool_blocks must be at least 1", dict(blocks=0))):
            L.ns_hip_reset_error()
            assert fn(**kw) == -1 and text in pkg.last_error(), (fn.__name__, text, pkg.last_error())
    assert append(mode=4) == -1 and "modes 0 and 2" in pkg.last_error()
    assert append(ext=1.0) == -1 and "YaRN" in pkg.last_error()
    assert store(pos0=c.cap - 8, n=16) == -1 and "behind the request's capacity" in pkg.last_error()
    torch.cuda.synchronize()
    assert bool(torch.all(dd == 7.0)) and attn_stats(L) == a0
    pk, pv = p.download()
    assert np.array_equal(pk, p.k) and np.array_equal(pv, p.v)
    L.ns_hip_reset_error()

"""KV caches above 4 GiB: every attention and cache-write kernel at element offsets of 2^31 and more (byte offsets of 2^32 and more), and the two
32-bit rules (attn_page_in32, attn_in32) at their boundaries.  docs/kernels/attention.md, "Addresses".

Every case runs twice.  The NEAR twin is the problem in a compact buffer, as the other attention tests run it; it is also checked against the fp64
model under the bar of the test it is taken from (check() / check_case() / check_rag(): rel_l2 < 1e-3 over the tensor and the per-row bound).  The FAR
twin is the same Q, the same K / V rows and the same table shape with the blocks or slabs at high offsets of one large allocation that is otherwise
never touched (torch.empty: only the live rows and the traps are written).  Both twins take the same kernel — asserted through the stats entries,
the near twin pinned with "attn_stream" where the 32-bit rule changes the far twin's path — so outputs and written cache cells are BIT-EQUAL.

Alias traps: 0x7f bytes (an fp16 NaN) lie where a truncated address would land — the element offset mod 2^31 and mod 2^32, the byte offset mod 2^32
(tests/tools/attn_far_layout.py, aliases) — and directly before and after every live block or slab; the layout asserts on the host that no trap
touches live data.  A read of a trap shows as NaN in the output, a write as a changed trap.

Not pinned, and why: the prefill calls past the slab rule run attn_mfma2_kernel, which only the environment variable NS_ATTN_PIPE selects for a
compact buffer — those far runs have no bit twin and are held to check() against the reference alone."""
import contextlib
import ctypes as C
import gc
import importlib.util
import os

import numpy as np
import pytest

from test_gpu_attention_paths import check, rounding_model
from test_gpu_attn_block_paged import Rag, block_stats, check_rag, run_block
from test_gpu_attn_paged import delta, family, paged_stats, run_paged
from test_gpu_attn_rows import CAUSAL, Case, attn_stats, check_case, rows_stats, stream_ptr

pytestmark = pytest.mark.gpu
_spec = importlib.util.spec_from_file_location("attn_far_layout", os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools", "attn_far_layout.py"))
FL = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(FL)
HN, HKV, TRAP, NAN16, E31, E32 = FL.HN, FL.HKV, FL.TRAP, FL.NAN16, FL.E31, FL.E32
DEFAULTS = {"attn_stream": 1, "attn_inlaunch": 0, "attn_block_split": 0}
RING, REGS = 3, 2  # slots of ns_hip_attn_stats (AttnPath, ns_attn.h): 1 attn_kernel, 4 attn_mfma_kernel, 5 attn_mfma2_kernel, 6 attn_mfma3_kernel, 7 block split


# ---- helpers ---------------------------------------------------------------------------------------------------------------------------------------
def s16(pattern):
    return int(np.array(pattern, np.uint16).view(np.int16))


def need(nbytes):
    import torch
    free = torch.cuda.mem_get_info()[0]
    if free < nbytes + (2 << 30):
        pytest.skip("%.1f GiB of device memory free; the case allocates %.1f GiB and leaves 2 GiB" % (free / 2.0 ** 30, nbytes / 2.0 ** 30))


def release():
    import torch
    gc.collect()
    torch.cuda.empty_cache()


@contextlib.contextmanager
def tuning(L, **knobs):
    try:
        for key, value in knobs.items():
            assert L.ns_hip_set_tuning(key.encode(), value) == 0
        yield
    finally:
        for key in knobs:
            L.ns_hip_set_tuning(key.encode(), DEFAULTS[key])


def same_bits(x, y):
    return x.shape == y.shape and np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))


class Far:
    """`total` fp16 elements.  traps: allocated and left as it is but for the traps (FL.traps_of around the live extents) and what put() writes; no
    traps (a near twin): NaN everywhere first, as the other attention tests fill their dead cells."""

    def __init__(self, total, extents, strip, dead=(), traps=True):
        import torch
        self.total = total
        self.traps = FL.traps_of(extents, strip, total, dead) if traps else []
        self.buf = torch.empty(total, dtype=torch.int16, device="cuda")
        if not traps:
            self.buf.fill_(s16(NAN16))
        for off, n in self.traps:
            self.buf[off:off + n].fill_(s16(TRAP))
        self.ptr = self.buf.data_ptr()

    def put(self, off, strides, x):
        """x (numpy, 16-bit) to the elements off + sum(index * stride)"""
        import torch
        t = torch.from_numpy(np.array(x, order="C").view(np.int16)).cuda()  # (a copy: the cases' arrays are read-only)
        torch.as_strided(self.buf, t.shape, strides, off).copy_(t)

    def paint(self, off, shape, strides, pattern):
        import torch
        torch.as_strided(self.buf, shape, strides, off).fill_(s16(pattern))

    def get(self, off, shape, strides):
        import torch
        return torch.as_strided(self.buf, shape, strides, off).cpu().numpy().view(np.uint16)

    def traps_intact(self):
        return all(bool((self.buf[off:off + n] == s16(TRAP)).all()) for off, n in self.traps)


# ---- paged pools -------------------------------------------------------------------------------------------------------------------------------------
class Pages:
    """K and V pools of position-major blocks with the table of FL.place: size "near" (compact), "under" (the largest pool attn_page_in32 accepts;
    the live blocks but one at byte offsets in [2^31, 2^32)) or "over" (1.4 * 2^31 elements; the live blocks but one beyond 2^31 elements).  Live
    blocks start as NaN (0xFFFF); traps around them, at their aliases and in block 0, which the table entries behind a live length name.  Has the
    attributes run_paged / run_block (tests/test_gpu_attn_paged.py, test_gpu_attn_block_paged.py) read of their Pools."""

    def __init__(self, size, hs, bk, live):
        import torch
        self.hs, self.bk, self.ts = hs, bk, FL.PAGED_CAP[bk] // bk
        self.block_step = step = FL.block_step(hs, bk)
        self.step_sl, self.step_head = HKV * hs, hs
        self.pool_blocks = FL.pool_blocks(size, step, sum(live))
        self.table, self.ids = FL.place(live, self.ts, self.pool_blocks)
        high = [i for i in self.ids.values() if i != 2]
        assert size != "under" or all(E31 <= 2 * i * step < E32 for i in high)  # byte offsets a signed or wrapped 32-bit value cannot hold
        assert size != "over" or all(i * step > E31 for i in high)
        total = self.pool_blocks * step
        if size != "near":
            need(4 * total)
        extents = [(i * step, step) for i in self.ids.values()]
        self.k, self.v = (Far(total, extents, step, dead=[(0, step)], traps=size != "near") for _ in range(2))
        for x in (self.k, self.v):
            for off, n in extents:
                x.buf[off:off + n].fill_(s16(NAN16))
        self.dt = torch.from_numpy(self.table).cuda()
        self.kp, self.vp = self.k.ptr, self.v.ptr

    def table_args(self):
        return C.c_void_p(self.dt.data_ptr()), self.ts, self.bk, self.pool_blocks, self.block_step

    def fill_keys(self, k, v, lens):
        """keys [0, lens[b]) of request b (numpy [requests][..][HKV][hs]) to the cells the table names"""
        for b, n in enumerate(lens):
            for j in range(-(-n // self.bk)):
                cnt, off = min(self.bk, n - j * self.bk), self.ids[(b, j)] * self.block_step
                self.k.put(off, (self.step_sl, self.hs, 1), k[b, j * self.bk:j * self.bk + cnt])
                self.v.put(off, (self.step_sl, self.hs, 1), v[b, j * self.bk:j * self.bk + cnt])
        return self

    def blocks(self):
        """{(request, logical block): (K block, V block)} as uint16 [bk][HKV][hs]"""
        shape, strides = (self.bk, HKV, self.hs), (self.step_sl, self.hs, 1)
        return {key: (self.k.get(i * self.block_step, shape, strides), self.v.get(i * self.block_step, shape, strides)) for key, i in self.ids.items()}

    def keys(self, b, n):
        """the first n keys of request b as the pools hold them: fp16 [1][n][HKV][hs] of K and of V"""
        got = self.blocks()
        return tuple(np.concatenate([got[(b, j)][x] for j in range(-(-n // self.bk))])[:n].view(np.float16)[None] for x in (0, 1))

    def traps_intact(self):
        return self.k.traps_intact() and self.v.traps_intact()


_cases = {}


def paged_case(nso, hs, bk):
    if ("paged", hs, bk) not in _cases:
        _cases[("paged", hs, bk)] = Case(nso, 2, HN, HKV, hs, FL.PAGED_CAP[bk], FL.PAGED_LENS[bk])
    return _cases[("paged", hs, bk)]


def live_blocks(lens, bk):
    return [-(-n // bk) for n in lens]


def decode_twins(L, pkg, c, near, far, size, inlaunch=0):
    """ns_hip_attn_decode_paged over both twins: the far one under the shipped knobs — the plan alone must answer a pool over the limit with the
    register kernel and one under it with the ring kernel — the near one pinned to that kernel.  Same counters, same bits, no NaN."""
    want = "ring" if size == "under" else "registers"
    with tuning(L, attn_inlaunch=inlaunch, attn_stream=1 if want == "ring" else 0):
        g0 = paged_stats(L)
        out_n = run_paged(L, pkg, c, near)
        dn = delta(g0, paged_stats(L))
    with tuning(L, attn_inlaunch=inlaunch):
        g0 = paged_stats(L)
        out_f = run_paged(L, pkg, c, far)
        df = delta(g0, paged_stats(L))
    assert family(df) == want and df == dn, (size, want, df, dn)
    assert dn[2] == (0 if inlaunch else 1), dn  # (both shapes have ranges: the merge launch, or the merge inside the launch)
    assert np.all(np.isfinite(out_f)), "a trap or a dead cell was consumed"
    assert same_bits(out_f, out_n)
    return out_n


PAGED = pytest.mark.parametrize("hs,bk", FL.PAGED_SHAPES, ids=["hs%d_bk%d" % s for s in FL.PAGED_SHAPES])
WRITES = pytest.mark.parametrize("hs,bk", [(64, 16), (128, 128)], ids=["hs64_bk16", "hs128_bk128"])
SIZES = pytest.mark.parametrize("size", ["under", "over"])


@SIZES
@PAGED
def test_decode_paged(L, pkg, nso, size, hs, bk):
    c = paged_case(nso, hs, bk)
    near = far = None
    try:
        near = Pages("near", hs, bk, live_blocks(c.lens, bk)).fill_keys(c.k, c.v, c.lens)
        far = Pages(size, hs, bk, live_blocks(c.lens, bk)).fill_keys(c.k, c.v, c.lens)
        for inlaunch in (0, 1):
            out = decode_twins(L, pkg, c, near, far, size, inlaunch)
            check_case(nso, "far addresses, near twin: decode_paged %s hs %d bk %d inlaunch %d" % (size, hs, bk, inlaunch), c, out)
        assert far.traps_intact()
    finally:
        near = far = None
        release()


_rags = {}


@SIZES
@PAGED
def test_block_paged(L, pkg, nso, size, hs, bk):
    """query blocks of 1, 5 and 40 rows in one call, the partials in the caller's workspace"""
    import torch
    if (hs, bk) not in _rags:
        _rags[(hs, bk)] = Rag(nso, HN, HKV, hs, FL.PAGED_CAP[bk], FL.BLOCK_Q, FL.BLOCK_KV[bk], seed=31)
    c = _rags[(hs, bk)]
    near = far = tmp = None
    try:
        near = Pages("near", hs, bk, live_blocks(c.kvlens, bk)).fill_keys(c.k, c.v, c.kvlens)
        far = Pages(size, hs, bk, live_blocks(c.kvlens, bk)).fill_keys(c.k, c.v, c.kvlens)
        ws = L.ns_hip_attn_block_paged_workspace_size(c.bs, HN, HKV, hs, max(c.qlens), c.cap)
        assert ws > 0
        tmp = torch.empty(ws, dtype=torch.uint8, device="cuda")
        s0 = block_stats(L)
        out_n = run_block(L, pkg, c, near, tmp=tmp)[0]
        s1 = block_stats(L)
        out_f = run_block(L, pkg, c, far, tmp=tmp)[0]
        dn, df = delta(s0, s1), delta(s1, block_stats(L))
        assert dn == df == ([1, 0, 1, 0] if hs == 64 else [0, 1, 1, 0]), (dn, df)
        check_rag(nso, "far addresses, near twin: block_paged %s hs %d bk %d" % (size, hs, bk), c, out_n)
        assert np.all(np.isfinite(out_f)), "a trap or a dead cell was consumed"
        assert same_bits(out_f, out_n)
        assert far.traps_intact()
    finally:
        near = far = tmp = None
        release()


def check_against_the_pools(nso, tag, c, lens, near, out):
    """the near twin's output against the oracle over the keys as its pools hold them"""
    for b, n in enumerate(lens):
        kb, vb = near.keys(b, n)
        assert np.all(np.isfinite(kb.astype(np.float32))) and np.all(np.isfinite(vb.astype(np.float32))), (tag, b)
        qb = c.q[b:b + 1]
        check(nso, "%s request %d (%d keys)" % (tag, b, n), out[b:b + 1], nso.attn_ref(qb, kb, vb, c.scale, CAUSAL), rounding_model(qb, kb, vb, c.scale, CAUSAL))


def written_cells_equal(near, far, cells):
    """every live block of the far twin holds the near twin's bits (the written cells, and nothing else of a block changed); cells [(request, position)]
    were written; the traps — neighbours, aliases, block 0 — are as painted"""
    bn, bf = near.blocks(), far.blocks()
    for key in bn:
        assert same_bits(bn[key][0], bf[key][0]) and same_bits(bn[key][1], bf[key][1]), key
    for b, n in cells:
        assert far.ids[(b, n // far.bk)] != 2  # a high block
        for x in (0, 1):
            assert np.all(bf[(b, n // far.bk)][x][n % far.bk] != NAN16), (b, n)
    assert far.traps_intact(), "a write landed in a trap"


@SIZES
@WRITES
@pytest.mark.parametrize("form", ["rows", "seq"])
def test_append_paged_then_decode(L, pkg, nso, size, hs, bk, form):
    """rows: ns_hip_rope_qkv_append_paged, one row per request at its last position.  seq: ns_hip_rope_qkv_append_paged_seq (NeoX pairs), two rows of
    request 1 — its last two positions, one high block — and one of request 0.  Then ns_hip_attn_decode_paged reads the blocks back."""
    import torch
    c = paged_case(nso, hs, bk)
    row_req, pos = ([0, 1], [c.lens[0] - 1, c.lens[1] - 1]) if form == "rows" else ([1, 1, 0], [c.lens[1] - 2, c.lens[1] - 1, c.lens[0] - 1])
    assert form == "rows" or pos[0] // bk == pos[1] // bk
    prior = [min(n for r, n in zip(row_req, pos) if r == b) for b in range(c.bs)]
    rows = len(pos)
    rng = np.random.default_rng(hs + bk + rows)
    q = rng.standard_normal((rows, HN, hs)).astype(np.float32)
    k = rng.standard_normal((rows, HKV, hs)).astype(np.float32)
    v = rng.standard_normal((rows, HKV, hs)).astype(np.float32)
    dk, dv = torch.from_numpy(k).cuda(), torch.from_numpy(v).cuda()
    dpos, dreq = torch.tensor(pos, dtype=torch.int32, device="cuda"), torch.tensor(row_req, dtype=torch.int32, device="cuda")

    def append(p):
        dq = torch.from_numpy(q).cuda()
        if form == "rows":
            pkg.check(L.ns_hip_rope_qkv_append_paged(dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), p.kp, p.vp, rows, HN, HKV, hs, dpos.data_ptr(), c.cap, hs, 0, 10000.0,
                                                     0.75, 0.0, 1.1, *p.table_args(), p.step_sl, p.step_head, stream_ptr()))
        else:
            pkg.check(L.ns_hip_rope_qkv_append_paged_seq(dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), p.kp, p.vp, rows, HN, HKV, hs, dpos.data_ptr(), c.cap, hs // 2, 2,
                                                         10000.0, 0.75, 0.0, 1.1, dreq.data_ptr(), c.bs, *p.table_args(), p.step_sl, p.step_head, stream_ptr()))
        torch.cuda.synchronize()
        return dq.cpu().numpy()

    near = far = None
    try:
        near = Pages("near", hs, bk, live_blocks(c.lens, bk)).fill_keys(c.k, c.v, prior)
        far = Pages(size, hs, bk, live_blocks(c.lens, bk)).fill_keys(c.k, c.v, prior)
        qn, qf = append(near), append(far)
        assert same_bits(qn, qf) and not np.array_equal(qn, q)
        written_cells_equal(near, far, list(zip(row_req, pos)))
        out = decode_twins(L, pkg, c, near, far, size)
        check_against_the_pools(nso, "far addresses, near twin: decode after append_paged (%s) %s hs %d bk %d" % (form, size, hs, bk), c, c.lens, near, out)
    finally:
        near = far = None
        release()


@SIZES
@WRITES
@pytest.mark.parametrize("vec", [8, 1], ids=["16_byte_copies", "element_wise"])
def test_kv_paged_store_then_decode(L, pkg, nso, size, hs, bk, vec):
    """every live row of request 1 from a small slab into its (high) blocks; vec 1: slab rows HKV * hs + 4 elements apart, which no 16-byte copy takes"""
    import torch
    c = paged_case(nso, hs, bk)
    n = c.lens[1]
    s_sl, s_head = HKV * hs + (0 if vec == 8 else 4), hs
    slab_k, slab_v = (torch.zeros(n * s_sl, dtype=torch.int16, device="cuda") for _ in range(2))
    for slab, x in ((slab_k, c.k), (slab_v, c.v)):
        torch.as_strided(slab, (n, HKV, hs), (s_sl, s_head, 1)).copy_(torch.from_numpy(np.array(x[1, :n], order="C").view(np.int16)).cuda())

    def store(p):
        row = C.c_void_p(p.dt.data_ptr() + 4 * p.ts)  # request 1's table row
        pkg.check(L.ns_hip_kv_paged_store(slab_k.data_ptr(), slab_v.data_ptr(), s_sl, s_head, 0, n, HKV, hs, p.kp, p.vp, row, p.ts, bk, p.pool_blocks, p.block_step,
                                          p.step_sl, p.step_head, stream_ptr()))
        torch.cuda.synchronize()

    near = far = None
    try:
        near = Pages("near", hs, bk, live_blocks(c.lens, bk)).fill_keys(c.k, c.v, [c.lens[0], 0])
        far = Pages(size, hs, bk, live_blocks(c.lens, bk)).fill_keys(c.k, c.v, [c.lens[0], 0])
        store(near), store(far)
        written_cells_equal(near, far, [(1, x) for x in range(n)])
        kb, vb = far.keys(1, n)
        assert same_bits(kb[0], c.k[1, :n]) and same_bits(vb[0], c.v[1, :n])
        out = decode_twins(L, pkg, c, near, far, size)
        check_case(nso, "far addresses, near twin: decode after kv_paged_store (vec %d) %s hs %d bk %d" % (vec, size, hs, bk), c, out)
    finally:
        near = far = None
        release()


# ---- slabs: the strides place a small problem far out -------------------------------------------------------------------------------------------------
def geometry(kind, hs, rows, far):
    """K / V of [bs][rows][HKV][hs]: (bs, K strides (batch, row, head, dim), V strides, K extents, V extents)"""
    row = HKV * hs
    if kind == "batch":  # position-major slabs; far: entry 2 starts beyond 2^31 elements
        sbs = FL.SLAB_STEP if far else rows * row
        st = (sbs, row, hs, 1)
        ext = [(b * sbs, rows * row) for b in range(3)]
        return 3, st, st, ext, ext
    if kind == "head":  # head-major slabs; far: (entry 1, kv head 1) starts beyond 2^31 elements
        shead = FL.HEAD_STEP if far else rows * hs
        sbs = FL.SLAB_STEP if far else HKV * shead
        st = (sbs, hs, shead, 1)
        ext = [(b * sbs + h * shead, rows * hs) for b in range(2) for h in range(HKV)]
        assert not far or ext[-1][0] > E31
        return 2, st, st, ext, ext
    assert kind == "k_transposed"  # K [bs][HKV][hs][rows]: attn_kernel
    sbs = FL.SLAB_STEP if far else rows * row
    ext = [(b * sbs, rows * row) for b in range(3)]
    return 3, (sbs, 1, hs * rows, rows), (sbs, row, hs, 1), ext, ext


def slabs(kind, hs, k, v, far):
    """(K, V as Far, K strides, V strides) holding k / v [bs][rows][HKV][hs]"""
    rows = k.shape[1]
    bs, ks, vs, kext, vext = geometry(kind, hs, rows, far)
    assert bs == k.shape[0]
    total = max(o + n for o, n in kext) + HKV * hs
    assert not far or max(o for o, _ in kext) > E31
    if far:
        need(4 * total)
    K, V = Far(total, kext, HKV * hs, traps=far), Far(total, vext, HKV * hs, traps=far)
    K.put(0, ks, k), V.put(0, vs, v)
    return K, V, ks, vs


def slab_args(pkg, a, ks, vs):
    a.step_k_bs, a.step_k_sl, a.step_k_head_num, a.step_k_head_size = ks
    a.step_v_bs, a.step_v_sl, a.step_v_head_num, a.step_v_head_size = vs
    return a


def forward(L, pkg, q, K, V, ks, vs, sl_kv, shadow):
    """ns_hip_attn_fp32_fp16_fp16_fp32_forward (shadow: _forward_h with an fp16 shadow); (dst, shadow or None, the slots ns_hip_attn_stats moved by)"""
    import torch
    bs, sl_q, hn, hs = q.shape
    dq = torch.from_numpy(q.copy()).cuda()
    dd = torch.full(q.shape, 7.0, device="cuda")
    d16 = torch.full(q.shape, 7.0, device="cuda", dtype=torch.float16) if shadow else None
    a = slab_args(pkg, pkg.attn_args(dq.data_ptr(), K.ptr, V.ptr, dd.data_ptr(), bs, hn, HKV, hs, sl_q, sl_kv, float(1.0 / np.sqrt(hs)), CAUSAL), ks, vs)
    s0 = attn_stats(L)
    if shadow:
        pkg.check(L.ns_hip_attn_fp32_fp16_fp16_fp32_forward_h(C.byref(a), d16.data_ptr(), stream_ptr()))
    else:
        pkg.check(L.ns_hip_attn_fp32_fp16_fp16_fp32_forward(C.byref(a), stream_ptr()))
    torch.cuda.synchronize()
    return dd.cpu().numpy(), (d16.cpu().numpy() if shadow else None), delta(s0, attn_stats(L))


def one_slot(d, slot):
    return d == [1 if i == slot else 0 for i in range(8)]


FORWARD = {  # name: (geometry, query rows, keys, knobs of both twins, slot of ns_hip_attn_stats, fp16 shadow)
    "batch_1_row_ring": ("batch", 1, 200, {}, RING, False),
    "batch_1_row_registers": ("batch", 1, 200, {"attn_stream": 0}, REGS, False),
    "batch_5_rows": ("batch", 5, 200, {}, RING, False),
    "batch_40_rows_mfma": ("batch", 40, 200, {}, 4, True),
    "batch_130_rows_mfma3": ("batch", 130, 200, {}, 6, True),
    "batch_16_rows_300_keys_block_split": ("batch", 16, 300, {"attn_block_split": 256}, 7, False),
    "head_1_row": ("head", 1, 200, {}, RING, False),
    "head_40_rows_mfma": ("head", 40, 200, {}, 4, False),
    "k_transposed_1_row_generic": ("k_transposed", 1, 200, {}, 1, False),
}
_fwd = {}


def forward_inputs(nso, bs, hs, sl_q, sl_kv):
    """q, k, v, reference and rounding model of a shape: made once, read-only"""
    key = (bs, hs, sl_q, sl_kv)
    if key not in _fwd:
        rng = np.random.default_rng(sl_q * 1000 + sl_kv + hs + bs)
        q = rng.standard_normal((bs, sl_q, HN, hs)).astype(np.float32)
        k = rng.standard_normal((bs, sl_kv, HKV, hs)).astype(np.float16)
        v = rng.standard_normal((bs, sl_kv, HKV, hs)).astype(np.float16)
        scale = float(1.0 / np.sqrt(hs))
        _fwd[key] = (q, k, v, nso.attn_ref(q, k, v, scale, CAUSAL), rounding_model(q, k, v, scale, CAUSAL))
        for x in _fwd[key]:
            x.setflags(write=False)
    return _fwd[key]


@pytest.mark.parametrize("hs", [64, 128])
@pytest.mark.parametrize("name", list(FORWARD))
def test_forward_on_far_slabs(L, pkg, nso, name, hs):
    """every batch entry and head is compared, the far ones among them"""
    kind, sl_q, sl_kv, knobs, slot, shadow = FORWARD[name]
    bs = geometry(kind, hs, sl_kv, False)[0]
    q, k, v, ref, model = forward_inputs(nso, bs, hs, sl_q, sl_kv)
    near = far = None
    try:
        near, far = slabs(kind, hs, k, v, False), slabs(kind, hs, k, v, True)
        with tuning(L, **knobs):
            out_n, h_n, dn = forward(L, pkg, q, *near, sl_kv, shadow)
            out_f, h_f, df = forward(L, pkg, q, *far, sl_kv, shadow)
        assert one_slot(dn, slot) and df == dn, (name, dn, df)
        check(nso, "far addresses, near twin: forward %s hs %d" % (name, hs), out_n, ref, model)
        assert np.all(np.isfinite(out_f)), "a trap or a dead cell was consumed"
        assert same_bits(out_f, out_n)
        if shadow:
            assert same_bits(h_f, h_n) and same_bits(h_n, out_n.astype(np.float16))
        assert far[0].traps_intact() and far[1].traps_intact()
    finally:
        near = far = None
        release()


@pytest.mark.parametrize("hs", [64, 128])
def test_rows_entries_on_far_slabs(L, pkg, nso, hs):
    """ns_hip_rope_qkv_append_rows writes each request's last position, ns_hip_attn_decode_rows reads the slabs back (ring and register kernel): three
    requests a batch step of 2^30 + 2^21 elements apart, the last one beyond 2^31"""
    import torch
    bs, cap, lens = 3, 256, [70, 200, 150]
    if ("rows", hs) not in _cases:
        _cases[("rows", hs)] = Case(nso, bs, HN, HKV, hs, cap, lens)
    c = _cases[("rows", hs)]
    k, v = c.behind(NAN16, [n - 1 for n in lens])  # (keys [0, len - 1); NaN from the position the append writes on, the 64 rows behind the capacity included)
    rows_alloc = k.shape[1]
    rng = np.random.default_rng(hs + 5)
    q = rng.standard_normal((bs, HN, hs)).astype(np.float32)
    kn = rng.standard_normal((bs, HKV, hs)).astype(np.float32)
    vn = rng.standard_normal((bs, HKV, hs)).astype(np.float32)
    dk, dv = torch.from_numpy(kn).cuda(), torch.from_numpy(vn).cuda()
    dpos = torch.tensor([n - 1 for n in lens], dtype=torch.int32, device="cuda")

    def append(K, V, ks, vs):
        dq = torch.from_numpy(q).cuda()
        pkg.check(L.ns_hip_rope_qkv_append_rows(dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), K.ptr, V.ptr, bs, HN, HKV, hs, dpos.data_ptr(), cap, hs, 0, 10000.0, 0.75,
                                                0.0, 1.1, ks[0], ks[1], ks[2], stream_ptr()))
        torch.cuda.synchronize()
        return dq.cpu().numpy(), K.get(0, (bs, rows_alloc, HKV, hs), ks), V.get(0, (bs, rows_alloc, HKV, hs), vs)

    def decode(K, V, ks, vs):
        dq = torch.from_numpy(c.q.copy()).cuda()
        dd = torch.full((bs, 1, HN, hs), 7.0, device="cuda")
        a = slab_args(pkg, pkg.attn_args(dq.data_ptr(), K.ptr, V.ptr, dd.data_ptr(), bs, HN, HKV, hs, 1, cap, c.scale, CAUSAL), ks, vs)
        r0 = rows_stats(L)
        pkg.check(L.ns_hip_attn_decode_rows(C.byref(a), C.c_void_p(dpos.data_ptr()), 1, None, stream_ptr()))
        torch.cuda.synchronize()
        return dd.cpu().numpy(), delta(r0, rows_stats(L))

    near = far = None
    try:
        near, far = slabs("batch", hs, k, v, False), slabs("batch", hs, k, v, True)
        (qn, kn_, vn_), (qf, kf_, vf_) = append(*near), append(*far)
        assert same_bits(qn, qf) and not np.array_equal(qn, q)
        assert same_bits(kn_, kf_) and same_bits(vn_, vf_)  # every request's slab, the first and the last among them
        for b, n in enumerate(lens):
            assert np.all(kf_[b, n - 1] != NAN16) and np.all(kf_[b, n:] == NAN16) and same_bits(vf_[b, n - 1], vn[b].astype(np.float16))
        assert far[0].traps_intact() and far[1].traps_intact(), "a write landed in a trap"
        for stream in (1, 0):
            with tuning(L, attn_stream=stream):
                out_n, dn = decode(*near)
                out_f, df = decode(*far)
            assert dn == df and dn[1 - stream] == 1 and dn[stream] == 0 and dn[3] == 0, (stream, dn, df)
            assert np.all(np.isfinite(out_f)) and same_bits(out_f, out_n)
            for b, n in enumerate(lens):
                kb, vb = kn_[b:b + 1, :n].view(np.float16), vn_[b:b + 1, :n].view(np.float16)
                check(nso, "far addresses, near twin: decode_rows stream %d hs %d request %d" % (stream, hs, b), out_n[b:b + 1],
                      nso.attn_ref(c.q[b:b + 1], kb, vb, c.scale, CAUSAL), rounding_model(c.q[b:b + 1], kb, vb, c.scale, CAUSAL))
    finally:
        near = far = None
        release()


@pytest.mark.parametrize("seq", [1, 16], ids=["decode_form", "table_form"])
def test_rope_qkv_append_at_a_far_position(L, pkg, seq):
    """n_past 2100 with cache rows 2^20 elements apart: the written rows start beyond 2^31 elements (4.4 GiB of K and of V).  The rows and Q hold the
    bits of the call on a compact cache, Q those of ns_hip_rope_f32 at that position; the rows in front of and behind the written ones, the row the
    offset mod 2^31 names (position 52 on) and the strips around them are unchanged."""
    import torch
    hs, n_past = 64, FL.ROPE_PAST
    row = HKV * hs
    rng = np.random.default_rng(seq)
    q = rng.standard_normal((1, seq, HN, hs)).astype(np.float32)
    k = rng.standard_normal((1, seq, HKV, hs)).astype(np.float32)
    v = rng.standard_normal((1, seq, HKV, hs)).astype(np.float32)
    dk, dv = torch.from_numpy(k).cuda(), torch.from_numpy(v).cuda()
    st = stream_ptr()
    rq, rk = torch.from_numpy(q).cuda(), dk.clone()
    pkg.check(L.ns_hip_rope_f32(rq.data_ptr(), rq.data_ptr(), 1, seq, HN, hs, n_past, hs, 0, 10000.0, 1.0, 0.0, 1.0, st))
    pkg.check(L.ns_hip_rope_f32(rk.data_ptr(), rk.data_ptr(), 1, seq, HKV, hs, n_past, hs, 0, 10000.0, 1.0, 0.0, 1.0, st))

    def run(c_sl, traps):
        total = (n_past + seq + 1) * c_sl
        extents = [((n_past + i) * c_sl, row) for i in range(seq)]
        dead = [((n_past - 1) * c_sl, row), ((n_past + seq) * c_sl, row)]
        assert not traps or extents[0][0] > E31
        if traps:
            need(4 * total)
        K, V = (Far(total, extents, row, dead=dead if traps else (), traps=traps) for _ in range(2))
        for x in (K, V):
            x.paint(extents[0][0], (seq, row), (c_sl, 1), 0x5A5B)
        dq = torch.from_numpy(q).cuda()
        pkg.check(L.ns_hip_rope_qkv_append(dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), K.ptr, V.ptr, seq, HN, HKV, hs, n_past, hs, 0, 10000.0, 1.0, 0.0, 1.0, c_sl, hs, st))
        torch.cuda.synchronize()
        got = dq, K.get(extents[0][0], (seq, HKV, hs), (c_sl, hs, 1)), V.get(extents[0][0], (seq, HKV, hs), (c_sl, hs, 1))
        assert K.traps_intact() and V.traps_intact(), "a write landed in a trap"
        return got

    try:
        qn, kn, vn = run(row, False)
        qf, kf, vf = run(FL.ROPE_SL, True)
        assert torch.equal(qn, rq) and torch.equal(qf, rq)
        assert same_bits(kf, kn) and same_bits(vf, vn)
        assert same_bits(kf, rk[0].half().cpu().numpy()) and same_bits(vf, v[0].astype(np.float16)) and np.all(kf != 0x5A5B)
    finally:
        release()


# ---- the slab rule's boundary: a few hundred keys a very large row step apart ------------------------------------------------------------------------
def edge_slabs(hs, k, v, step_sl, dead_rows, far):
    """K / V [1][n][HKV][hs] with rows step_sl apart; dead_rows: the rows behind the last key a kernel may ask for — poisoned where they lie inside
    the tensor, and where their byte offsets mod 2^32 point"""
    n, row = k.shape[1], HKV * hs
    extents = [(r * step_sl, row) for r in range(n)]
    dead = [(r * step_sl, row) for r in range(n, n + dead_rows)]
    total = (n - 1 + (dead_rows if far == "with_dead_rows" else 0)) * step_sl + 2 * row
    if far:
        need(4 * total)
    K, V = (Far(total, extents, row, dead=dead if far else (), traps=bool(far)) for _ in range(2))
    st = (0, step_sl, hs, 1)  # (one batch entry: no batch step)
    K.put(0, st, k), V.put(0, st, v)
    return K, V, st, st


@pytest.mark.parametrize("hs", [64, 128])
@pytest.mark.parametrize("side", ["below", "above"])
def test_slab_rule_boundary_decode(L, pkg, nso, side, hs):
    """300 keys, rows as far apart as attn_in32 lets the ring kernel take them (descriptor offsets up to 2^32 - 4096 bytes), and one step of 8 elements
    more, which the register kernel serves.  The ring kernel also requests up to 128 rows behind the last key; their offsets wrap, they are read from
    inside the descriptor — the places hold traps — and must count as zeros."""
    n = FL.EDGE_KEYS
    below, above = FL.edge_steps(n)
    q, k, v, ref, model = forward_inputs(nso, 1, hs, 1, n)
    want = RING if side == "below" else REGS
    near = far = None
    try:
        near = edge_slabs(hs, k, v, HKV * hs, 0, False)
        far = edge_slabs(hs, k, v, below if side == "below" else above, 128, "far")
        with tuning(L, attn_stream=1 if want == RING else 0):
            out_n, _, dn = forward(L, pkg, q, *near, n, False)
        out_f, _, df = forward(L, pkg, q, *far, n, False)
        assert one_slot(df, want) and df == dn, (side, dn, df)
        check(nso, "far addresses, near twin: slab rule %s, decode hs %d" % (side, hs), out_n, ref, model)
        assert np.all(np.isfinite(out_f)), "a trap was consumed"
        assert same_bits(out_f, out_n)
    finally:
        near = far = None
        release()


@pytest.mark.parametrize("hs", [64, 128])
@pytest.mark.parametrize("side", ["below", "above", "between_keys_and_tiles"])
def test_slab_rule_boundary_prefill(L, pkg, nso, side, hs):
    """130 query rows over 300 keys.  attn_mfma3_kernel requests whole 64-key tiles, so its rule counts the 320 rows of five tiles: below it the DMA kernel
    runs with offsets up to 2^32 - 4096 bytes and equals its compact twin bit for bit; one step above it, and at the largest step that keeps the 300
    KEYS inside a descriptor (where the rows 301 .. 319 wrap: the plan used to send this call to the DMA kernel, which then multiplied zero weights
    with whatever the wrapped offsets held), attn_mfma2_kernel serves.  It has no compact twin (module docstring): reference and bar alone."""
    n, sl_q = FL.EDGE_KEYS, 130
    below, above = FL.edge_steps(FL.tile_rows(n))
    step = {"below": below, "above": above, "between_keys_and_tiles": FL.edge_steps(n)[0]}[side]
    assert below < above < FL.edge_steps(n)[0]
    q, k, v, ref, model = forward_inputs(nso, 1, hs, sl_q, n)
    near = far = None
    try:
        far = edge_slabs(hs, k, v, step, FL.tile_rows(n) - n, "with_dead_rows")
        out_f, _, df = forward(L, pkg, q, *far, n, False)
        assert one_slot(df, 6 if side == "below" else 5), (side, df)
        assert np.all(np.isfinite(out_f)), "a trap was consumed"
        check(nso, "far addresses: slab rule %s, prefill hs %d" % (side, hs), out_f, ref, model)
        if side == "below":
            near = edge_slabs(hs, k, v, HKV * hs, 0, False)
            out_n, _, dn = forward(L, pkg, q, *near, n, False)
            assert dn == df and same_bits(out_f, out_n)
    finally:
        near = far = None
        release()

"""Batched decode over per-request context lengths: ns_hip_rope_qkv_append_rows (one position per row, one cache slab per request) and
ns_hip_attn_decode_rows (one query row per request, each over its own live keys; the one-row split kernels' ROWS instantiations, planned for the
capacity of a slab, the live length read per batch entry inside the launch).  docs/kernels/attention.md, "Decode over per-request context lengths".

Reference and bounds are the project's: nso.attn_ref per request, check() / rounding_model() of tests/test_gpu_attention_paths.py (rel_l2 < 1e-3 over
the tensor and the per-row bound).  Two flags the two do not know get an fp64 model written here (model64): the tanh cap, which the oracle's
attention does not have (the fp64 model is then the reference too), and ALiBi in the rounding model.

A cache slab here has 64 allocated rows behind its capacity, and every row from a request's live length on holds 0xFF bytes (fp16 NaN) unless a test
says otherwise: whatever consumes a byte behind a live length shows as NaN, and a wrong clamp does not become an access outside the allocation."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_attention_paths import check, rounding_model

pytestmark = pytest.mark.gpu
SLACK = 64
CAUSAL, ALIBI, TANH = 1, 2, 8
PM, HM = "position-major", "head-major"


# ---- shared helpers ---------------------------------------------------------------------------------------------------------------
def stream_ptr():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def strides(layout, rows, hkv, hs):
    """(step_bs, step_sl, step_head) in elements of a slab with `rows` allocated rows"""
    return (rows * hkv * hs, hkv * hs, hs) if layout == PM else (hkv * rows * hs, hs, rows * hs)


def to_slabs(x, layout):
    """numpy [bs][rows][hkv][hs] -> the device tensor of the layout"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(x if layout == PM else x.transpose(0, 2, 1, 3))).cuda()


def rows_stats(L):
    out = (C.c_ulonglong * 4)()
    L.ns_hip_attn_rows_stats(out)
    return list(out)


def attn_stats(L):
    out = (C.c_uint64 * 8)()
    L.ns_hip_attn_stats(out)
    return list(out)


def model64(q, k, v, scale, flags, rounded):
    """fp64 attention of ONE request (q [1][1][hn][hs], k / v [1][len][hkv][hs]) with ALiBi and the tanh cap; rounded: the operand roundings of
    rounding_model (Q to fp16, the unnormalised weights to fp16 in front of P.V)"""
    hn, hs = q.shape[2], q.shape[3]
    hkv = k.shape[2]
    lf = 1 << int(np.floor(np.log2(hn)))
    m0, m1 = 2.0 ** (-8.0 / lf), 2.0 ** (-4.0 / lf)
    qq = q.astype(np.float16).astype(np.float64) if rounded else q.astype(np.float64)
    out = np.zeros(q.shape, np.float64)
    for h in range(hn):
        kk, vv = k[0, :, h // (hn // hkv)].astype(np.float64), v[0, :, h // (hn // hkv)].astype(np.float64)
        s = kk @ qq[0, 0, h] * float(np.float32(scale))
        if flags & TANH:
            s = 30.0 * np.tanh(s / 30.0)
        if flags & ALIBI:
            s = s + np.arange(len(s)) * (m0 ** (h + 1) if h < lf else m1 ** (2 * (h - lf) + 1))
        p = np.exp(s - s.max())
        pv = p.astype(np.float16).astype(np.float64) if rounded else p
        out[0, 0, h] = (pv @ vv) / p.sum()
    return out


class Case:
    """inputs of one case, made once: q fp32 [bs][1][hn][hs], k / v fp16 [bs][cap + SLACK][hkv][hs] (valid everywhere: the tests decide what lies
    behind a live length), the per-request reference and rounding model"""

    def __init__(self, nso, bs, hn, hkv, hs, cap, lens, flags=CAUSAL, scales=(1.0, 1.0, 1.0, 1.0), qmul=1.0):
        self.bs, self.hn, self.hkv, self.hs, self.cap, self.lens, self.flags, self.scales = bs, hn, hkv, hs, cap, list(lens), flags, scales
        rng = np.random.default_rng(hs * 7 + cap + bs)
        self.q = (rng.standard_normal((bs, 1, hn, hs)) * qmul).astype(np.float32)
        self.k = rng.standard_normal((bs, cap + SLACK, hkv, hs)).astype(np.float16)
        self.v = rng.standard_normal((bs, cap + SLACK, hkv, hs)).astype(np.float16)
        self.scale = float(1.0 / np.sqrt(hs))
        self.ref, self.model = {}, {}
        for b, n in enumerate(self.lens):
            if n == 0:
                continue
            qb, kb, vb = self.q[b:b + 1], self.k[b:b + 1, :n], self.v[b:b + 1, :n]
            if flags & (ALIBI | TANH):
                mult = scales[2] / scales[3]
                sc = self.scale * scales[0] * scales[1]
                self.model[b] = model64(qb, kb, vb, sc, flags, True) * mult
                self.ref[b] = model64(qb, kb, vb, sc, flags, False) * mult if flags & TANH else nso.attn_ref(qb, kb, vb, self.scale, flags & ~TANH, scales=scales)
            else:
                self.ref[b] = nso.attn_ref(qb, kb, vb, self.scale, flags, scales=scales)
                self.model[b] = rounding_model(qb, kb, vb, self.scale, flags, scales)
        for x in (self.q, self.k, self.v):
            x.setflags(write=False)

    def behind(self, fill, lens=None):
        """k, v with every row from a request's live length on (the slack rows included) holding the 16-bit pattern `fill`"""
        k, v = self.k.copy(), self.v.copy()
        for b, n in enumerate(self.lens if lens is None else lens):
            k[b, n:].view(np.uint16)[...] = fill
            v[b, n:].view(np.uint16)[...] = fill
        return k, v


def run_rows(L, pkg, c, layout=PM, fill=0xFFFF, lens_dev=None, bias=1, dst16=False, dst_pad=0, tmp=None, behind_lens=None):
    """ns_hip_attn_decode_rows on case c; lens_dev: the values of dKvLens (default: live length - bias).  Returns (dst [bs][1][hn][hs] numpy, the
    fp16 shadow or None, the whole dst buffer): dst starts as 7.0; dst_pad > 0: rows hs + dst_pad floats apart, heads and requests accordingly."""
    import torch
    k, v = c.behind(fill, behind_lens)
    dk, dv = to_slabs(k, layout), to_slabs(v, layout)
    dq = torch.from_numpy(c.q.copy()).cuda()
    row = c.hs + dst_pad
    dd = torch.full((c.bs, 1, c.hn, row), 7.0, device="cuda")
    d16 = torch.full((c.bs, 1, c.hn, row), 7.0, device="cuda", dtype=torch.float16) if dst16 else None
    vals = [n - bias for n in c.lens] if lens_dev is None else lens_dev
    dl = torch.tensor(vals, dtype=torch.int32, device="cuda")
    a = pkg.attn_args(dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), dd.data_ptr(), c.bs, c.hn, c.hkv, c.hs, 1, c.cap, c.scale, c.flags)
    a.Q_sc, a.K_sc, a.V_sc, a.dst_sc = c.scales
    a.step_k_bs, a.step_k_sl, a.step_k_head_num = strides(layout, c.cap + SLACK, c.hkv, c.hs)
    a.step_v_bs, a.step_v_sl, a.step_v_head_num = strides(layout, c.cap + SLACK, c.hkv, c.hs)
    a.step_dst_bs, a.step_dst_head_num, a.step_dst_sl = c.hn * row, row, c.hn * row
    if tmp is not None:
        a.tmp = tmp.data_ptr()
    pkg.check(L.ns_hip_attn_decode_rows(C.byref(a), C.c_void_p(dl.data_ptr()), bias, C.c_void_p(d16.data_ptr()) if dst16 else None, stream_ptr()))
    torch.cuda.synchronize()
    whole = dd.cpu().numpy()
    return np.ascontiguousarray(whole[..., :c.hs]), (d16.cpu().numpy() if dst16 else None), whole


def check_case(nso, tag, c, out, lens=None):
    for b, n in enumerate(c.lens if lens is None else lens):
        if n == 0:
            assert np.all(out[b] == 0.0), (tag, b)
        else:
            check(nso, "%s request %d (%d keys)" % (tag, b, n), out[b:b + 1], c.ref[b], c.model[b])


# ---- 1. RoPE rows ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pos", [[0, 7, 300, 2047, -1], [0, 2048, 300, 2047, -1]], ids=["idle_negative", "idle_at_pos_cap"])
@pytest.mark.parametrize("layout", [PM, HM])
@pytest.mark.parametrize("mode,n_dims", [(0, 64), (2, 64), (2, 32)])
def test_rope_rows_are_bit_equal_to_the_per_request_loop(L, pkg, nso, mode, n_dims, layout, pos):
    """5 rows, 4 / 2 heads of size 64, pos_cap 2048; caches pre-filled with a byte pattern.  The per-request loop is ns_hip_rope_qkv_append(seq 1,
    n_past = pos[r]) on slab r's pointers for the live rows: Q, and both caches whole, must hold the same bits — so the cells (r, pos[r]) are the
    loop's, every other cache byte is untouched, and the idle rows' Q stays as it was."""
    import torch
    rows, heads, hkv, hs, pos_cap = 5, 4, 2, 64, 2048
    c_bs, c_sl, c_head = strides(layout, pos_cap, hkv, hs)
    rng = np.random.default_rng(mode * 100 + n_dims)
    q = rng.standard_normal((rows, heads, hs)).astype(np.float32)
    k = rng.standard_normal((rows, hkv, hs)).astype(np.float32)
    v = rng.standard_normal((rows, hkv, hs)).astype(np.float32)
    dk, dv, dpos = torch.from_numpy(k).cuda(), torch.from_numpy(v).cuda(), torch.tensor(pos, dtype=torch.int32, device="cuda")
    st = stream_ptr()
    pattern = 0x5A5B
    res = {}
    for form in ("rows", "loop"):
        dq = torch.from_numpy(q).cuda()
        kc = torch.full((rows * c_bs,), pattern, dtype=torch.int16, device="cuda")
        vc = torch.full((rows * c_bs,), pattern, dtype=torch.int16, device="cuda")
        if form == "rows":
            pkg.check(L.ns_hip_rope_qkv_append_rows(dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), kc.data_ptr(), vc.data_ptr(), rows, heads, hkv, hs,
                                                    dpos.data_ptr(), pos_cap, n_dims, mode, 10000.0, 0.75, 0.0, 1.1, c_bs, c_sl, c_head, st))
        else:
            for r, p in enumerate(pos):
                if 0 <= p < pos_cap:
                    pkg.check(L.ns_hip_rope_qkv_append(dq[r].data_ptr(), dk[r].data_ptr(), dv[r].data_ptr(), kc.data_ptr() + 2 * r * c_bs,
                                                       vc.data_ptr() + 2 * r * c_bs, 1, heads, hkv, hs, p, n_dims, mode, 10000.0, 0.75, 0.0, 1.1, c_sl,
                                                       c_head, st))
        torch.cuda.synchronize()
        res[form] = (dq.cpu().numpy(), kc.cpu().numpy(), vc.cpu().numpy())
    for x, y in zip(res["rows"], res["loop"]):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    # said once more without the loop: what was written, and where
    dq, kc, vc = res["rows"]
    touched = np.zeros(rows * c_bs, bool)
    for r, p in enumerate(pos):
        if 0 <= p < pos_cap:
            for h in range(hkv):
                o = r * c_bs + p * c_sl + h * c_head
                touched[o:o + hs] = True
                assert np.array_equal(vc[o:o + hs].view(np.float16), v[r, h].astype(np.float16))
            assert not np.array_equal(dq[r], q[r])
        else:
            assert np.array_equal(dq[r], q[r])
    assert touched.sum() == sum(0 <= p < pos_cap for p in pos) * hkv * hs
    assert np.all(kc[~touched] == pattern) and np.all(vc[~touched] == pattern) and np.all(kc[touched] != pattern)


def test_rope_rows_refusals(L, pkg):
    import torch
    t = torch.zeros(4096, device="cuda")
    p = torch.zeros(4, dtype=torch.int32, device="cuda")
    args = lambda mode, ext, pos: (t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), 2, 4, 2, 64, pos, 16, 64, mode, 10000.0, 1.0, ext,
                                   1.0, 2048, 128, 64, stream_ptr())
    assert L.ns_hip_rope_qkv_append_rows(*args(4, 0.0, p.data_ptr())) == -1 and "modes 0 and 2" in pkg.last_error()
    assert L.ns_hip_rope_qkv_append_rows(*args(0, 1.0, p.data_ptr())) == -1 and "YaRN" in pkg.last_error()
    assert L.ns_hip_rope_qkv_append_rows(*args(0, 0.0, None)) == -1 and "invalid argument" in pkg.last_error()
    L.ns_hip_reset_error()


# ---- 2. attention against the reference ---------------------------------------------------------------------------------------------------
ATTN_CASES = {  # name: (batch, heads, kv heads, head size, capacity, lengths, flags, layout, serving kernel: slot of ns_hip_attn_rows_stats)
    "one_key_and_full": (4, 4, 4, 128, 512, [1, 37, 256, 512], CAUSAL, PM, 0),
    "gqa_eight_lanes": (3, 8, 2, 64, 1024, [1000, 129, 5], CAUSAL, HM, 0),
    "idle_slot_one_kv_head": (5, 8, 1, 128, 300, [300, 0, 64, 65, 299], CAUSAL | ALIBI, PM, 0),
    "regs_256": (2, 4, 4, 256, 512, [511, 3], CAUSAL | TANH, PM, 1),
    "regs_32": (2, 4, 4, 32, 256, [256, 33], CAUSAL, HM, 1),
    "many_ranges": (8, 8, 2, 128, 4096, [4096, 1, 2048, 17, 3000, 129, 1024, 700], CAUSAL, PM, 0),
}
_cases, _outs = {}, {}


def attn_case(nso, name):
    if name not in _cases:
        bs, hn, hkv, hs, cap, lens, flags, layout, slot = ATTN_CASES[name]
        _cases[name] = Case(nso, bs, hn, hkv, hs, cap, lens, flags, qmul=3.0 if flags & TANH else 1.0)  # (scores large enough for the cap to matter)
    return _cases[name]


def rows_out(L, pkg, nso, name):
    """the default call's output of a case: computed once, shared, never written to"""
    if name not in _outs:
        _outs[name] = run_rows(L, pkg, attn_case(nso, name), ATTN_CASES[name][7])[0]
        _outs[name].setflags(write=False)
    return _outs[name]


@pytest.mark.parametrize("name", list(ATTN_CASES))
def test_attention_rows_against_the_reference(L, pkg, nso, name):
    c, layout, slot = attn_case(nso, name), ATTN_CASES[name][7], ATTN_CASES[name][8]
    _outs.pop(name, None)
    r0, a0 = rows_stats(L), attn_stats(L)
    out = rows_out(L, pkg, nso, name)
    r1, a1 = rows_stats(L), attn_stats(L)
    check_case(nso, "rows %s" % name, c, out)
    # which kernel served, and that nothing else moved: one launch on the ring (slot 0) or the register kernel (slot 1), the merge launch if
    # the capacity has ranges, no refusal; in ns_hip_attn_stats the same launch by kernel family ([3] ring, [2] registers)
    dr, da = [y - x for x, y in zip(r0, r1)], [y - x for x, y in zip(a0, a1)]
    assert dr[slot] == 1 and dr[1 - slot] == 0 and dr[2] in (0, 1) and dr[3] == 0, dr
    assert da == [1 if i == (3 if slot == 0 else 2) else 0 for i in range(8)], da
    if name == "many_ranges":
        assert dr[2] == 1


# ---- 3. against the existing device entry, once per request with sl_kv = len_b ----------------------------------------------------------
@pytest.mark.parametrize("name", list(ATTN_CASES))
def test_rows_against_one_uniform_call_per_request(L, pkg, nso, name):
    """Bound: 2e-6 relative L2, over the case's tensor and over every request of it: the project's figure for two one-row launches that split a context differently
    (tests/test_gpu_attention.py: the ring kernel against the register kernel).  Here the kernel is the same and only the ranges differ: the uniform
    call plans for (batch 1, len_b keys), the per-request call for (batch, capacity) with the range rule applied to len_b.
    Measured on an MI355X, rel_l2 over the tensor / worst request (also in docs/kernels/attention.md, "Decode over per-request context lengths"):
    one_key_and_full 3.8e-08 / 1.4e-07, gqa_eight_lanes 3.2e-08 / 1.8e-07, idle_slot_one_kv_head 8.6e-08 / 1.1e-07, regs_256 0 / 0, regs_32 0 / 0,
    many_ranges 2.3e-08 / 2.6e-07 — the register kernel's cases land on the same ranges in both forms."""
    import torch
    c, layout = attn_case(nso, name), ATTN_CASES[name][7]
    out = rows_out(L, pkg, nso, name)
    k, v = c.behind(0xFFFF)
    dk, dv, dq = to_slabs(k, layout), to_slabs(v, layout), torch.from_numpy(c.q.copy()).cuda()
    dd = torch.zeros((c.bs, 1, c.hn, c.hs), device="cuda")
    s_bs, s_sl, s_head = strides(layout, c.cap + SLACK, c.hkv, c.hs)
    for b, n in enumerate(c.lens):
        if n == 0:
            continue
        a = pkg.attn_args(dq[b].data_ptr(), dk[b].data_ptr(), dv[b].data_ptr(), dd[b].data_ptr(), 1, c.hn, c.hkv, c.hs, 1, n, c.scale, c.flags)
        a.step_k_bs, a.step_k_sl, a.step_k_head_num = s_bs, s_sl, s_head
        a.step_v_bs, a.step_v_sl, a.step_v_head_num = s_bs, s_sl, s_head
        pkg.check(L.ns_hip_attn_fp32_fp16_fp16_fp32_forward(C.byref(a), stream_ptr()))
    torch.cuda.synchronize()
    loop = dd.cpu().numpy()
    assert np.all(np.isfinite(loop))
    per = [nso.rel_l2(out[b], loop[b]) for b, n in enumerate(c.lens) if n]
    e = nso.rel_l2(out, loop)
    print("ATTN_ROWS %s: rows vs per-request uniform calls rel_l2 %.3g (worst request %.3g)" % (name, e, max(per)))
    assert e < 2e-6 and max(per) < 2e-6, (name, e, per)


# ---- 4. nothing behind a live length is consumed ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["one_key_and_full", "gqa_eight_lanes", "regs_256", "many_ranges"])
def test_nothing_behind_a_live_length_is_consumed(L, pkg, nso, name):
    c, layout = attn_case(nso, name), ATTN_CASES[name][7]
    nan = rows_out(L, pkg, nso, name)  # (0xFF bytes from len_b on, the 64 rows behind the capacity included)
    zeros = run_rows(L, pkg, c, layout, fill=0)[0]
    assert np.all(np.isfinite(nan))
    assert np.array_equal(nan.view(np.uint32), zeros.view(np.uint32))
    # bias 0 gives the same bits as positions with bias 1
    assert np.array_equal(run_rows(L, pkg, c, layout, bias=0)[0].view(np.uint32), nan.view(np.uint32))


def test_the_clamp_of_the_lengths(L, pkg, nso):
    """capacity + 100 gives the bits of capacity (the 64 rows behind the capacity hold NaN: a wrong clamp shows), -3 the zero row"""
    name = "one_key_and_full"
    c, layout = attn_case(nso, name), ATTN_CASES[name][7]
    full = [c.cap, c.cap, 0, 0]
    at_cap = run_rows(L, pkg, c, layout, lens_dev=[c.cap, c.cap, 0, 0], bias=0, behind_lens=full)[0]
    beyond = run_rows(L, pkg, c, layout, lens_dev=[c.cap + 100, 2 ** 31 - 1, -3, -2 ** 31], bias=0, behind_lens=full)[0]
    assert np.all(np.isfinite(beyond))
    assert np.array_equal(at_cap.view(np.uint32), beyond.view(np.uint32))
    assert np.all(beyond[2:] == 0.0) and np.all(beyond[:2] != 0.0)
    # (a request's bits do not depend on its neighbours' lengths)
    assert np.array_equal(at_cap[0:1].view(np.uint32), run_rows(L, pkg, c, layout, lens_dev=[c.cap, 1, 1, 1], bias=0, behind_lens=[c.cap, 1, 1, 1])[0][0:1].view(np.uint32))


# ---- 5. captured and replayed while the lengths grow -----------------------------------------------------------------------------------------
def live_ranges(n, nsplit, min_keys, batch_keys, single_below):
    """attn_live_kps / attn_live_splits (ns_attn.h) restated"""
    if n <= single_below:
        return 1
    want = max(1, min(nsplit, -(-n // min_keys)))
    kps = -(-n // want)
    if batch_keys > 1 and want > 1:
        kps = -(-kps // batch_keys) * batch_keys
    return max(1, -(-n // kps))


def test_captured_step_replayed_while_the_lengths_grow(L, pkg, nso):
    """{rope rows; attention rows; pos += 1} captured once on a side stream (after one eager call, which allocates the stream's scratch) and replayed
    four times with new Q / K / V rows in the input buffers: every step equals the eager calls of that step bit for bit — output and both caches —
    and passes check() against the reference over the cache as it then stands.  3 requests at positions [5, 130, 255], capacity 300.
    With the shipped range rule a request goes from one live range to two at 128 -> 129 keys or below, which none of these positions crosses in four
    steps; "attn_stream_min_keys" 133 (put back afterwards) moves that step to 133 -> 134 keys, which request 1 takes at the fourth replay."""
    import torch
    bs, hn, hkv, hs, cap, pos0 = 3, 4, 2, 128, 300, [5, 130, 255]
    min_keys = 133
    # the plan of (3, 4 / 2 heads, 128, capacity 300) under that key: 2 head-group workgroups x 3 requests per range -> min(256 / 6, ceil(300 / 133)) = 3 ranges;
    # a softmax update of a two-head workgroup covers 64 keys (attn_stream_kernel, sixteen lanes per key); fewer than 32 workgroups per range: no single_below
    ranges = [[live_ranges(p + 1 + s, 3, min_keys, 64, 0) for s in range(4)] for p in pos0]
    assert ranges[1] == [1, 1, 1, 2] and ranges[0] == [1, 1, 1, 1] and ranges[2][0] >= 2, ranges
    rng = np.random.default_rng(300)
    s_bs, s_sl, s_head = strides(PM, cap + SLACK, hkv, hs)
    k0 = rng.standard_normal((bs, cap + SLACK, hkv, hs)).astype(np.float16)
    v0 = rng.standard_normal((bs, cap + SLACK, hkv, hs)).astype(np.float16)
    for b, p in enumerate(pos0):
        k0[b, p:].view(np.uint16)[...] = 0xFFFF
        v0[b, p:].view(np.uint16)[...] = 0xFFFF
    scale = float(1.0 / np.sqrt(hs))
    side = torch.cuda.Stream()
    try:
        assert L.ns_hip_set_tuning(b"attn_stream_min_keys", min_keys) == 0
        with torch.cuda.stream(side):
            qin = torch.zeros((bs, 1, hn, hs), device="cuda")
            kin, vin = torch.zeros((bs, hkv, hs), device="cuda"), torch.zeros((bs, hkv, hs), device="cuda")

            class State:
                def __init__(self):
                    self.kc, self.vc = torch.from_numpy(k0).cuda(), torch.from_numpy(v0).cuda()
                    self.pos = torch.tensor(pos0, dtype=torch.int32, device="cuda")
                    self.q = torch.zeros_like(qin)
                    self.dst = torch.full_like(qin, 7.0)
                    self.a = pkg.attn_args(self.q.data_ptr(), self.kc.data_ptr(), self.vc.data_ptr(), self.dst.data_ptr(), bs, hn, hkv, hs, 1, cap, scale, CAUSAL)
                    self.a.step_k_bs, self.a.step_k_sl, self.a.step_k_head_num = s_bs, s_sl, s_head
                    self.a.step_v_bs, self.a.step_v_sl, self.a.step_v_head_num = s_bs, s_sl, s_head

                def step(self):
                    st = stream_ptr()
                    self.q.copy_(qin)
                    pkg.check(L.ns_hip_rope_qkv_append_rows(self.q.data_ptr(), kin.data_ptr(), vin.data_ptr(), self.kc.data_ptr(), self.vc.data_ptr(), bs, hn, hkv,
                                                            hs, self.pos.data_ptr(), cap, hs, 0, 10000.0, 1.0, 0.0, 1.0, s_bs, s_sl, s_head, st))
                    pkg.check(L.ns_hip_attn_decode_rows(C.byref(self.a), C.c_void_p(self.pos.data_ptr()), 1, None, st))
                    self.pos.add_(1)

            State().step()  # the eager call in front of the capture
            side.synchronize()
            graphed, eager = State(), State()
            r0 = rows_stats(L)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                graphed.step()
            assert [y - x for x, y in zip(r0, rows_stats(L))] == [1, 0, 1, 0]  # (captured: the ring kernel and the merge launch, nothing run yet)
            assert graphed.pos.cpu().tolist() == pos0
            for s in range(4):
                step_rng = np.random.default_rng(1000 + s)
                qin.copy_(torch.from_numpy(step_rng.standard_normal(tuple(qin.shape)).astype(np.float32)))
                kin.copy_(torch.from_numpy(step_rng.standard_normal(tuple(kin.shape)).astype(np.float32)))
                vin.copy_(torch.from_numpy(step_rng.standard_normal(tuple(vin.shape)).astype(np.float32)))
                g.replay()
                eager.step()
                side.synchronize()
                lens = [p + 1 + s for p in pos0]
                assert graphed.pos.cpu().tolist() == lens and eager.pos.cpu().tolist() == lens
                assert torch.equal(graphed.dst, eager.dst), s
                assert torch.equal(graphed.kc.view(torch.int16), eager.kc.view(torch.int16)) and torch.equal(graphed.vc.view(torch.int16), eager.vc.view(torch.int16)), s
                out, q = graphed.dst.cpu().numpy(), graphed.q.cpu().numpy()
                kc, vc = graphed.kc.cpu().numpy(), graphed.vc.cpu().numpy()
                for b, n in enumerate(lens):
                    assert np.all(np.isfinite(kc[b, :n].astype(np.float32))) and np.all(np.isnan(kc[b, n:].astype(np.float32)))
                    assert np.array_equal(vc[b, n - 1], vin[b].cpu().numpy().astype(np.float16))
                    ref = nso.attn_ref(q[b:b + 1], kc[b:b + 1, :n], vc[b:b + 1, :n], scale, CAUSAL)
                    check(nso, "replay %d request %d (%d keys)" % (s, b, n), out[b:b + 1], ref, rounding_model(q[b:b + 1], kc[b:b + 1, :n], vc[b:b + 1, :n], scale, CAUSAL))
    finally:
        L.ns_hip_set_tuning(b"attn_stream_min_keys", 32)
    torch.cuda.synchronize()


# ---- 6. the merge inside the launch -----------------------------------------------------------------------------------------------------------
def test_merge_inside_the_launch_gives_the_bits_of_the_merge_launch(L, pkg, nso):
    name = "many_ranges"
    c, layout = attn_case(nso, name), ATTN_CASES[name][7]
    want = rows_out(L, pkg, nso, name)
    try:
        assert L.ns_hip_set_tuning(b"attn_inlaunch", 1) == 0
        r0 = rows_stats(L)
        got = [run_rows(L, pkg, c, layout)[0] for _ in range(2)]  # (twice: the tickets reset themselves)
        dr = [y - x for x, y in zip(r0, rows_stats(L))]
    finally:
        L.ns_hip_set_tuning(b"attn_inlaunch", 0)
    assert dr == [2, 0, 0, 0], dr  # no merge launch
    for x in got:
        assert np.array_equal(x.view(np.uint32), want.view(np.uint32))


# ---- 7. dst16, strided dst, tensor scales, the caller's workspace ----------------------------------------------------------------------------
def test_fp16_shadow_equals_the_rounded_output(L, pkg, nso):
    for name in ("idle_slot_one_kv_head", "regs_32"):
        c, layout = attn_case(nso, name), ATTN_CASES[name][7]
        out, o16, _ = run_rows(L, pkg, c, layout, dst16=True)
        assert np.array_equal(out.view(np.uint32), rows_out(L, pkg, nso, name).view(np.uint32))
        assert np.array_equal(o16.view(np.uint16), out.astype(np.float16).view(np.uint16))  # (the idle slot's row: zeros in both)


def test_strided_dst_and_the_callers_workspace(L, pkg, nso):
    import torch
    name = "many_ranges"
    c, layout = attn_case(nso, name), ATTN_CASES[name][7]
    shape = pkg.AttnShape(c.bs, c.hn, c.hkv, c.hs, 1, c.cap)
    ws = torch.empty(L.bestla_fusion_attn_workspace_size(C.byref(shape)), dtype=torch.uint8, device="cuda")
    out, o16, whole = run_rows(L, pkg, c, layout, dst16=True, dst_pad=8, tmp=ws)
    assert np.array_equal(out.view(np.uint32), rows_out(L, pkg, nso, name).view(np.uint32))
    assert np.all(whole[..., c.hs:] == 7.0) and np.all(o16[..., c.hs:] == 7.0)
    assert np.array_equal(np.ascontiguousarray(o16[..., :c.hs]).view(np.uint16), out.astype(np.float16).view(np.uint16))


def test_tensor_scales(L, pkg, nso):
    c = Case(nso, 3, 8, 2, 64, 1024, [1000, 129, 5], CAUSAL, scales=(0.5, 2.0, 3.0, 1.5))
    out = run_rows(L, pkg, c, HM)[0]
    check_case(nso, "rows with tensor scales", c, out)


# ---- 8. refusals --------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_dst_untouched(L, pkg, nso):
    import torch
    bs, hn, hkv, hs, cap = 2, 4, 4, 128, 256
    q = torch.randn((bs, 2, hn, hs), device="cuda")
    kv = torch.randn((bs * (cap + 1) * hkv * (hs + 4) + 8,), device="cuda").half()
    lens = torch.tensor([5, 9], dtype=torch.int32, device="cuda")
    dd = torch.full((bs, 2, hn, hs), 7.0, device="cuda")

    def args(sl_q=1, sl_kv=cap, k_trans=False, row=hs, off=0):
        a = pkg.attn_args(q.data_ptr(), kv.data_ptr() + off, kv.data_ptr() + off, dd.data_ptr(), bs, hn, hkv, hs, sl_q, max(sl_kv, 1), 0.1, CAUSAL, k_trans)
        a.sl_kv = sl_kv
        if row != hs:
            a.step_k_sl = a.step_v_sl = hkv * row
            a.step_k_head_num = a.step_v_head_num = row
            a.step_k_bs = a.step_v_bs = cap * hkv * row
        return a

    calls = [("one query row", args(sl_q=2), lens.data_ptr()), ("dKvLens is null", args(), None), ("contiguous in the head dimension", args(k_trans=True), lens.data_ptr()),
             ("16-byte aligned", args(row=hs + 4), lens.data_ptr()), ("16-byte aligned", args(off=2), lens.data_ptr()), ("capacity of a request's slab", args(sl_kv=0), lens.data_ptr())]
    r0, a0 = rows_stats(L), attn_stats(L)
    for n, (text, a, lp) in enumerate(calls):
        L.ns_hip_reset_error()
        assert L.ns_hip_attn_decode_rows(C.byref(a), C.c_void_p(lp) if lp else None, 1, None, stream_ptr()) == -1, text
        assert text in pkg.last_error(), (text, pkg.last_error())
        assert [y - x for x, y in zip(r0, rows_stats(L))] == [0, 0, 0, n + 1]
    torch.cuda.synchronize()
    assert bool(torch.all(dd == 7.0)) and attn_stats(L) == a0
    L.ns_hip_reset_error()

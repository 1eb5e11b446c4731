"""FP8 weights (E4M3 / E5M2, E8M0 or fp32 scales) on gemm3_kernel — the tiled prefill GEMM — and on the entries that exist only
there: fp16-only operands, the one-launch fused QKV, QKV + RoPE + kv-append, the gate/up tile pairs, the grouped mixture-of-experts
GEMM.  Everything against the oracle's fp64 product on the same blob (docs/kernels/gemm3.md, "FP8 weights").

Bars (the project's own): 1e-3 against the fp32-activation product, 5e-4 against the fp16-activation product above 64 rows
(the product code * scale is rounded once to fp16, 2^-12 relative: TOL_A16_GEMM of tests/test_gpu_parity.py), 2e-3 where two
rounded factors are multiplied, 3e-5 for the exact-scale kernels the switch restores."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
TOL, TOL_A16, TOL_MUL, TOL_EXACT = 1e-3, 5e-4, 2e-3, 3e-5
F8 = [("F8_E4M3", "F8_E8M0"), ("F8_E4M3", "F32"), ("F8_E5M2", "F8_E8M0"), ("F8_E5M2", "F32")]

HOST_CASES = [  # group, n, k, m, core
    (32, 256, 512, 256, "CORE_AVX512F"),
    (32, 263, 448, 193, "CORE_AVX512F"),    # ragged N, K = 3.5 x 128, ragged M
    (64, 129, 2048, 512, "CORE_AVX512F"),   # few tiles: split-K
    (32, 384, 576, 257, "CORE_AMX_BF16"),   # K = 9 x 64
    (-1, 144, 1000, 70, "CORE_AVX512F"),    # per-channel scales, K not a multiple of 64, 70 rows
]


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _blob(nso, w, f8, st, bs=32, core="CORE_AVX512F"):
    return nso.quant_pack(w, bs, getattr(nso, f8), getattr(nso, st), False, getattr(nso, core))


def _spread(rng, n, k, log2):
    """rows of w (output columns) scaled by 2^+-log2: group scales that span 2 * log2 binades"""
    w = (rng.standard_normal((n, k)) * 0.05).astype(np.float32)
    w[0::3] *= np.float32(2.0 ** log2)
    w[1::3] *= np.float32(2.0 ** -log2)
    return w


@pytest.mark.parametrize("bm", [64, 128, 256])
@pytest.mark.parametrize("bs,n,k,m,core", HOST_CASES)
@pytest.mark.parametrize("f8,st", F8)
def test_fp8_gemm3_host_api(L, pkg, nso, f8, st, bs, n, k, m, core, bm):
    rng = np.random.default_rng(n * 7 + k + m + bm)
    w = (rng.standard_normal((n, k)) * 0.05).astype(np.float32)
    a = rng.standard_normal((m, k)).astype(np.float32)
    blob = _blob(nso, w, f8, st, bs, core)
    ref, ref16 = nso.gemm_f64(a, blob), nso.gemm_f64(a, blob, a16=True)
    assert L.ns_hip_set_tuning(b"g3_bm", bm) == 0
    try:
        out = np.zeros((m, n), np.float32)
        L.bestla_f32f32_forward(nso.ptr(a), nso.ptr(blob), nso.ptr(out), m, n, k, k, n, None)
        e, e16 = nso.rel_l2(out, ref), nso.rel_l2(out, ref16)
        print("fp8 host api", f8, st, (bs, n, k, m), bm, "rel_l2 %.3g  a16 %.3g" % (e, e16))
        assert e < TOL and e16 < TOL_A16
    finally:
        L.ns_hip_set_tuning(b"g3_bm", 0)
        L.ns_hip_cache_clear()


@pytest.mark.parametrize("log2", [3, 10])
@pytest.mark.parametrize("f8", ["F8_E4M3", "F8_E5M2"])
def test_fp8_group_scales_over_many_binades(L, pkg, nso, f8, log2):
    """the range rule: fp32 scales, rows of w scaled by 2^+-log2.  2^+-3 lies inside the rule of both encodings (the tiled kernel
    multiplies), 2^+-10 is beyond E5M2's 2^13 and at the edge of E4M3's 2^20 — where the rule refuses, the call runs where it ran
    before; the bars hold either way, and every COLUMN meets the fp32-activation bar on its own"""
    rng = np.random.default_rng(41 + log2)
    n, k, m = 192, 512, 200
    w = _spread(rng, n, k, log2)
    a = rng.standard_normal((m, k)).astype(np.float32)
    blob = _blob(nso, w, f8, "F32")
    ref, ref16 = nso.gemm_f64(a, blob), nso.gemm_f64(a, blob, a16=True)
    out = np.zeros((m, n), np.float32)
    L.bestla_f32f32_forward(nso.ptr(a), nso.ptr(blob), nso.ptr(out), m, n, k, k, n, None)
    L.ns_hip_cache_clear()
    e, e16 = nso.rel_l2(out, ref), nso.rel_l2(out, ref16)
    cols = max(nso.rel_l2(out[:, c], ref[:, c]) for c in range(n))
    print("fp8 spread", f8, log2, "rel_l2 %.3g  a16 %.3g  worst column %.3g" % (e, e16, cols))
    assert e < TOL and e16 < TOL_A16 and cols < TOL


@pytest.mark.parametrize("bm", [64, 128, 256])
@pytest.mark.parametrize("epi", ["none", "add", "mul", "add_gelu", "gelu", "silu"])
@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("f8,st", [("F8_E4M3", "F8_E8M0"), ("F8_E5M2", "F32")])
def test_fp8_epilogues_and_shadow(L, pkg, nso, f8, st, bm, epi, aligned):
    import torch
    n, k, m = 320, 512, 260
    ldc = n if aligned else n + 1
    rng = np.random.default_rng(len(epi) + bm)
    w = (rng.standard_normal((n, k)) * 0.05).astype(np.float32)
    blob = _blob(nso, w, f8, st)
    s = _stream()
    wt = pkg.Weight.from_host_blob(nso.ptr(blob), s)
    a = rng.standard_normal((m, k)).astype(np.float32)
    d = rng.standard_normal((m, ldc)).astype(np.float32)
    da, dd = torch.from_numpy(a).cuda(), torch.from_numpy(d).cuda()
    da16 = da.half()
    dc = torch.full((m, ldc), -7.0, device="cuda")
    dc16 = torch.zeros((m, ldc), device="cuda", dtype=torch.float16)
    code = {"none": pkg.EPI_NONE, "add": pkg.EPI_ADD, "mul": pkg.EPI_MUL, "add_gelu": pkg.EPI_ADD_GELU, "gelu": pkg.EPI_GELU,
            "silu": pkg.EPI_SILU}[epi]
    assert L.ns_hip_set_tuning(b"g3_bm", bm) == 0
    try:
        pkg.check(L.ns_hip_f32f32_forward_h(da.data_ptr(), da16.data_ptr(), wt.h, dc.data_ptr(), dc16.data_ptr(), m, k, ldc, code,
                                            dd.data_ptr() if epi in ("add", "mul", "add_gelu") else None, ldc, s))
        torch.cuda.synchronize()
    finally:
        L.ns_hip_set_tuning(b"g3_bm", 0)
    g = nso.gemm_f64(a, blob)
    gelu = lambda x: 0.5 * x * (1 + np.tanh(0.7978845834732056 * (x + 0.044714998453855515 * x ** 3)))
    dv = d[:, :n].astype(np.float64)
    ref = {"none": g, "add": g + dv, "mul": g * dv, "add_gelu": gelu(g + dv), "gelu": gelu(g), "silu": g / (1 + np.exp(-g))}[epi]
    out = dc.cpu().numpy()
    assert nso.rel_l2(out[:, :n], ref) < (TOL_MUL if epi == "mul" else TOL)
    if not aligned:
        assert np.all(out[:, n] == -7.0)  # nothing written past N
    assert np.allclose(dc16.float().cpu().numpy()[:, :n], out[:, :n], rtol=2e-3, atol=2e-3)


@pytest.mark.parametrize("m", [40, 300])
@pytest.mark.parametrize("f8,st", F8)
def test_fp8_fp16_only_operands(L, pkg, nso, f8, st, m):
    """ns_hip_f32f32_forward_h with dA = NULL and with dC = NULL (both exist on the tiled kernel only: from 17 rows); with the
    switch off the same calls are refused as before"""
    import torch
    n, k = 384, 512
    rng = np.random.default_rng(m)
    w = (rng.standard_normal((n, k)) * 0.05).astype(np.float32)
    blob = _blob(nso, w, f8, st)
    s = _stream()
    wt = pkg.Weight.from_host_blob(nso.ptr(blob), s)
    a = rng.standard_normal((m, k)).astype(np.float32)
    da16 = torch.from_numpy(a).cuda().half()
    a16 = da16.float().cpu().numpy()
    ref = nso.gemm_f64(a16, blob, a16=True)
    dc = torch.zeros((m, n), device="cuda")
    pkg.check(L.ns_hip_f32f32_forward_h(None, da16.data_ptr(), wt.h, dc.data_ptr(), None, m, k, n, pkg.EPI_NONE, None, 0, s))
    dc16 = torch.zeros((m, n), device="cuda", dtype=torch.float16)
    pkg.check(L.ns_hip_f32f32_forward_h(None, da16.data_ptr(), wt.h, None, dc16.data_ptr(), m, k, n, pkg.EPI_NONE, None, 0, s))
    torch.cuda.synchronize()
    e = nso.rel_l2(dc.cpu().numpy(), ref)
    e16 = nso.rel_l2(dc16.float().cpu().numpy(), ref)
    print("fp8 fp16-only", f8, st, m, "fp32 out %.3g  fp16 out %.3g" % (e, e16))
    assert e < TOL_A16
    assert e16 < TOL   # the output itself is rounded to fp16 (2^-11 per element)
    assert L.ns_hip_set_tuning(b"g3_f8", 0) == 0
    try:
        assert L.ns_hip_f32f32_forward_h(None, da16.data_ptr(), wt.h, dc.data_ptr(), None, m, k, n, pkg.EPI_NONE, None, 0, s) == -1
        assert L.ns_hip_f32f32_forward_h(None, da16.data_ptr(), wt.h, None, dc16.data_ptr(), m, k, n, pkg.EPI_NONE, None, 0, s) == -1
    finally:
        L.ns_hip_set_tuning(b"g3_f8", -1)
        L.ns_hip_reset_error()


@pytest.mark.parametrize("f8,st", F8)
def test_fp8_fused_qkv_in_one_launch(L, pkg, nso, f8, st):
    """ragged / GQA widths: each matrix against the oracle and against three separate launches"""
    import torch
    rng = np.random.default_rng(17)
    m, k, widths = 200, 512, (392, 136, 136)
    s = _stream()
    blobs = [_blob(nso, (rng.standard_normal((n, k)) * 0.05).astype(np.float32), f8, st) for n in widths]
    ws = [pkg.Weight.from_host_blob(nso.ptr(b), s) for b in blobs]
    a = rng.standard_normal((m, k)).astype(np.float32)
    da = torch.from_numpy(a).cuda()
    da16 = da.half()
    ldc = widths[0]
    fused = torch.full((3, m, ldc), 7.0, device="cuda")
    pkg.check(L.ns_hip_fusion_qkv_forward_h(da.data_ptr(), da16.data_ptr(), ws[0].h, ws[1].h, ws[2].h, fused.data_ptr(), None, m, k, ldc, s))
    sep = torch.zeros((3, m, ldc), device="cuda")
    for i in range(3):
        pkg.check(L.ns_hip_f32f32_forward_h(da.data_ptr(), da16.data_ptr(), ws[i].h, sep[i].data_ptr(), None, m, k, ldc, pkg.EPI_NONE, None, 0, s))
    torch.cuda.synchronize()
    for i, n in enumerate(widths):
        out = fused[i][:, :n].cpu().numpy()
        assert nso.rel_l2(out, nso.gemm_f64(a, blobs[i])) < TOL
        assert nso.rel_l2(out, nso.gemm_f64(a, blobs[i], a16=True)) < TOL_A16
        assert nso.rel_l2(out, sep[i][:, :n].cpu().numpy().astype(np.float64)) < TOL_A16
        if n < ldc:
            assert bool((fused[i][:, n:] == 7.0).all())


@pytest.mark.parametrize("m,heads,hkv,hs", [(300, 8, 8, 128), (77, 16, 4, 64), (40, 4, 2, 128)])
@pytest.mark.parametrize("f8,st", F8)
def test_fp8_qkv_rope_cache_append_at_prompt_size(L, pkg, nso, f8, st, m, heads, hkv, hs):
    """ns_hip_fusion_qkv_rope_forward_x above 16 rows on fp8 weights: q / k rotated, k / v in the fp16 cache cells, with and without
    the fp32 k / v tensors — against separate forwards + ns_hip_rope_qkv_append and against fp64"""
    import torch
    rng = np.random.default_rng(m + hs)
    s = _stream()
    d, dkv, n_past = heads * hs, hkv * hs, 19
    assert d % 128 == 0 and dkv % 128 == 0
    ctx = n_past + m + 5
    mats = [(rng.standard_normal((n, d)) * 0.05).astype(np.float32) for n in (d, dkv, dkv)]
    blobs = [_blob(nso, w, f8, st) for w in mats]
    wq, wk, wv = [pkg.Weight.from_host_blob(nso.ptr(b), s) for b in blobs]
    x = torch.from_numpy(rng.standard_normal((m, d)).astype(np.float32)).cuda()
    x16 = x.half()
    ldc = d
    # the separate chain (through the entries that serve fp8 at this row count), then RoPE + append on packed copies
    qkv_a = torch.zeros(3, m, ldc, device="cuda")
    for i, w in enumerate((wq, wk, wv)):
        pkg.check(L.ns_hip_f32f32_forward_h(x.data_ptr(), x16.data_ptr(), w.h, qkv_a[i].data_ptr(), None, m, d, ldc, pkg.EPI_NONE, None, 0, s))
    q_a, k_a, v_a = qkv_a[0].contiguous(), qkv_a[1][:, :dkv].contiguous(), qkv_a[2][:, :dkv].contiguous()
    kc_a = torch.zeros(1, ctx, hkv, hs, device="cuda", dtype=torch.float16)
    vc_a = torch.zeros_like(kc_a)
    pkg.check(L.ns_hip_rope_qkv_append(q_a.data_ptr(), k_a.data_ptr(), v_a.data_ptr(), kc_a.data_ptr(), vc_a.data_ptr(), m, heads, hkv, hs, n_past, hs, 0,
                                       10000.0, 1.0, 0.0, 1.0, hkv * hs, hs, s))
    tab = torch.zeros(m, hs // 2, 2, device="cuda")
    pkg.check(L.ns_hip_rope_cos_sin(m, n_past, hs, 10000.0, 1.0, 1.0, tab.data_ptr(), s))
    f = lambda t: t.float().cpu().numpy().astype(np.float64)
    for flags in (0, 1):
        qkv_b = torch.full((3, m, ldc), 7.0, device="cuda")
        kc_b, vc_b = torch.zeros_like(kc_a), torch.zeros_like(kc_a)
        rp = pkg.QkvRope(kc_b.data_ptr(), vc_b.data_ptr(), tab.data_ptr(), heads, hkv, hs, n_past, hs, 0, hkv * hs, hs, flags)
        pkg.check(L.ns_hip_fusion_qkv_rope_forward_x(x.data_ptr(), x16.data_ptr(), wq.h, wk.h, wv.h, qkv_b.data_ptr(), m, d, ldc, None, C.byref(rp), s))
        torch.cuda.synchronize()
        assert nso.rel_l2(f(qkv_b[0]), f(q_a)) < TOL_A16, flags
        assert nso.rel_l2(f(kc_b), f(kc_a)) < TOL and nso.rel_l2(f(vc_b), f(vc_a)) < TOL, flags   # fp16 cells
        assert torch.count_nonzero(kc_b[0, n_past:n_past + m]) > 0 and torch.count_nonzero(kc_b[0, :n_past]) == 0
        assert torch.count_nonzero(kc_b[0, n_past + m:]) == 0 and torch.count_nonzero(vc_b[0, n_past + m:]) == 0
        if flags == 0:
            kr = kc_b[0, n_past:n_past + m].reshape(m, dkv).float()
            assert torch.equal(qkv_b[1][:, :dkv].half().float(), kr)
            assert nso.rel_l2(f(qkv_b[2][:, :dkv]), nso.gemm_f64(f(x16).astype(np.float32), blobs[2], a16=True)) < TOL_A16
        else:
            assert bool((qkv_b[1] == 7.0).all()) and bool((qkv_b[2] == 7.0).all())
    # against fp64: GEMM -> rope (closed form)
    kr = nso.gemm_f64(f(x16).astype(np.float32), blobs[1], a16=True).reshape(m, hkv, hs)
    ts = 10000.0 ** (-2.0 / hs)
    ref = kr.copy()
    for i in range(m):
        th = (n_past + i) * ts ** np.arange(hs // 2)
        c, sn = np.cos(th), np.sin(th)
        ref[i, :, 0::2] = kr[i, :, 0::2] * c - kr[i, :, 1::2] * sn
        ref[i, :, 1::2] = kr[i, :, 0::2] * sn + kr[i, :, 1::2] * c
    assert nso.rel_l2(f(kc_b[0, n_past:n_past + m]), ref) < TOL_MUL
    L.ns_hip_set_tuning(b"g3_f8", 0)
    try:
        assert L.ns_hip_fusion_qkv_rope_forward_x(x.data_ptr(), x16.data_ptr(), wq.h, wk.h, wv.h, qkv_b.data_ptr(), m, d, ldc, None, C.byref(rp), s) == -1
    finally:
        L.ns_hip_set_tuning(b"g3_f8", -1)
        L.ns_hip_reset_error()


@pytest.mark.parametrize("m", [48, 200])
@pytest.mark.parametrize("f8,st", F8)
def test_fp8_gate_up_tile_pairs(L, pkg, nso, f8, st, m):
    import torch
    rng = np.random.default_rng(m + 1)
    s = _stream()
    fin, fmid, fout = 512, 4096, 384   # 256 column tiles: the tiled kernel serves such a weight from 33 rows
    # (the up matrix four times as loud: the two weights' range factors differ, the tile pairs carry one per matrix)
    b1, b3 = [_blob(nso, (rng.standard_normal((fmid, fin)) * sc).astype(np.float32), f8, st) for sc in (0.05, 0.2)]
    b2 = _blob(nso, (rng.standard_normal((fout, fmid)) * 0.05).astype(np.float32), f8, st)
    w1, w3, w2 = [pkg.Weight.from_host_blob(nso.ptr(b), s) for b in (b1, b3, b2)]
    a = rng.standard_normal((m, fin)).astype(np.float32)
    da = torch.from_numpy(a).cuda()
    da16 = da.half()
    a16 = da16.float().cpu().numpy()
    gate = nso.gemm_f64(a16, b1, a16=True)
    act = gate / (1 + np.exp(-gate))
    ref = act * nso.gemm_f64(a16, b3, a16=True)
    # all three outputs
    t1, t2 = torch.zeros((m, fmid), device="cuda"), torch.zeros((m, fmid), device="cuda")
    t2h = torch.zeros((m, fmid), device="cuda", dtype=torch.float16)
    pkg.check(L.ns_hip_fusion_ffn3_gateup_h(da.data_ptr(), da16.data_ptr(), w1.h, w3.h, t1.data_ptr(), t2.data_ptr(), t2h.data_ptr(), m, pkg.EPI_SILU, s))
    torch.cuda.synchronize()
    assert nso.rel_l2(t1.cpu().numpy(), act) < TOL
    assert nso.rel_l2(t2.cpu().numpy(), ref) < TOL_MUL
    assert nso.rel_l2(t2h.float().cpu().numpy(), ref) < TOL_MUL
    # the fp16 output only, fp16-only activations (the tiled kernel's tile pairs alone serve this form)
    t2h2 = torch.zeros((m, fmid), device="cuda", dtype=torch.float16)
    pkg.check(L.ns_hip_fusion_ffn3_gateup_h(None, da16.data_ptr(), w1.h, w3.h, None, None, t2h2.data_ptr(), m, pkg.EPI_SILU, s))
    torch.cuda.synchronize()
    assert nso.rel_l2(t2h2.float().cpu().numpy(), ref) < TOL_MUL
    # the whole FFN with null temporaries (fp16 intermediate) against the same call with every temporary requested
    o_null, o_all = torch.zeros((m, fout), device="cuda"), torch.zeros((m, fout), device="cuda")
    pkg.check(L.ns_hip_fusion_ffn3_forward_h(da.data_ptr(), da16.data_ptr(), w1.h, w2.h, w3.h, None, None, None, o_null.data_ptr(), None, m, pkg.EPI_SILU, s))
    pkg.check(L.ns_hip_fusion_ffn3_forward_h(da.data_ptr(), da16.data_ptr(), w1.h, w2.h, w3.h, t1.data_ptr(), t2.data_ptr(), t2h.data_ptr(), o_all.data_ptr(), None, m,
                                             pkg.EPI_SILU, s))
    torch.cuda.synchronize()
    down = nso.gemm_f64(ref.astype(np.float32), b2)
    assert nso.rel_l2(o_null.cpu().numpy(), down) < TOL_MUL and nso.rel_l2(o_all.cpu().numpy(), down) < TOL_MUL
    assert nso.rel_l2(o_null.cpu().numpy(), o_all.cpu().numpy().astype(np.float64)) < TOL_MUL
    L.ns_hip_set_tuning(b"g3_f8", 0)
    try:
        assert L.ns_hip_fusion_ffn3_gateup_h(None, da16.data_ptr(), w1.h, w3.h, None, None, t2h2.data_ptr(), m, pkg.EPI_SILU, s) == -1
    finally:
        L.ns_hip_set_tuning(b"g3_f8", -1)
        L.ns_hip_reset_error()


@pytest.mark.parametrize("f8,st", F8)
def test_fp8_experts_mul_mat_id_at_prefill_size(L, pkg, nso, f8, st):
    """fp8 experts: the grouped GEMM (one tiled launch per expert) from 65 token rows, the per-row loop below"""
    import torch
    rng = np.random.default_rng(23)
    n_as, n, k, topk = 4, 200, 832, 2
    blobs = [_blob(nso, (rng.standard_normal((n, k)) * 0.05).astype(np.float32), f8, st) for _ in range(n_as)]
    weights = [pkg.Weight.from_host_blob(nso.ptr(b)) for b in blobs]
    arr = (C.c_void_p * n_as)(*[w.h for w in weights])
    g = L.ns_hip_expert_group_create(arr, n_as)
    assert g, pkg.last_error()
    s = _stream()
    for m, tol16 in ((150, TOL_A16), (5, TOL_EXACT)):
        a = rng.standard_normal((m, k)).astype(np.float32)
        ids = rng.integers(0, n_as, size=(m, topk)).astype(np.int32)
        ids[0, :] = 3
        dA, dI = torch.from_numpy(a).cuda(), torch.from_numpy(ids).cuda()
        for sel in range(topk):
            dC = torch.full((m, n), 7.0, device="cuda")
            pkg.check(L.ns_hip_mul_mat_id(dA.data_ptr(), dI.data_ptr(), topk, sel, g, dC.data_ptr(), m, k, n, pkg.EPI_NONE, None, 0, s))
            torch.cuda.synchronize()
            out = dC.cpu().numpy()
            ref = np.concatenate([nso.gemm_f64(a[t:t + 1], blobs[ids[t, sel]]) for t in range(m)], axis=0)
            ref16 = np.concatenate([nso.gemm_f64(a[t:t + 1], blobs[ids[t, sel]], a16=True) for t in range(m)], axis=0)
            e, e16 = nso.rel_l2(out, ref), nso.rel_l2(out, ref16)
            print("fp8 moe", f8, st, m, sel, "rel_l2 %.3g a16 %.3g" % (e, e16))
            assert e < TOL and e16 < tol16
    L.ns_hip_expert_group_free(g)


@pytest.mark.parametrize("f8,st", F8)
def test_fp8_switch_off_equals_the_earlier_path(L, pkg, nso, f8, st):
    """g3_f8 = 0: a plain forward at 130 rows runs on the first-generation kernel again — exact scales in fp32, 3e-5 from the
    fp16-activation product; switched on the same call is the tiled kernel's (2^-12 per weight: above that budget, inside 5e-4)"""
    rng = np.random.default_rng(130)
    n, k, m = 272, 1024, 130
    w = (rng.standard_normal((n, k)) * 0.02).astype(np.float32)
    a = rng.standard_normal((m, k)).astype(np.float32)
    blob = _blob(nso, w, f8, st)
    ref16 = nso.gemm_f64(a, blob, a16=True)
    assert L.ns_hip_set_tuning(b"g3_f8", 0) == 0
    try:
        out = np.zeros((m, n), np.float32)
        L.bestla_f32f32_forward(nso.ptr(a), nso.ptr(blob), nso.ptr(out), m, n, k, k, n, None)
        e_off = nso.rel_l2(out, ref16)
    finally:
        L.ns_hip_set_tuning(b"g3_f8", -1)
    out2 = np.zeros((m, n), np.float32)
    L.bestla_f32f32_forward(nso.ptr(a), nso.ptr(blob), nso.ptr(out2), m, n, k, k, n, None)
    L.ns_hip_cache_clear()
    e_on = nso.rel_l2(out2, ref16)
    print("fp8 switch", f8, st, "off %.3g  on %.3g" % (e_off, e_on))
    assert e_off < TOL_EXACT
    assert e_on < TOL_A16

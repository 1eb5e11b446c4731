"""NeoX-style rotary (RoPE mode 2) inside the fused QKV launch: ns_hip_fusion_qkv_rope_forward_x with NS_QKV_ROPE_NEOX and the table of
ns_hip_rope_cos_sin_mode(mode 2).  The yardstick is the two-launch form it replaces — the fused QKV launch followed by
ns_hip_rope_qkv_append(mode 2), which tests/test_rope.py pins to the reference operator — bit for bit, and numpy fp64 (norm -> GEMM ->
NeoX rotation, closed form) with the bound the mode-0 test of the same entry uses."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
BASE = 10000.0


def _rms(x, g, eps):
    return x / np.sqrt((x * x).mean(-1, keepdims=True) + eps) * g


def _w(pkg, nso, rng, n, k, st, qt=None, bs=32, asym=False):
    w = (rng.standard_normal((n, k)) * (1.0 / np.sqrt(k))).astype(np.float32)
    blob = nso.quant_pack(w, bs, nso.S4 if qt is None else qt, nso.BF16, asym, nso.CORE_AVX512_VNNI_KB)
    return pkg.Weight.from_host_blob(nso.ptr(blob), st), nso.unpack_fp32(blob).astype(np.float64), blob


def _neox_fp64(kr, n_past, hs, fscale=1.0, attn=1.0):
    """kr [m][heads][hs] fp64 -> NeoX rotation; the reference's NeoX branch applies freq_scale twice (ne_layers.c)"""
    m, half = kr.shape[0], hs // 2
    ts = BASE ** (-2.0 / hs)
    ref = kr.copy()
    for i in range(m):
        th = (n_past + i) * fscale * fscale * ts ** np.arange(half)
        c, s = np.cos(th) * attn, np.sin(th) * attn
        ref[i, :, :half] = kr[i, :, :half] * c - kr[i, :, half:] * s
        ref[i, :, half:] = kr[i, :, :half] * s + kr[i, :, half:] * c
    return ref


def _st():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---- a) the table ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n_past", [(1, 0), (4, 77)])
@pytest.mark.parametrize("fscale,attn", [(1.0, 1.0), (0.5, 1.25)])
def test_mode0_table_is_the_old_entrys(L, pkg, m, n_past, fscale, attn):
    import torch
    st = _st()
    a, b = torch.zeros(m, 32, 2, device="cuda"), torch.ones(m, 32, 2, device="cuda")
    pkg.check(L.ns_hip_rope_cos_sin(m, n_past, 64, BASE, fscale, attn, a.data_ptr(), st))
    pkg.check(L.ns_hip_rope_cos_sin_mode(m, n_past, 64, 0, BASE, fscale, attn, b.data_ptr(), st))
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.count_nonzero(a) > 0


@pytest.mark.parametrize("m,n_past", [(1, 0), (4, 77), (1, 77), (4, 0)])
@pytest.mark.parametrize("hs", [64, 128])
@pytest.mark.parametrize("fscale,attn", [(1.0, 1.0), (0.5, 1.25)])
def test_mode2_table_rotates_like_the_rope_operator(L, pkg, m, n_past, hs, fscale, attn):
    """a host rotation with the table's (cos, sin), products and sums rounded one by one in fp32, == ns_hip_rope_f32(mode 2)"""
    import torch
    st = _st()
    heads, half = 3, hs // 2
    rng = np.random.default_rng(hs + m + n_past)
    x = rng.standard_normal((m, heads, hs)).astype(np.float32)
    dx = torch.from_numpy(x).cuda()
    dy = torch.zeros_like(dx)
    tab = torch.zeros(m, half, 2, device="cuda")
    pkg.check(L.ns_hip_rope_cos_sin_mode(m, n_past, hs, 2, BASE, fscale, attn, tab.data_ptr(), st))
    pkg.check(L.ns_hip_rope_f32(dx.data_ptr(), dy.data_ptr(), 1, m, heads, hs, n_past, hs, 2, BASE, fscale, 0.0, attn, st))
    torch.cuda.synchronize()
    t = tab.cpu().numpy()
    c, s = t[:, None, :, 0], t[:, None, :, 1]
    x0, x1 = x[:, :, :half], x[:, :, half:]
    y = np.concatenate([(x0 * c).astype(np.float32) - (x1 * s).astype(np.float32), (x0 * s).astype(np.float32) + (x1 * c).astype(np.float32)], axis=-1)
    assert y.dtype == np.float32 and np.array_equal(y, dy.cpu().numpy())


# ---- b) decode size -------------------------------------------------------------------------------------------------------------
def _decode_case(L, pkg, nso, m, n_past, heads, hkv, hs, norm, qt=None, asym=False, fscale=1.0, attn=1.0):
    import torch
    rng = np.random.default_rng(heads * hs + m + (7 if norm else 0))
    st = _st()
    d, dkv, ctx, eps = heads * hs, hkv * hs, 128, 1e-5
    wq, _a, _0 = _w(pkg, nso, rng, d, d, st, qt, asym=asym)
    wk, Wk, _1 = _w(pkg, nso, rng, dkv, d, st, qt, asym=asym)
    wv, _b, _2 = _w(pkg, nso, rng, dkv, d, st, qt, asym=asym)
    x = torch.from_numpy(rng.standard_normal((m, d)).astype(np.float32)).cuda()
    if norm:
        gam = torch.from_numpy((1.0 + 0.2 * rng.standard_normal(d)).astype(np.float32)).cuda()
        parts = (d + 15) // 16
        stride = (parts + 3) & ~3
        x16, ssq = torch.zeros(m, d, device="cuda", dtype=torch.float16), torch.zeros(m, stride, device="cuda")
        pkg.check(L.ns_hip_norm_prep(m, d, x.data_ptr(), d, gam.data_ptr(), x16.data_ptr(), ssq.data_ptr(), stride, st))
        lk = pkg.NormLink(ssq.data_ptr(), parts, stride, eps, d, None, None, 0)
        link = C.byref(lk)
        h = _rms(x.cpu().numpy().astype(np.float64), gam.cpu().numpy().astype(np.float64), eps)
    else:
        x16, link = x.half(), None
        h = x16.float().cpu().numpy().astype(np.float64)
    ldc = d
    # two launches: fused QKV, then RoPE (mode 2) + append on packed copies of its outputs
    qkv_a = torch.zeros(3, m, ldc, device="cuda")
    kc_a = torch.full((1, ctx, hkv, hs), 9.0, device="cuda", dtype=torch.float16)
    vc_a = torch.full_like(kc_a, 9.0)
    pkg.check(L.ns_hip_fusion_qkv_forward_x(x.data_ptr(), x16.data_ptr(), wq.h, wk.h, wv.h, qkv_a.data_ptr(), None, m, d, ldc, link, st))
    q_a, k_a, v_a = qkv_a[0].contiguous(), qkv_a[1][:, :dkv].contiguous(), qkv_a[2][:, :dkv].contiguous()
    v_raw = v_a.clone()
    pkg.check(L.ns_hip_rope_qkv_append(q_a.data_ptr(), k_a.data_ptr(), v_a.data_ptr(), kc_a.data_ptr(), vc_a.data_ptr(), m, heads, hkv, hs, n_past, hs, 2,
                                       BASE, fscale, 0.0, attn, hkv * hs, hs, st))
    # one launch
    qkv_b = torch.zeros(3, m, ldc, device="cuda")
    kc_b, vc_b = torch.full_like(kc_a, 9.0), torch.full_like(kc_a, 9.0)
    tab = torch.zeros(m, hs // 2, 2, device="cuda")
    pkg.check(L.ns_hip_rope_cos_sin_mode(m, n_past, hs, 2, BASE, fscale, attn, tab.data_ptr(), st))
    rp = pkg.QkvRope(kc_b.data_ptr(), vc_b.data_ptr(), tab.data_ptr(), heads, hkv, hs, n_past, hs, 2, hkv * hs, hs, pkg.QKV_ROPE_NEOX)
    pkg.check(L.ns_hip_fusion_qkv_rope_forward_x(x.data_ptr(), x16.data_ptr(), wq.h, wk.h, wv.h, qkv_b.data_ptr(), m, d, ldc, link, C.byref(rp), st))
    torch.cuda.synchronize()
    err = nso.rel_l2(kc_b[0, n_past:n_past + m].float().cpu().numpy(), _neox_fp64((h @ Wk).reshape(m, hkv, hs), n_past, hs, fscale, attn))
    print("decode m %d heads %d/%d hs %d norm %d: q equal %s, k cache equal %s, v cache equal %s, fp64 rel_l2 %.3e" %
          (m, heads, hkv, hs, norm, torch.equal(qkv_b[0], q_a), torch.equal(kc_b, kc_a), torch.equal(vc_b, vc_a), err))
    assert torch.equal(qkv_b[0], q_a)
    assert torch.equal(kc_b, kc_a) and torch.equal(vc_b, vc_a)
    rows = kc_b[0, n_past:n_past + m].reshape(m, dkv)
    assert torch.equal(qkv_b[1][:, :dkv].half(), rows) and torch.equal(qkv_b[2][:, :dkv], v_raw)
    assert torch.count_nonzero(rows) > 0
    assert bool((kc_b[0, :n_past] == 9.0).all()) and bool((vc_b[0, :n_past] == 9.0).all())  # below n_past: untouched
    assert bool((kc_b[0, n_past + m:] == 9.0).all()) and bool((vc_b[0, n_past + m:] == 9.0).all())
    assert err < 2e-3


DECODE_SHAPES = [(1, 0, 2, 2, 32), (1, 77, 4, 4, 64), (4, 30, 8, 2, 128), (16, 5, 4, 1, 128), (3, 9, 2, 2, 256)]


@pytest.mark.parametrize("norm", [True, False])
@pytest.mark.parametrize("m,n_past,heads,hkv,hs", DECODE_SHAPES)
def test_neox_epilogue_at_decode_size(L, pkg, nso, m, n_past, heads, hkv, hs, norm):
    _decode_case(L, pkg, nso, m, n_past, heads, hkv, hs, norm)


def test_neox_epilogue_at_decode_size_asymmetric_s4(L, pkg, nso):
    _decode_case(L, pkg, nso, 4, 30, 8, 2, 128, True, asym=True)


def test_neox_epilogue_at_decode_size_s8(L, pkg, nso):
    _decode_case(L, pkg, nso, 1, 77, 4, 4, 64, True, qt=nso.S8)


def test_neox_epilogue_at_decode_size_freq_scale(L, pkg, nso):
    _decode_case(L, pkg, nso, 4, 30, 8, 2, 128, True, fscale=0.5)


# ---- c) prefill size ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,heads,hkv,hs,qt", [(77, 16, 4, 64, "s8"), (130, 2, 1, 128, None), (300, 8, 4, 32, None), (300, 8, 2, 128, None)])
def test_neox_epilogue_at_prefill_size(L, pkg, nso, m, heads, hkv, hs, qt):
    _prefill_case(L, pkg, nso, m, heads, hkv, hs, qt)


def _prefill_case(L, pkg, nso, m, heads, hkv, hs, qt):
    import torch
    rng = np.random.default_rng(m + hs)
    st = _st()
    d, dkv, n_past = heads * hs, hkv * hs, 19
    ctx = n_past + m + 5
    q8 = nso.S8 if qt == "s8" else None
    wq, _a, _0 = _w(pkg, nso, rng, d, d, st, q8)
    wk, Wk, _1 = _w(pkg, nso, rng, dkv, d, st, q8)
    wv, _b, _2 = _w(pkg, nso, rng, dkv, d, st, q8)
    x = torch.from_numpy(rng.standard_normal((m, d)).astype(np.float32)).cuda()
    x16 = x.half()
    ldc = d
    qkv_a = torch.zeros(3, m, ldc, device="cuda")
    pkg.check(L.ns_hip_fusion_qkv_forward_h(x.data_ptr(), x16.data_ptr(), wq.h, wk.h, wv.h, qkv_a.data_ptr(), None, m, d, ldc, st))
    q_a, k_a, v_a = qkv_a[0].contiguous(), qkv_a[1][:, :dkv].contiguous(), qkv_a[2][:, :dkv].contiguous()
    v_raw = v_a.clone()
    kc_a = torch.zeros(1, ctx, hkv, hs, device="cuda", dtype=torch.float16)
    vc_a = torch.zeros_like(kc_a)
    pkg.check(L.ns_hip_rope_qkv_append(q_a.data_ptr(), k_a.data_ptr(), v_a.data_ptr(), kc_a.data_ptr(), vc_a.data_ptr(), m, heads, hkv, hs, n_past, hs, 2,
                                       BASE, 1.0, 0.0, 1.0, hkv * hs, hs, st))
    tab = torch.zeros(m, hs // 2, 2, device="cuda")
    pkg.check(L.ns_hip_rope_cos_sin_mode(m, n_past, hs, 2, BASE, 1.0, 1.0, tab.data_ptr(), st))
    for flags in (pkg.QKV_ROPE_NEOX, pkg.QKV_ROPE_NEOX | pkg.QKV_ROPE_KV_CACHE_ONLY):
        qkv_b = torch.full((3, m, ldc), 7.0, device="cuda")
        kc_b, vc_b = torch.zeros_like(kc_a), torch.zeros_like(kc_a)
        rp = pkg.QkvRope(kc_b.data_ptr(), vc_b.data_ptr(), tab.data_ptr(), heads, hkv, hs, n_past, hs, 2, hkv * hs, hs, flags)
        pkg.check(L.ns_hip_fusion_qkv_rope_forward_x(x.data_ptr(), x16.data_ptr(), wq.h, wk.h, wv.h, qkv_b.data_ptr(), m, d, ldc, None, C.byref(rp), st))
        torch.cuda.synchronize()
        print("prefill m %d hs %d flags %d: q equal %s, k cache equal %s, v cache equal %s" %
              (m, hs, flags, torch.equal(qkv_b[0], q_a), torch.equal(kc_b, kc_a), torch.equal(vc_b, vc_a)))
        assert torch.equal(qkv_b[0], q_a), flags
        assert torch.equal(kc_b, kc_a) and torch.equal(vc_b, vc_a), flags
        assert torch.count_nonzero(kc_b[0, n_past:n_past + m]) > 0 and torch.count_nonzero(kc_b[0, :n_past]) == 0
        if flags == pkg.QKV_ROPE_NEOX:  # k comes out rotated, v as it is — the fp32 tensors a graph may read
            kr = kc_a[0, n_past:n_past + m].reshape(m, dkv).float()
            assert torch.equal(qkv_b[1][:, :dkv].half().float(), kr) and torch.equal(qkv_b[2][:, :dkv], v_raw)
        else:
            assert bool((qkv_b[1] == 7.0).all()) and bool((qkv_b[2] == 7.0).all())
    kr = (x16.float().cpu().numpy().astype(np.float64) @ Wk).reshape(m, hkv, hs)
    err = nso.rel_l2(kc_b[0, n_past:n_past + m].float().cpu().numpy(), _neox_fp64(kr, n_past, hs))
    print("prefill m %d hs %d: fp64 rel_l2 %.3e" % (m, hs, err))
    assert err < 2e-3


# ---- d) refusals ----------------------------------------------------------------------------------------------------------------
def test_neox_refusals_leave_everything_untouched(L, pkg, nso):
    import torch
    st = _st()
    rng = np.random.default_rng(3)
    ws = {}

    def attempt(m, heads, hs, mode, flags, n_dims=None):
        d = heads * hs
        if d not in ws:
            ws[d] = [_w(pkg, nso, rng, d, d, st)[0] for _ in range(3)]
        wq, wk, wv = ws[d]
        x = torch.ones(m, d, device="cuda")
        x16 = x.half()
        out = torch.full((3, m, d), 7.0, device="cuda")
        kc = torch.full((1, m + 4, heads, hs), 9.0, device="cuda", dtype=torch.float16)
        vc = torch.full_like(kc, 9.0)
        tab = torch.zeros(m, hs // 2, 2, device="cuda")
        rp = pkg.QkvRope(kc.data_ptr(), vc.data_ptr(), tab.data_ptr(), heads, heads, hs, 0, hs if n_dims is None else n_dims, mode, heads * hs, hs, flags)
        r = L.ns_hip_fusion_qkv_rope_forward_x(x.data_ptr(), x16.data_ptr(), wq.h, wk.h, wv.h, out.data_ptr(), m, d, d, None, C.byref(rp), st)
        torch.cuda.synchronize()
        assert r != 0, (m, heads, hs, mode, flags, n_dims)
        assert pkg.last_error()
        assert bool((out == 7.0).all()) and bool((kc == 9.0).all()) and bool((vc == 9.0).all())
        L.ns_hip_reset_error()

    neox = pkg.QKV_ROPE_NEOX
    for m in (1, 300):
        attempt(m, 2, 128, 2, 0)               # mode 2 without the bit: the unchanged contract
        attempt(m, 2, 128, 0, neox)            # the bit with mode 0
        attempt(m, 2, 128, 2, neox, n_dims=64)  # partial rotary
        attempt(m, 2, 128, 2, neox | 4)        # unknown flag bits
    attempt(1, 2, 80, 2, neox)                 # decode size: head_size must be a multiple of 32
    attempt(300, 1, 256, 2, neox)              # prefill size: the head does not fit a 128-column block (two-launch form)
    assert "ns_hip_rope_qkv_append" in _last_text(L, pkg, nso, st, ws[256])


def _last_text(L, pkg, nso, st, w3):
    """the refusal at prefill size names the two-launch form"""
    import torch
    m, d = 300, 256
    x = torch.ones(m, d, device="cuda")
    x16 = x.half()
    out = torch.zeros(3, m, d, device="cuda")
    kc = torch.zeros(1, m, 1, 256, device="cuda", dtype=torch.float16)
    tab = torch.zeros(m, 128, 2, device="cuda")
    rp = pkg.QkvRope(kc.data_ptr(), kc.data_ptr(), tab.data_ptr(), 1, 1, 256, 0, 256, 2, 256, 256, pkg.QKV_ROPE_NEOX)
    assert L.ns_hip_fusion_qkv_rope_forward_x(x.data_ptr(), x16.data_ptr(), w3[0].h, w3[1].h, w3[2].h, out.data_ptr(), m, d, d, None, C.byref(rp), st) != 0
    text = pkg.last_error()
    L.ns_hip_reset_error()
    return text


# ---- e) mode 0 unchanged -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 300])
def test_mode0_through_the_new_table_entry(L, pkg, nso, m):
    import torch
    st = _st()
    rng = np.random.default_rng(m)
    heads, hs, n_past = 2, 128, 11
    d = heads * hs
    wq, wk, wv = [_w(pkg, nso, rng, d, d, st)[0] for _ in range(3)]
    x = torch.from_numpy(rng.standard_normal((m, d)).astype(np.float32)).cuda()
    x16 = x.half()
    outs = []
    for new in (False, True):
        tab = torch.zeros(m, hs // 2, 2, device="cuda")
        if new:
            pkg.check(L.ns_hip_rope_cos_sin_mode(m, n_past, hs, 0, BASE, 1.0, 1.0, tab.data_ptr(), st))
        else:
            pkg.check(L.ns_hip_rope_cos_sin(m, n_past, hs, BASE, 1.0, 1.0, tab.data_ptr(), st))
        out = torch.zeros(3, m, d, device="cuda")
        kc = torch.zeros(1, n_past + m, heads, hs, device="cuda", dtype=torch.float16)
        vc = torch.zeros_like(kc)
        rp = pkg.QkvRope(kc.data_ptr(), vc.data_ptr(), tab.data_ptr(), heads, heads, hs, n_past, hs, 0, heads * hs, hs, 0)
        pkg.check(L.ns_hip_fusion_qkv_rope_forward_x(x.data_ptr(), x16.data_ptr(), wq.h, wk.h, wv.h, out.data_ptr(), m, d, d, None, C.byref(rp), st))
        torch.cuda.synchronize()
        outs.append((out, kc, vc))
    assert all(torch.equal(a, b) for a, b in zip(outs[0], outs[1])) and torch.count_nonzero(outs[1][1]) > 0

"""gemv_kernel's one-row instantiation (ns_hip_set_tuning "gv_rows1", csrc/ns_gemv.hip): a launch of ONE activation row returns the
same bits with the one-row form (1, the default) and with the general, up-to-16-row form (0) in everything it writes — fp32 output,
fp16 shadow, the gate / up launch's tmp1, the appended kv-cache rows, the carried norm's partial sums.

Shapes are the smallest that reach every path of the kernel: n = 40 (three 16-column tiles, the last one partial) and 64;
K = 128 (one k-step of a nibble record), 160 and 416 (a partial last k-step with one live 32-deep slice), 192 (two live slices),
512; 2 .. 16 waves per tile forced through "gv_nw" (the rule never gives a tile more waves than k-steps, so with few k-steps the
forced count is halved: every count from 1 up is met); 4-bit symmetric / asymmetric and 8-bit weights; one scale per 32 columns
(bf16 and fp32 scales) and per 128 (the packer pads K to whole groups; in the int8-reference mode the activation k-block is then 128
columns and, where it does not divide K, the quantizer runs as a launch of its own in front)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL_FP16 = 1e-3   # tests/test_gpu_parity.py: TOL, decode GEMV against the fp64 product on the dequantized weights
TOL_INT8 = 2e-6   # tests/test_gpu_int8_mode.py: int8-reference numerics against the oracle's gemv_4bit_u8s8_fp32

FORMATS = [  # qtype, scale dtype, asymmetric, group
    ("S4", "BF16", False, 32),
    ("S4", "BF16", True, 32),
    ("S8", "BF16", False, 32),
    ("S4", "F32", False, 32),
    ("S4", "BF16", False, 128),
]
NS = (40, 64)
KS = (128, 160, 192, 416, 512)
WAVES = (2, 4, 8, 16)
SENTINEL = 7.0


def _weight(pkg, nso, rng, n, k, fmt, st):
    qt, sd, asym, bs = fmt
    w = (rng.standard_normal((n, k)) * (1.0 / np.sqrt(k))).astype(np.float32)
    if asym:
        w += 0.05  # off-centre groups: non-trivial zero points
    blob = nso.quant_pack(w, bs, getattr(nso, qt), getattr(nso, sd), asym, nso.CORE_AVX512_VNNI_KB)
    return pkg.Weight.from_host_blob(nso.ptr(blob), st), blob


def _bits(t):
    a = t.detach().cpu().numpy()
    return a.view(np.uint16 if a.dtype == np.float16 else np.uint32)


def _ab(L, run, what):
    """run() launches once and returns the tensors the launch wrote (each prefilled, so that what it must NOT write is compared too);
    once per setting of the switch — equal bits"""
    got = []
    try:
        for on in (1, 0):
            assert L.ns_hip_set_tuning(b"gv_rows1", on) == 0
            got.append([_bits(t) for t in run()])
    finally:
        L.ns_hip_set_tuning(b"gv_rows1", 1)
    assert len(got[0]) == len(got[1]) and len(got[0]) > 0
    for i, (x, y) in enumerate(zip(got[0], got[1])):
        assert np.array_equal(x, y), (what, i, int((x != y).sum()))
    return got[0]


class _Waves:
    def __init__(self, L, nw):
        self.L, self.nw = L, nw

    def __enter__(self):
        assert self.L.ns_hip_set_tuning(b"gv_nw", self.nw) == 0

    def __exit__(self, *exc):
        self.L.ns_hip_set_tuning(b"gv_nw", 0)


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _full(shape, dtype=None):
    import torch
    return torch.full(shape, SENTINEL, device="cuda", dtype=dtype or torch.float32)


def _plain_h(L, pkg, w, x, x16, n, k, epi, d):
    """single forward, fp16 shadow in and out"""
    def run():
        c, c16 = _full((1, n)), _full((1, n), x16.dtype)
        pkg.check(L.ns_hip_f32f32_forward_h(x.data_ptr(), x16.data_ptr(), w.h, c.data_ptr(), c16.data_ptr(), 1, k, n, epi,
                                            d.data_ptr() if epi in (pkg.EPI_ADD, pkg.EPI_MUL, pkg.EPI_ADD_GELU) else None, n, _stream()))
        return [c, c16]
    return run


def _gateup_h(L, pkg, w1, w3, x, x16, n, k, act, with_c2, link=None):
    def run():
        import torch
        t1, t2, t2h = _full((1, n)), _full((1, n)), _full((1, n), torch.float16)
        pkg.check(L.ns_hip_fusion_ffn3_gateup_x(x.data_ptr(), x16.data_ptr() if x16 is not None else None, w1.h, w3.h,
                                                t1.data_ptr() if with_c2 else None, t2.data_ptr(), t2h.data_ptr(), 1, act,
                                                C.byref(link) if link is not None else None, _stream()))
        return [t2, t2h] + ([t1] if with_c2 else [])
    return run


QKV_N = (64, 32, 32)  # unequal widths: the k / v matrices end inside the q matrix' leading dimension


def _qkv_h(L, pkg, ws, x, x16, k, link=None):
    def run():
        import torch
        c, c16 = _full((3, 1, 64)), _full((3, 1, 64), torch.float16)
        pkg.check(L.ns_hip_fusion_qkv_forward_x(x.data_ptr(), x16.data_ptr() if x16 is not None else None, ws[0].h, ws[1].h, ws[2].h,
                                                c.data_ptr(), c16.data_ptr(), 1, k, 64, C.byref(link) if link is not None else None, _stream()))
        return [c, c16]
    return run


@pytest.fixture(scope="module")
def weights(pkg, nso):
    """every weight of this module, made once: {(format index, n, k): (w1, w3)} and {(format index, k): (wq, wk, wv)}"""
    import torch
    st = _stream()
    rng = np.random.default_rng(2024)
    pair, qkv, blobs = {}, {}, []
    for fi, fmt in enumerate(FORMATS):
        for k in KS:
            for n in NS:
                made = [_weight(pkg, nso, rng, n, k, fmt, st) for _ in range(2)]
                pair[(fi, n, k)] = tuple(w for w, _ in made)
                blobs += [b for _, b in made]
            made = [_weight(pkg, nso, rng, nq, k, fmt, st) for nq in QKV_N]
            qkv[(fi, k)] = tuple(w for w, _ in made)
            blobs += [b for _, b in made]
    torch.cuda.synchronize()
    return pair, qkv, blobs


@pytest.mark.parametrize("fi", range(len(FORMATS)), ids=["%s-%s-%s-g%d" % (q, s, "asym" if a else "sym", b) for q, s, a, b in FORMATS])
def test_one_row_form_returns_the_general_forms_bits_fp16(L, pkg, nso, weights, fi):
    """plain forward with every epilogue and an operand, fused gate / up (SiLU / GeLU, with and without tmp1), fused QKV of unequal
    widths; the _x entries: carried norm in, carried norm out, RoPE (adjacent pairs) + kv-append epilogue"""
    import torch
    pair, qkv, _ = weights
    rng = np.random.default_rng(fi)
    eps = 1e-5
    for k in KS:
        x = torch.from_numpy(rng.standard_normal((1, k)).astype(np.float32)).cuda()
        x16 = x.half()
        # the carried norm's consumer side: gamma-scaled shadow + partial sums of squares of x
        parts = (k + 15) // 16
        stride = (parts + 3) & ~3
        gam = torch.from_numpy((1.0 + 0.2 * rng.standard_normal(k)).astype(np.float32)).cuda()
        xg16, ssq = torch.zeros(1, k, device="cuda", dtype=torch.float16), torch.zeros(1, stride, device="cuda")
        pkg.check(L.ns_hip_norm_prep(1, k, x.data_ptr(), k, gam.data_ptr(), xg16.data_ptr(), ssq.data_ptr(), stride, _stream()))
        lk_in = pkg.NormLink(ssq.data_ptr(), parts, stride, eps, k, None, None, 0)
        wq = qkv[(fi, k)]
        for nw in (0,) + WAVES:
            with _Waves(L, nw):
                _ab(L, _qkv_h(L, pkg, wq, x, x16, k), ("qkv", k, nw))
                if nw in (0, 4):
                    _ab(L, _qkv_h(L, pkg, wq, x, xg16, k, lk_in), ("qkv norm in", k, nw))

                    def rope_run():
                        heads, hkv, hs, n_past, ctx = 2, 1, 32, 3, 8
                        c = _full((3, 1, 64))
                        kc, vc = _full((1, ctx, hkv, hs), torch.float16), _full((1, ctx, hkv, hs), torch.float16)
                        tab = torch.zeros(1, hs // 2, 2, device="cuda")
                        pkg.check(L.ns_hip_rope_cos_sin(1, n_past, hs, 10000.0, 1.0, 1.0, tab.data_ptr(), _stream()))
                        rp = pkg.QkvRope(kc.data_ptr(), vc.data_ptr(), tab.data_ptr(), heads, hkv, hs, n_past, hs, 0, hkv * hs, hs, 0)
                        pkg.check(L.ns_hip_fusion_qkv_rope_forward_x(x.data_ptr(), xg16.data_ptr(), wq[0].h, wq[1].h, wq[2].h, c.data_ptr(), 1, k, 64,
                                                                     C.byref(lk_in), C.byref(rp), _stream()))
                        assert torch.count_nonzero(kc[0, n_past] != SENTINEL) > 0 and bool((kc[0, :n_past] == SENTINEL).all())
                        return [c, kc, vc]
                    _ab(L, rope_run, ("qkv rope", k, nw))
        for n in NS:
            w1, w3 = pair[(fi, n, k)]
            d = torch.from_numpy(rng.standard_normal((1, n)).astype(np.float32)).cuda()
            for nw in (0,) + WAVES:
                with _Waves(L, nw):
                    epis = range(6) if nw == 0 else (nw % 5,)
                    for epi in epis:
                        out = _ab(L, _plain_h(L, pkg, w1, x, x16, n, k, epi, d), ("plain", n, k, nw, epi))
                        assert not (out[0] == np.float32(SENTINEL).view(np.uint32)).all()
                    _ab(L, _gateup_h(L, pkg, w1, w3, x, x16, n, k, pkg.EPI_SILU, nw != 2), ("gate/up silu", n, k, nw))
                    if nw in (0, 8):
                        _ab(L, _gateup_h(L, pkg, w1, w3, x, x16, n, k, pkg.EPI_GELU, True), ("gate/up gelu", n, k, nw))
                        _ab(L, _gateup_h(L, pkg, w1, w3, x, x16, n, k, pkg.EPI_GELU, False), ("gate/up gelu, no tmp1", n, k, nw))
                        _ab(L, _gateup_h(L, pkg, w1, w3, x, xg16, n, k, pkg.EPI_SILU, True, lk_in), ("gate/up norm in", n, k, nw))

                        def x_run(link_in, link_out):
                            def run():
                                tiles = (n + 15) // 16
                                ostride = (tiles + 3) & ~3
                                c, c16, ossq = _full((1, n)), _full((1, n), torch.float16), _full((1, ostride))
                                g2 = torch.linspace(0.5, 1.5, n, device="cuda")
                                lk = pkg.NormLink(ssq.data_ptr() if link_in else None, parts if link_in else 0, stride if link_in else 0,
                                                  eps if link_in else 0.0, k if link_in else 0, g2.data_ptr() if link_out else None,
                                                  ossq.data_ptr() if link_out else None, ostride if link_out else 0)
                                pkg.check(L.ns_hip_f32f32_forward_x(x.data_ptr(), (xg16 if link_in else x16).data_ptr(), w1.h, c.data_ptr(), c16.data_ptr(),
                                                                    1, k, n, pkg.EPI_ADD, d.data_ptr(), n, C.byref(lk), _stream()))
                                return [c, c16, ossq]
                            return run
                        _ab(L, x_run(True, False), ("forward_x norm in", n, k, nw))
                        out = _ab(L, x_run(False, True), ("forward_x norm out", n, k, nw))
                        assert not (out[2][0, :(n + 15) // 16] == np.float32(SENTINEL).view(np.uint32)).any()
                        _ab(L, x_run(True, True), ("forward_x norm in + out", n, k, nw))


def _rows(rng, k):
    """activation rows that drive the in-launch quantizer to its corners"""
    r = rng.standard_normal((1, k)).astype(np.float32)
    return {"random": r, "all equal": np.full((1, k), 0.37, np.float32), "zeros": np.zeros((1, k), np.float32),
            "near 1e4": (r * 1e4).astype(np.float32)}


@pytest.mark.parametrize("fi", range(len(FORMATS)), ids=["%s-%s-%s-g%d" % (q, s, "asym" if a else "sym", b) for q, s, a, b in FORMATS])
def test_one_row_form_returns_the_general_forms_bits_int8_reference(L, pkg, nso, weights, fi):
    """the same plain / QKV / gate-up calls under ns_hip_set_compute_mode(1): groups of 32 and 128 make the activation k-block 32 and
    128 columns; fp32 rows quantized inside the launch, and (a row that is not 16-byte aligned) by the quantizer launch in front"""
    import torch
    pair, qkv, _ = weights
    rng = np.random.default_rng(100 + fi)
    prev = L.ns_hip_set_compute_mode(1)
    try:
        for k in KS:
            wq = qkv[(fi, k)]
            for name, row in _rows(rng, k).items():
                buf = torch.zeros(k + 4, device="cuda")
                for off in (0, 1):  # off = 1: 4 bytes past a 16-byte boundary — the launch takes codes from the quantizer launch
                    if off and name != "random":
                        continue
                    x = buf[off:off + k].view(1, k)
                    x.copy_(torch.from_numpy(row))
                    waves = (0,) + WAVES if name == "random" and off == 0 else (0,)
                    for nw in waves:
                        with _Waves(L, nw):
                            _ab(L, _qkv_h(L, pkg, wq, x, None, k), ("int8 qkv", k, name, off, nw))
                            for n in NS:
                                w1, w3 = pair[(fi, n, k)]
                                d = torch.from_numpy(rng.standard_normal((1, n)).astype(np.float32)).cuda()
                                for epi in (range(6) if (nw == 0 and name == "random") else ((nw + off) % 6,)):
                                    def run():
                                        c = _full((1, n))
                                        pkg.check(L.ns_hip_f32f32_forward(x.data_ptr(), w1.h, c.data_ptr(), 1, k, n, epi,
                                                                          d.data_ptr() if epi in (1, 2, 3) else None, n, _stream()))
                                        return [c]
                                    _ab(L, run, ("int8 plain", n, k, name, off, nw, epi))
                                _ab(L, _gateup_h(L, pkg, w1, w3, x, None, n, k, pkg.EPI_SILU, nw != 2), ("int8 gate/up silu", n, k, name, off, nw))
                                if nw == 0:
                                    _ab(L, _gateup_h(L, pkg, w1, w3, x, None, n, k, pkg.EPI_GELU, off == 0), ("int8 gate/up gelu", n, k, name, off))
    finally:
        L.ns_hip_set_compute_mode(prev)


def test_one_row_form_against_the_oracle(L, pkg, nso):
    """one fp16 and one int8-reference launch of the one-row form, held to the bars the general form is held to"""
    import torch
    rng = np.random.default_rng(7)
    n, k = 64, 512
    w = (rng.standard_normal((n, k)) * 0.02).astype(np.float32)
    a = rng.standard_normal((1, k)).astype(np.float32)
    blob = nso.quant_pack(w, 32, nso.S4, nso.BF16, False, nso.CORE_AVX512_VNNI_KB)
    wt = pkg.Weight.from_host_blob(nso.ptr(blob))
    x = torch.from_numpy(a).cuda()
    x16 = x.half()
    assert L.ns_hip_set_tuning(b"gv_rows1", 1) == 0
    c = _full((1, n))
    pkg.check(L.ns_hip_f32f32_forward_h(x.data_ptr(), x16.data_ptr(), wt.h, c.data_ptr(), None, 1, k, n, 0, None, 0, _stream()))
    err = nso.rel_l2(c.cpu().numpy(), nso.gemm_f64(a, blob))
    assert err < TOL_FP16, err
    prev = L.ns_hip_set_compute_mode(1)
    try:
        c8 = _full((1, n))
        pkg.check(L.ns_hip_f32f32_forward(x.data_ptr(), wt.h, c8.data_ptr(), 1, k, n, 0, None, 0, _stream()))
        err8 = nso.rel_l2(c8.cpu().numpy(), nso.gemm_u8s8(a, blob))
    finally:
        L.ns_hip_set_compute_mode(prev)
    assert err8 < TOL_INT8, err8


def test_one_row_form_captured_in_a_graph_and_replayed(L, pkg, nso, weights):
    import torch
    pair, _, _ = weights
    n, k = 40, 416
    w1, w3 = pair[(0, n, k)]
    x = torch.randn((1, k), device="cuda")
    x16 = x.half()
    t2_eager, t2, t1 = _full((1, n)), _full((1, n)), _full((1, n))
    try:
        assert L.ns_hip_set_tuning(b"gv_rows1", 0) == 0
        pkg.check(L.ns_hip_fusion_ffn3_gateup_h(x.data_ptr(), x16.data_ptr(), w1.h, w3.h, None, t2_eager.data_ptr(), None, 1, pkg.EPI_SILU, _stream()))
        torch.cuda.synchronize()
        assert L.ns_hip_set_tuning(b"gv_rows1", 1) == 0
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            pkg.check(L.ns_hip_fusion_ffn3_gateup_h(x.data_ptr(), x16.data_ptr(), w1.h, w3.h, t1.data_ptr(), t2.data_ptr(), None, 1, pkg.EPI_SILU, _stream()))
        for _ in range(2):
            t2.fill_(SENTINEL)
            g.replay()
            torch.cuda.synchronize()
            assert np.array_equal(_bits(t2), _bits(t2_eager))
    finally:
        L.ns_hip_set_tuning(b"gv_rows1", 1)


def test_the_switch_changes_nothing_at_two_rows(L, pkg, nso, weights):
    import torch
    pair, _, _ = weights
    n, k = 40, 512
    w1, _w3 = pair[(1, n, k)]
    x = torch.randn((2, k), device="cuda")
    x16 = x.half()

    def run():
        c, c16 = _full((2, n)), _full((2, n), torch.float16)
        pkg.check(L.ns_hip_f32f32_forward_h(x.data_ptr(), x16.data_ptr(), w1.h, c.data_ptr(), c16.data_ptr(), 2, k, n, 0, None, 0, _stream()))
        return [c, c16]
    out = _ab(L, run, "two rows")
    assert not (out[0] == np.float32(SENTINEL).view(np.uint32)).any()


def test_the_key_is_accepted(L):
    assert L.ns_hip_set_tuning(b"gv_rows1", 0) == 0
    assert L.ns_hip_set_tuning(b"gv_rows1", 1) == 0

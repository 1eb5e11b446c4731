"""GPU parity tests proper: every call goes through the C ABI of libns_hip.so and is compared with the CPU oracle
on the same seeded inputs.

Bars (north_star): bit-exact for the quantize / pack step and for unpack; GEMM outputs within 1e-3 relative
(metric = ||y - y_ref||_2 / ||y_ref||_2, the reference's own cmpData.diff2, tests/test_python_api.py:27-33) of the
comp-fp32 semantics evaluated in fp64.  A tighter secondary bar isolates kernel error from the fp16 rounding of
the activations: against the oracle fed the same fp16-rounded activations the HIP result must agree to 3e-5
(integer weights: only fp32 accumulation order differs) / 6e-4 (f4 weights: LUT values are rounded to fp16).
"""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

_spec = importlib.util.spec_from_file_location("gemm_blocks", os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools", "gemm_blocks.py"))
gb = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gb)

pytestmark = pytest.mark.gpu

TOL = 1e-3        # north_star tolerance
TOL_A16_INT = 3e-5   # small-M kernels: exact (code - zp) * scale in fp32, only A is rounded to fp16
TOL_A16_F4 = 6e-4
TOL_A16_GEMM = 5e-4  # M > 64 (prefill GEMM): weights are rounded to fp16 AFTER scaling, 2^-12 relative each


def _w(rng, n, k, kind="normal"):
    if kind == "uniform":
        return rng.uniform(-0.5, 0.5, (n, k)).astype(np.float32)
    return (rng.standard_normal((n, k)) * 0.02).astype(np.float32)


def _gpu_quant_pack(L, pkg, nso, w, bs, qt, st, asym, comp, is_trans=True):
    n, k = w.shape if is_trans else w.shape[::-1]
    size = L.ns_BTLAGemmPackBSize(n, k, bs & 0xFFFFFFFFFFFFFFFF, qt, st, asym, comp, None)
    assert size > 0, pkg.last_error()
    blob = nso.aligned_bytes(size)
    ok = L.ns_BTLAGemmQuantPackB(nso.ptr(blob), nso.ptr(w), n, k, w.shape[1], bs & 0xFFFFFFFFFFFFFFFF, qt, st, asym,
                                 comp, is_trans, None)
    assert ok, pkg.last_error()
    return blob


# ---------------------------------------------------------------------------------------------- quantize / pack
ALL_QT = [("S%d" % b, b | (1 << 8)) for b in range(1, 9)] + [("NF4", 4 | (2 << 16)), ("BNB", 4 | (1 << 16)), ("E2M1", 4)]


@pytest.mark.parametrize("name,qt", ALL_QT)
@pytest.mark.parametrize("asym", [False, True])
def test_quant_pack_bit_exact(L, pkg, nso, name, qt, asym):
    is_int = ((qt >> 8) & 0xff) == 1
    if asym and not is_int:
        pytest.skip("float weights have no zero point")
    rng = np.random.default_rng(qt & 0xffff)
    for core, comp in [(nso.CORE_AVX512_VNNI_KB, pkg.COMP_INT8), (nso.CORE_AVX512F, pkg.COMP_F32),
                       (nso.CORE_AMX_BF16, pkg.COMP_BF16)]:
        if core == nso.CORE_AVX512_VNNI_KB and (not is_int or (qt == pkg.S8 and asym)):
            continue  # bestla_gemm.cpp:250: falls through to the next compute type
        for (n, k, bs, st) in [(96, 128, 32, pkg.BF16), (100, 160, 32, pkg.F32), (48, 256, 128, pkg.F16),
                               (50, 100, 32, pkg.BF16), (64, 96, -1, pkg.F32)]:
            if not is_int and st == pkg.F16:
                st = pkg.BF16
            if core == nso.CORE_AMX_BF16 and (bs % 32 or bs < 0):
                continue
            for kind in ("normal", "uniform"):
                w = _w(rng, n, k, kind)
                if kind == "normal":
                    w[0, 0:32] = 0.0  # all-zero group
                    w[1, 0:32] = np.abs(w[1, 0:32])  # dominant-positive group
                L.ns_set_pack_core(core)
                try:
                    mine = _gpu_quant_pack(L, pkg, nso, w, bs, qt, st, asym, comp)
                finally:
                    L.ns_set_pack_core(pkg.CORE_AUTO)
                ref = nso.quant_pack(w, bs, qt, st, asym, core)
                assert mine.size == ref.size
                if not np.array_equal(mine, ref):
                    bad = np.nonzero(mine != ref)[0]
                    bi = nso.parse(ref)
                    raise AssertionError("blob differs at %d bytes, first %d (q_off %d s_off %d z_off %d r_off %d) %s" % (
                        bad.size, bad[0], bi.q_off, bi.scale_off, bi.zp_off, bi.red_off, (name, asym, core, n, k, bs, st)))


def test_quant_pack_not_transposed_and_ld(L, pkg, nso):
    rng = np.random.default_rng(5)
    n, k, bs = 80, 128, 32
    w_kn = np.ascontiguousarray(_w(rng, n, k).T)  # [K][N]
    mine = _gpu_quant_pack(L, pkg, nso, w_kn, bs, pkg.S4, pkg.BF16, False, pkg.COMP_INT8, is_trans=False)
    ref = nso.quant_pack(w_kn, bs, nso.S4, nso.BF16, False, nso.CORE_AVX512_VNNI_KB, is_trans=False)
    assert np.array_equal(mine, ref)


@pytest.mark.parametrize("bits", [2, 3, 4, 5, 8])
def test_pack_q_bit_exact(L, pkg, nso, bits):
    rng = np.random.default_rng(bits)
    n, k, bs = 70, 128, 32
    full = 1 << (bits - 1)
    q = rng.integers(-full, full, (k, n), dtype=np.int8)
    sc = rng.uniform(0.001, 0.02, (k // bs, n)).astype(np.float32)
    zp = rng.integers(-full, full, (k // bs, n), dtype=np.int8)
    qt = pkg.INT_TYPES[bits]
    for asym in (False, True):
        size = L.ns_BTLAGemmPackBSize(n, k, bs, qt, pkg.BF16, asym, pkg.COMP_INT8, None)
        blob = nso.aligned_bytes(size)
        assert L.ns_BTLAGemmPackB(nso.ptr(blob), nso.ptr(q), nso.ptr(sc), nso.ptr(zp) if asym else None, n, k, n, bs, qt,
                                  pkg.BF16, asym, pkg.COMP_INT8, None, None), pkg.last_error()
        # asymmetric S8 is not offered on the int8 cores (bestla_gemm.cpp:250): the size function falls through to bf16
        core = nso.CORE_AMX_BF16 if (bits == 8 and asym) else nso.CORE_AVX512_VNNI_KB
        ref = nso.pack_q(q, sc, zp if asym else None, bs, qt, nso.BF16, core)
        assert np.array_equal(blob, ref)


# ---------------------------------------------------------------------------------------------- unpack
@pytest.mark.parametrize("qt,st,asym,core", [
    ("S4", "BF16", False, "CORE_AVX512_VNNI_KB"), ("S4", "F32", True, "CORE_AVX512F"), ("S4", "F16", True, "CORE_AMX_BF16"),
    ("S8", "BF16", False, "CORE_AVX512F"), ("S8", "F32", True, "CORE_AVX2"), ("F4_NF4", "BF16", False, "CORE_AVX512F"),
    ("F4_BNB", "F32", False, "CORE_AMX_BF16"), ("F4_E2M1", "F32", False, "CORE_AVX2"), ("S4", "BF16", False, "CORE_AMX_INT8_KB"),
    ("S4", "BF16", True, "CORE_AVX_VNNI_KB")])
def test_unpack_bit_exact(L, pkg, nso, qt, st, asym, core):
    rng = np.random.default_rng(17)
    for n, k, bs in [(100, 256, 32), (48, 128, 128), (33, 192, 64), (64, 320, -1), (70, 100, 32)]:
        if core in ("CORE_AMX_BF16",) and (bs < 0 or bs % 32):
            continue
        if core == "CORE_AMX_INT8_KB" and bs % 64:
            continue
        w = _w(rng, n, k)
        blob = nso.quant_pack(w, bs, getattr(nso, qt), getattr(nso, st), asym, getattr(nso, core))
        out = np.zeros((k, n + 3), np.float32)
        L.bestla_unpackweight_fp32(nso.ptr(blob), n, k, nso.ptr(out), n + 3)
        ref = nso.unpack_fp32(blob)
        assert np.array_equal(out[:, :n].view(np.uint32), ref.view(np.uint32)), (n, k, bs)
        assert np.all(out[:, n:] == 0)


# ---------------------------------------------------------------------------------------------- forward parity
FWD_FORMATS = [
    ("S4", "BF16", False, "CORE_AVX512_VNNI_KB", 32),   # "Q4_0" of the BesTLA path (core/README.md:97)
    ("S4", "F32", False, "CORE_AVX512F", 32),
    ("S4", "BF16", True, "CORE_AVX512_VNNI_KB", 32),
    ("S4", "F16", True, "CORE_AVX512F", 64),
    ("S4", "BF16", False, "CORE_AMX_INT8_KB", 128),
    ("S4", "F32", True, "CORE_AMX_BF16", 256),
    ("S4", "F32", False, "CORE_AVX512F", -1),
    ("S8", "BF16", False, "CORE_AVX512F", 32),
    ("S8", "F32", True, "CORE_AVX512F", 64),
    ("S8", "BF16", False, "CORE_AMX_BF16", 128),
    ("F4_NF4", "BF16", False, "CORE_AVX512F", 128),
    ("F4_NF4", "F32", False, "CORE_AMX_BF16", 32),
    ("F4_BNB", "F32", False, "CORE_AVX512F", 32),
    ("F4_E2M1", "BF16", False, "CORE_AVX512F", 64),
]


def _check(nso, out, a, blob, is_f4):
    ref = nso.gemm_f64(a, blob)
    ref16 = nso.gemm_f64(a, blob, a16=True)
    e = nso.rel_l2(out, ref)
    e16 = nso.rel_l2(out, ref16)
    assert e < TOL, "rel l2 vs fp32-activation oracle %g" % e
    tol16 = TOL_A16_F4 if is_f4 else (TOL_A16_GEMM if out.shape[0] > 64 else TOL_A16_INT)
    assert e16 < tol16, "rel l2 vs fp16-activation oracle %g" % e16
    # row by row and 16-column tile by tile as well: one wrong row or tile must not hide behind the others (tests/tools/gemm_blocks.py)
    gb.check_rows_tiles(out, ref, TOL, "fp32-activation oracle")
    gb.check_rows_tiles(out, ref16, tol16, "fp16-activation oracle")
    return e, e16


@pytest.mark.parametrize("qt,st,asym,core,bs", FWD_FORMATS)
@pytest.mark.parametrize("m", [1, 4, 8])
def test_forward_formats(L, pkg, nso, qt, st, asym, core, bs, m):
    rng = np.random.default_rng(1000 + m)
    n, k = 272, 1024  # 17 tiles, 8 (4-bit) / 16 (8-bit) k-steps
    w = _w(rng, n, k)
    a = rng.standard_normal((m, k)).astype(np.float32)
    blob = nso.quant_pack(w, bs, getattr(nso, qt), getattr(nso, st), asym, getattr(nso, core))
    out = np.zeros((m, n), np.float32)
    L.bestla_f32f32_forward(nso.ptr(a), nso.ptr(blob), nso.ptr(out), m, n, k, k, n, None)
    _check(nso, out, a, blob, qt.startswith("F4"))


@pytest.mark.parametrize("bits", [1, 2, 3, 5, 6, 7])
@pytest.mark.parametrize("m", [1, 3, 70])
def test_forward_odd_bit_widths(L, pkg, nso, bits, m):
    """S1..S3 / S5..S7 (the reference GEMV's 1,2,3,5,6,7-bit twins, kernel_ref.h:2533-3370): bit-plane blobs are widened
    to the nibble / byte containers at load; the forward must match the oracle like the native widths do."""
    rng = np.random.default_rng(40 + bits * 7 + m)
    n, k, bs = 144, 768, 32
    w = _w(rng, n, k)
    a = rng.standard_normal((m, k)).astype(np.float32)
    for asym, st, core in ((False, nso.BF16, nso.CORE_AVX512_VNNI_KB), (True, nso.F32, nso.CORE_AVX512F)):
        blob = nso.quant_pack(w, bs, nso.INT_TYPES[bits], st, asym, core)
        out = np.zeros((m, n), np.float32)
        L.bestla_f32f32_forward(nso.ptr(a), nso.ptr(blob), nso.ptr(out), m, n, k, k, n, None)
        _check(nso, out, a, blob, False)
        # and the device unpack agrees with the reference's dequantisation bit for bit
        deq = np.zeros((k, n), np.float32)
        L.bestla_unpackweight_fp32(nso.ptr(blob), n, k, nso.ptr(deq), n)
        assert np.array_equal(deq, nso.unpack_fp32(blob))


@pytest.mark.parametrize("m", [1, 2, 3, 5, 16, 17, 32, 33, 64, 65, 130])
def test_forward_row_counts(L, pkg, nso, m):
    rng = np.random.default_rng(m)
    n, k, bs = 96, 512, 32
    w = _w(rng, n, k)
    a = rng.standard_normal((m, k)).astype(np.float32)
    blob = nso.quant_pack(w, bs, nso.S4, nso.BF16, False, nso.CORE_AVX512_VNNI_KB)
    out = np.zeros((m, n), np.float32)
    L.bestla_f32f32_forward(nso.ptr(a), nso.ptr(blob), nso.ptr(out), m, n, k, k, n, None)
    _check(nso, out, a, blob, False)


@pytest.mark.parametrize("n,k", [(16, 128), (1, 128), (17, 160), (100, 96), (250, 1000), (48, 4096), (333, 2176)])
def test_forward_ragged_shapes(L, pkg, nso, n, k):
    """N not a multiple of 16/48, K not a multiple of 128 (tail k-step zero padded, tail quant block)."""
    rng = np.random.default_rng(n * 7 + k)
    for m in (1, 7):
        w = _w(rng, n, k)
        a = rng.standard_normal((m, k)).astype(np.float32)
        for qt, core in ((nso.S4, nso.CORE_AVX512F), (nso.S8, nso.CORE_AVX512F)):
            blob = nso.quant_pack(w, 32, qt, nso.BF16, False, core)
            out = np.full((m, n + 2), -5.0, np.float32)
            L.bestla_f32f32_forward(nso.ptr(a), nso.ptr(blob), nso.ptr(out), m, n, k, k, n + 2, None)
            assert np.all(out[:, n:] == -5.0)  # ldo honoured, nothing written past N
            _check(nso, np.ascontiguousarray(out[:, :n]), a, blob, False)


def test_prefill_fp16_shadow_in_and_out(L, pkg, nso):
    """M > 64 (gemm2_kernel): a caller-provided fp16 activation shadow gives bit-identical results to the internal
    conversion pass, and the fp16 output shadow equals the rounded fp32 output."""
    import torch
    import ctypes as C
    rng = np.random.default_rng(123)
    n, k, m, bs = 272, 1024, 150, 32
    w = _w(rng, n, k)
    a = rng.standard_normal((m, k)).astype(np.float32)
    blob = nso.quant_pack(w, bs, nso.S4, nso.BF16, False, nso.CORE_AVX512_VNNI_KB)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    wt = pkg.Weight.from_host_blob(nso.ptr(blob), st)
    da = torch.from_numpy(a).cuda()
    da16 = da.half()
    c0 = torch.zeros((m, n), device="cuda")
    c1 = torch.zeros((m, n), device="cuda")
    c16 = torch.zeros((m, n), device="cuda", dtype=torch.float16)
    pkg.check(L.ns_hip_f32f32_forward(da.data_ptr(), wt.h, c0.data_ptr(), m, k, n, pkg.EPI_NONE, None, 0, st))
    pkg.check(L.ns_hip_f32f32_forward_h(da.data_ptr(), da16.data_ptr(), wt.h, c1.data_ptr(), c16.data_ptr(), m, k, n,
                                        pkg.EPI_NONE, None, 0, st))
    torch.cuda.synchronize()
    assert torch.equal(c0, c1)
    assert torch.equal(c16, c1.half())
    _check(nso, c1.cpu().numpy(), a, blob, False)
    wt.free()


@pytest.mark.parametrize("m,k,bs", [(1, 4096, 32), (5, 1000, 128), (3, 96, 64), (2, 130, 32)])
def test_activation_u8_quantize_bit_exact(L, pkg, nso, m, k, bs):
    """a9: quantize_fp_u8_colblock (kernel_ref.h:1824-1883) on the GPU == the oracle (itself pinned to the reference),
    byte for byte: codes, scales, zero points, block sums; tail blocks, all-zero and one-sided blocks included."""
    import torch
    import ctypes as C
    rng = np.random.default_rng(m * 31 + k)
    a = rng.standard_normal((m, k + 3)).astype(np.float32)
    a[0, : min(k, bs)] = 0.0                       # all-zero block
    if k >= 2 * bs:
        a[0, bs:2 * bs] = np.abs(a[0, bs:2 * bs])  # one-sided block (min stays 0)
    nblk = (k + bs - 1) // bs
    q = np.zeros((m, k), np.uint8)
    sc = np.zeros((m, nblk), np.float32)
    zp = np.zeros((m, nblk), np.uint8)
    red = np.zeros((m, nblk), np.float32)
    assert nso.lib().nso_quantize_fp_u8_colblock(m, k, nso.ptr(a), k + 3, nso.ptr(q), k, nso.ptr(sc), nblk, nso.ptr(zp), bs,
                                                 nso.ptr(red)) == 0
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    da = torch.from_numpy(a).cuda()
    dq = torch.zeros((m, k), dtype=torch.uint8, device="cuda")
    dsc = torch.zeros((m, nblk), device="cuda")
    dzp = torch.zeros((m, nblk), dtype=torch.uint8, device="cuda")
    dred = torch.zeros((m, nblk), device="cuda")
    pkg.check(L.ns_hip_quantize_fp_u8_colblock(m, k, da.data_ptr(), k + 3, dq.data_ptr(), k, dsc.data_ptr(), nblk,
                                               dzp.data_ptr(), bs, dred.data_ptr(), st))
    torch.cuda.synchronize()
    assert np.array_equal(dq.cpu().numpy(), q)
    assert np.array_equal(dsc.cpu().numpy().view(np.uint32), sc.view(np.uint32))
    assert np.array_equal(dzp.cpu().numpy(), zp)
    assert np.array_equal(dred.cpu().numpy().view(np.uint32), red.view(np.uint32))


@pytest.mark.parametrize("m,k,bs,pad", [(64, 4096, 32, 4), (33, 1024, 128, 8), (16, 512, 64, 0), (40, 256, 256, 12)])
def test_activation_u8_quantize_gemm_sized_form_bit_exact(L, pkg, nso, m, k, bs, pad):
    """a9 at GEMM size (16 rows and up, no block sums): the vector form of the quantizer (aquant_u8_vec_kernel: 16-byte loads,
    dword stores, eight lanes per k-block) == the oracle byte for byte: codes, scales, zero points; all-zero, one-sided and
    constant blocks included."""
    import torch
    import ctypes as C
    rng = np.random.default_rng(m * 17 + k)
    a = (rng.standard_normal((m, k + pad)) * rng.uniform(0.01, 30.0, (m, 1))).astype(np.float32)
    a[0, :bs] = 0.0
    a[1, :bs] = np.abs(a[1, :bs])
    a[2, :bs] = -np.abs(a[2, :bs])
    a[3, :bs] = 2.5
    nblk = k // bs
    q = np.zeros((m, k), np.uint8)
    sc = np.zeros((m, nblk), np.float32)
    zp = np.zeros((m, nblk), np.uint8)
    red = np.zeros((m, nblk), np.float32)
    assert nso.lib().nso_quantize_fp_u8_colblock(m, k, nso.ptr(a), k + pad, nso.ptr(q), k, nso.ptr(sc), nblk, nso.ptr(zp), bs,
                                                 nso.ptr(red)) == 0
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    da = torch.from_numpy(a).cuda()
    dq = torch.zeros((m, k), dtype=torch.uint8, device="cuda")
    dsc = torch.zeros((m, nblk), device="cuda")
    dzp = torch.zeros((m, nblk), dtype=torch.uint8, device="cuda")
    pkg.check(L.ns_hip_quantize_fp_u8_colblock(m, k, da.data_ptr(), k + pad, dq.data_ptr(), k, dsc.data_ptr(), nblk,
                                               dzp.data_ptr(), bs, None, st))
    torch.cuda.synchronize()
    assert np.array_equal(dq.cpu().numpy(), q)
    assert np.array_equal(dsc.cpu().numpy().view(np.uint32), sc.view(np.uint32))
    assert np.array_equal(dzp.cpu().numpy(), zp)


def test_forward_lda_and_uniform_distribution(L, pkg, nso):
    rng = np.random.default_rng(77)
    n, k, bs, m = 128, 768, 32, 3
    w = _w(rng, n, k, "uniform")  # reference UT distribution (ut/bestla_ut.h:129-134)
    abig = rng.uniform(-0.5, 0.5, (m, k + 5)).astype(np.float32)
    blob = nso.quant_pack(w, bs, nso.S4, nso.F32, False, nso.CORE_AVX512F)
    out = np.zeros((m, n), np.float32)
    L.bestla_f32f32_forward(nso.ptr(abig), nso.ptr(blob), nso.ptr(out), m, n, k, k + 5, n, None)
    a = np.ascontiguousarray(abig[:, :k])
    _check(nso, out, a, blob, False)
    # the reference's two-sided check (ut/bestla_prologue_b.cpp:673-722): vs the ORIGINAL weights at quant-noise
    # tolerance INT4_ERR = 3.5 abs at K = 4096 scaled by sqrt(K) (ut/bestla_ut.h:80-127)
    full = a.astype(np.float64) @ w.astype(np.float64).T
    assert np.max(np.abs(out - full)) < 3.5 * np.sqrt(k / 4096.0)


def test_forward_adversarial_values(L, pkg, nso):
    rng = np.random.default_rng(99)
    n, k, bs = 64, 256, 32
    w = _w(rng, n, k)
    w[0, :] = 0.0                      # all-zero column: scale -0.0
    w[1, :32] = np.abs(w[1, :32]) + 1  # dominant positive -> negative scale
    w[2, 5] = 40.0                     # outlier
    w[3, :32] = 0.5 * np.where(np.arange(32) % 2 == 0, 1, -1)  # max == -min tie
    a = rng.standard_normal((1, k)).astype(np.float32)
    a[0, 7] = 300.0                    # large activation (fp16 range ok)
    a[0, 9] = 1e-7                     # flushes to an fp16 subnormal / zero
    for asym in (False, True):
        blob = nso.quant_pack(w, bs, nso.S4, nso.BF16, asym, nso.CORE_AVX512_VNNI_KB)
        out = np.zeros((1, n), np.float32)
        L.bestla_f32f32_forward(nso.ptr(a), nso.ptr(blob), nso.ptr(out), 1, n, k, k, n, None)
        assert out[0, 0] == 0.0
        _check(nso, out, a, blob, False)



@pytest.mark.parametrize("mag", [1e-7, 3e-5, 1.0, 2e4, 1e9])
@pytest.mark.parametrize("qt,st", [("S4", "F32"), ("S8", "F32"), ("F4_NF4", "F32"), ("S4", "BF16")])
def test_forward_weight_magnitudes(L, pkg, nso, mag, qt, st):
    """The reference dequantises and accumulates in fp32, so weights of any magnitude work.  The prefill GEMM keeps
    scaled weights in fp16: its load-time power-of-two normalisation must make that invisible, also when one column's
    scales are far below the rest."""
    rng = np.random.default_rng(int(abs(np.log2(mag)) * 10) + len(qt))
    n, k, bs = 160, 512, 32
    w = (_w(rng, n, k).astype(np.float64) * (mag / 0.02)).astype(np.float32)
    w[5, :] *= 2.0 ** -12   # a quiet column
    w[6, :64] *= 2.0 ** 7   # and a loud group
    blob = nso.quant_pack(w, bs, getattr(nso, qt), getattr(nso, st), False, nso.CORE_AVX512F)
    wq = nso.unpack_fp32(blob).astype(np.float64)   # [K][N]
    keep = np.arange(n) != 6
    for m in (2, 130):
        a = rng.standard_normal((m, k)).astype(np.float32)
        out = np.zeros((m, n), np.float32)
        L.bestla_f32f32_forward(nso.ptr(a), nso.ptr(blob), nso.ptr(out), m, n, k, k, n, None)
        assert np.all(np.isfinite(out))
        ref = nso.gemm_f64(a, blob)
        # every column on its own, against the size of its terms (a cancellation-proof yardstick: the loud column would
        # otherwise own the matrix norm, the quiet one would vanish in it)
        terms = np.abs(a.astype(np.float64)) @ np.abs(wq)
        assert np.max(np.abs(out - ref) / terms) < TOL
        # and the usual norm-wise budget without the loud column
        assert nso.rel_l2(out[:, keep], ref[:, keep]) < TOL
        assert nso.rel_l2(out[:, 5], ref[:, 5]) < 4 * TOL   # 2 .. 130 numbers: a loose norm-wise bound on the quiet column


# ---------------------------------------------------------------------------------------------- fp8 weights
F8_CASES = [("F8_E4M3", "F8_E8M0"), ("F8_E4M3", "F32"), ("F8_E5M2", "F8_E8M0"), ("F8_E5M2", "F32")]


@pytest.mark.parametrize("f8,st", F8_CASES)
def test_fp8_quant_pack_and_unpack_bit_exact(L, pkg, nso, f8, st):
    """fp8 weights with shared-exponent (E8M0) or fp32 scales (quant_utils.cpp:307-341 -> WeightKBlockNFloat,
    kernel_ref.h:1721-1799): the GPU quantizer's blob and the device unpack against the oracle, byte for byte."""
    qt, sdt = getattr(nso, f8), getattr(nso, st)
    rng = np.random.default_rng(sum(map(ord, f8 + st)))
    for core, comp in [(nso.CORE_AVX512F, pkg.COMP_F32), (nso.CORE_AMX_BF16, pkg.COMP_BF16)]:
        for (n, k, bs) in [(96, 128, 32), (100, 160, 32), (48, 256, 128), (50, 100, 32), (64, 96, -1)]:
            if core == nso.CORE_AMX_BF16 and (bs % 32 or bs < 0):
                continue
            for kind in ("normal", "uniform"):
                w = _w(rng, n, k, kind)
                w[0, 0:32] = 0.0                                   # all-zero group: shared exponent clamps at -127
                w[1, 0:32] *= np.float32(2.0) ** rng.integers(-24, 4, 32).astype(np.float32)  # wide in-group range
                w[2, 0] = np.nextafter(np.float32(0.25), np.float32(0))  # absmax a hair below a power of two
                L.ns_set_pack_core(core)
                try:
                    mine = _gpu_quant_pack(L, pkg, nso, w, bs, qt, sdt, False, comp)
                finally:
                    L.ns_set_pack_core(pkg.CORE_AUTO)
                ref = nso.quant_pack(w, bs, qt, sdt, False, core)
                assert mine.size == ref.size
                if not np.array_equal(mine, ref):
                    bad = np.nonzero(mine != ref)[0]
                    bi = nso.parse(ref)
                    raise AssertionError("blob differs at %d bytes, first %d (q_off %d s_off %d) %s" % (
                        bad.size, bad[0], bi.q_off, bi.scale_off, (f8, st, core, n, k, bs, kind)))
                out = np.zeros((k, n), np.float32)
                L.bestla_unpackweight_fp32(nso.ptr(ref), n, k, nso.ptr(out), n)
                assert np.array_equal(out.view(np.uint32), nso.unpack_fp32(ref).view(np.uint32)), (n, k, bs)


@pytest.mark.parametrize("f8,st", F8_CASES)
@pytest.mark.parametrize("m", [1, 4, 8, 33, 70, 130])
def test_fp8_forward(L, pkg, nso, f8, st, m):
    rng = np.random.default_rng(500 + m)
    for n, k, bs, core in [(272, 1024, 32, nso.CORE_AVX512F), (100, 320, 64, nso.CORE_AMX_BF16), (48, 200, -1, nso.CORE_AVX512F)]:
        w = _w(rng, n, k)
        a = rng.standard_normal((m, k)).astype(np.float32)
        blob = nso.quant_pack(w, bs, getattr(nso, f8), getattr(nso, st), False, core)
        out = np.zeros((m, n), np.float32)
        L.bestla_f32f32_forward(nso.ptr(a), nso.ptr(blob), nso.ptr(out), m, n, k, k, n, None)
        _check(nso, out, a, blob, False)   # fp8 -> fp16 is exact, the group scale is applied in fp32: integer-class budget


def test_fp8_every_code_and_zero_weights(L, pkg, nso):
    """All 256 codes of both encodings go through the kernels' bit-level fp8 -> fp16 conversion, including the E5M2 codes
    with a zero exponent field that land on fp16 subnormals; an all-zero weight column is NOT zero in the reference's
    encoding (code 0x00 = 2^-7 / 2^-15 times the scale) and must come out the same way here."""
    rng = np.random.default_rng(8)
    n, k, bs = 32, 256, 32
    for f8 in ("F8_E4M3", "F8_E5M2"):
        qt = getattr(nso, f8)
        w = _w(rng, n, k)
        w[3, :] = 0.0
        blob = nso.quant_pack(w, bs, qt, nso.F32, False, nso.CORE_AVX512F)
        bi = nso.parse(blob)
        # overwrite the code image: column c of tile 0 holds codes (c * 8 + r) % 256 — every code appears
        img = blob[bi.q_off: bi.q_off + bi.q_bytes]
        img[:] = (np.arange(img.size) * 37 + 11) % 256
        if f8 == "F8_E5M2":
            # exponent field 31 is >= 65536: beyond the reference quantizer's max_norm (57344) and beyond fp16 — such a
            # blob is refused at load (checked below); fold those codes back into range here
            hot = (img & 0x7c) == 0x7c
            img[hot] &= 0xbf
        sc = blob[bi.scale_off: bi.scale_off + bi.scale_bytes].view(np.float32)
        sc[:] = 2.0 ** -3   # power of two: products with a one-hot activation are exact
        deq = nso.unpack_fp32(blob)
        assert np.unique(np.abs(deq)).size >= 100
        out = np.zeros((k, n), np.float32)
        L.bestla_unpackweight_fp32(nso.ptr(blob), n, k, nso.ptr(out), n)
        assert np.array_equal(out.view(np.uint32), deq.view(np.uint32))
        # one-hot activations read single weights back through the MFMA path: exact, also for subnormal fp16 operands
        for m in (1, 70):
            a = np.zeros((m, k), np.float32)
            rows = rng.integers(0, k, m)
            a[np.arange(m), rows] = 1.0
            c = np.zeros((m, n), np.float32)
            L.bestla_f32f32_forward(nso.ptr(a), nso.ptr(blob), nso.ptr(c), m, n, k, k, n, None)
            assert np.array_equal(c, deq[rows, :]), (f8, m)
    # an E5M2 code outside fp16 makes the load fail loudly instead of producing inf / nan
    bad = nso.aligned_bytes(blob.size)
    bad[:] = blob
    bad[bi.q_off + 5] = 0x7d
    print("(the error line below is expected)")
    c = np.full((1, n), 7.0, np.float32)
    L.bestla_f32f32_forward(nso.ptr(a[:1]), nso.ptr(bad), nso.ptr(c), 1, n, k, k, n, None)
    assert "exponent field 31" in pkg.last_error()

# ---------------------------------------------------------------------------------------------- fused entry points
def test_fusion_add_bias(L, pkg, nso):
    rng = np.random.default_rng(3)
    n, k, m = 112, 512, 5
    w = _w(rng, n, k)
    a = rng.standard_normal((m, k)).astype(np.float32)
    blob = nso.quant_pack(w, 32, nso.S4, nso.BF16, False, nso.CORE_AVX512_VNNI_KB)
    assert L.bestla_fusion_add_f32f32_support(nso.ptr(blob), m, n, k)
    ref = nso.gemm_f64(a, blob)
    for bcast in (True, False):
        bias = rng.standard_normal((1 if bcast else m, n)).astype(np.float32)
        out = np.zeros((m, n), np.float32)
        L.bestla_fusion_add_f32f32_forward(nso.ptr(a), nso.ptr(blob), nso.ptr(bias), nso.ptr(out), m, n, k, k, n, bcast, None)
        assert nso.rel_l2(out, ref + bias) < TOL


@pytest.mark.parametrize("m", [1, 6, 70])
def test_fusion_qkv(L, pkg, nso, m):
    rng = np.random.default_rng(4)
    n, k = 160, 512
    a = rng.standard_normal((m, k)).astype(np.float32)
    blobs = [nso.quant_pack(_w(rng, n, k), 32, nso.S4, nso.BF16, False, nso.CORE_AVX512_VNNI_KB) for _ in range(3)]
    assert L.bestla_fusion_QKV_f32f32_support(*[nso.ptr(b) for b in blobs], m, n, k)
    other = nso.quant_pack(_w(rng, n, k), 128, nso.S4, nso.BF16, False, nso.CORE_AVX512_VNNI_KB)
    assert not L.bestla_fusion_QKV_f32f32_support(nso.ptr(blobs[0]), nso.ptr(other), nso.ptr(blobs[2]), m, n, k)
    out = np.zeros((3, m, n), np.float32)
    L.bestla_fusion_QKV_f32f32_forward(nso.ptr(a), *[nso.ptr(b) for b in blobs], nso.ptr(out), m, n, k, k, n, None)
    for i in range(3):
        assert nso.rel_l2(out[i], nso.gemm_f64(a, blobs[i])) < TOL


def _act(nso, x, name):
    f = nso.lib().nso_silu if name == "silu" else nso.lib().nso_gelu
    return np.vectorize(lambda v: f(float(v)))(x.astype(np.float32)).astype(np.float64)


@pytest.mark.parametrize("m", [1, 4, 66])
@pytest.mark.parametrize("act", ["silu", "gelu"])
def test_fusion_ffn3(L, pkg, nso, m, act):
    """tmp1 = act(A*W1), tmp2 = (A*W3)*tmp1, out = tmp2*W2 (ip_fusion_ffn.cpp:364-406)"""
    rng = np.random.default_rng(6)
    fin, fmid, fout = 256, 352, 256
    a = rng.standard_normal((m, fin)).astype(np.float32)
    mk = lambda n, k: nso.quant_pack(_w(rng, n, k) * 3, 32, nso.S4, nso.BF16, False, nso.CORE_AVX512_VNNI_KB)
    b1, b3, b2 = mk(fmid, fin), mk(fmid, fin), mk(fout, fmid)
    sup = L.bestla_fusion_FFN_SiLu_f32f32_support if act == "silu" else L.bestla_fusion_FFN_Gelu_Mul_f32f32_support
    fwd = L.bestla_fusion_FFN_SiLu_f32f32_forward if act == "silu" else L.bestla_fusion_FFN_Gelu_Mul_f32f32_forward
    assert sup(nso.ptr(b1), nso.ptr(b2), nso.ptr(b3), m, fin, fmid, fout)
    t1 = np.zeros((m, fmid), np.float32)
    t2 = np.zeros((m, fmid), np.float32)
    out = np.zeros((m, fout), np.float32)
    fwd(nso.ptr(a), nso.ptr(b1), nso.ptr(b2), nso.ptr(b3), nso.ptr(t1), nso.ptr(t2), nso.ptr(out), m, fin, fmid, fout, None)
    r1 = _act(nso, nso.gemm_f64(a, b1), act)
    r2 = nso.gemm_f64(a, b3) * r1
    assert nso.rel_l2(t1, r1) < TOL
    assert nso.rel_l2(t2, r2) < TOL
    # last GEMM checked against the oracle fed the HIP tmp2 (isolates it), and end to end
    assert nso.rel_l2(out, nso.gemm_f64(t2, b2)) < TOL
    assert nso.rel_l2(out, nso.gemm_f64(r2.astype(np.float32), b2)) < 2 * TOL


def test_fusion_ffn2_gelu_and_add_gelu(L, pkg, nso):
    rng = np.random.default_rng(8)
    m, fin, fmid, fout = 3, 256, 320, 128
    a = rng.standard_normal((m, fin)).astype(np.float32)
    mk = lambda n, k: nso.quant_pack(_w(rng, n, k) * 3, 32, nso.S4, nso.BF16, False, nso.CORE_AVX512_VNNI_KB)
    b1, b2 = mk(fmid, fin), mk(fout, fmid)
    assert L.bestla_fusion_FFN_GeLu_f32f32_support(nso.ptr(b1), nso.ptr(b2), m, fin, fmid, fout)
    t1 = np.zeros((m, fmid), np.float32)
    out = np.zeros((m, fout), np.float32)
    L.bestla_fusion_FFN_GeLu_f32f32_forward(nso.ptr(a), nso.ptr(b1), nso.ptr(b2), nso.ptr(t1), nso.ptr(out), m, fin, fmid, fout, None)
    r1 = _act(nso, nso.gemm_f64(a, b1), "gelu")
    assert nso.rel_l2(t1, r1) < TOL
    assert nso.rel_l2(out, nso.gemm_f64(t1, b2)) < TOL
    for bcast in (True, False):
        bias1 = rng.standard_normal((1 if bcast else m, fmid)).astype(np.float32)
        bias2 = rng.standard_normal((1 if bcast else m, fout)).astype(np.float32)
        L.bestla_fusion_FFN_Add_GeLu_f32f32_forward(nso.ptr(a), nso.ptr(b1), nso.ptr(b2), nso.ptr(bias1), nso.ptr(bias2),
                                                    nso.ptr(t1), nso.ptr(out), m, fin, fmid, fout, bcast, None)
        r1 = _act(nso, nso.gemm_f64(a, b1) + bias1, "gelu")
        assert nso.rel_l2(t1, r1) < TOL
        assert nso.rel_l2(out, nso.gemm_f64(t1, b2) + bias2) < TOL


def test_packweight_copyattr_roundtrip(L, pkg, nso):
    """bestla_split_weight pattern (model_files.h:1538-1563): unpack -> slice -> re-quantize with copied attributes."""
    rng = np.random.default_rng(12)
    n, k = 96, 256
    src = nso.quant_pack(_w(rng, n, k), 32, nso.S4, nso.BF16, True, nso.CORE_AVX512_VNNI_KB)
    deq = np.zeros((k, n), np.float32)
    L.bestla_unpackweight_fp32(nso.ptr(src), n, k, nso.ptr(deq), n)
    half = np.ascontiguousarray(deq[:, : n // 2])  # ROW split (N slice)
    size = nso.pack_size(n // 2, k, 32, nso.S4, nso.BF16, True, nso.CORE_AVX512_VNNI_KB)
    dst = nso.aligned_bytes(size)
    L.bestla_packweight_copyattr(nso.ptr(half), nso.ptr(dst), n // 2, k, n // 2, nso.ptr(src))
    ref = nso.quant_pack(half, 32, nso.S4, nso.BF16, True, nso.CORE_AVX512_VNNI_KB, is_trans=False)
    assert np.array_equal(dst, ref)


def test_elementwise_entries(L, pkg, nso):
    rng = np.random.default_rng(13)
    x = rng.standard_normal((5, 300)).astype(np.float32)
    out = np.zeros_like(x)
    L.bestla_layernormalization(5, 300, True, 1e-6, nso.ptr(x), nso.ptr(out))
    ref = x / np.sqrt((x.astype(np.float64) ** 2).mean(-1, keepdims=True) + 1e-6)
    assert nso.rel_l2(out, ref) < 1e-6
    L.bestla_layernormalization(5, 300, False, 1e-5, nso.ptr(x), nso.ptr(out))
    xd = x.astype(np.float64)
    ref = (xd - xd.mean(-1, keepdims=True)) / np.sqrt(xd.var(-1, keepdims=True) + 1e-5)
    assert nso.rel_l2(out, ref) < 1e-5
    v = rng.standard_normal((1, 300)).astype(np.float32)
    L.bestla_mul(5, 300, nso.ptr(x), nso.ptr(v), 0, nso.ptr(out))
    assert np.array_equal(out, x * v)
    L.bestla_add(5, 300, nso.ptr(x), nso.ptr(x), 300, nso.ptr(out))
    assert np.array_equal(out, x + x)
    # device-pointer twins: bit-identical to the host-pointer entries
    import torch
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    dx, dv = torch.from_numpy(x).cuda(), torch.from_numpy(v).cuda()
    do = torch.zeros_like(dx)
    pkg.check(L.ns_hip_layernormalization(5, 300, True, 1e-6, dx.data_ptr(), do.data_ptr(), st))
    L.bestla_layernormalization(5, 300, True, 1e-6, nso.ptr(x), nso.ptr(out))
    torch.cuda.synchronize()
    assert np.array_equal(do.cpu().numpy(), out)
    pkg.check(L.ns_hip_mul(5, 300, dx.data_ptr(), dv.data_ptr(), 0, do.data_ptr(), st))
    torch.cuda.synchronize()
    assert np.array_equal(do.cpu().numpy(), x * v)
    pkg.check(L.ns_hip_add(5, 300, dx.data_ptr(), dx.data_ptr(), 300, do.data_ptr(), st))
    torch.cuda.synchronize()
    assert np.array_equal(do.cpu().numpy(), x + x)
    # fused norm * gamma (+ fp16 shadow) == the two separate operators, bit for bit
    d16 = torch.zeros((5, 300), dtype=torch.float16, device="cuda")
    pkg.check(L.ns_hip_norm_mul_h(5, 300, True, 1e-6, dx.data_ptr(), dv.data_ptr(), do.data_ptr(), d16.data_ptr(), st))
    torch.cuda.synchronize()
    L.bestla_layernormalization(5, 300, True, 1e-6, nso.ptr(x), nso.ptr(out))
    assert np.array_equal(do.cpu().numpy(), out * v)
    assert torch.equal(d16, do.half())


# ---------------------------------------------------------------------------------------------- device-resident API
def test_device_api_and_device_quantizer(L, pkg, nso):
    import torch
    rng = np.random.default_rng(21)
    n, k, bs, m = 256, 1024, 32, 2
    w = _w(rng, n, k)
    a = rng.standard_normal((m, k)).astype(np.float32)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    dW = torch.from_numpy(w).cuda()
    size = L.ns_BTLAGemmPackBSize(n, k, bs, pkg.S4, pkg.BF16, False, pkg.COMP_INT8, None)
    dBlob = torch.zeros(size, dtype=torch.uint8, device="cuda")
    assert dBlob.data_ptr() % 64 == 0
    pkg.check(L.ns_hip_quant_pack_device(dBlob.data_ptr(), dW.data_ptr(), n, k, k, bs, pkg.S4, pkg.BF16, False,
                                         pkg.COMP_INT8, True, st))
    torch.cuda.synchronize()
    ref_blob = nso.quant_pack(w, bs, nso.S4, nso.BF16, False, nso.CORE_AVX512_VNNI_KB)
    assert np.array_equal(dBlob.cpu().numpy(), ref_blob)
    wt = pkg.Weight.from_device_blob(dBlob.data_ptr(), size, st)
    assert (wt.n, wt.k, wt.bits, wt.blocksize) == (n, k, 4, bs)
    assert wt.stream_bytes == n * k // 2 + n * (k // bs) * 2
    dA = torch.from_numpy(a).cuda()
    dC = torch.empty((m, n), dtype=torch.float32, device="cuda")
    pkg.check(L.ns_hip_f32f32_forward(dA.data_ptr(), wt.h, dC.data_ptr(), m, k, n, pkg.EPI_NONE, None, 0, st))
    torch.cuda.synchronize()
    assert nso.rel_l2(dC.cpu().numpy(), nso.gemm_f64(a, ref_blob)) < TOL
    # idempotence: same launch twice gives the same bits (deterministic reduction order, no atomics)
    dC2 = torch.empty_like(dC)
    pkg.check(L.ns_hip_f32f32_forward(dA.data_ptr(), wt.h, dC2.data_ptr(), m, k, n, pkg.EPI_NONE, None, 0, st))
    torch.cuda.synchronize()
    assert torch.equal(dC, dC2)


# ---------------------------------------------------------------------------------------------- BASELINE sizes
@pytest.mark.parametrize("n,k", [(4096, 4096), (11008, 4096), (4096, 11008)])
def test_full_size_properties(L, pkg, nso, n, k):
    """Llama-2-7B shapes (BASELINE.json config 2), size-independent properties instead of the (slow) CPU oracle:
       (a) GPU quantize -> GPU unpack == oracle dequant of the oracle-quantized SAMPLE columns (bit-exact);
       (b) GEMV == fp64 matmul against the device-unpacked weights (the reference's own 'vs unpacked W' check);
       (c) linearity in the activation."""
    import torch
    rng = np.random.default_rng(n + k)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    g = torch.Generator(device="cuda").manual_seed(1000 + n)
    dW = torch.randn((n, k), generator=g, device="cuda", dtype=torch.float32) * 0.02
    size = L.ns_BTLAGemmPackBSize(n, k, 32, pkg.S4, pkg.BF16, False, pkg.COMP_INT8, None)
    dBlob = torch.zeros(size, dtype=torch.uint8, device="cuda")
    pkg.check(L.ns_hip_quant_pack_device(dBlob.data_ptr(), dW.data_ptr(), n, k, k, 32, pkg.S4, pkg.BF16, False,
                                         pkg.COMP_INT8, True, st))
    torch.cuda.synchronize()
    blob = nso.aligned_bytes(size)
    blob[:] = dBlob.cpu().numpy()
    deq = np.zeros((k, n), np.float32)
    L.bestla_unpackweight_fp32(nso.ptr(blob), n, k, nso.ptr(deq), n)
    # (a) sample 48 columns, quantize them with the oracle
    cols = np.sort(rng.choice(n, 48, replace=False))
    wsub = dW[torch.from_numpy(cols).cuda()].cpu().numpy()
    sub = nso.unpack_fp32(nso.quant_pack(wsub, 32, nso.S4, nso.BF16, False, nso.CORE_AVX512_VNNI_KB))
    assert np.array_equal(sub.view(np.uint32), deq[:, cols].view(np.uint32))
    # (b), (c)
    a1 = rng.standard_normal((1, k)).astype(np.float32)
    a2 = rng.standard_normal((1, k)).astype(np.float32)
    outs = []
    for a in (a1, a2, a1 + a2):
        o = np.zeros((1, n), np.float32)
        L.bestla_f32f32_forward(nso.ptr(a), nso.ptr(blob), nso.ptr(o), 1, n, k, k, n, None)
        ref = a.astype(np.float64) @ deq.astype(np.float64)
        assert nso.rel_l2(o, ref) < TOL
        outs.append(o.astype(np.float64))
    assert nso.rel_l2(outs[0] + outs[1], outs[2]) < 2 * TOL


# ---------------------------------------------------------------------------------------------- TP shard producer
@pytest.mark.parametrize("qt,st,asym,bs", [("S4", "BF16", False, 32), ("S4", "F32", True, 128), ("S8", "BF16", False, 32),
                                           ("F4_NF4", "BF16", False, 64), ("S4", "BF16", False, -1)])
def test_weight_slice_tp_shards(L, pkg, nso, qt, st, asym, bs):
    """ns_hip_weight_slice (bestla_split_weight's job, model_files.h:1538-1563) — ROW split = N slices whose outputs
    concatenate, COLUMN split = K slices whose partial outputs sum (the all-reduce), both equal to the unsharded GEMM."""
    import torch
    rng = np.random.default_rng(31)
    n, k, m, ws = 256, 1024, 2, 4
    w = _w(rng, n, k)
    a = rng.standard_normal((m, k)).astype(np.float32)
    blob = nso.quant_pack(w, bs, getattr(nso, qt), getattr(nso, st), asym, nso.CORE_AVX512F)
    ref = nso.gemm_f64(a, blob)
    full = pkg.Weight.from_host_blob(nso.ptr(blob))
    st_ = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    dA = torch.from_numpy(a).cuda()
    # ROW split
    outs = []
    for r in range(ws):
        sh = full.slice(r * n // ws, (r + 1) * n // ws, 0, k, st_)
        assert (sh.n, sh.k) == (n // ws, k)
        dC = torch.empty((m, n // ws), dtype=torch.float32, device="cuda")
        pkg.check(L.ns_hip_f32f32_forward(dA.data_ptr(), sh.h, dC.data_ptr(), m, k, n // ws, 0, None, 0, st_))
        outs.append(dC)
    torch.cuda.synchronize()
    got = torch.cat(outs, dim=1).cpu().numpy()
    dF = torch.empty((m, n), dtype=torch.float32, device="cuda")
    pkg.check(L.ns_hip_f32f32_forward(dA.data_ptr(), full.h, dF.data_ptr(), m, k, n, 0, None, 0, st_))
    torch.cuda.synchronize()
    assert np.array_equal(got, dF.cpu().numpy())  # column tiles are independent: bit-identical to the unsharded launch
    assert nso.rel_l2(got, ref) < TOL
    # COLUMN split
    acc = torch.zeros((m, n), dtype=torch.float32, device="cuda")
    for r in range(ws):
        k0, k1 = r * k // ws, (r + 1) * k // ws
        sh = full.slice(0, n, k0, k1, st_)
        dAs = dA[:, k0:k1].contiguous()
        dC = torch.empty((m, n), dtype=torch.float32, device="cuda")
        pkg.check(L.ns_hip_f32f32_forward(dAs.data_ptr(), sh.h, dC.data_ptr(), m, k1 - k0, n, 0, None, 0, st_))
        acc += dC
    torch.cuda.synchronize()
    assert nso.rel_l2(acc.cpu().numpy(), ref) < TOL
    # misaligned requests are refused
    assert not L.ns_hip_weight_slice(full.h, 8, 64, 0, k, st_)
    assert not L.ns_hip_weight_slice(full.h, 0, n, 48, k, st_)


def test_fp16_shadow_variants_are_bit_identical(L, pkg, nso):
    """_h entry points: feeding the fp16 copy of A and asking for the fp16 copy of C must not change a single bit of C,
    and C16 must be the RNE rounding of C."""
    import torch
    rng = np.random.default_rng(77)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for (n, k, m) in [(256, 1024, 1), (96, 512, 3), (250, 1000, 1), (256, 4096, 1)]:
        blob = nso.quant_pack(_w(rng, n, k), 32, nso.S4, nso.BF16, False, nso.CORE_AVX512_VNNI_KB)
        wt = pkg.Weight.from_host_blob(nso.ptr(blob))
        a = torch.from_numpy(rng.standard_normal((m, k)).astype(np.float32)).cuda()
        lda = k
        a16 = a.to(torch.float16)
        c0 = torch.empty((m, n), dtype=torch.float32, device="cuda")
        c1 = torch.empty_like(c0)
        c16 = torch.empty((m, n), dtype=torch.float16, device="cuda")
        pkg.check(L.ns_hip_f32f32_forward(a.data_ptr(), wt.h, c0.data_ptr(), m, lda, n, 0, None, 0, st))
        a_dummy = torch.zeros_like(a) if k % 8 == 0 else a  # with a shadow the fp32 A must not be needed
        pkg.check(L.ns_hip_f32f32_forward_h(a_dummy.data_ptr(), a16.data_ptr() if k % 8 == 0 else None, wt.h, c1.data_ptr(),
                                            c16.data_ptr(), m, lda, n, 0, None, 0, st))
        torch.cuda.synchronize()
        assert torch.equal(c0, c1), (n, k, m)
        assert torch.equal(c16, c0.to(torch.float16))


def test_host_entry_points_from_several_threads(L, pkg, nso):
    """The reference drives this surface from one thread (n_tasks = 1); the drop-in shares staging buffers between calls,
    so concurrent callers must be serialised inside, not corrupt each other."""
    import threading
    rng = np.random.default_rng(21)
    n, k, bs = 128, 512, 32
    jobs = []
    for t in range(4):
        w = _w(rng, n, k)
        blob = nso.quant_pack(w, bs, nso.S4, nso.BF16, False, nso.CORE_AVX512_VNNI_KB)
        a = rng.standard_normal((3, k)).astype(np.float32)
        jobs.append((blob, a, nso.gemm_f64(a, blob)))
    errs = []

    def run(blob, a, ref):
        for _ in range(50):
            out = np.zeros((a.shape[0], n), np.float32)
            L.bestla_f32f32_forward(nso.ptr(a), nso.ptr(blob), nso.ptr(out), a.shape[0], n, k, k, n, None)
            e = nso.rel_l2(out, ref)
            if not e < TOL:
                errs.append(e)
                return

    threads = [threading.Thread(target=run, args=j) for j in jobs]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errs, errs


def test_device_silu_and_dup(L, pkg, nso):
    """the last two members of the reference's device-backend operator set (ne_bestla.h:103-109): SiLU and the 4-D strided
    fp32 -> fp32 / fp16 copy the graph uses for kv-cache writes and permutes"""
    import torch
    rng = np.random.default_rng(2)
    x = (rng.standard_normal(5000) * 4).astype(np.float32)
    dx = torch.from_numpy(x).cuda()
    dy = torch.zeros_like(dx)
    pkg.check(L.ns_hip_silu_f32(dx.data_ptr(), dy.data_ptr(), x.size, None))
    torch.cuda.synchronize()
    want = x.astype(np.float64) / (1 + np.exp(-x.astype(np.float64)))
    assert np.max(np.abs(dy.cpu().numpy() - want)) < 1e-6 * max(1.0, np.max(np.abs(want)))
    # permute [seq][head][dim] -> [head][dim][seq] while converting to fp16 (a V-cache style write)
    seq, heads, dim = 7, 3, 16
    src = rng.standard_normal((seq, heads, dim)).astype(np.float32)
    dsrc = torch.from_numpy(src).cuda()
    ddst = torch.zeros((heads, dim, seq + 2), dtype=torch.float16, device="cuda")   # padded rows stay untouched
    ne = (C.c_longlong * 4)(seq, dim, heads, 1)                        # dst extents, fastest first
    snb = (C.c_longlong * 4)(heads * dim * 4, 4, dim * 4, 0)           # src byte strides for (seq, dim, head)
    dnb = (C.c_longlong * 4)(2, (seq + 2) * 2, dim * (seq + 2) * 2, 0)
    pkg.check(L.ns_hip_dup_f32(dsrc.data_ptr(), ddst.data_ptr(), ne, snb, dnb, True, None))
    torch.cuda.synchronize()
    got = ddst.cpu().numpy()
    assert np.array_equal(got[:, :, :seq], src.transpose(1, 2, 0).astype(np.float16))
    assert np.all(got[:, :, seq:] == 0)
    # fp32 -> fp32 contiguous copy with a leading-dimension change
    d32 = torch.zeros((seq, heads * dim + 5), device="cuda")
    ne = (C.c_longlong * 4)(heads * dim, seq, 1, 1)
    snb = (C.c_longlong * 4)(4, heads * dim * 4, 0, 0)
    dnb = (C.c_longlong * 4)(4, (heads * dim + 5) * 4, 0, 0)
    pkg.check(L.ns_hip_dup_f32(dsrc.data_ptr(), d32.data_ptr(), ne, snb, dnb, False, None))
    torch.cuda.synchronize()
    assert np.array_equal(d32.cpu().numpy()[:, :heads * dim], src.reshape(seq, -1))

"""Calls of 17..64 rows: the first-generation weight-streaming kernel (ns_kernels.hip: smallm_kernel, MB = 2 for 17..32 rows,
MB = 4 for 33..64) and what forward_impl (ns_dispatch.cpp) sends elsewhere in this band — the tiled kernel from tiled_from_rows,
the first-generation gemm_kernel for fp8 weights once the staging-traffic rule (140e6 bytes) leaves the streaming kernel — through
every epilogue, the fp16 shadows in and out, dD with ldd = ldc / ldd > n / ldd = 0, the three-segment QKV grid, the unfused FFN
composition and the int8-reference mode's shared activation quantization.

Every output is one row taller and one column wider than the call (ldc = n + 1) and filled with a sentinel that must survive; every
comparison is made over the whole output AND row by row (the per-row form of tests/test_gpu_int8_mode.py), so that one wrong 16-row
block cannot hide behind the others.

Bars — none is new:
  1e-3   north_star, tests/test_gpu_parity.py TOL: against the oracle's fp64 GEMM (and its fp64 epilogue: the bar of
         test_epilogues_with_and_without_split_k in tests/test_gpu_gemvs.py)
  3e-5   TOL_A16_INT of tests/test_gpu_parity.py: integer and fp8 weights against the fp64 product of the fp16-rounded activations (only
         the fp32 summation order differs; ns_gemm_plan.cpp names it for the exact-scale fp8 kernels)
  6e-4   TOL_A16_F4, the same for f4 weights (the table is rounded to fp16)
  2e-3   a product of two rounded factors: tmp2 of the tiled gate/up launch (tests/test_gpu_gemm3.py) and the FFN end to end
         (test_fusion_ffn3: 2 * TOL)
  2e-6   the same products in another fp32 order: test_every_format_and_row_count_against_the_oracle (tests/test_gpu_gemvs.py) and the
         int8-reference mode against nso.gemm_u8s8 (tests/test_gpu_int8_mode.py)
  1e-5   tests/test_gpu_int8_mode.py: per row in int8-reference mode, and the fp64 activation of the oracle's int8 products
(5e-4, TOL_A16_GEMM, is the tiled kernel's bar against the fp16-activation product; nothing here needs it: the tiled side of the
gate/up tests is held to test_gpu_gemm3.py's 1e-3 / 2e-3.)

LDS the launcher asks for (launch_smallm: rows * (8 * kstep + 8) * 2 bytes, a chunk cannot shrink below nw = 8 k-steps):
  4-bit records (kstep 128): 63,984 B at 31 rows, 66,048 B at 32 rows, 132,096 B at 64 rows
  8-bit / fp8 records (kstep 64): 65,520 B at 63 rows, 66,560 B at 64 rows
Both crossings of 64 KiB are pinned in test_staging_chunks_and_the_64_kib_crossing; what the runtime did is in docs/kernels/smallm.md.

The print lines give the largest error each bar saw (run with -s)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = 1e-3
TOL_A16_INT = 3e-5
TOL_A16_F4 = 6e-4
TOL_MUL = 2e-3
TOL_ORDER = 2e-6
TOL_I8, TOL_I8_ROW, TOL_I8_ACT = 2e-6, 1e-5, 1e-5
SENT = -7.0
N = 263  # 17 tiles, the last one 7 columns wide

FMT = {  # qtype, scale dtype, group, asym, reference core the host blob is packed for (None: fp8, blob from the device quantizer)
    "s4_bf16_g32": ("S4", "BF16", 32, False, "CORE_AVX512_VNNI_KB"),
    "s4_f32_g32": ("S4", "F32", 32, False, "CORE_AVX512F"),
    "s4_asym_f32_g128": ("S4", "F32", 128, True, "CORE_AVX512F"),
    "s4_f32_per_channel": ("S4", "F32", -1, False, "CORE_AVX512F"),
    "s8_bf16_g32": ("S8", "BF16", 32, False, "CORE_AVX512F"),
    "s8_asym_f32_g64": ("S8", "F32", 64, True, "CORE_AVX512F"),
    "nf4_bf16_g128": ("F4_NF4", "BF16", 128, False, "CORE_AVX512F"),
    "s3_bf16_g32": ("S3", "BF16", 32, False, "CORE_AVX512_VNNI_KB"),
    "f8_e4m3_e8m0_g32": ("F8_E4M3", "F8_E8M0", 32, False, None),
    "f8_e5m2_f32_g32": ("F8_E5M2", "F32", 32, False, None),
    "f8_e4m3_f32_g32": ("F8_E4M3", "F32", 32, False, None),
    "s8_bf16_g64_int8core": ("S8", "BF16", 64, False, "CORE_AVX512_VNNI_KB"),
}
# K = 1088 = 8.5 k-steps of 128: a partial last k-step on the 4-bit records whose group divides it; 1024 elsewhere
K_OF = {"s4_bf16_g32": 1088, "s4_f32_per_channel": 1088, "s3_bf16_g32": 1088}


def _k_of(fmt):
    return K_OF.get(fmt, 1024)


def _tol16(fmt):
    return TOL_A16_F4 if fmt.startswith("nf4") else TOL_A16_INT


def _st():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _gelu(v):
    return 0.5 * v * (1.0 + np.tanh(0.7978845834732056 * (v + 0.044714998453855515 * v ** 3)))


def _silu(v):
    return v * (0.5 + 0.5 * np.tanh(0.5 * v))   # v / (1 + exp(-v)) without the overflow of exp at large -v


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32 if x.dtype == np.float32 else np.uint16)


def _row_err(out, ref):
    out, ref = np.asarray(out, np.float64), np.asarray(ref, np.float64)
    return np.sqrt(((out - ref) ** 2).sum(-1) / np.maximum((ref ** 2).sum(-1), 1e-30))


_SEEN = {}


def _close(nso, out, ref, tol, what, row_tol=None):
    """whole output and every row of it within tol (row_tol where the source of the bar has a per-row bar of its own)"""
    e, rows = nso.rel_l2(out, ref), _row_err(out, ref)
    worst = max(e, float(rows.max()))
    _SEEN[tol] = max(_SEEN.get(tol, 0.0), e)
    _SEEN[row_tol or tol, "row"] = max(_SEEN.get((row_tol or tol, "row"), 0.0), float(rows.max()))
    assert e < tol, (what, "rel_l2", e)
    assert rows.max() < (row_tol or tol), (what, "row", int(rows.argmax()), float(rows.max()))
    return worst


class _Bank:
    """weights, activations and fp64 references of the module, each made once and never changed"""

    def __init__(self, L, pkg, nso):
        self.L, self.pkg, self.nso = L, pkg, nso
        self.w, self.a, self.r, self.keep = {}, {}, {}, []

    def weight(self, fmt, n, k, seed=0, wscale=0.02):
        import torch
        key = (fmt, n, k, seed, wscale)
        if key not in self.w:
            L, pkg, nso = self.L, self.pkg, self.nso
            qt, sdt, bs, asym, core = FMT[fmt]
            if core is None:  # fp8: the device quantizer (bit-exact with the oracle's packer, which takes minutes at these sizes)
                g = torch.Generator(device="cuda").manual_seed(seed * 7919 + n + k)
                dW = torch.randn((n, k), generator=g, device="cuda") * wscale
                size = L.ns_BTLAGemmPackBSize(n, k, bs, getattr(pkg, qt), getattr(pkg, sdt), asym, pkg.COMP_F32, None)
                assert size > 0, pkg.last_error()
                dBlob = torch.zeros(size, dtype=torch.uint8, device="cuda")
                pkg.check(L.ns_hip_quant_pack_device(dBlob.data_ptr(), dW.data_ptr(), n, k, k, bs, getattr(pkg, qt), getattr(pkg, sdt), asym,
                                                     pkg.COMP_F32, True, _st()))
                torch.cuda.synchronize()
                blob = nso.aligned_bytes(size)
                blob[:] = dBlob.cpu().numpy()
                wt = pkg.Weight.from_device_blob(dBlob.data_ptr(), size, _st())
                torch.cuda.synchronize()
                self.keep.append(dBlob)
            else:
                rng = np.random.default_rng(seed * 7919 + n * 3 + k)
                w = (rng.standard_normal((n, k)) * wscale).astype(np.float32)
                blob = nso.quant_pack(w, bs, getattr(nso, qt), getattr(nso, sdt), asym, getattr(nso, core))
                wt = pkg.Weight.from_host_blob(nso.ptr(blob), _st())
                torch.cuda.synchronize()
            self.w[key] = (blob, wt)
        return self.w[key]

    def acts(self, k, seed=0):
        """64 rows of activations; a call of m rows takes the first m (GEMM rows are independent, so one reference serves every m)"""
        if (k, seed) not in self.a:
            self.a[(k, seed)] = np.random.default_rng(1000 + k + seed).standard_normal((64, k)).astype(np.float32)
        return self.a[(k, seed)]

    def refs(self, fmt, n, k, seed=0, wscale=0.02, aseed=0):
        key = (fmt, n, k, seed, wscale, aseed)
        if key not in self.r:
            self.r[key] = self.nso.gemm_f64_pair(self.acts(k, aseed), self.weight(fmt, n, k, seed, wscale)[0])
        return self.r[key]

    def close(self):
        for _blob, wt in self.w.values():
            wt.free()
        self.L.ns_hip_cache_clear()


@pytest.fixture(scope="module")
def bank(L, pkg, nso):
    b = _Bank(L, pkg, nso)
    yield b
    b.close()
    print("rows17_64 largest error seen per bar:", {str(k): "%.3g" % v for k, v in sorted(_SEEN.items(), key=str)})


def _fwd(L, pkg, wt, dA, m, n, lda, a16=None, want16=False, epi=0, dD=None, ldd=0):
    """ns_hip_f32f32_forward_h into a sentinel-filled (m + 1) x (n + 1) output; must return 0 and leave row m and column n alone"""
    import torch
    ldc = n + 1
    dC = torch.full((m + 1, ldc), SENT, dtype=torch.float32, device="cuda")
    dC16 = torch.full((m + 1, ldc), SENT, dtype=torch.float16, device="cuda") if want16 else None
    rc = L.ns_hip_f32f32_forward_h(dA.data_ptr(), a16.data_ptr() if a16 is not None else None, wt.h, dC.data_ptr(),
                                   dC16.data_ptr() if want16 else None, m, lda, ldc, epi, dD.data_ptr() if dD is not None else None, ldd, _st())
    assert rc == 0, pkg.last_error()
    torch.cuda.synchronize()
    c = dC.cpu().numpy()
    assert (c[:, n] == SENT).all() and (c[m] == SENT).all(), "fp32 output: written outside m x n"
    if not want16:
        return np.ascontiguousarray(c[:m, :n]), None
    c16 = dC16.cpu().numpy()
    assert (c16[:, n] == np.float16(SENT)).all() and (c16[m] == np.float16(SENT)).all(), "fp16 shadow: written outside m x n"
    return np.ascontiguousarray(c[:m, :n]), np.ascontiguousarray(c16[:m, :n])


def _three_forms(L, pkg, nso, wt, a, m, n, k, ref, ref16, tol16, what):
    """no shadow / dA16 in / dA16 in + dC16 out: one C bit for bit (the kernel rounds A to fp16 itself), dC16 = RNE(C), bars of A"""
    import torch
    dA = torch.from_numpy(np.ascontiguousarray(a[:m])).cuda()
    dA16 = dA.half()
    c0, _ = _fwd(L, pkg, wt, dA, m, n, k)
    c1, _ = _fwd(L, pkg, wt, dA, m, n, k, a16=dA16)
    c2, c216 = _fwd(L, pkg, wt, dA, m, n, k, a16=dA16, want16=True)
    assert np.array_equal(_bits(c0), _bits(c1)), (what, "dA16 in changed C", int((_bits(c0) != _bits(c1)).sum()))
    assert np.array_equal(_bits(c0), _bits(c2)), (what, "dC16 out changed C", int((_bits(c0) != _bits(c2)).sum()))
    assert np.array_equal(_bits(c216), _bits(c2.astype(np.float16))), (what, "dC16 != RNE(C)")
    e = _close(nso, c0, ref[:m], TOL, what)
    e16 = _close(nso, c0, ref16[:m], tol16, what + " a16")
    print("rows17_64", what, "rel_l2 %.3g  a16 %.3g" % (e, e16))
    return c0


# ------------------------------------------------------------------------------------------------ A: every format, plain forward
A_FORMATS = ["s4_bf16_g32", "s4_asym_f32_g128", "s4_f32_per_channel", "s8_bf16_g32", "s8_asym_f32_g64", "nf4_bf16_g128", "s3_bf16_g32",
             "f8_e4m3_e8m0_g32", "f8_e5m2_f32_g32"]


@pytest.mark.parametrize("m", [17, 32, 33, 64])
@pytest.mark.parametrize("fmt", A_FORMATS)
def test_every_format_three_shadow_forms(L, pkg, nso, bank, fmt, m):
    """ns_hip_f32f32_forward_h on 263 columns (last tile 7 wide), K = 1024 / 1088, at both ends of MB = 2 (17, 32) and MB = 4 (33, 64)"""
    k = _k_of(fmt)
    _blob, wt = bank.weight(fmt, N, k)
    ref, ref16 = bank.refs(fmt, N, k)
    _three_forms(L, pkg, nso, wt, bank.acts(k), m, N, k, ref, ref16, _tol16(fmt), "A %s m=%d" % (fmt, m))


@pytest.mark.parametrize("m", [31, 40])
def test_a_shadow_that_cannot_be_used_falls_back_to_the_fp32_activations(L, pkg, nso, bank, m):
    """lda = K + 4: the fp16 shadow's rows are not 16-byte units, the kernel stages the fp32 activations instead — the same bits as the
    dense call, with and without the shadow"""
    import torch
    fmt = "s4_bf16_g32"
    k = _k_of(fmt)
    _blob, wt = bank.weight(fmt, N, k)
    a = bank.acts(k)[:m]
    dense, _ = _fwd(L, pkg, wt, torch.from_numpy(np.ascontiguousarray(a)).cuda(), m, N, k)
    wide = torch.full((m, k + 4), 1e4, dtype=torch.float32, device="cuda")   # (padding that would show in any sum)
    wide[:, :k] = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    c0, _ = _fwd(L, pkg, wt, wide, m, N, k + 4)
    c1, c116 = _fwd(L, pkg, wt, wide, m, N, k + 4, a16=wide.half(), want16=True)
    assert np.array_equal(_bits(c0), _bits(dense)) and np.array_equal(_bits(c1), _bits(dense))
    assert np.array_equal(_bits(c116), _bits(c1.astype(np.float16)))
    _close(nso, c1, bank.refs(fmt, N, k)[1][:m], TOL_A16_INT, "A lda=K+4 m=%d" % m)


# ------------------------------------------------------------------------------------------------ B: every epilogue, both MB
@pytest.mark.parametrize("m", [31, 47])
@pytest.mark.parametrize("fmt", ["s4_bf16_g32", "s8_asym_f32_g64", "f8_e4m3_e8m0_g32"])
def test_every_epilogue_and_every_d_stride(L, pkg, nso, bank, fmt, m):
    """NONE, ADD, MUL, ADD_GELU, GELU, SILU with dD at ldd = ldc, ldd = n + 5 and ldd = 0 (one bias row, what the host FFN entries pass),
    against the fp64 epilogue of the oracle's product.  ADD and MUL are ONE fp32 operation on the deterministic reduction's result, so
    they equal numpy's float32 add / multiply of the same call's NONE output bit for bit.  dC16 is asked for in every call."""
    import torch
    k = _k_of(fmt)
    _blob, wt = bank.weight(fmt, N, k)
    x = bank.refs(fmt, N, k)[0][:m]
    dA = torch.from_numpy(np.ascontiguousarray(bank.acts(k)[:m])).cuda()
    dA16 = dA.half()

    def run(epi, dD=None, ldd=0):
        c, c16 = _fwd(L, pkg, wt, dA, m, N, k, a16=dA16, want16=True, epi=epi, dD=dD, ldd=ldd)
        assert np.array_equal(_bits(c16), _bits(c.astype(np.float16))), (fmt, m, epi, ldd, "dC16 != RNE(C)")
        return c
    none = run(pkg.EPI_NONE)
    worst = _close(nso, none, x, TOL, "B none")
    worst = max(worst, _close(nso, run(pkg.EPI_GELU), _gelu(x), TOL, "B gelu"), _close(nso, run(pkg.EPI_SILU), _silu(x), TOL, "B silu"))
    g = torch.Generator(device="cuda").manual_seed(m)
    for ldd in (N + 1, N + 5, 0):
        dD = torch.randn((1 if ldd == 0 else m, max(ldd, N)), generator=g, device="cuda")
        d = np.ascontiguousarray(dD.cpu().numpy()[:, :N])   # (m, n), or (1, n) broadcast over the rows
        d64 = d.astype(np.float64)
        add, mul, addgelu = run(pkg.EPI_ADD, dD, ldd), run(pkg.EPI_MUL, dD, ldd), run(pkg.EPI_ADD_GELU, dD, ldd)
        worst = max(worst, _close(nso, add, x + d64, TOL, "B add ldd=%d" % ldd), _close(nso, mul, x * d64, TOL, "B mul ldd=%d" % ldd),
                    _close(nso, addgelu, _gelu(x + d64), TOL, "B add_gelu ldd=%d" % ldd))
        assert np.array_equal(_bits(add), _bits((none + d).astype(np.float32))), (fmt, m, ldd, "ADD is not one fp32 add of the NONE output")
        assert np.array_equal(_bits(mul), _bits((none * d).astype(np.float32))), (fmt, m, ldd, "MUL is not one fp32 multiply of the NONE output")
    print("rows17_64 B", fmt, m, "worst rel_l2 (whole or row) %.3g" % worst)


# ------------------------------------------------------------------------------------------------ C: against the decode kernels
@pytest.mark.parametrize("fmt", ["s4_bf16_g32", "nf4_bf16_g128"])
def test_rows_of_a_40_row_call_against_16_row_calls(L, pkg, nso, bank, fmt):
    """rows 0..15 and 24..39 of a 40-row call (MB = 4, the third 16-row block partial) against the same rows sent as 16-row calls, which
    gemvs_kernel serves: the same products in another fp32 order"""
    import torch
    m, k = 40, 2048
    _blob, wt = bank.weight(fmt, N, k)
    dA = torch.from_numpy(np.ascontiguousarray(bank.acts(k)[:m])).cuda()
    dA16 = dA.half()
    full, _ = _fwd(L, pkg, wt, dA, m, N, k, a16=dA16)
    assert L.ns_hip_set_tuning(b"gvs", 3) == 0   # pin gemvs_kernel, as tests/test_gpu_gemvs.py does
    try:
        for r0 in (0, 24):
            part, _ = _fwd(L, pkg, wt, dA[r0:r0 + 16], 16, N, k, a16=dA16[r0:r0 + 16])
            rows = _row_err(full[r0:r0 + 16], part)
            print("rows17_64 C", fmt, "rows %d..%d worst row %.3g" % (r0, r0 + 15, rows.max()))
            assert rows.max() < TOL_ORDER, (fmt, r0, int(rows.argmax()), float(rows.max()))
    finally:
        L.ns_hip_set_tuning(b"gvs", 1)
    ref, ref16 = bank.refs(fmt, N, k)
    _close(nso, full, ref[:m], TOL, "C full")
    _close(nso, full, ref16[:m], _tol16(fmt), "C full a16")


# ------------------------------------------------------------------------------------------------ D: staging chunks, 64 KiB
@pytest.mark.parametrize("m", [31, 32, 63, 64])
@pytest.mark.parametrize("fmt,k", [("s4_bf16_g32", 4096), ("s8_bf16_g32", 4096), ("s4_bf16_g32", 128), ("s8_bf16_g32", 16384)])
def test_staging_chunks_and_the_64_kib_crossing(L, pkg, nso, bank, fmt, k, m):
    """K = 4096: the activations are staged in chunks of 8 k-steps (S4: 4 chunks, S8: 8 chunks at 64 rows), a barrier between them;
    K = 128: ONE k-step padded out to a chunk of 8; K = 16384 on S8: 32 chunks, so 31 chunk boundaries in each of the 17 workgroups of
    every call (a missing barrier there is a race, which no single pass is certain to lose).  The launcher asks for rows * (8 * kstep + 8) * 2 bytes of LDS —
    4-bit: 63,984 B at 31 rows, 66,048 B at 32, 132,096 B at 64; 8-bit: 65,520 B at 63 rows, 66,560 B at 64 — by a plain launch, so
    32 rows (4-bit) and 64 rows (8-bit) are the first above 64 KiB: every call must return 0 and meet the bars of A"""
    _blob, wt = bank.weight(fmt, N, k)
    ref, ref16 = bank.refs(fmt, N, k)
    _three_forms(L, pkg, nso, wt, bank.acts(k), m, N, k, ref, ref16, _tol16(fmt), "D %s K=%d m=%d" % (fmt, k, m))


# ------------------------------------------------------------------------------------------------ E: fused QKV
QKV_NS = (1000, 200, 136)


@pytest.mark.parametrize("m", [17, 40, 64])
@pytest.mark.parametrize("fmt", ["s4_bf16_g32", "s8_bf16_g32"])
def test_fused_qkv_device_entry(L, pkg, nso, bank, fmt, m):
    """ns_hip_fusion_qkv_forward_h, widths 1000 / 200 / 136 (two of them end inside a tile): three segments in one grid of smallm_kernel.
    Each block against its oracle product, bit-identical to the single forward of that weight (the same kernel, 8 waves, the same
    order), each shadow = RNE(block), nothing past a block's own columns; with and without dA16 / dC16"""
    import torch
    k = _k_of(fmt)
    ws = [bank.weight(fmt, n, k, seed=i + 1) for i, n in enumerate(QKV_NS)]
    dA = torch.from_numpy(np.ascontiguousarray(bank.acts(k)[:m])).cuda()
    dA16 = dA.half()
    ldc = max(QKV_NS) + 1
    outs = []
    for shadow in (False, True):
        out = torch.full((3 * m + 1, ldc), SENT, device="cuda")
        out16 = torch.full((3 * m + 1, ldc), SENT, device="cuda", dtype=torch.float16)
        rc = L.ns_hip_fusion_qkv_forward_h(dA.data_ptr(), dA16.data_ptr() if shadow else None, ws[0][1].h, ws[1][1].h, ws[2][1].h, out.data_ptr(),
                                           out16.data_ptr() if shadow else None, m, k, ldc, _st())
        assert rc == 0, pkg.last_error()
        torch.cuda.synchronize()
        f, f16 = out.cpu().numpy(), out16.cpu().numpy()
        assert (f[3 * m] == SENT).all() and (f16[3 * m] == np.float16(SENT)).all()
        if not shadow:
            assert (f16 == np.float16(SENT)).all()
        for i, n in enumerate(QKV_NS):
            blk, blk16 = f[i * m:(i + 1) * m], f16[i * m:(i + 1) * m]
            assert (blk[:, n:] == SENT).all() and (blk16[:, n:] == np.float16(SENT)).all(), (i, n, "written past the block's columns")
            if shadow:
                assert np.array_equal(_bits(blk16[:, :n]), _bits(blk[:, :n].astype(np.float16))), (i, "shadow != RNE(block)")
        outs.append(f)
    assert np.array_equal(_bits(outs[0]), _bits(outs[1])), "the shadows changed C"
    for i, n in enumerate(QKV_NS):
        blk = np.ascontiguousarray(outs[1][i * m:(i + 1) * m, :n])
        ref, ref16 = bank.refs(fmt, n, k, seed=i + 1)
        e = _close(nso, blk, ref[:m], TOL, "E block %d" % i)
        e16 = _close(nso, blk, ref16[:m], TOL_A16_INT, "E block %d a16" % i)
        single, _ = _fwd(L, pkg, ws[i][1], dA, m, n, k, a16=dA16)
        assert np.array_equal(_bits(blk), _bits(single)), (fmt, m, i, "segment differs from the single forward", int((_bits(blk) != _bits(single)).sum()))
        print("rows17_64 E device", fmt, m, "block", i, "rel_l2 %.3g  a16 %.3g" % (e, e16))


@pytest.mark.parametrize("m", [17, 40, 64])
@pytest.mark.parametrize("fmt", ["s4_bf16_g32", "s8_bf16_g32"])
def test_fused_qkv_host_entry(L, pkg, nso, bank, fmt, m):
    """bestla_fusion_QKV_f32f32_forward (one n for the three weights: 520, the last tile 8 wide) into ldo = n + 1"""
    k, n = _k_of(fmt), 520
    blobs = [bank.weight(fmt, n, k, seed=i + 11)[0] for i in range(3)]
    a = np.ascontiguousarray(bank.acts(k)[:m])
    assert L.bestla_fusion_QKV_f32f32_support(*[nso.ptr(b) for b in blobs], m, n, k)
    out = np.full((3 * m + 1, n + 1), SENT, np.float32)
    L.bestla_fusion_QKV_f32f32_forward(nso.ptr(a), *[nso.ptr(b) for b in blobs], nso.ptr(out), m, n, k, k, n + 1, None)
    assert (out[:, n] == SENT).all() and (out[3 * m] == SENT).all()
    for i in range(3):
        blk = np.ascontiguousarray(out[i * m:(i + 1) * m, :n])
        ref, ref16 = bank.refs(fmt, n, k, seed=i + 11)
        e = _close(nso, blk, ref[:m], TOL, "E host block %d" % i)
        e16 = _close(nso, blk, ref16[:m], TOL_A16_INT, "E host block %d a16" % i)
        single = np.full((m + 1, n + 1), SENT, np.float32)
        L.bestla_f32f32_forward(nso.ptr(a), nso.ptr(blobs[i]), nso.ptr(single), m, n, k, k, n + 1, None)
        assert (single[:, n] == SENT).all() and (single[m] == SENT).all()
        assert np.array_equal(_bits(blk), _bits(np.ascontiguousarray(single[:m, :n]))), (fmt, m, i, "segment differs from the single forward")
        print("rows17_64 E host", fmt, m, "block", i, "rel_l2 %.3g  a16 %.3g" % (e, e16))


# ------------------------------------------------------------------------------------------------ F: FFN entries
FIN, FMID, FOUT = 256, 360, 256   # narrow weights: the unfused composition on smallm_kernel (fmid = 22.5 tiles, K of the down projection 2.8 k-steps)
FFN_SCALE = 0.06


def _ffn_blobs(bank, three):
    b1 = bank.weight("s4_bf16_g32", FMID, FIN, seed=21, wscale=FFN_SCALE)
    b2 = bank.weight("s4_bf16_g32", FOUT, FMID, seed=22, wscale=FFN_SCALE)
    b3 = bank.weight("s4_bf16_g32", FMID, FIN, seed=23, wscale=FFN_SCALE) if three else None
    return b1, b2, b3


def _check_ffn3(nso, a, b1, b2, b3, act, t1, t2, out, what):
    """as test_fusion_ffn3 (tests/test_gpu_parity.py): tmp1, tmp2, the last GEMM against the oracle fed the device's own tmp2, end to end"""
    r1 = act(nso.gemm_f64(a, b1))
    r2 = nso.gemm_f64(a, b3) * r1
    es = (_close(nso, t1, r1, TOL, what + " tmp1"), _close(nso, t2, r2, TOL, what + " tmp2"),
          _close(nso, out, nso.gemm_f64(t2, b2), TOL, what + " down"),
          _close(nso, out, nso.gemm_f64(r2.astype(np.float32), b2), TOL_MUL, what + " end to end"))
    print("rows17_64 F", what, "tmp1 %.3g tmp2 %.3g down %.3g end-to-end %.3g" % es)


@pytest.mark.parametrize("m", [17, 33, 64])
@pytest.mark.parametrize("name", ["SiLu", "Gelu_Mul"])
def test_ffn3_host_entries(L, pkg, nso, bank, name, m):
    """bestla_fusion_FFN_{SiLu,Gelu_Mul}_f32f32_forward: act and MUL epilogues of smallm_kernel, then the down projection"""
    (b1, _w1), (b2, _w2), (b3, _w3) = _ffn_blobs(bank, True)
    a = np.ascontiguousarray(bank.acts(FIN)[:m])
    assert getattr(L, "bestla_fusion_FFN_%s_f32f32_support" % name)(nso.ptr(b1), nso.ptr(b2), nso.ptr(b3), m, FIN, FMID, FOUT)
    t1, t2, out = (np.full((m, w), SENT, np.float32) for w in (FMID, FMID, FOUT))
    getattr(L, "bestla_fusion_FFN_%s_f32f32_forward" % name)(nso.ptr(a), nso.ptr(b1), nso.ptr(b2), nso.ptr(b3), nso.ptr(t1), nso.ptr(t2),
                                                             nso.ptr(out), m, FIN, FMID, FOUT, None)
    _check_ffn3(nso, a, b1, b2, b3, _silu if name == "SiLu" else _gelu, t1, t2, out, "host %s m=%d" % (name, m))


@pytest.mark.parametrize("m", [17, 33, 64])
def test_ffn2_host_entries(L, pkg, nso, bank, m):
    """bestla_fusion_FFN_GeLu / _Add_GeLu (one bias row, ldd = 0, and a full bias): GELU, ADD_GELU and ADD epilogues"""
    (b1, _w1), (b2, _w2), _ = _ffn_blobs(bank, False)
    a = np.ascontiguousarray(bank.acts(FIN)[:m])
    rng = np.random.default_rng(m)
    assert L.bestla_fusion_FFN_GeLu_f32f32_support(nso.ptr(b1), nso.ptr(b2), m, FIN, FMID, FOUT)
    t1, out = np.full((m, FMID), SENT, np.float32), np.full((m, FOUT), SENT, np.float32)
    L.bestla_fusion_FFN_GeLu_f32f32_forward(nso.ptr(a), nso.ptr(b1), nso.ptr(b2), nso.ptr(t1), nso.ptr(out), m, FIN, FMID, FOUT, None)
    x1 = nso.gemm_f64(a, b1)
    es = [_close(nso, t1, _gelu(x1), TOL, "ffn2 tmp1"), _close(nso, out, nso.gemm_f64(t1, b2), TOL, "ffn2 out")]
    assert L.bestla_fusion_FFN_Add_GeLu_f32f32_support(nso.ptr(b1), nso.ptr(b2), m, FIN, FMID, FOUT)
    for bcast in (True, False):
        bias1 = rng.standard_normal((1 if bcast else m, FMID)).astype(np.float32)
        bias2 = rng.standard_normal((1 if bcast else m, FOUT)).astype(np.float32)
        t1[:], out[:] = SENT, SENT
        L.bestla_fusion_FFN_Add_GeLu_f32f32_forward(nso.ptr(a), nso.ptr(b1), nso.ptr(b2), nso.ptr(bias1), nso.ptr(bias2), nso.ptr(t1), nso.ptr(out),
                                                    m, FIN, FMID, FOUT, bcast, None)
        es += [_close(nso, t1, _gelu(x1 + bias1), TOL, "ffn2 add_gelu tmp1 bcast=%d" % bcast),
               _close(nso, out, nso.gemm_f64(t1, b2) + bias2, TOL, "ffn2 add out bcast=%d" % bcast)]
    print("rows17_64 F ffn2 m=%d" % m, " ".join("%.3g" % e for e in es))


@pytest.mark.parametrize("m", [17, 33, 64])
@pytest.mark.parametrize("act", ["silu", "gelu"])
def test_ffn3_device_entry_with_and_without_temporaries(L, pkg, nso, bank, act, m):
    """ns_hip_fusion_ffn3_forward_h: with tmp1 / tmp2 / tmp2's shadow / out's shadow handed over, and with none of them (fmid = 360 is no
    multiple of 64, so the intermediate lives in fp32 scratch and the down projection rounds it itself): the same bits out"""
    import torch
    (b1, w1), (b2, w2), (b3, w3) = _ffn_blobs(bank, True)
    a = np.ascontiguousarray(bank.acts(FIN)[:m])
    dA = torch.from_numpy(a).cuda()
    dA16 = dA.half()
    code = pkg.EPI_SILU if act == "silu" else pkg.EPI_GELU
    t1, t2 = torch.full((m + 1, FMID), SENT, device="cuda"), torch.full((m + 1, FMID), SENT, device="cuda")
    t216 = torch.full((m + 1, FMID), SENT, device="cuda", dtype=torch.float16)
    out, out_b = torch.full((m + 1, FOUT), SENT, device="cuda"), torch.full((m + 1, FOUT), SENT, device="cuda")
    out16 = torch.full((m + 1, FOUT), SENT, device="cuda", dtype=torch.float16)
    pkg.check(L.ns_hip_fusion_ffn3_forward_h(dA.data_ptr(), dA16.data_ptr(), w1.h, w2.h, w3.h, t1.data_ptr(), t2.data_ptr(), t216.data_ptr(),
                                             out.data_ptr(), out16.data_ptr(), m, code, _st()))
    pkg.check(L.ns_hip_fusion_ffn3_forward_h(dA.data_ptr(), None, w1.h, w2.h, w3.h, None, None, None, out_b.data_ptr(), None, m, code, _st()))
    torch.cuda.synchronize()
    for t in (t1, t2, t216, out, out16, out_b):
        assert (t[m] == SENT).all()
    assert torch.equal(out, out_b), "the temporaries / shadows changed the output"
    assert torch.equal(t216[:m], t2[:m].half()) and torch.equal(out16[:m], out[:m].half())
    _check_ffn3(nso, a, b1, b2, b3, _silu if act == "silu" else _gelu, t1[:m].cpu().numpy(), t2[:m].cpu().numpy(), out[:m].cpu().numpy(),
                "device %s m=%d" % (act, m))


@pytest.mark.parametrize("fmt,n,k,m_stream,m_tiled", [("s4_f32_g32", 4096, 256, 32, 33), ("s4_bf16_g32", 8192, 128, 16, 17)])
def test_gate_up_on_both_sides_of_tiled_from_rows(L, pkg, nso, bank, fmt, n, k, m_stream, m_tiled):
    """ns_hip_fusion_ffn3_gateup_h around tiled_from_rows (ns_dispatch.cpp): 256 tiles, K < 8192 -> the tiled kernel's gate / up tile
    pairs from 33 rows, the streaming composition (act epilogue, then MUL epilogue) at 32; 512 tiles -> tile pairs from 17, the fused
    streaming launch at 16.  Streaming side: 1e-3 for tmp1 and tmp2 (test_fused_gate_up); tiled side: 1e-3 / 2e-3
    (tests/test_gpu_gemm3.py); the rows both calls share agree within 2e-3.  (A 4-bit code times a bf16 scale is exact in fp16, so with
    bf16 scales the two kernels differ by summation order only; with fp32 scales the tiled kernel's rounding of the scaled weight shows)"""
    import torch
    (b1, w1), (b3, w3) = bank.weight(fmt, n, k, seed=31, wscale=0.05), bank.weight(fmt, n, k, seed=33, wscale=0.05)
    a = bank.acts(k)
    g, u = nso.gemm_f64(a[:m_tiled], b1), nso.gemm_f64(a[:m_tiled], b3)
    r1 = _silu(g)
    r2 = r1 * u
    got = {}
    for m, tol2 in ((m_stream, TOL), (m_tiled, TOL_MUL)):
        dA = torch.from_numpy(np.ascontiguousarray(a[:m])).cuda()
        dA16 = dA.half()
        t1, t2 = torch.full((m + 1, n), SENT, device="cuda"), torch.full((m + 1, n), SENT, device="cuda")
        t216 = torch.full((m + 1, n), SENT, device="cuda", dtype=torch.float16)
        pkg.check(L.ns_hip_fusion_ffn3_gateup_h(dA.data_ptr(), dA16.data_ptr(), w1.h, w3.h, t1.data_ptr(), t2.data_ptr(), t216.data_ptr(), m,
                                                pkg.EPI_SILU, _st()))
        torch.cuda.synchronize()
        assert (t1[m] == SENT).all() and (t2[m] == SENT).all() and (t216[m] == SENT).all()
        assert torch.equal(t216[:m], t2[:m].half())
        e1 = _close(nso, t1[:m].cpu().numpy(), r1[:m], TOL, "gate/up %dx%d m=%d tmp1" % (n, k, m))
        e2 = _close(nso, t2[:m].cpu().numpy(), r2[:m], tol2, "gate/up %dx%d m=%d tmp2" % (n, k, m))
        print("rows17_64 F gate/up", (n, k, m), "tmp1 %.3g tmp2 %.3g" % (e1, e2))
        got[m] = t2[:m].cpu().numpy()
    e = _close(nso, got[m_tiled][:m_stream], got[m_stream], TOL_MUL, "gate/up %dx%d streaming vs tiled" % (n, k))
    print("rows17_64 F gate/up", (n, k), "streaming vs tiled %.3g" % e)


# ------------------------------------------------------------------------------------------------ G: dispatch edges
def test_conversion_pass_gives_the_callers_own_shadow_bits(L, pkg, nso, bank):
    """S4 4096 x 2048 at 32 rows, fp32 activations only, lda == K: 256 tiles x 32 x 2048 x 4 = 67e6 bytes of staging — forward_impl
    converts A to fp16 once and stays on the streaming kernel.  The same bits as with the caller's own dA16 (33e6, no pass) and as with
    lda = K + 8 (no pass: the kernel converts while staging)"""
    import torch
    fmt, n, k, m = "s4_bf16_g32", 4096, 2048, 32
    _blob, wt = bank.weight(fmt, n, k, seed=41)
    a = np.ascontiguousarray(bank.acts(k)[:m])
    dA = torch.from_numpy(a).cuda()
    c_pass, _ = _fwd(L, pkg, wt, dA, m, n, k)
    c_own, _ = _fwd(L, pkg, wt, dA, m, n, k, a16=dA.half())
    wide = torch.full((m, k + 8), 1e4, dtype=torch.float32, device="cuda")
    wide[:, :k] = dA
    c_wide, _ = _fwd(L, pkg, wt, wide, m, n, k + 8)
    assert np.array_equal(_bits(c_pass), _bits(c_own)), "the conversion pass changed C"
    assert np.array_equal(_bits(c_wide), _bits(c_own)), "staging from fp32 changed C"
    ref, ref16 = bank.refs(fmt, n, k, seed=41)
    e, e16 = _close(nso, c_pass, ref[:m], TOL, "G conversion pass"), _close(nso, c_pass, ref16[:m], TOL_A16_INT, "G conversion pass a16")
    print("rows17_64 G conversion pass rel_l2 %.3g  a16 %.3g" % (e, e16))


F8_WIDE = ("f8_e4m3_f32_g32", 8192, 1152)  # 512 tiles: 64 rows of fp32 activations are 151e6 bytes of staging, 48 rows 113e6


def test_fp8_wide_at_48_rows_stays_on_the_streaming_kernel(L, pkg, nso, bank):
    fmt, n, k = F8_WIDE
    _blob, wt = bank.weight(fmt, n, k, seed=51)
    ref, ref16 = bank.refs(fmt, n, k, seed=51)
    _three_forms(L, pkg, nso, wt, bank.acts(k), 48, n, k, ref, ref16, TOL_A16_INT, "G fp8 8192x1152 m=48")


def test_fp8_wide_at_64_rows_runs_on_the_first_generation_gemm_kernel(L, pkg, nso, bank):
    """fp32 activations only: 151e6 > 140e6, launch_gemm2 refuses a plain fp8 call of up to 64 rows, gemm_kernel<WK_F8> serves it —
    EPI_NONE, EPI_ADD with one bias row (ldd = 0), and (what launch_gemm used to refuse with hipErrorInvalidValue) the fp16 shadow of
    the output: the call returns 0, C does not depend on the shadow pointer, dC16 = RNE(C)"""
    import torch
    fmt, n, k = F8_WIDE
    m = 64
    _blob, wt = bank.weight(fmt, n, k, seed=51)
    ref, ref16 = bank.refs(fmt, n, k, seed=51)
    dA = torch.from_numpy(bank.acts(k)).cuda()
    c, _ = _fwd(L, pkg, wt, dA, m, n, k)
    e, e16 = _close(nso, c, ref, TOL, "G fp8 gemm_kernel"), _close(nso, c, ref16, TOL_A16_INT, "G fp8 gemm_kernel a16")
    bias = torch.randn((1, n), generator=torch.Generator(device="cuda").manual_seed(3), device="cuda")
    b = bias.cpu().numpy()
    cb, _ = _fwd(L, pkg, wt, dA, m, n, k, epi=pkg.EPI_ADD, dD=bias, ldd=0)
    eb, eb16 = _close(nso, cb, ref + b, TOL, "G fp8 gemm_kernel add"), _close(nso, cb, ref16 + b, TOL_A16_INT, "G fp8 gemm_kernel add a16")
    assert np.array_equal(_bits(cb), _bits((c + b).astype(np.float32)))
    print("rows17_64 G fp8 8192x1152 m=64 rel_l2 %.3g  a16 %.3g  add %.3g  add a16 %.3g" % (e, e16, eb, eb16))
    for epi, dD, want in ((pkg.EPI_NONE, None, c), (pkg.EPI_ADD, bias, cb)):
        cs, cs16 = _fwd(L, pkg, wt, dA, m, n, k, want16=True, epi=epi, dD=dD, ldd=0)
        assert np.array_equal(_bits(cs), _bits(want)), "asking for dC16 changed C"
        assert np.array_equal(_bits(cs16), _bits(cs.astype(np.float16))), "dC16 != RNE(C)"


# ------------------------------------------------------------------------------------------------ H: int8-reference mode
@pytest.fixture()
def int8_mode(L):
    prev = L.ns_hip_set_compute_mode(1)
    assert prev in (0, 1)
    yield
    L.ns_hip_set_compute_mode(prev)


def _unrelated_int8_forward(L, pkg, wt, m, k, n, seed):
    """leaves ANOTHER call's quantized activations of the same shape in the per-stream scratch"""
    import torch
    other = torch.randn((m, k), generator=torch.Generator(device="cuda").manual_seed(seed), device="cuda") * 3.0
    junk = torch.empty((m, n), device="cuda")
    pkg.check(L.ns_hip_f32f32_forward(other.data_ptr(), wt.h, junk.data_ptr(), m, k, n, 0, None, 0, _st()))
    return other, junk


@pytest.mark.parametrize("m", [9, 40])
@pytest.mark.parametrize("fmt", ["s4_bf16_g32", "s8_bf16_g64_int8core"])
def test_int8_mode_shared_activation_quantization(L, pkg, nso, bank, int8_mode, fmt, m):
    """fused QKV and gate/up in int8-reference mode: the second and third weight reuse the first one's quantized activations
    (shares_act_quant: one K, one group size).  An unrelated int8 forward of the same shape runs first on the same stream: its
    quantized activations must not be the ones reused"""
    import torch
    k = 1024
    ws = [bank.weight(fmt, N, k, seed=61 + i, wscale=0.05) for i in range(3)]
    a = bank.acts(k, seed=7)[:m].copy()
    a[m // 2] *= 30.0   # one row with a very different activation scale
    dA = torch.from_numpy(a).cuda()
    refs = [nso.gemm_u8s8(a, b) for b, _w in ws]
    ldc = N + 1
    keep = _unrelated_int8_forward(L, pkg, ws[0][1], m, k, N, seed=m)
    out = torch.full((3 * m + 1, ldc), SENT, device="cuda")
    pkg.check(L.ns_hip_fusion_qkv_forward_h(dA.data_ptr(), None, ws[0][1].h, ws[1][1].h, ws[2][1].h, out.data_ptr(), None, m, k, ldc, _st()))
    torch.cuda.synchronize()
    f = out.cpu().numpy()
    assert (f[:, N] == SENT).all() and (f[3 * m] == SENT).all()
    es = [_close(nso, f[i * m:(i + 1) * m, :N], refs[i], TOL_I8, "H qkv block %d" % i, row_tol=TOL_I8_ROW) for i in range(3)]
    keep = _unrelated_int8_forward(L, pkg, ws[2][1], m, k, N, seed=m + 100)
    t1, t2 = torch.full((m + 1, N), SENT, device="cuda"), torch.full((m + 1, N), SENT, device="cuda")
    pkg.check(L.ns_hip_fusion_ffn3_gateup_h(dA.data_ptr(), None, ws[0][1].h, ws[1][1].h, t1.data_ptr(), t2.data_ptr(), None, m, pkg.EPI_SILU, _st()))
    torch.cuda.synchronize()
    del keep
    assert (t1[m] == SENT).all() and (t2[m] == SENT).all()
    g, u = refs[0].astype(np.float64), refs[1].astype(np.float64)
    e1 = _close(nso, t1[:m].cpu().numpy(), _silu(g), TOL_I8_ACT, "H gate/up tmp1")
    e2 = _close(nso, t2[:m].cpu().numpy(), _silu(g) * u, TOL_I8_ACT, "H gate/up tmp2")
    print("rows17_64 H", fmt, m, "qkv worst %.3g  tmp1 %.3g  tmp2 %.3g" % (max(es), e1, e2))

"""Weight group sizes above one k-step on every GEMM and GEMV kernel.  Every matrix kernel finds the scale / zero-point row of
k-step s as (s * srow_mul) >> srow_shift (srow_rule / srow_params, ns_gemm_plan.cpp), in three regimes:
  group <= one k-step (128 columns of 4-bit records, 64 of 8-bit and fp8 ones)   the row is the k-step; INTERLEAVED layout
  group = 2^j k-steps, or per-channel                                           a shift, or row 0; THREE-ARRAY layout
  group = any other whole number of k-steps (384, 640; 8-bit 192, 320)          a 20-bit reciprocal multiply; three arrays
The ladder: 4-bit records 128 (control), 256, 384, 512, 640, per-channel; 8-bit and fp8 records 64 (control), 128, 192, 320,
per-channel — S4 / BF16, S4 / F32 asymmetric, NF4 / BF16, S4 / F16 (group 384), S8 / BF16, S8 / F32 asymmetric, F8_E4M3 with F32 and
E8M0 scales — on N = 263 (17 tiles, the last 7 wide; three 128-column blocks) and K = 1920 / 2048 / 1952: between them every group size
sees whole groups, a last group cut short by K, and a partial last k-step inside a short last group; K splits (gemvs slices, the
tiled kernels' split-K) cut through the 384- and 640-wide groups.

Every family at the smallest rows that reach it, pinned with the tuning keys (restored afterwards), every output with a sentinel row
and column (ldc = n + 1) and through check_blocks (tests/tools/gemm_blocks.py: whole output, rows, 16-column tiles, (tile x row block)
and element-wise term errors; its docstring has the bars).  The weights, activations and references are made once per module.

What the library refuses.  At LOAD nothing of the ladder (REFUSED below is empty, and an undocumented refusal fails the test; fp8 weights
load at all five groups with both scale types).  The PLANS refuse the calls below, silently, and the next kernel serves them; every one
is pinned on the CPU for exactly these shapes (tests/test_stream_plan.py::test_the_group_size_ladder_is_planned_as_the_gpu_module_says),
and where the next server can be pinned on the GPU the test asserts that its bits are the result:
  * ABOUT THE GROUP SIZE, one: gemv_kernel's int8-reference variant (1 .. 4 rows) takes power-of-two k-blocks — "int8-reference numerics:
    integer weights, up to 4 rows, power-of-two k-blocks, aligned codes" (plan_i8) — so groups 384 / 640 (8-bit: 192 / 320) at 1 and 3
    rows run on i8ref_kernel; the reciprocal-multiply regime does not exist on that variant.
  * several rows over K = 1952 (not whole k-steps: a row's padding would read the next row): gemvs_kernel "K: a multiple of 8, and of the
    k-step for several rows", gemv_kernel "activations: aligned fp16 or fp32 rows; several rows need whole k-steps" (int8 variant at 3
    rows alike: i8ref_kernel).  smallm_kernel serves 2 .. 16 rows there, the fused m = 8 launches included: the partial last k-step inside
    a short last group runs on gemv_kernel at ONE row only, on gemvs_kernel never, and on smallm_kernel, the tiled and int8 kernels.
  * 16 rows on gemv_kernel: K = 2048 "the staged activations exceed 64 KiB" (16 x 2056 x 2 = 65,792 B); K = 1920 without the caller's
    fp16 shadow "more fp32 activation pieces than the waves hold in registers".  So 16 rows reach gemv_kernel at K = 1920 with the
    shadow only; smallm_kernel serves the rest (with "gvs" at its default gemvs_kernel would: 16 rows are its by shape).
  * ns_hip_mul_mat_id's grouped path takes K in whole 64s (moe_mm_plan): 40 rows over K = 1952 count as "refused" in ns_hip_moe_stats and
    run on the loop kernel.
  * gemm2_kernel does not take fp8 weights ("the RoPE epilogue and the fp8 conversion are gemm3_kernel's"): gemm_kernel serves them.
  * an fp16-only output of fp8 weights outside gemm3_kernel's scale-range rule: "forward: fp16-only activations / outputs need a weight
    the tiled kernel takes as is ..."; the fp32 call of the same test is then the result.
Knob values that change nothing for a format (gemm_plan, tests/test_gemm_plan.py): "g3_bm" 257 is the tall 256 x 32 wave tile for 4-bit
integer codes only — NF4, 8-bit and fp8 weights get the automatic 128-row tile; "g3_wide" 1 is the per-wave epilogue again on the plain
256-row tile.  Every forced "gvs_slices" x "gvs_waves" pair of this module is planned as forced at K = 1920 / 2048 (the same CPU test).

The two measured bars of check_blocks (block and term errors against max(floor, factor x the numpy model's error)) take their factors
from THIS module's control formats — group 128 on 4-bit records, 64 on 8-bit and fp8 ones, the interleaved layout — with a margin of
2: the floors, the factors, the ratios they were taken from and the largest values the ladder then showed are in the docstring of
tests/tools/gemm_blocks.py and in docs/measurement.md.  Run with -s: the last line printed is the largest value every bar saw, control
formats and ladder apart."""
import contextlib
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("gemm_blocks", os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools", "gemm_blocks.py"))
gb = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gb)

SENT = -7.0
N = 263
KS = (1920, 2048, 1952)
ROWS = 257        # rows of activations per K: a call of m rows takes the first m (GEMM rows are independent)
ROWS_I8 = 200
TOL_MUL = 2e-3    # a product of two rounded factors (tests/test_gpu_gemm3.py, tests/test_gpu_rows17_64.py)
TOL_LOOP_A16 = 5e-5   # moe_gemv_kernel against the fp16-activation product (tests/test_gpu_moe_paths.py)
G4, G8 = (128, 256, 384, 512, 640, -1), (64, 128, 192, 320, -1)
FMT = {  # qtype, scale dtype, asym, reference core of the host blob (None: fp8, blob from the device quantizer), groups, control group
    "s4_bf16": ("S4", "BF16", False, "CORE_AVX512F", G4, 128),
    "s4_asym_f32": ("S4", "F32", True, "CORE_AVX512F", G4, 128),
    "nf4_bf16": ("F4_NF4", "BF16", False, "CORE_AVX512F", G4, 128),
    "s4_f16": ("S4", "F16", False, "CORE_AVX512F", (384,), 128),
    "s8_bf16": ("S8", "BF16", False, "CORE_AVX512F", G8, 64),
    "s8_asym_f32": ("S8", "F32", True, "CORE_AVX512F", G8, 64),
    "f8_e4m3_f32": ("F8_E4M3", "F32", False, None, G8, 64),
    "f8_e4m3_e8m0": ("F8_E4M3", "F8_E8M0", False, None, G8, 64),
}
LADDER = [(f, g) for f, v in FMT.items() for g in v[4]]
INT_LADDER = [(f, g) for f, g in LADDER if f.startswith("s")]
# one format of each regime: interleaved control, shift, reciprocal multiply (4-bit and 8-bit), row 0
REGIMES = [("s4_bf16", 128), ("s4_bf16", 256), ("s4_asym_f32", 384), ("s8_bf16", 192), ("nf4_bf16", -1)]
# (format, group) the library refuses, with the text of its refusal
REFUSED = {}
DEFAULTS = {"gvs": 1, "gvs_slices": 0, "gvs_waves": 0, "gvs_finalize": 1, "gemv2": 1, "gv_rows1": 1, "gv_nw": 0, "g3_bm": 0, "g3_wide": -1,
            "g3_min_m": 0, "i8_mfma": 2, "i8_tile": 0}


def _id(v):
    return "g%s" % ("pc" if v == -1 else v) if isinstance(v, int) and (v < 0 or v in G4 + G8) else "K%d" % v if isinstance(v, int) else str(v)


def _ladder(cases):
    return pytest.mark.parametrize("fmt,group,k", [(f, g, k) for f, g in cases for k in KS], ids=lambda v: _id(v))


@contextlib.contextmanager
def tuned(L, **kv):
    try:
        for key, v in kv.items():
            assert L.ns_hip_set_tuning(key.encode(), v) == 0, key
        yield
    finally:
        for key in kv:
            L.ns_hip_set_tuning(key.encode(), DEFAULTS[key])


def _st():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32 if x.dtype == np.float32 else np.uint16)


def _silu(v):
    return v * (0.5 + 0.5 * np.tanh(0.5 * v))


class _Refused(Exception):
    pass


class _Bank:
    """weights, activations and references of the module, each made once and never changed"""

    def __init__(self, L, pkg, nso):
        self.L, self.pkg, self.nso = L, pkg, nso
        self.w, self.a, self.p, self.p8, self.keep = {}, {}, {}, {}, []

    def acts(self, k):
        if k not in self.a:
            self.a[k] = np.random.default_rng(1000 + k).standard_normal((ROWS, k)).astype(np.float32)
        return self.a[k]

    def acts8(self, k):
        """int8-reference mode: the same rows, one of them (row 2) with a very different activation scale"""
        if (k, 8) not in self.a:
            a = self.acts(k)[:ROWS_I8].copy()
            a[2] *= 30.0
            self.a[(k, 8)] = a
        return self.a[(k, 8)]

    def weight(self, fmt, group, k, seed=0, n=N, wscale=0.02):
        """(host blob, device weight); _Refused(message) where the library refuses the format"""
        import torch
        key = (fmt, group, k, seed, n, wscale)
        if key not in self.w:
            L, pkg, nso = self.L, self.pkg, self.nso
            qt, sdt, asym, core = FMT[fmt][:4]
            try:
                if core is None:  # fp8: the device quantizer (bit-exact with the oracle's packer, which takes minutes at these sizes)
                    gen = torch.Generator(device="cuda").manual_seed(seed * 7919 + n + k)
                    dW = torch.randn((n, k), generator=gen, device="cuda") * wscale
                    bs = group & 0xFFFFFFFFFFFFFFFF
                    size = L.ns_BTLAGemmPackBSize(n, k, bs, getattr(pkg, qt), getattr(pkg, sdt), asym, pkg.COMP_F32, None)
                    if not size:
                        raise _Refused(pkg.last_error())
                    dBlob = torch.zeros(size, dtype=torch.uint8, device="cuda")
                    if L.ns_hip_quant_pack_device(dBlob.data_ptr(), dW.data_ptr(), n, k, k, bs, getattr(pkg, qt), getattr(pkg, sdt), asym,
                                                  pkg.COMP_F32, True, _st()):
                        raise _Refused(pkg.last_error())
                    torch.cuda.synchronize()
                    blob = nso.aligned_bytes(size)
                    blob[:] = dBlob.cpu().numpy()
                    h = L.ns_hip_weight_from_device_blob(dBlob.data_ptr(), size, _st())
                    self.keep.append(dBlob)
                else:
                    rng = np.random.default_rng(seed * 7919 + n * 3 + k + (group & 1023))
                    w = (rng.standard_normal((n, k)) * wscale).astype(np.float32)
                    blob = nso.quant_pack(w, group, getattr(nso, qt), getattr(nso, sdt), asym, getattr(nso, core))
                    h = L.ns_hip_weight_from_blob(nso.ptr(blob), _st())
                if not h:
                    raise _Refused(pkg.last_error())
                torch.cuda.synchronize()
                self.w[key] = (blob, pkg.Weight(h))
            except _Refused as r:
                L.ns_hip_reset_error()
                self.w[key] = r
        if isinstance(self.w[key], _Refused):
            raise self.w[key]
        return self.w[key]

    def prob(self, fmt, group, k, seed=0, n=N, wscale=0.02):
        key = (fmt, group, k, seed, n, wscale)
        if key not in self.p:
            self.p[key] = gb.Problem(self.nso, self.acts(k), self.weight(fmt, group, k, seed, n, wscale)[0], f4=fmt.startswith("nf4"))
        return self.p[key]

    def prob8(self, fmt, group, k):
        key = (fmt, group, k)
        if key not in self.p8:
            self.p8[key] = gb.Problem(self.nso, self.acts8(k), self.weight(fmt, group, k)[0], i8=True)
        return self.p8[key]

    def close(self):
        for v in self.w.values():
            if not isinstance(v, _Refused):
                v[1].free()
        self.L.ns_hip_cache_clear()


@pytest.fixture(scope="module")
def bank(L, pkg, nso):
    b = _Bank(L, pkg, nso)
    yield b
    b.close()
    print("group_sizes largest value seen per bar:", gb.seen_report())


def _get(bank, fmt, group, k, **kw):
    """(blob, weight, Problem) of a ladder entry — or, for an entry the library refuses, the assertion that it is a documented refusal
    (the test then ends: there is no weight to multiply)"""
    try:
        blob, wt = bank.weight(fmt, group, k, **kw)
    except _Refused as r:
        assert (fmt, group) in REFUSED and REFUSED[(fmt, group)] in str(r), ("an undocumented refusal", fmt, group, k, str(r))
        return None
    assert (fmt, group) not in REFUSED, ("documented as refused, but loaded", fmt, group)
    return blob, wt, bank.prob(fmt, group, k, **kw)


def _kstep(fmt):
    return 64 if fmt.startswith(("s8", "f8")) else 128


def _gemv_takes(fmt, k, m, shadow=True):
    """gemv_plan's envelope at this module's shapes (module docstring; pinned in tests/test_stream_plan.py): whole k-steps for several
    rows, 64 KiB of staged activations, 16 rows only from the caller's fp16 shadow"""
    cols = -(-k // _kstep(fmt)) * _kstep(fmt)
    return (m == 1 or k % _kstep(fmt) == 0) and m * (cols + 8) * 2 <= 64 * 1024 and (shadow or m < 16)


def _control(fmt, group):
    return group == FMT[fmt][5]


def _fwd(L, pkg, wt, dA, m, n, lda, a16=None, want16=False, want32=True, epi=0):
    """ns_hip_f32f32_forward_h into sentinel-filled (m + 1) x (n + 1) outputs; returns (rc, C, C16)"""
    import torch
    ldc = n + 1
    dC = torch.full((m + 1, ldc), SENT, dtype=torch.float32, device="cuda")
    dC16 = torch.full((m + 1, ldc), SENT, dtype=torch.float16, device="cuda")
    rc = L.ns_hip_f32f32_forward_h(dA.data_ptr() if dA is not None else None, a16.data_ptr() if a16 is not None else None, wt.h,
                                   dC.data_ptr() if want32 else None, dC16.data_ptr() if want16 else None, m, lda, ldc, epi, None, 0, _st())
    torch.cuda.synchronize()
    if rc != 0:
        return rc, None, None
    c, c16 = dC.cpu().numpy(), dC16.cpu().numpy()
    if want32:
        assert (c[:, n] == SENT).all() and (c[m] == SENT).all(), "fp32 output: written outside m x n"
    else:
        assert (c == SENT).all(), "fp32 output written although none was asked for"
    if want16:
        assert (c16[:, n] == np.float16(SENT)).all() and (c16[m] == np.float16(SENT)).all(), "fp16 output: written outside m x n"
    else:
        assert (c16 == np.float16(SENT)).all(), "fp16 output written although none was asked for"
    return 0, np.ascontiguousarray(c[:m, :n]), np.ascontiguousarray(c16[:m, :n])


def _both_forms(L, pkg, nso, wt, prob, m, k, family, what, control):
    """fp32-only activations, then the fp16 shadow in and out: one C bit for bit, C16 = RNE(C), every bar of check_blocks"""
    import torch
    dA = torch.from_numpy(np.ascontiguousarray(prob.a[:m])).cuda()
    rc, c0, _ = _fwd(L, pkg, wt, dA, m, N, k)
    assert rc == 0, (what, pkg.last_error())
    rc, c1, c116 = _fwd(L, pkg, wt, dA, m, N, k, a16=dA.half(), want16=True)
    assert rc == 0, (what, pkg.last_error())
    assert np.array_equal(_bits(c0), _bits(c1)), (what, "the shadows changed C", int((_bits(c0) != _bits(c1)).sum()))
    assert np.array_equal(_bits(c116), _bits(c1.astype(np.float16))), (what, "dC16 != RNE(C)")
    gb.check_blocks(nso, c0, None, None, family, prob=prob, what=what, control=control)
    return c0


def _host(L, nso, a, blob, m, k):
    out = np.full((m + 1, N + 1), SENT, np.float32)
    L.bestla_f32f32_forward(nso.ptr(a), nso.ptr(blob), nso.ptr(out), m, N, k, k, N + 1, None)
    assert (out[:, N] == SENT).all() and (out[m] == SENT).all(), "host entry: written outside m x n"
    return np.ascontiguousarray(out[:m, :N])


# ------------------------------------------------------------------------------------------------ gemv_kernel
@_ladder(LADDER)
def test_gemv_kernel(L, pkg, nso, bank, fmt, group, k):
    """"gvs" 0: one row on the one-row instantiation and on the general one (the same bits), 4 and 16 rows, 2 / by shape / 16 waves.  Where
    gemv_plan refuses the rows (_gemv_takes: K = 1952 from two rows, 16 rows at K = 2048) smallm_kernel is the server: the result must be
    the bits of the call that pins it ("gemv2" 0)"""
    got = _get(bank, fmt, group, k)
    if got is None:
        return
    _blob, wt, prob = got
    ctl = _control(fmt, group)
    with tuned(L, gvs=0):
        one = {}
        for rows1 in (1, 0):
            with tuned(L, gv_rows1=rows1):
                one[rows1] = _both_forms(L, pkg, nso, wt, prob, 1, k, "stream", "gemv rows1=%d" % rows1, ctl)
        assert np.array_equal(_bits(one[0]), _bits(one[1])), "the one-row instantiation's bits differ from the general one's"
        for m in (4, 16):
            took = _gemv_takes(fmt, k, m)
            c = _both_forms(L, pkg, nso, wt, prob, m, k, "stream", "gemv m=%d%s" % (m, "" if took else " (refused: smallm_kernel)"), ctl)
            if not took:
                with tuned(L, gemv2=0):
                    pinned = _both_forms(L, pkg, nso, wt, prob, m, k, "stream", "smallm m=%d" % m, ctl)
                assert np.array_equal(_bits(c), _bits(pinned)), (m, k, "gemv_kernel refuses these rows: smallm_kernel's bits expected")
        for nw in (2, 16):   # ("gv_nw" 0, by shape, is every call above)
            with tuned(L, gv_nw=nw):
                _both_forms(L, pkg, nso, wt, prob, 1, k, "stream", "gemv nw=%d" % nw, ctl)


def _qkv(L, pkg, nso, bank, fmt, group, k, m, family, what):
    """ns_hip_fusion_qkv_forward_h on three weights of one format: every block through check_blocks, nothing written outside"""
    import torch
    ws = [_get(bank, fmt, group, k, seed=s) for s in (1, 2, 3)]
    dA = torch.from_numpy(np.ascontiguousarray(bank.acts(k)[:m])).cuda()
    dA16 = dA.half()
    ldc = N + 1
    out = torch.full((3 * m + 1, ldc), SENT, device="cuda")
    out16 = torch.full((3 * m + 1, ldc), SENT, device="cuda", dtype=torch.float16)
    rc = L.ns_hip_fusion_qkv_forward_h(dA.data_ptr(), dA16.data_ptr(), ws[0][1].h, ws[1][1].h, ws[2][1].h, out.data_ptr(), out16.data_ptr(),
                                       m, k, ldc, _st())
    assert rc == 0, pkg.last_error()
    torch.cuda.synchronize()
    f, f16 = out.cpu().numpy(), out16.cpu().numpy()
    assert (f[:, N] == SENT).all() and (f[3 * m] == SENT).all() and (f16[:, N] == np.float16(SENT)).all() and (f16[3 * m] == np.float16(SENT)).all()
    for i in range(3):
        blk = np.ascontiguousarray(f[i * m:(i + 1) * m, :N])
        assert np.array_equal(_bits(f16[i * m:(i + 1) * m, :N]), _bits(blk.astype(np.float16))), (what, i, "shadow != RNE(block)")
        gb.check_blocks(nso, blk, None, None, family, prob=ws[i][2], what="%s block %d" % (what, i), control=_control(fmt, group))


def _gateup(L, pkg, nso, bank, fmt, group, k, m, tol2, what):
    """ns_hip_fusion_ffn3_gateup_h: tmp1 = silu(A W1), tmp2 = tmp1 * (A W3) against the fp64 epilogue: whole, rows and tiles.  tmp2 as a
    whole within tol2; its rows and tiles within 2e-3, the bar of a product of two rounded factors: on the 16 numbers of a tile of ONE
    row the two factors' errors add up, and the numpy model of this very computation reaches 1.4e-3 there (0.7e-3 on tmp1)"""
    import torch
    (_b1, w1, p1), (_b3, w3, p3) = (_get(bank, fmt, group, k, seed=s) for s in (4, 5))
    dA = torch.from_numpy(np.ascontiguousarray(bank.acts(k)[:m])).cuda()
    dA16 = dA.half()
    t1, t2 = torch.full((m + 1, N), SENT, device="cuda"), torch.full((m + 1, N), SENT, device="cuda")
    t216 = torch.full((m + 1, N), SENT, device="cuda", dtype=torch.float16)
    rc = L.ns_hip_fusion_ffn3_gateup_h(dA.data_ptr(), dA16.data_ptr(), w1.h, w3.h, t1.data_ptr(), t2.data_ptr(), t216.data_ptr(), m,
                                       pkg.EPI_SILU, _st())
    assert rc == 0, pkg.last_error()
    torch.cuda.synchronize()
    assert (t1[m] == SENT).all() and (t2[m] == SENT).all() and (t216[m] == SENT).all()
    assert torch.equal(t216[:m], t2[:m].half())
    r1 = _silu(p1.ref[:m])
    gb.check_rows_tiles(t1[:m].cpu().numpy(), r1, gb.TOL, what + " tmp1")
    gb.check_rows_tiles(t2[:m].cpu().numpy(), r1 * p3.ref[:m], tol2, what + " tmp2", row_tol=TOL_MUL)


@_ladder(REGIMES)
@pytest.mark.parametrize("m", [1, 8])
def test_gemv_kernel_fused_launches(L, pkg, nso, bank, fmt, group, k, m):
    """the fused QKV and gate/up decode launches of gemv_kernel, one format of each regime (8 rows over K = 1952: refused for its
    partial k-step, smallm_kernel's three-segment grid and its gate / up composition serve them)"""
    with tuned(L, gvs=0):
        _qkv(L, pkg, nso, bank, fmt, group, k, m, "stream", "gemv qkv m=%d" % m)
        _gateup(L, pkg, nso, bank, fmt, group, k, m, gb.TOL, "gemv gate/up m=%d" % m)


# ------------------------------------------------------------------------------------------------ gemvs_kernel
@_ladder(LADDER)
def test_gemvs_kernel(L, pkg, nso, bank, fmt, group, k):
    """"gvs" 3 at K = 1920 / 2048: 2, 8 and 16 rows x 1 / 2 / 4 / 8 slices of K x 3 / 7 streaming waves (15 or 16 k-steps of 128, twice
    as many of 64: the slice boundaries fall inside the 384- and 640-wide groups; every pair is planned as forced, tests/test_stream_plan.py),
    and split-K finished in the launch against the finalize launch: the same slice order, the same bits.  K = 1952 is refused for every row
    count of this kernel (module docstring), by gemv_kernel as well: one call, which must return smallm_kernel's bits"""
    import torch
    got = _get(bank, fmt, group, k)
    if got is None:
        return
    _blob, wt, prob = got
    ctl = _control(fmt, group)
    if k % _kstep(fmt):
        with tuned(L, gvs=3):
            c = _both_forms(L, pkg, nso, wt, prob, 8, k, "stream", "gemvs m=8 (refused: smallm_kernel)", ctl)
        with tuned(L, gvs=0, gemv2=0):
            pinned = _both_forms(L, pkg, nso, wt, prob, 8, k, "stream", "smallm m=8", ctl)
        assert np.array_equal(_bits(c), _bits(pinned)), (k, "gemvs_kernel and gemv_kernel refuse this K: smallm_kernel's bits expected")
        return
    with tuned(L, gvs=3):
        for m in (2, 8, 16):
            dA = torch.from_numpy(np.ascontiguousarray(prob.a[:m])).cuda()
            dA16 = dA.half()
            for slices in (1, 2, 4, 8):
                for waves in (3, 7):
                    what = "gemvs m=%d slices=%d waves=%d" % (m, slices, waves)
                    with tuned(L, gvs_slices=slices, gvs_waves=waves):
                        rc, c, c16 = _fwd(L, pkg, wt, dA, m, N, k, a16=dA16, want16=True)
                        assert rc == 0, (what, pkg.last_error())
                        gb.check_blocks(nso, c, None, None, "stream", prob=prob, what=what, control=ctl)
                        assert np.array_equal(_bits(c16), _bits(c.astype(np.float16))), (what, "dC16 != RNE(C)")
                        if slices > 1 and waves == 7:
                            with tuned(L, gvs_finalize=0):
                                rc, c2, _ = _fwd(L, pkg, wt, dA, m, N, k, a16=dA16, want16=True)
                            assert rc == 0, (what, pkg.last_error())
                            assert np.array_equal(_bits(c), _bits(c2)), (what, "in-launch split-K differs from the finalize launch")
        _both_forms(L, pkg, nso, wt, prob, 8, k, "stream", "gemvs m=8 by plan", ctl)


# ------------------------------------------------------------------------------------------------ smallm_kernel
@_ladder(LADDER)
def test_smallm_kernel(L, pkg, nso, bank, fmt, group, k):
    """"gemv2" 0 (and "gvs" 0): the first-generation streaming kernel at 1 and 8 rows; 17, 33 and 64 rows as dispatched (MB = 2 / 4)"""
    got = _get(bank, fmt, group, k)
    if got is None:
        return
    _blob, wt, prob = got
    ctl = _control(fmt, group)
    with tuned(L, gemv2=0, gvs=0):
        for m in (1, 8):
            _both_forms(L, pkg, nso, wt, prob, m, k, "stream", "smallm gemv2=0 m=%d" % m, ctl)
    for m in (17, 33, 64):
        _both_forms(L, pkg, nso, wt, prob, m, k, "stream", "smallm m=%d" % m, ctl)


# ------------------------------------------------------------------------------------------------ gemm2_kernel
@_ladder(LADDER)
def test_gemm2_kernel(L, pkg, nso, bank, fmt, group, k):
    """"g3_min_m" above the call's rows: 100 and 150 rows (3 column blocks x 2 row blocks: split-K by 2 or 4).  fp8 weights are not
    gemm2_kernel's: the first-generation gemm_kernel serves them, silently, and is held to the same bars"""
    got = _get(bank, fmt, group, k)
    if got is None:
        return
    _blob, wt, prob = got
    with tuned(L, g3_min_m=1 << 20):
        for m in (100, 150):
            _both_forms(L, pkg, nso, wt, prob, m, k, "tiled", "gemm2 m=%d" % m, _control(fmt, group))


# ------------------------------------------------------------------------------------------------ gemm3_kernel
@_ladder(LADDER)
def test_gemm3_kernel(L, pkg, nso, bank, fmt, group, k):
    """192 and 257 rows x "g3_bm" 128 / 256 / 257 x "g3_wide" 0 / 1 through the device entry (K = 1920 / 1952: two splits of 1024,
    which cut a 384-wide group at 2 2/3; 257 is a tile of its own for 4-bit integer codes only, module docstring); the host entry; the
    fp16-only output"""
    import torch
    got = _get(bank, fmt, group, k)
    if got is None:
        return
    blob, wt, prob = got
    ctl = _control(fmt, group)
    for m in (192, 257):
        for bm in (128, 256, 257):
            for wide in (0, 1):
                with tuned(L, g3_bm=bm, g3_wide=wide):
                    _both_forms(L, pkg, nso, wt, prob, m, k, "tiled", "gemm3 m=%d bm=%d wide=%d" % (m, bm, wide), ctl)
    try:
        gb.check_blocks(nso, _host(L, nso, prob.a, blob, ROWS, k), None, None, "tiled", prob=prob, what="gemm3 host entry", control=ctl)
    finally:
        L.ns_hip_cache_clear()
    # fp16-only output (the consumer is the library's next GEMM).  Its rounding, 2^-11 of every element, is in neither the numpy model
    # nor the fp16-activation bar, so the output is tied to the fp32 output of the same weight, which went through check_blocks: the two
    # launches differ by the K split at most (an fp16-only launch never splits K) — by fp32 summation order, which the standard bound
    # K * 2^-24 * (|a| @ |wq|) covers for each of the two sums (it matters where a sum cancels: there the fp16 spacing is finer than
    # that) — so every element is within one fp16 ulp of the fp32 one (2^-10 relative; 2^-24, the subnormal spacing, near zero) plus
    # those two bounds; and the fp32 bars, whole, rows and tiles
    m = 257
    dA = torch.from_numpy(np.ascontiguousarray(prob.a[:m])).cuda()
    dA16 = dA.half()
    rc, c32, _ = _fwd(L, pkg, wt, dA, m, N, k, a16=dA16)
    assert rc == 0, pkg.last_error()
    gb.check_blocks(nso, c32, None, None, "tiled", prob=prob, what="gemm3 m=257", control=ctl)
    rc, _c, c16 = _fwd(L, pkg, wt, dA, m, N, k, a16=dA16, want16=True, want32=False)
    if rc != 0:   # only fp8 weights outside gemm3_kernel's scale-range rule may be refused here; the fp32 call above served them
        assert fmt.startswith("f8") and "need a weight the tiled kernel takes as is" in pkg.last_error(), pkg.last_error()
        L.ns_hip_reset_error()
    else:
        gap = np.abs(c16.astype(np.float64) - c32)
        room = 2.0 ** -10 * np.abs(c32) + 2.0 ** -24 + 2 * k * 2.0 ** -24 * prob.mag[:m]
        assert (gap <= room).all(), ("fp16-only output further than one fp16 ulp from the fp32 output", float((gap / room).max()), int((gap > room).sum()))
        gb.check_rows_tiles(c16.astype(np.float64), prob.ref[:m], gb.TOL, "gemm3 fp16-only output")


@_ladder(REGIMES)
def test_gemm3_kernel_fused_launches(L, pkg, nso, bank, fmt, group, k):
    """fused QKV (three matrices side by side) and gate / up tile pairs at 200 rows, one format of each regime"""
    _qkv(L, pkg, nso, bank, fmt, group, k, 200, "tiled", "gemm3 qkv")
    _gateup(L, pkg, nso, bank, fmt, group, k, 200, TOL_MUL, "gemm3 gate/up")


# ------------------------------------------------------------------------------------------------ int8-reference mode
@pytest.fixture()
def int8_mode(L):
    prev = L.ns_hip_set_compute_mode(1)
    assert prev in (0, 1)
    yield
    L.ns_hip_set_compute_mode(prev)


@_ladder(INT_LADDER)
def test_int8_reference_mode(L, pkg, nso, bank, int8_mode, fmt, group, k):
    """against nso.gemm_u8s8: 1 and 3 rows, 9 (i8ref_kernel), 16 / 77 / 200 on both matrix-core kernels ("i8_mfma" 2 in its workgroup
    tiles "i8_tile" 1 / 4, and "i8_mfma" 1).  1 and 3 rows are gemv_kernel's int8 variant for power-of-two groups and per-channel (3 rows:
    at K = 1920 / 2048); it REFUSES the reciprocal-multiply groups 384 / 640 / 192 / 320 ("... power-of-two k-blocks ...", module
    docstring) and 3 rows over K = 1952: i8ref_kernel serves those, held to the same bars"""
    got = _get(bank, fmt, group, k)
    if got is None:
        return
    blob = got[0]
    prob = bank.prob8(fmt, group, k)
    ctl = _control(fmt, group)
    try:
        for m in (1, 3, 9):
            gb.check_blocks(nso, _host(L, nso, prob.a, blob, m, k), None, None, "i8", prob=prob, what="int8 m=%d" % m, control=ctl)
        for m in (16, 77, 200):
            for gen, tile in ((2, 1), (2, 4), (1, 0)):
                with tuned(L, i8_mfma=gen, i8_tile=tile):
                    gb.check_blocks(nso, _host(L, nso, prob.a, blob, m, k), None, None, "i8", prob=prob,
                                    what="int8 m=%d i8_mfma=%d i8_tile=%d" % (m, gen, tile), control=ctl)
    finally:
        L.ns_hip_cache_clear()


# ------------------------------------------------------------------------------------------------ ns_hip_mul_mat_id
MOE_PATHS = {4: ("decode", (0, 1, 0, 0), "stream", None), 12: ("loop", (0, 0, 1, 0), "stream", TOL_LOOP_A16), 40: ("grouped", (1, 0, 0, 0), "tiled", None)}
MOE_REFUSED_THEN_LOOP = (0, 0, 1, 1)   # the grouped path takes K in whole 64s (moe_mm_plan, ns_moe_plan.cpp): K = 1952 is the loop kernel's


def _moe_stats(L):
    out = (C.c_uint64 * 4)()
    L.ns_hip_moe_stats(out)
    return np.array(list(out), np.int64)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("m", sorted(MOE_PATHS))
@pytest.mark.parametrize("group", [256, 384])
@pytest.mark.parametrize("fmt", ["s4_bf16", "s4_asym_f32"])
def test_mul_mat_id(L, pkg, nso, bank, fmt, group, m, k):
    """four experts of 263 columns: 4 rows on the decode launches, 12 on the loop kernel, 40 on the grouped path (the default thresholds;
    confirmed by ns_hip_moe_stats), every row against ITS expert's references.  The grouped path refuses K = 1952 (not whole 64s) whatever
    the group size: the statistics must say refused, and the loop kernel, the next server, is held to its own bars"""
    import torch
    n_as = 4
    path, delta, family, tol16 = MOE_PATHS[m]
    if path == "grouped" and k % 64:
        path, delta, family, tol16 = "grouped refused, loop", MOE_REFUSED_THEN_LOOP, "stream", TOL_LOOP_A16
    es = [_get(bank, fmt, group, k, seed=10 + e) for e in range(n_as)]
    arr = (C.c_void_p * n_as)(*[e[1].h for e in es])
    grp = L.ns_hip_expert_group_create(arr, n_as)
    assert grp, pkg.last_error()
    try:
        ids = np.random.default_rng(m).integers(0, n_as, size=(m, 2)).astype(np.int32)
        dA, dI = torch.from_numpy(np.ascontiguousarray(bank.acts(k)[:m])).cuda(), torch.from_numpy(ids).cuda()
        for sel in range(2):
            dC = torch.full((m + 1, N + 1), SENT, device="cuda")
            before = _moe_stats(L)
            rc = L.ns_hip_mul_mat_id(dA.data_ptr(), dI.data_ptr(), 2, sel, grp, dC.data_ptr(), m, k, N + 1, pkg.EPI_NONE, None, 0, _st())
            assert rc == 0, pkg.last_error()
            torch.cuda.synchronize()
            assert tuple(_moe_stats(L) - before) == delta, (path, tuple(_moe_stats(L) - before))
            c = dC.cpu().numpy()
            assert (c[:, N] == SENT).all() and (c[m] == SENT).all()
            prob = gb.Problem.of_rows([e[2] for e in es], [int(i) for i in ids[:, sel]])
            gb.check_blocks(nso, np.ascontiguousarray(c[:m, :N]), None, None, family, prob=prob, what="mul_mat_id %s sel=%d" % (path, sel),
                            tol16=tol16)
    finally:
        L.ns_hip_expert_group_free(grp)


# ------------------------------------------------------------------------------------------------ load and quantize
@_ladder(REGIMES)
def test_unpack_and_device_quantizer(L, pkg, nso, bank, fmt, group, k):
    """bestla_unpackweight_fp32 bit-equal to nso.unpack_fp32; ns_hip_quant_pack_device byte-equal to nso.quant_pack"""
    import torch
    blob, _wt, prob = _get(bank, fmt, group, k)
    out = np.zeros((k, N + 3), np.float32)
    L.bestla_unpackweight_fp32(nso.ptr(blob), N, k, nso.ptr(out), N + 3)
    L.ns_hip_cache_clear()
    assert np.array_equal(_bits(out[:, :N]), _bits(prob.wq)), "unpack differs from the oracle's"
    assert np.all(out[:, N:] == 0)
    qt, sdt, asym, core = FMT[fmt][:4]
    w = (np.random.default_rng(k + group).standard_normal((N, k)) * 0.02).astype(np.float32)
    want = nso.quant_pack(w, group, getattr(nso, qt), getattr(nso, sdt), asym, getattr(nso, core))
    bs = group & 0xFFFFFFFFFFFFFFFF
    L.ns_set_pack_core(getattr(nso, core))
    try:
        size = L.ns_BTLAGemmPackBSize(N, k, bs, getattr(pkg, qt), getattr(pkg, sdt), asym, pkg.COMP_F32, None)
        assert size == want.size, (size, want.size, pkg.last_error())
        dBlob, dW = torch.zeros(size, dtype=torch.uint8, device="cuda"), torch.from_numpy(w).cuda()
        pkg.check(L.ns_hip_quant_pack_device(dBlob.data_ptr(), dW.data_ptr(), N, k, k, bs, getattr(pkg, qt),
                                             getattr(pkg, sdt), asym, pkg.COMP_F32, True, _st()))
        torch.cuda.synchronize()
    finally:
        L.ns_set_pack_core(pkg.CORE_AUTO)
    mine = dBlob.cpu().numpy()
    assert np.array_equal(mine, want), ("device quantizer differs from the oracle's packer at", int((mine != want).sum()), "bytes")


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("fmt,group", [("s4_bf16", 384), ("s4_asym_f32", 384), ("s8_bf16", 192)])
def test_weight_slice_on_a_group_boundary(L, pkg, nso, bank, fmt, group, k):
    """ns_hip_weight_slice along K on a boundary of the reciprocal-multiply groups (3 groups | the rest: each shard's scale rows start
    at its own row 0, the second one keeps the short last group) — the partial products sum to the unsliced one — and along N (128
    | 135 columns): the unsliced columns bit for bit"""
    import torch
    _blob, wt, prob = _get(bank, fmt, group, k)
    m = 8
    a = prob.a[:m]
    dA = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    rc, full, _ = _fwd(L, pkg, wt, dA, m, N, k)
    assert rc == 0, pkg.last_error()
    kcut = 3 * group
    shards = [wt.slice(0, N, 0, kcut, _st()), wt.slice(0, N, kcut, k, _st())]
    try:
        acc = np.zeros((m, N), np.float64)
        for sh, (k0, k1) in zip(shards, ((0, kcut), (kcut, k))):
            assert (sh.n, sh.k) == (N, k1 - k0)
            rc, part, _ = _fwd(L, pkg, sh, dA[:, k0:k1].contiguous(), m, N, k1 - k0)
            assert rc == 0, pkg.last_error()
            acc += part
        # two fp32 partial sums added in fp64: closer to the references than the one launch, never further than its bars
        gb.check_blocks(nso, acc.astype(np.float32), None, None, "stream", prob=prob, what="K shards", control=False)
    finally:
        for sh in shards:
            sh.free()
    cols = []
    for n0, n1 in ((0, 128), (128, N)):
        sh = wt.slice(n0, n1, 0, k, _st())
        try:
            rc, part, _ = _fwd(L, pkg, sh, dA, m, n1 - n0, k)
            assert rc == 0, pkg.last_error()
            cols.append(part)
        finally:
            sh.free()
    assert np.array_equal(_bits(np.concatenate(cols, axis=1)), _bits(full)), "N shards differ from the unsliced columns"
    gb.check_blocks(nso, full, None, None, "stream", prob=prob, what="unsliced", control=False)

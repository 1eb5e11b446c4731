"""The operators BETWEEN the GEMMs (second half of csrc/ns_quant.hip: norm_kernel<true / false>, norm_prep_kernel, silu_kernel, silu_mul2_kernel,
bcast_kernel, dup_kernel / dup_vec4_kernel / dup_transpose_kernel), every kernel variant against a numpy model computed here: fp64 where a bar is
given, exact fp32 where bit equality is asked.  docs/kernels/device_ops.md ("What tests which kernel variant") says which test pins which form.

Bars, and where each comes from:
  * norms against fp64, PER ROW (a wrong row must not hide behind the others): 1e-6 for RMS and for LayerNorm on zero-mean rows, 1e-5 for
    LayerNorm on rows with a mean of two standard deviations (var = sum(x^2) / n - mean^2 cancels) — the bars of
    test_gpu_parity.py::test_elementwise_entries, taken over, not measured.  A correct fp32 norm with a tree-shaped sum stays under 1.3e-7 /
    1.4e-7 / 6.7e-7 on these inputs at widths 299 ... 8192.
  * fp16 shadow: exactly RNE(fp32 output) where the fp32 output is written; with the shadow alone, within 2^-11 relative of fp64 per element
    (half an fp16 ulp), plus 2^-25 absolute: below 2^-14 fp16 is subnormal, its spacing is 2^-24 whatever the value, and a product of two
    normal deviates lands there a few times in 10^4 elements (20 of the 36 cases below hold such cells and 18 miss a bare 2^-11 there, as any fp16 writer would).
    MEASURED, LayerNorm on the rows with a mean only: a correct kernel misses that bound at 1 cell of 2 x 4096 and 3 cells of 2 x 8192, where
    x - mean nearly cancels and the rounding of the fp32 mean (half an ulp of 6 is 2.4e-7, 8e-8 of the row's deviation) is no longer small
    beside the cell.  norm_kernel's summation order restated in numpy fp32 (per-thread strided sums, 64-lane butterfly, four wave sums left to
    right; it reproduces the GPU's per-row errors to every printed digit) misses fp16 rounding of fp64 by at most 5.5e-8 x |gamma| on these
    inputs; the bar for those rows adds 2 x that, SHADOW_MEAN_SLACK x |gamma|.  Every other shadow-alone case holds the bound as stated.
  * fused outputs (gamma, shadow, out_plain of the lazy pair) against the separate operators: bit for bit, on the register-cached AND on the
    load-per-iteration form.  (Both launches must take the same form: the two forms add the row's squares in a different order.)
  * norm_prep: x16 == float16(float32(x) * float32(gamma)) exactly; the sum of squares per 16-column tile == the 16-lane butterfly restated in
    numpy fp32, bit for bit (the file is compiled with -ffp-contract=off).
  * SiLU against fp64 x / (1 + exp(-x)) per element: |err| <= 1e-6 * max(1, |ref|), the bar of test_gpu_parity.py::test_device_silu_and_dup.
  * broadcast add / mul and the strided copy: exact.
Each load-per-iteration case asserts the launcher's selecting condition (width, alignment of the data_ptr()) instead of trusting the allocator.
So does each fused multiply: lazy_mul_plan's condition, restated in lazy_mul_form, must say that the recorded node is consumed by the fused kernel.
The gpu mark sits on each test, not on the module: the last two tests need no GPU.  One shows that the per-row and per-tile checks have teeth, the other
holds norm_restated, the restatement the measured slack comes from, and measures it again.
"""
import ctypes as C

import numpy as np
import pytest

RMS_BAR = 1e-6        # test_elementwise_entries: RMS against fp64
LN_BAR = 1e-6         # LayerNorm, zero-mean rows (the same test's bar for RMS; its LayerNorm bar is the next one)
LN_MEAN_BAR = 1e-5    # test_elementwise_entries: LayerNorm against fp64
SHADOW_MEAN_SLACK = 2 * 5.501e-8  # x |gamma|; LayerNorm rows with a mean, shadow alone: 2 x what the restatement measures (header, last test)
SILU_BAR = 1e-6       # test_device_silu_and_dup
SENT = -77.0          # sentinel behind and between outputs (exact in fp16 and fp32)


# ---- assertion helpers (the CPU self-check at the end of the file imports nothing else) ---------------------------------------------------
def row_errors(out, ref):
    """rel_l2 of each row against the fp64 model"""
    out, ref = np.asarray(out, np.float64), np.asarray(ref, np.float64)
    return np.sqrt(((out - ref) ** 2).sum(-1) / np.maximum((ref ** 2).sum(-1), 1e-300))


def failing_rows(out, ref, bar):
    """indices of the rows whose rel_l2 reaches the bar (NaN fails)"""
    return [int(r) for r in np.nonzero(~(row_errors(out, ref) < bar))[0]]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def differing_cells(got, want):
    """indices of the cells that do not hold the wanted BITS (so -0.0 != 0.0 and a NaN equals itself)"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    return [tuple(int(i) for i in w) for w in np.argwhere(bits(got) != bits(want))]


def tile_ssq(x, n):
    """norm_prep_kernel's sum of squares per 16-column tile, restated: t = x * x in fp32, then the four levels of the 16-lane xor butterfly
    (lane 0 ends up with ((t0 + t1) + (t2 + t3)) + ... : pairwise); columns past n count as 0"""
    x = np.asarray(x, np.float32)[:, :n]
    tiles = (n + 15) // 16
    t = np.zeros((x.shape[0], tiles * 16), np.float32)
    t[:, :n] = x * x
    for _ in range(4):
        t = t[:, 0::2] + t[:, 1::2]
    assert t.dtype == np.float32 and t.shape == (x.shape[0], tiles)
    return t


def shadow_errors(h, ref, slack=0.0):
    """cells of an fp16 shadow written WITHOUT its fp32 twin that are further from fp64 than fp16 rounding allows (slack: what the fp32 value
    under the rounding may be off by, per cell — see SHADOW_MEAN_SLACK)"""
    h, ref = np.asarray(h, np.float64), np.asarray(ref, np.float64)
    return [tuple(int(i) for i in w) for w in np.argwhere(~(np.abs(h - ref) <= 2.0 ** -11 * np.abs(ref) + 2.0 ** -25 + slack))]


# ---- inputs and fp64 models --------------------------------------------------------------------------------------------------------------
def scale_rows(a):
    """one row scaled by 1e-3 and one by 1e3 (in every 2-D tensor with two rows or more): a sum that leaks between rows shows"""
    a = np.array(a, np.float32)
    if a.ndim == 2 and a.shape[0] >= 2:
        a[0] *= np.float32(1e-3)
        a[1] *= np.float32(1e3)
    return a


def norm_input(rows, cols, with_mean, seed):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((rows, cols)) * 3).astype(np.float32)
    if with_mean:
        x = x + np.float32(6)
    return scale_rows(x), rng.standard_normal(cols).astype(np.float32)


def norm_f64(x, isrms, eps):
    x = np.asarray(x, np.float64)
    eps = float(np.float32(eps))
    if isrms:
        return x / np.sqrt((x * x).mean(-1, keepdims=True) + eps)
    return (x - x.mean(-1, keepdims=True)) / np.sqrt(x.var(-1, keepdims=True) + eps)


def takes_cached(cols, *ptrs16, out16=0, gamma=0):
    """launch_rmsnorm / launch_rmsnorm_mul2: the register-cached form needs a row of at most 4096 floats, a multiple of 4, 16-byte aligned fp32
    pointers, an 8-byte aligned fp16 pointer and a 4-byte aligned gamma (NULL counts as aligned)"""
    return cols <= 4096 and cols % 4 == 0 and all(p % 16 == 0 for p in ptrs16) and out16 % 8 == 0 and gamma % 4 == 0


# ---- device plumbing ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def fns(L):
    vp, ll4, i, f, b = C.c_void_p, C.POINTER(C.c_longlong), C.c_int, C.c_float, C.c_bool
    L.ns_hip_lazy_flush.restype = C.c_int
    L.ns_hip_lazy_rms_norm.argtypes = [i, i, f, vp, vp, vp]
    L.ns_hip_lazy_silu.argtypes = [vp, vp, C.c_size_t, vp]
    L.ns_hip_lazy_mul.argtypes = [vp, vp, vp, ll4, ll4, ll4, ll4, ll4, vp]
    L.ns_hip_binary_nd_f32.argtypes = [i, vp, vp, vp, ll4, ll4, ll4, ll4, ll4, vp]
    L.ns_hip_layernormalization.argtypes = [i, i, b, f, vp, vp, vp]
    L.ns_hip_norm_mul_h.argtypes = [i, i, b, f, vp, vp, vp, vp, vp]
    L.ns_hip_norm_prep.argtypes = [i, i, vp, i, vp, vp, vp, i, vp]
    L.ns_hip_silu_f32.argtypes = [vp, vp, C.c_size_t, vp]
    L.ns_hip_mul.argtypes = [i, i, vp, vp, i, vp, vp]
    L.ns_hip_add.argtypes = [i, i, vp, vp, i, vp, vp]
    L.ns_hip_dup_f32.argtypes = [vp, vp, ll4, ll4, ll4, b, vp]
    return L


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ll(*v):
    return (C.c_longlong * 4)(*v)


def _dims(t):
    ne = list(reversed(t.shape)) + [1] * (4 - t.dim())
    nb, s = [], 4
    for e in ne:
        nb.append(s)
        s *= e
    return _ll(*ne), _ll(*nb)


def _packed(ne, nb):
    return nb[0] == 4 and nb[1] == 4 * ne[0] and nb[2] == nb[1] * ne[1] and nb[3] == nb[2] * ne[2]


def lazy_mul_form(node, a, b, d, ne0, nb0, ne1, nb1, nbd):
    """lazy_mul_plan (ns_device_plan.cpp) restated: what ns_hip_lazy_mul makes of the recorded node (kind 1 rms norm / 2 silu, src, dst, cols, n; on the
    multiply's stream) — "norm_mul" (norm_kernel with out_plain), "silu_first" / "silu_second" (silu_mul2_kernel) or "plain" (the node's own kernel,
    then the plain multiply)"""
    kind, src, dst, cols, n = node
    if not kind or not a or not b or not d or not _packed(ne0, nb0) or not _packed(ne0, nbd):
        return "plain"
    if d == src or d == dst or ne0[0] * ne0[1] * ne0[2] * ne0[3] != n:
        return "plain"
    if kind == 1 and a == dst and ne0[0] == cols and ne1[0] == cols and ne1[1] <= 1 and ne1[2] <= 1 and ne1[3] <= 1 and nb1[0] == 4:
        return "norm_mul"
    same_shape = all(ne1[i] == ne0[i] for i in range(4)) and _packed(ne1, nb1)
    if kind == 2 and same_shape and (a == dst) != (b == dst):
        return "silu_first" if a == dst else "silu_second"
    return "plain"


def _nd_mul(fn, a, b, d, st, is_mul=None, node=None, form=None):
    """a * b -> d through ns_hip_lazy_mul (is_mul None; `node` is what was recorded, `form` what the multiply must make of it — asserted from the
    arguments as they are passed) or ns_hip_binary_nd_f32.  b has a's shape or is a row vector: only a dimension that is really broadcast gets a
    stride of 0, an operand of a's shape keeps its packed strides (lazy_mul_plan asks for them before it fuses a recorded silu)."""
    ne0, nb0 = _dims(a)
    ne1, nb1 = _dims(b)
    nb1 = _ll(*[0 if (i > 0 and ne1[i] == 1 and ne0[i] != 1) else nb1[i] for i in range(4)])
    _, nbd = _dims(d)
    if form is not None:
        assert lazy_mul_form(node, a.data_ptr(), b.data_ptr(), d.data_ptr(), ne0, nb0, ne1, nb1, nbd) == form
    args = [a.data_ptr(), b.data_ptr(), d.data_ptr(), ne0, nb0, ne1, nb1, nbd, st]
    return fn(*([is_mul] + args if is_mul is not None else args))


class Out:
    """a (rows, cols) device output with one more row of sentinels behind it and `lead` elements of sentinels in front (lead > 0 misaligns it)"""

    def __init__(self, rows, cols, dtype, lead=0):
        import torch
        self.rows, self.cols, self.lead = rows, cols, lead
        self.flat = torch.full((lead + (rows + 1) * cols,), SENT, dtype=dtype, device="cuda")
        self.t = self.flat[lead:lead + rows * cols].view(rows, cols)

    def ptr(self):
        return self.t.data_ptr()

    def get(self):
        """the rows; the sentinels in front and behind must have survived"""
        a = self.flat.cpu().numpy()
        guard = np.concatenate([a[:self.lead], a[self.lead + self.rows * self.cols:]])
        assert guard.size == self.lead + self.cols and np.all(guard == SENT), "written outside the rows"
        return a[self.lead:self.lead + self.rows * self.cols].reshape(self.rows, self.cols)


def _dev_in(a, lead=0):
    """a on the device, `lead` floats behind an aligned address"""
    import torch
    flat = torch.zeros((lead + a.size,), dtype=torch.float32, device="cuda")
    t = flat[lead:lead + a.size].view(*a.shape)
    t.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return t


# ---- norms -------------------------------------------------------------------------------------------------------------------------------
# (name, rows, cols, floats in front of the input, halfs in front of the fp16 output, cached form for [calls without fp16, calls with fp16])
NORM_CASES = [
    ("3x4", 3, 4, 0, 0, (True, True)),
    ("5x300", 5, 300, 0, 0, (True, True)),
    ("2x4096", 2, 4096, 0, 0, (True, True)),
    ("3x299-width-not-4n", 3, 299, 0, 0, (False, False)),
    ("2x4100-over-the-limit", 2, 4100, 0, 0, (False, False)),
    ("2x5120", 2, 5120, 0, 0, (False, False)),
    ("2x8192", 2, 8192, 0, 0, (False, False)),
    ("3x1024-input-off-one-float", 3, 1024, 1, 0, (False, False)),
    ("3x1024-fp16-off-two-bytes", 3, 1024, 0, 1, (True, False)),
]


@pytest.mark.gpu
@pytest.mark.parametrize("with_mean", [False, True], ids=["zero-mean", "mean-2-sigma"])
@pytest.mark.parametrize("isrms", [True, False], ids=["rms", "layernorm"])
@pytest.mark.parametrize("case", NORM_CASES, ids=[c[0] for c in NORM_CASES])
def test_norm_forms_and_outputs_against_fp64_per_row(fns, pkg, case, isrms, with_mean):
    """plain, gamma, gamma + fp16 shadow, the shadow alone and (RMS) the lazy pair's two tensors: each row against fp64, the fused outputs bit for
    bit against the separate operators, nothing written outside the rows — on the form the case is meant to take."""
    import torch
    L, st = fns, _stream()
    name, rows, cols, in_lead, h_lead, (cached32, cached16) = case
    eps = 1e-6 if isrms else 1e-5
    x, gam = norm_input(rows, cols, with_mean, seed=cols * 4 + rows + 2 * isrms + with_mean)
    dx, dg = _dev_in(x, in_lead), _dev_in(gam)
    bar = RMS_BAR if isrms else (LN_MEAN_BAR if with_mean else LN_BAR)
    ref = norm_f64(x, isrms, eps)
    refg = ref * gam.astype(np.float64)
    prodg = lambda a: a * gam  # exact fp32 product, as the separate multiply computes it

    plain, og, ogs, o16, s16, prod = (Out(rows, cols, torch.float32), Out(rows, cols, torch.float32), Out(rows, cols, torch.float32),
                                      Out(rows, cols, torch.float16, h_lead), Out(rows, cols, torch.float16, h_lead), Out(rows, cols, torch.float32))
    # the form each call takes, from the launcher's own condition
    assert takes_cached(cols, dx.data_ptr(), plain.ptr()) == cached32, name
    assert takes_cached(cols, dx.data_ptr(), og.ptr(), gamma=dg.data_ptr()) == cached32, name
    assert takes_cached(cols, dx.data_ptr(), ogs.ptr(), out16=o16.ptr(), gamma=dg.data_ptr()) == cached16, name
    assert takes_cached(cols, dx.data_ptr(), 0, out16=s16.ptr(), gamma=dg.data_ptr()) == cached16, name
    if in_lead:
        assert dx.data_ptr() % 16 == 4
    if h_lead:
        assert o16.ptr() % 8 == 2 and s16.ptr() % 8 == 2

    pkg.check(L.ns_hip_layernormalization(rows, cols, isrms, eps, dx.data_ptr(), plain.ptr(), st))
    pkg.check(L.ns_hip_norm_mul_h(rows, cols, isrms, eps, dx.data_ptr(), dg.data_ptr(), og.ptr(), None, st))
    pkg.check(L.ns_hip_norm_mul_h(rows, cols, isrms, eps, dx.data_ptr(), dg.data_ptr(), ogs.ptr(), o16.ptr(), st))
    pkg.check(L.ns_hip_norm_mul_h(rows, cols, isrms, eps, dx.data_ptr(), dg.data_ptr(), None, s16.ptr(), st))
    pkg.check(L.ns_hip_mul(rows, cols, plain.ptr(), dg.data_ptr(), 0, prod.ptr(), st))
    torch.cuda.synchronize()
    a_plain, a_og, a_ogs, a_o16, a_s16, a_prod = plain.get(), og.get(), ogs.get(), o16.get(), s16.get(), prod.get()
    got = {"plain": (a_plain, ref), "gamma": (a_og, refg), "gamma+shadow": (a_ogs, refg)}

    if isrms:  # the lazy pair: recorded norm, then the multiply that consumes it — one launch writing out_plain and the product
        la, lb = Out(rows, cols, torch.float32), Out(rows, cols, torch.float32)
        assert takes_cached(cols, dx.data_ptr(), la.ptr(), lb.ptr(), gamma=dg.data_ptr()) == cached32, name
        pkg.check(L.ns_hip_lazy_rms_norm(rows, cols, eps, dx.data_ptr(), la.ptr(), st))
        pkg.check(_nd_mul(L.ns_hip_lazy_mul, la.t, dg, lb.t, st, node=(1, dx.data_ptr(), la.ptr(), cols, rows * cols), form="norm_mul"))
        torch.cuda.synchronize()
        a_la, a_lb = la.get(), lb.get()
        got["lazy out_plain"], got["lazy product"] = (a_la, ref), (a_lb, refg)

    errs = {k: row_errors(o, r) for k, (o, r) in got.items()}
    print("ELEMENTWISE norm %s %s %s: worst row %s (bar %.0e)" % (name, "rms" if isrms else "layernorm", "mean" if with_mean else "zero-mean",
                                                                 ", ".join("%s %.3g" % (k, e.max()) for k, e in errs.items()), bar))
    for k, (o, r) in got.items():
        assert failing_rows(o, r, bar) == [], (k, errs[k])
    # fp16 shadow: the rounding of the fp32 output beside it; alone, the same bits — and fp64 within fp16's rounding
    assert differing_cells(a_o16, a_ogs.astype(np.float16)) == []
    assert differing_cells(a_s16, a_o16) == []
    assert shadow_errors(a_s16, refg, SHADOW_MEAN_SLACK * np.abs(gam) if with_mean and not isrms else 0.0) == []
    # fused == separate, bit for bit (where both launches take the same form: the fp16-off-two-bytes case moves only the calls with a shadow)
    assert differing_cells(a_prod, prodg(a_plain)) == []  # bcast_kernel itself, vstep 0
    assert differing_cells(a_og, a_prod) == []
    if cached32 == cached16:
        assert differing_cells(a_ogs, a_prod) == []
    if isrms:
        assert differing_cells(a_la, a_plain) == [] and differing_cells(a_lb, a_prod) == []


# ---- norm_prep ---------------------------------------------------------------------------------------------------------------------------
PREP_SHAPES = [(1, 4096, 4096), (3, 1000, 1000), (2, 40, 48), (1, 16, 16)]
PREP_VARIANTS = ["all", "no-gamma", "no-x16", "no-ssq", "wide-ssq-stride"]


@pytest.mark.gpu
@pytest.mark.parametrize("variant", PREP_VARIANTS)
@pytest.mark.parametrize("m,n,ldx", PREP_SHAPES)
def test_norm_prep_shadow_and_tile_sums_bit_for_bit(fns, pkg, m, n, ldx, variant):
    import torch
    L, st = fns, _stream()
    rng = np.random.default_rng(n + ldx + m)
    x = scale_rows((rng.standard_normal((m, ldx)) * 3).astype(np.float32))  # (the padding columns hold numbers too: they must not be read into a sum)
    gam = rng.standard_normal(n).astype(np.float32)
    tiles = (n + 15) // 16
    stride = tiles + 3 if variant == "wide-ssq-stride" else tiles
    dx, dg = _dev_in(x), _dev_in(gam)
    x16, ssq = Out(m, ldx, torch.float16), Out(m, stride, torch.float32)
    pkg.check(L.ns_hip_norm_prep(m, n, dx.data_ptr(), ldx, None if variant == "no-gamma" else dg.data_ptr(), None if variant == "no-x16" else x16.ptr(),
                                 None if variant == "no-ssq" else ssq.ptr(), stride, st))
    torch.cuda.synchronize()
    a16, assq = x16.get(), ssq.get()
    want16 = np.full((m, ldx), SENT, np.float16)
    if variant != "no-x16":
        with np.errstate(over="ignore"):  # (the row scaled by 1e3 may pass fp16's largest number: infinity on both sides)
            want16[:, :n] = (x[:, :n] if variant == "no-gamma" else x[:, :n] * gam).astype(np.float16)
    wantssq = np.full((m, stride), SENT, np.float32)
    if variant != "no-ssq":
        wantssq[:, :tiles] = tile_ssq(x, n)
    assert differing_cells(a16, want16) == []       # the shadow, and the sentinels in the padding columns n <= col < ldx
    assert differing_cells(assq, wantssq) == []     # every tile's sum, and the sentinels in the unused tail of each row


# ---- SiLU --------------------------------------------------------------------------------------------------------------------------------
SILU_FIXED = [0.0, -0.0, 1e-30, -1e-30, 20.0, -20.0, 88.0, -88.0, 100.0, -100.0, 1e4, -1e4]


def silu_input(n):
    """the fixed points, rotated by n, then N(0, 4^2); a vector shorter than the list holds its first n only (n = 1: one of them — the test runs the
    others as launches of their own)"""
    rng = np.random.default_rng(n)
    x = (rng.standard_normal(max(n, len(SILU_FIXED))) * 4).astype(np.float32)
    x[:len(SILU_FIXED)] = np.roll(np.array(SILU_FIXED, np.float32), -(n % len(SILU_FIXED) + 3))  # (n = 1 starts at 20: a product that is not a zero)
    return x[:n], rng.standard_normal(n).astype(np.float32)


def silu_f64(x):
    x = np.asarray(x, np.float64)
    with np.errstate(over="ignore"):
        return x / (1 + np.exp(-x))


def silu_failures(x, got):
    """elements off the fp64 model by more than the bar, or — at x <= -100, where expf(-x) overflows or nearly does — anything but a zero or a
    subnormal carrying the minus sign"""
    ref = silu_f64(x)
    bad = ~(np.abs(got.astype(np.float64) - ref) <= SILU_BAR * np.maximum(1.0, np.abs(ref)))
    big_neg = x <= -100
    bad |= big_neg & ~(np.signbit(got) & (np.abs(got) < np.finfo(np.float32).tiny))
    return [int(i) for i in np.nonzero(bad)[0]]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 255, 256, 257, 5000])
def test_silu_alone_and_fused_with_the_product(fns, pkg, n):
    import torch
    L, st = fns, _stream()
    x, up = silu_input(n)
    dx, dup = _dev_in(x), _dev_in(up)
    s, p = Out(1, n, torch.float32), Out(1, n, torch.float32)
    pkg.check(L.ns_hip_silu_f32(dx.data_ptr(), s.ptr(), n, st))
    pkg.check(_nd_mul(L.ns_hip_binary_nd_f32, s.t[0], dup, p.t[0], st, 1))
    torch.cuda.synchronize()
    a_s, a_p = s.get()[0], p.get()[0]
    assert silu_failures(x, a_s) == []
    assert differing_cells(a_p, a_s * up) == []
    for silu_first in (True, False):  # the recorded silu and the multiply that consumes it: silu_mul2_kernel, asserted from the multiply's arguments
        fs, fp = Out(1, n, torch.float32), Out(1, n, torch.float32)
        node = (2, dx.data_ptr(), fs.ptr(), 0, n)
        pkg.check(L.ns_hip_lazy_silu(dx.data_ptr(), fs.ptr(), n, st))
        pkg.check(_nd_mul(L.ns_hip_lazy_mul, fs.t[0], dup, fp.t[0], st, node=node, form="silu_first") if silu_first else
                  _nd_mul(L.ns_hip_lazy_mul, dup, fs.t[0], fp.t[0], st, node=node, form="silu_second"))
        torch.cuda.synchronize()
        assert differing_cells(fs.get()[0], a_s) == [], silu_first
        assert differing_cells(fp.get()[0], a_p) == [], silu_first
    if n == 1:  # a vector of one element starts at one fixed point only: every fixed point as a launch of one element
        for v in SILU_FIXED:
            one = np.array([v], np.float32)
            d1, o = _dev_in(one), Out(1, 1, torch.float32)
            pkg.check(L.ns_hip_silu_f32(d1.data_ptr(), o.ptr(), 1, st))
            torch.cuda.synchronize()
            assert silu_failures(one, o.get()[0]) == [], v


# ---- broadcast add / mul -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("batch,vsize,vstep", [(5, 300, 0), (5, 300, 300), (4, 33, 40), (1, 1, 0), (3, 4097, 4097)])
def test_broadcast_add_and_mul_are_exact(fns, pkg, batch, vsize, vstep):
    import torch
    L, st = fns, _stream()
    rng = np.random.default_rng(batch * 7 + vsize + vstep)
    t = scale_rows(rng.standard_normal((batch, vsize)).astype(np.float32))
    v = rng.standard_normal((batch - 1) * vstep + vsize).astype(np.float32)
    if vstep:  # a row of its own per batch entry (vstep >= vsize: they do not overlap), two of them scaled
        for b, s in ((0, 1e-3), (1, 1e3)):
            v[b * vstep:b * vstep + vsize] *= np.float32(s)
    vrows = np.stack([v[b * vstep:b * vstep + vsize] for b in range(batch)])
    dt, dv = _dev_in(t), _dev_in(v)
    for fn, want in ((L.ns_hip_mul, t * vrows), (L.ns_hip_add, t + vrows)):
        o = Out(batch, vsize, torch.float32)
        pkg.check(fn(batch, vsize, dt.data_ptr(), dv.data_ptr(), vstep, o.ptr(), st))
        torch.cuda.synchronize()
        assert differing_cells(o.get(), want) == []


# ---- strided copy ------------------------------------------------------------------------------------------------------------------------
def dup_form(src_ptr, dst_ptr, ne, snb, dnb, f16):
    """launch_dup's choice outside a replayed route (no moving cache cell, no mirror): "transpose<ax>", "vec4" or "elementwise\""""
    total = ne[0] * ne[1] * ne[2] * ne[3]
    if total >= 1 << 16 and ne[0] >= 32 and dnb[0] == (2 if f16 else 4) and snb[0] != 4:
        for ax in (1, 2, 3):
            if ne[ax] >= 32 and snb[ax] == 4:
                o1, o2 = (2 if ax == 1 else 1), (2 if ax == 3 else 3)
                if ne[o1] * ne[o2] <= 65535:
                    return "transpose%d" % ax
                break
    if (not f16 and total >= 1 << 16 and ne[0] % 4 == 0 and snb[0] == 4 and dnb[0] == 4 and (src_ptr | dst_ptr) % 16 == 0
            and all(ne[i] <= 1 or (snb[i] | dnb[i]) % 16 == 0 for i in (1, 2, 3))):
        return "vec4"
    return "elementwise"


def _dup(L, pkg, src, dst_flat, dst_off_bytes, ne, snb, dnb, f16, form):
    """src (numpy fp32) -> the flat destination array (numpy, sentinels) at a byte offset; returns the destination as it came back"""
    import torch
    dsrc, ddst = torch.from_numpy(src).cuda(), torch.from_numpy(dst_flat).cuda()
    dptr = ddst.data_ptr() + dst_off_bytes
    assert dup_form(dsrc.data_ptr(), dptr, ne, snb, dnb, f16) == form
    pkg.check(L.ns_hip_dup_f32(dsrc.data_ptr(), dptr, _ll(*ne), _ll(*snb), _ll(*dnb), f16, _stream()))
    torch.cuda.synchronize()
    return ddst.cpu().numpy()


@pytest.mark.gpu
def test_transposing_copy_into_an_fp16_v_cache(fns, pkg):
    """the V-cache write of test_prompt_sized_cache_writes_... with dst_is_f16: [position][head][dim] rows into [head][dim][n_ctx] fp16 cells"""
    seq, heads, hs, n_ctx, pos = 70, 16, 64, 96, 5
    v = np.random.default_rng(70).standard_normal((seq, heads, hs)).astype(np.float32)
    vc = np.full((heads, hs, n_ctx), SENT, np.float16)
    got = _dup(fns, pkg, v, vc.reshape(-1), pos * 2, (seq, hs, heads, 1), (heads * hs * 4, 4, hs * 4, seq * heads * hs * 4),
               (2, n_ctx * 2, hs * n_ctx * 2, heads * hs * n_ctx * 2), True, "transpose1")
    vc[:, :, pos:pos + seq] = v.transpose(1, 2, 0).astype(np.float16)
    assert differing_cells(got.reshape(vc.shape), vc) == []


@pytest.mark.gpu
@pytest.mark.parametrize("f16", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("ax,ne", [(2, (40, 3, 600, 1)), (3, (40, 2, 2, 500)), (3, (40, 2, 3, 500))], ids=["2", "3", "3-unequal-z"])
def test_transposing_copy_along_source_axis_2_and_3(fns, pkg, ax, ne, f16):
    """The source runs along destination axis 2 (ne 40, 3, 600, 1) or 3 (ne 40, 2, 2, 500), the destination along axis 0 with a padded leading
    dimension; 40 and 600 / 500 leave ragged 32 x 32 tiles on both axes.  One more slab of sentinels lies behind the destination.  (40, 2, 3, 500)
    gives the two axes that blockIdx.z is taken apart into unequal extents: z % ne[o2] in place of z % ne[o1] shows."""
    ld, es = 44, 2 if f16 else 4
    src = np.random.default_rng(ax).standard_normal(ne).astype(np.float32)  # [i0][i1][i2][i3], C order: i3 contiguous, i2 when ne[3] == 1
    snb = (ne[1] * ne[2] * ne[3] * 4, ne[2] * ne[3] * 4, ne[3] * 4, 4 if ax == 3 else ne[0] * ne[1] * ne[2] * 4)
    dnb = (es, ld * es, ne[1] * ld * es, ne[2] * ne[1] * ld * es)
    dst = np.full((ne[3] + 1, ne[2], ne[1], ld), SENT, np.float16 if f16 else np.float32)  # [i3][i2][i1][i0 padded], and the slab behind
    got = _dup(fns, pkg, src, dst.reshape(-1), 0, ne, snb, dnb, f16, "transpose%d" % ax)
    dst[:ne[3], :, :, :ne[0]] = src.transpose(3, 2, 1, 0).astype(dst.dtype)
    assert differing_cells(got.reshape(dst.shape), dst) == []


@pytest.mark.gpu
@pytest.mark.parametrize("why,form", [("aligned-control", "vec4"), ("dst-off-4-bytes", "elementwise"), ("ne0-66", "elementwise"),
                                      ("fp16-dst", "elementwise")])
def test_what_the_16_byte_copy_refuses_goes_through_the_element_wise_kernel(fns, pkg, why, form):
    """the K-cache write of a prompt ([position][head][dim] rows into [head][n_ctx][dim] cells), eligible for dup_vec4_kernel by size: as it stands
    (the control, which takes the 16-byte form) and in the three ways that form must refuse it — the same cells either way"""
    seq, heads, n_ctx, pos = 70, 16, 96, 5
    hs = 66 if why == "ne0-66" else 64
    f16, lead = why == "fp16-dst", 1 if why == "dst-off-4-bytes" else 0
    es = 2 if f16 else 4
    k = np.random.default_rng(len(why)).standard_normal((seq, heads, hs)).astype(np.float32)
    flat = np.full(lead + heads * n_ctx * hs, SENT, np.float16 if f16 else np.float32)
    ne, snb = (hs, seq, heads, 1), (4, heads * hs * 4, hs * 4, seq * heads * hs * 4)
    dnb = (es, hs * es, n_ctx * hs * es, heads * n_ctx * hs * es)
    got = _dup(fns, pkg, k, flat, (lead + pos * hs) * es, ne, snb, dnb, f16, form)
    want = flat.copy()
    want[lead:].reshape(heads, n_ctx, hs)[:, pos:pos + seq, :] = k.transpose(1, 0, 2).astype(flat.dtype)
    assert differing_cells(got, want) == []


# ---- zero rows, zero elements ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_zero_rows_and_zero_elements_succeed_and_write_nothing(fns, pkg, nso, capfd):
    """norm_count = 0, batch = 0, n = 0, an extent of 0: the reference does nothing and succeeds, and so does every entry here (the norm, the
    broadcast and the column-gather launchers used to ask for a grid of zero workgroups, which the runtime refuses: -1, "norm launch")."""
    import torch
    L, st = fns, _stream()
    src = _dev_in(np.ones((2, 64), np.float32))
    o32, o16, o32b = Out(2, 64, torch.float32), Out(2, 64, torch.float16), Out(2, 64, torch.float32)
    ok = lambda rc, what: pkg.check(rc, what)
    for isrms in (True, False):
        ok(L.ns_hip_layernormalization(0, 64, isrms, 1e-6, src.data_ptr(), o32.ptr(), st), "layernormalization")
        ok(L.ns_hip_norm_mul_h(0, 64, isrms, 1e-6, src.data_ptr(), src.data_ptr(), o32.ptr(), o16.ptr(), st), "norm_mul_h")
        ok(L.ns_hip_norm_mul_h(0, 64, isrms, 1e-6, src.data_ptr(), src.data_ptr(), None, o16.ptr(), st), "norm_mul_h, shadow alone")
    ok(L.ns_hip_lazy_rms_norm(0, 64, 1e-6, src.data_ptr(), o32.ptr(), st), "lazy rms_norm")
    ok(L.ns_hip_lazy_flush(), "lazy flush")
    ok(L.ns_hip_mul(0, 64, src.data_ptr(), src.data_ptr(), 0, o32.ptr(), st), "mul")
    ok(L.ns_hip_add(0, 64, src.data_ptr(), src.data_ptr(), 64, o32.ptr(), st), "add")
    ok(L.ns_hip_silu_f32(src.data_ptr(), o32.ptr(), 0, st), "silu")
    ok(L.ns_hip_lazy_silu(src.data_ptr(), o32.ptr(), 0, st), "lazy silu")
    ok(L.ns_hip_lazy_flush(), "lazy flush")
    ok(L.ns_hip_norm_prep(0, 64, src.data_ptr(), 64, src.data_ptr(), o16.ptr(), o32b.ptr(), 4, st), "norm_prep, m = 0")
    ok(L.ns_hip_norm_prep(2, 0, src.data_ptr(), 64, src.data_ptr(), o16.ptr(), o32b.ptr(), 4, st), "norm_prep, n = 0")
    for f16, o in ((False, o32), (True, o16)):
        es = 2 if f16 else 4
        ok(L.ns_hip_dup_f32(src.data_ptr(), o.ptr(), _ll(64, 0, 1, 1), _ll(4, 256, 512, 512), _ll(es, 64 * es, 128 * es, 128 * es), f16, st), "dup")
    torch.cuda.synchronize()
    for o in (o32, o16, o32b):
        assert np.all(o.get() == SENT)
    # the host-pointer entry: silent for zero rows (it printed "Err: invalid parameters" when the launch was refused)
    x = np.ones((2, 64), np.float32)
    out = np.full((2, 64), SENT, np.float32)
    capfd.readouterr()
    L.bestla_layernormalization(0, 64, True, 1e-6, nso.ptr(x), nso.ptr(out))
    L.bestla_mul(0, 64, nso.ptr(x), nso.ptr(x), 0, nso.ptr(out))
    L.bestla_add(0, 64, nso.ptr(x), nso.ptr(x), 64, nso.ptr(out))
    C.CDLL(None).fflush(None)
    said = capfd.readouterr()
    assert "Err" not in said.out + said.err, said
    assert np.all(out == SENT)


# ---- the per-row and per-tile checks have teeth (no GPU) ---------------------------------------------------------------------------------
def test_one_wrong_row_and_one_wrong_tile_pass_the_tensor_metric_and_fail_these_checks(nso):
    """A row whose sum of squares misses its LAST element (an off-by-one in a tail loop) in a 32 x 4100 RMS norm, and one 16-column tile of the
    quiet row of a norm_prep result that misses its last lane: a whole-tensor rel_l2 < 1e-6 accepts both; the per-row bar and the per-tile bit
    comparison of this file name exactly the row and the tile."""
    rows, cols, eps = 32, 4100, 1e-6
    x, _ = norm_input(rows, cols, False, seed=1)
    ref = norm_f64(x, True, eps)
    good = ref.astype(np.float32)
    assert failing_rows(good, ref, RMS_BAR) == []
    xd = x.astype(np.float64)
    short = xd[:, :-1] ** 2  # the sum without the last element, still divided by n
    wrong_rows = xd / np.sqrt(short.sum(-1, keepdims=True) / cols + eps)
    e_rows = row_errors(wrong_rows, ref)
    cand = [r for r in range(rows) if 1.5e-6 < e_rows[r] < 5e-6]  # a last element small enough for the tensor metric to swallow the row
    assert cand, e_rows
    row = cand[0]
    wrong = good.copy()
    wrong[row] = wrong_rows[row].astype(np.float32)
    e = nso.rel_l2(wrong, ref)
    print("ELEMENTWISE one wrong row: tensor rel_l2 %.3g, row %d at %.3g against the bar %.0e" % (e, row, row_errors(wrong, ref)[row], RMS_BAR))
    assert e < 1e-6, e
    assert failing_rows(wrong, ref, RMS_BAR) == [row]
    # one tile sum of the row scaled by 1e-3, beside a row scaled by 1e3
    m, n = 3, 1000
    xp = scale_rows((np.random.default_rng(2).standard_normal((m, n)) * 3).astype(np.float32))
    ssq = tile_ssq(xp, n)
    assert ssq.shape == (m, 63) and differing_cells(ssq, ssq.copy()) == []
    bad = ssq.copy()
    bad[0, 17] = tile_ssq(np.concatenate([xp[:1, 17 * 16:17 * 16 + 15], np.zeros((1, 1), np.float32)], 1), 16)[0, 0]
    assert bad[0, 17] != ssq[0, 17]
    e = nso.rel_l2(bad, ssq)
    print("ELEMENTWISE one wrong tile: tensor rel_l2 %.3g" % e)
    assert e < 1e-6, e
    assert differing_cells(bad, ssq) == [(0, 17)]
    # and the restatement itself is a sum of squares: against fp64 within the rounding of one product and four adds
    exact = np.pad(xp.astype(np.float64) ** 2, ((0, 0), (0, 8))).reshape(m, 63, 16).sum(-1)
    assert np.all(np.abs(ssq - exact) <= 5 * 2.0 ** -24 * exact)


# ---- where the one measured bar comes from (no GPU) --------------------------------------------------------------------------------------
def norm_restated(x, gam, isrms, eps, cached):
    """norm_kernel<cached> with gamma in numpy fp32, in the kernel's summation order: 256 per-thread sums (cached: four float4 chunks per thread, each
    added as (x + y) + (z + w); else a strided loop), the 64-lane xor butterfly per wave, the four wave sums left to right, then mean, variance,
    1 / sqrt and the two products as the kernel rounds them (no contraction)"""
    f32 = np.float32
    x = np.asarray(x, f32)
    rows, n = x.shape
    out = np.zeros_like(x)

    def wave_sums(a):  # (256,) -> (4,): shfl_xor by 32, 16 ... 1
        a = a.reshape(4, 64)
        for h in (32, 16, 8, 4, 2, 1):
            a = a[:, :h] + a[:, h:2 * h]
        return a[:, 0]

    for r in range(rows):
        row = x[r]
        s, s2 = np.zeros(256, f32), np.zeros(256, f32)
        if cached:
            v = np.zeros(4096, f32)
            v[:n] = row
            for a in v.reshape(4, 256, 4):
                q = a * a
                s = s + ((a[:, 0] + a[:, 1]) + (a[:, 2] + a[:, 3]))
                s2 = s2 + ((q[:, 0] + q[:, 1]) + (q[:, 2] + q[:, 3]))
        else:
            for i0 in range(0, n, 256):
                blk = row[i0:i0 + 256]
                s[:blk.size] = s[:blk.size] + blk
                s2[:blk.size] = s2[:blk.size] + blk * blk
        w, w2 = wave_sums(s), wave_sums(s2)
        tot, tot2 = ((w[0] + w[1]) + w[2]) + w[3], ((w2[0] + w2[1]) + w2[2]) + w2[3]
        mean = tot / f32(n)
        sd = np.sqrt(tot2 / f32(n) + f32(eps)) if isrms else np.sqrt((tot2 / f32(n) - mean * mean) + f32(eps))
        inv = f32(1) / sd
        out[r] = (row * inv if isrms else (row - mean) * inv) * gam
    assert out.dtype == f32
    return out


def test_restated_norm_kernel_meets_the_row_bars_and_gives_the_measured_shadow_slack():
    """The inputs of every norm case above through norm_restated, on the form the calls with an fp16 shadow take: each row under its bar against fp64;
    the fp16 rounding of the result within 2^-11 relative + 2^-25 of fp64 everywhere EXCEPT on LayerNorm rows with a mean, where it overshoots by at
    most 5.5e-8 x |gamma| (x - mean nearly cancels; the fp32 mean carries its rounding) — SHADOW_MEAN_SLACK is 2 x that, and is used on those rows only."""
    worst = {}
    for name, rows, cols, _, _, (_, cached16) in NORM_CASES:
        for isrms in (True, False):
            for with_mean in (False, True):
                eps = 1e-6 if isrms else 1e-5
                x, gam = norm_input(rows, cols, with_mean, seed=cols * 4 + rows + 2 * isrms + with_mean)
                refg = norm_f64(x, isrms, eps) * gam.astype(np.float64)
                y = norm_restated(x, gam, isrms, eps, cached16)
                bar = RMS_BAR if isrms else (LN_MEAN_BAR if with_mean else LN_BAR)
                assert failing_rows(y, refg, bar) == [], (name, isrms, with_mean)
                over = np.abs(y.astype(np.float16).astype(np.float64) - refg) - 2.0 ** -11 * np.abs(refg) - 2.0 ** -25
                key = (isrms, with_mean)
                worst[key] = max(worst.get(key, 0.0), float(np.max(over / np.abs(gam))))
    print("ELEMENTWISE restated norm, worst overshoot of the shadow bound / |gamma|: %s" % worst)
    assert worst[(True, False)] <= 0 and worst[(True, True)] <= 0 and worst[(False, False)] <= 0
    assert 5.0e-8 < worst[(False, True)] < 5.6e-8
    assert 2 * worst[(False, True)] <= SHADOW_MEAN_SLACK <= 2.002 * worst[(False, True)]

"""ns_hip_mul_mat_id (csrc/ns_moe.cpp), every way it serves a call — the decode kernel (one gemv_kernel launch per row, expert picked on
the device), the per-row loop kernel (moe_gemv_kernel<KIND>) and the grouped path (rows sorted by expert on the host, one tiled GEMM per
expert, scatter + epilogue) — each PINNED with ns_hip_set_tuning("moe_gemv_rows" / "moe_grouped_rows") and CONFIRMED with the deltas of
ns_hip_moe_stats, every row against the oracle's fp64 product with that row's expert.

Bars (the project's own, none measured on the code under test): 1e-3 against the fp64 product of the fp32 activations; against the fp64
product of the fp16-rounded activations (what every default kernel multiplies) 5e-5 for the loop kernel (fp32 FMAs on exact weights: only
the summation order differs) and for the decode kernel on integer weights, 6e-4 for the decode kernel on the 4-bit float types (its value
table is rounded to fp16); fp8 experts and the grouped path take TOL / TOL_A16 / TOL_EXACT of tests/test_gpu_gemm3_fp8.py; the epilogue
cases take the bar of tests/test_gpu_gemvs.py::test_epilogues_with_and_without_split_k and its fp64 reference (tanh-form GELU)."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_gemm3_fp8 import TOL, TOL_A16, TOL_EXACT
from test_gpu_gemvs import TOL as TOL_EPI

pytestmark = pytest.mark.gpu

N_AS, TOPK = 4, 2
N, K = 200, 832   # ragged last column tile; 6.5 k-steps of the 128-deep formats (13 of the 64-deep ones)
DECODE, LOOP, GROUPED, REFUSED_THEN_LOOP = (0, 1, 0, 0), (0, 0, 1, 0), (1, 0, 0, 0), (0, 0, 1, 1)   # ns_hip_moe_stats deltas of ONE call
PATHS = {"decode": DECODE, "loop": LOOP, "grouped": GROUPED}
PATH_ROWS = {"decode": 6, "loop": 12, "grouped": 40}   # row counts the default thresholds (8 / 32) send to each path

# qtype, scale dtype, asym, group, core — the scale record of a k-step is (k-step length / group) x sizeof(scale) bytes per column
FORMATS = [
    ("S4", "F32", False, 32, "CORE_AVX512_VNNI_KB"),    # 16-byte scale record
    ("S4", "BF16", False, 32, "CORE_AVX512_VNNI_KB"),   # 8
    ("S4", "F32", True, 128, "CORE_AVX512F"),           # 4, with zero points
    ("S4", "BF16", False, 128, "CORE_AVX512F"),         # 2
    ("S4", "BF16", False, 64, "CORE_AVX512F"),          # g64: two scales per k-step
    ("S4", "F32", False, -1, "CORE_AVX512F"),           # per-channel: ONE scale row (srow_mul / srow_shift)
    ("S4", "F16", False, 32, "CORE_AVX512F"),           # fp16 scales
    ("S8", "BF16", False, 32, "CORE_AVX512_VNNI_KB"),
    ("S8", "F32", True, 32, "CORE_AVX512_VNNI_KB"),     # 8-bit zero points
    ("S3", "BF16", False, 32, "CORE_AVX512_VNNI_KB"),   # widened to nibbles at load
    ("S5", "BF16", False, 32, "CORE_AVX512_VNNI_KB"),   # widened to bytes at load
    ("F4_NF4", "BF16", False, 64, "CORE_AVX512F"),
    ("F4_E2M1", "F32", False, 32, "CORE_AVX512F"),      # another value table
]
F8_FORMATS = [
    ("F8_E4M3", "F32", False, 32, "CORE_AVX512F"),
    ("F8_E5M2", "F8_E8M0", False, 32, "CORE_AVX512F"),
]
S4 = FORMATS[1]
NF4 = FORMATS[11]
EPIS = ["none", "add", "mul", "add_gelu", "gelu", "silu"]


def _fid(f):
    return "%s-%s-g%d%s" % (f[0], f[1], f[3], "-asym" if f[2] else "")


def _cls(qt):
    return "f8" if qt.startswith("F8") else "f4" if qt.startswith("F4") else "int"


def _tol16(path, qt):
    if qt.startswith("F8"):
        return TOL_EXACT if path == "loop" else TOL_A16   # (the decode kernel does not take fp8 experts)
    if path == "grouped":
        return TOL_A16
    return 6e-4 if path == "decode" and qt.startswith("F4") else 5e-5


class _Group:
    def __init__(self, L, pkg, nso, fmt, n, k, n_as, seed):
        qt, st, asym, bs, core = fmt
        rng = np.random.default_rng(seed)
        self.fmt, self.n, self.k, self.n_as = fmt, n, k, n_as
        self.blobs = [nso.quant_pack((rng.standard_normal((n, k)) * 0.05).astype(np.float32), bs, getattr(nso, qt), getattr(nso, st),
                                     asym, getattr(nso, core)) for _ in range(n_as)]
        self.weights = [pkg.Weight.from_host_blob(nso.ptr(b)) for b in self.blobs]
        arr = (C.c_void_p * n_as)(*[w.h for w in self.weights])
        self.g = L.ns_hip_expert_group_create(arr, n_as)
        assert self.g, pkg.last_error()

    def free(self, L):
        L.ns_hip_expert_group_free(self.g)
        for w in self.weights:
            w.free()


@pytest.fixture(scope="module")
def groups(L, pkg, nso):
    """expert groups by (format, n, k), quantised and uploaded once for the whole module"""
    cache = {}

    def get(fmt, n=N, k=K, n_as=N_AS):
        key = (fmt, n, k, n_as)
        if key not in cache:
            cache[key] = _Group(L, pkg, nso, fmt, n, k, n_as, seed=len(cache) + 11)
        return cache[key]

    yield get
    for g in cache.values():
        g.free(L)


@pytest.fixture(autouse=True)
def _default_thresholds(L):
    yield
    assert L.ns_hip_set_tuning(b"moe_gemv_rows", 0) == 0 and L.ns_hip_set_tuning(b"moe_grouped_rows", 0) == 0


def _pin(L, path):
    """default thresholds serve PATH_ROWS as named; any other row count on the loop needs both other paths off"""
    if path == "loop":
        assert L.ns_hip_set_tuning(b"moe_gemv_rows", -1) == 0 and L.ns_hip_set_tuning(b"moe_grouped_rows", -1) == 0


def _stats(L):
    out = (C.c_uint64 * 4)()
    L.ns_hip_moe_stats(out)
    return np.array(list(out), np.int64)


def _ref_rows(nso, grp, a, idcol, a16=False):
    """fp64 product of every row with ITS expert (rows of an id outside the group: zero), one oracle call per expert"""
    ref = np.zeros((a.shape[0], grp.n))
    for e in range(grp.n_as):
        rows = np.nonzero(idcol == e)[0]
        if rows.size:
            ref[rows] = nso.gemm_f64(a[rows], grp.blobs[e], a16=a16)
    return ref


def _gelu(v):
    return 0.5 * v * (1.0 + np.tanh(0.7978845834732056 * (v + 0.044714998453855515 * v ** 3)))


def _epi_ref(epi, x, d):
    d = None if d is None else d.astype(np.float64)
    return {"none": lambda: x, "add": lambda: x + d, "mul": lambda: x * d, "add_gelu": lambda: _gelu(x + d), "gelu": lambda: _gelu(x),
            "silu": lambda: x / (1.0 + np.exp(-x))}[epi]()


def _epi_code(pkg, epi):
    return {"none": pkg.EPI_NONE, "add": pkg.EPI_ADD, "mul": pkg.EPI_MUL, "add_gelu": pkg.EPI_ADD_GELU, "gelu": pkg.EPI_GELU,
            "silu": pkg.EPI_SILU}[epi]


def _call(L, pkg, grp, a, ids, sel, expect, epi="none", d=None, pad_a=0, pad_c=0, pad_d=0):
    """one ns_hip_mul_mat_id call on the current stream; asserts the stats deltas `expect` and that nothing was written beyond column n;
    -> fp32 [m][n].  Padding columns of A hold 1000 (a kernel that read them would miss every bar), those of C hold 7."""
    import torch
    m, k, n = a.shape[0], grp.k, grp.n
    ah = np.full((m, k + pad_a), 1000.0, np.float32)
    ah[:, :k] = a
    dA, dI = torch.from_numpy(ah).cuda(), torch.from_numpy(np.ascontiguousarray(ids, np.int32)).cuda()
    dC = torch.full((m, n + pad_c), 7.0, device="cuda")
    dD = None
    if d is not None:
        dh = np.full((m, n + pad_d), -3.0, np.float32)
        dh[:, :n] = d
        dD = torch.from_numpy(dh).cuda()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    s0 = _stats(L)
    pkg.check(L.ns_hip_mul_mat_id(dA.data_ptr(), dI.data_ptr(), ids.shape[1], sel, grp.g, dC.data_ptr(), m, k + pad_a, n + pad_c,
                                  _epi_code(pkg, epi), dD.data_ptr() if dD is not None else None, n + pad_d, st))
    torch.cuda.synchronize()
    delta = tuple(int(v) for v in _stats(L) - s0)
    assert delta == expect, ("served by (grouped, decode, loop, grouped refused) = %s, expected %s" % (delta, expect))
    out = dC.cpu().numpy()
    assert np.all(out[:, n:] == 7.0)
    return out[:, :n]


def _inputs(seed, m, k, n_as=N_AS, width=TOPK):
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((m, k)).astype(np.float32)
    ids = rng.integers(0, n_as, size=(m, width)).astype(np.int32)
    return rng, a, ids


def _check(nso, tag, path, grp, out, a, idcol):
    qt = grp.fmt[0]
    e = nso.rel_l2(out, _ref_rows(nso, grp, a, idcol))
    e16 = nso.rel_l2(out, _ref_rows(nso, grp, a, idcol, a16=True))
    print("moe %s path=%s class=%s %s m=%d n=%d k=%d rel_l2 %.3g a16 %.3g" % (tag, path, _cls(qt), _fid(grp.fmt), a.shape[0], grp.n, grp.k, e, e16))
    assert e < TOL and e16 < _tol16(path, qt), (tag, path, _fid(grp.fmt), a.shape[0], e, e16)


# ---------------------------------------------------------------------------------------------------------------- the loop kernel
@pytest.mark.parametrize("fmt", FORMATS + F8_FORMATS, ids=_fid)
def test_loop_kernel_every_format(L, pkg, nso, groups, fmt):
    """moe_gemv_kernel<WK_INT4 / WK_INT8 / WK_F4 / WK_F8>: the four scale-record widths of fetch_corr, zero points, the one-row scale
    index of per-channel weights, fp16 scales, both value tables, both fp8 encodings; 1 row .. 31 rows"""
    grp = groups(fmt)
    _pin(L, "loop")
    for m in (1, 9, 20, 31):
        _, a, ids = _inputs(100 + m, m, K)
        out = _call(L, pkg, grp, a, ids, 1, LOOP)
        _check(nso, "formats", "loop", grp, out, a, ids[:, 1])


def _ksteps(wt, fmt):
    """k-steps of a loaded weight, from its device footprint (ns_hip_weight_info): [tiles][k-steps] records of 1024 code bytes, with the
    k-step's scales (and zero points) behind them when every k-step has its own scale row"""
    qt, st, asym, bs, _ = fmt
    kstep_len = 64 if wt.bits > 4 else 128
    assert 0 < bs <= kstep_len
    sps = kstep_len // bs
    rec = 1024 + 16 * sps * (4 if st == "F32" else 2) + (16 * sps if asym else 0)
    tiles = (wt.n + 15) // 16
    assert wt.device_bytes % (tiles * rec) == 0
    return wt.device_bytes // (tiles * rec), kstep_len


@pytest.mark.parametrize("fmt", [FORMATS[1], FORMATS[7], NF4], ids=_fid)
def test_loop_kernel_second_pass_with_one_live_slot(L, pkg, nso, groups, fmt):
    """more than 4 x 8 k-steps: the outer loop's second pass, where wave 0 alone has a record (the 33rd) and three of its four slots are
    dead.  K = 33 k-steps of the format's own depth, read back from a loaded weight, not assumed"""
    probe = groups(fmt)
    steps, kstep_len = _ksteps(probe.weights[0], fmt)
    assert steps == (K + kstep_len - 1) // kstep_len
    k = 33 * kstep_len
    grp = groups(fmt, n=48, k=k)
    assert _ksteps(grp.weights[0], fmt)[0] == 33
    if grp.weights[0].bits <= 4:
        assert k == 4224
    assert max(b.size for b in grp.blobs) < (1 << 20)
    _pin(L, "loop")
    _, a, ids = _inputs(7, 9, k)
    out = _call(L, pkg, grp, a, ids, 0, LOOP)
    _check(nso, "33 k-steps", "loop", grp, out, a, ids[:, 0])


# ---------------------------------------------------------------------------------------------------------------- the decode kernel
@pytest.mark.parametrize("fmt", FORMATS, ids=_fid)
def test_decode_kernel_every_format(L, pkg, nso, groups, fmt):
    grp = groups(fmt)
    for m in (1, 8):
        _, a, ids = _inputs(200 + m, m, K)
        out = _call(L, pkg, grp, a, ids, 1, DECODE)
        _check(nso, "formats", "decode", grp, out, a, ids[:, 1])


# ---------------------------------------------------------------------------------------------------------------- boundaries, arguments
def test_row_count_boundaries_at_the_default_thresholds(L, pkg, nso, groups):
    grp = groups(S4)
    for m, path in ((8, "decode"), (9, "loop"), (31, "loop"), (32, "grouped")):
        _, a, ids = _inputs(300 + m, m, K)
        out = _call(L, pkg, grp, a, ids, 0, PATHS[path])
        _check(nso, "boundary", path, grp, out, a, ids[:, 0])


def test_threshold_keys_zero_is_the_default_negative_is_off(L, pkg, nso, groups):
    grp = groups(S4)
    _, a, ids = _inputs(310, 20, K)
    for key, value, m, expect in ((b"moe_gemv_rows", 20, 20, DECODE), (b"moe_gemv_rows", -1, 4, LOOP), (b"moe_gemv_rows", 0, 8, DECODE),
                                  (b"moe_gemv_rows", 0, 9, LOOP), (b"moe_grouped_rows", 16, 20, GROUPED), (b"moe_grouped_rows", -1, 20, LOOP),
                                  (b"moe_grouped_rows", 0, 20, LOOP)):
        assert L.ns_hip_set_tuning(key, value) == 0
        out = _call(L, pkg, grp, a[:m], ids[:m], 1, expect)
        path = [p for p, v in PATHS.items() if v == expect][0]
        _check(nso, "keys", path, grp, out, a[:m], ids[:m, 1])
    _, a, ids = _inputs(311, 32, K)
    out = _call(L, pkg, grp, a, ids, 1, GROUPED)   # both back at their defaults
    _check(nso, "keys", "grouped", grp, out, a, ids[:, 1])


@pytest.mark.parametrize("path", ["decode", "loop", "grouped"])
def test_strides_and_id_column(L, pkg, nso, groups, path):
    """ids_stride = 3 with id = 2 (the other two columns name OTHER experts), lda = k + 4, ldc = n + 3 (columns beyond n keep their fill),
    ldd = n + 5 with the Add epilogue"""
    grp = groups(S4)
    m = PATH_ROWS[path]
    rng, a, ids = _inputs(320 + m, m, K, width=3)
    ids[:, 0] = (ids[:, 2] + 1) % N_AS
    ids[:, 1] = (ids[:, 2] + 2) % N_AS
    d = rng.standard_normal((m, N)).astype(np.float32)
    out = _call(L, pkg, grp, a, ids, 2, PATHS[path], epi="add", d=d, pad_a=4, pad_c=3, pad_d=5)
    x = _ref_rows(nso, grp, a, ids[:, 2])
    e = nso.rel_l2(out, x + d)
    print("moe strides path=%s rel_l2 %.3g" % (path, e))
    assert e < TOL_EPI
    out = _call(L, pkg, grp, a, ids, 2, PATHS[path], pad_a=4, pad_c=3)
    _check(nso, "strides", path, grp, out, a, ids[:, 2])


def test_unaligned_lda_is_refused_by_the_decode_kernel_and_served_by_the_loop(L, pkg, nso, groups):
    grp = groups(S4)
    _, a, ids = _inputs(330, 4, K)
    out = _call(L, pkg, grp, a, ids, 0, LOOP, pad_a=1)   # (rows of lda = k + 1 floats are not 16-byte aligned)
    _check(nso, "lda = k + 1", "loop", grp, out, a, ids[:, 0])


# ---------------------------------------------------------------------------------------------------------------- epilogues
@pytest.mark.parametrize("epi", EPIS)
@pytest.mark.parametrize("fmt", [S4, NF4], ids=_fid)
@pytest.mark.parametrize("path", ["decode", "loop", "grouped"])
def test_epilogues_on_every_path(L, pkg, nso, groups, path, fmt, epi):
    grp = groups(fmt)
    m = PATH_ROWS[path]
    rng, a, ids = _inputs(400 + m, m, K)
    d = rng.standard_normal((m, N)).astype(np.float32)
    out = _call(L, pkg, grp, a, ids, 1, PATHS[path], epi=epi, d=d if epi in ("add", "mul", "add_gelu") else None)
    want = _epi_ref(epi, _ref_rows(nso, grp, a, ids[:, 1]), d)
    e = nso.rel_l2(out, want)
    print("moe epilogue path=%s class=%s %s %s rel_l2 %.3g" % (path, _cls(fmt[0]), _fid(fmt), epi, e))
    assert e < TOL_EPI, (path, epi, e)


# ---------------------------------------------------------------------------------------------------------------- ids outside the group
@pytest.mark.parametrize("epi", EPIS)
def test_out_of_range_ids_give_the_epilogue_of_a_zero_product_on_every_path(L, pkg, nso, groups, epi):
    """dC[t] = epi(0, dD[t]) for an id outside [0, n_as): zero rows for none / mul / gelu / silu, dD[t] bit for bit for Add, gelu(dD[t])
    for Add_Gelu — the same bits from all three paths; the rows beside them are the usual products"""
    grp = groups(S4)
    rng = np.random.default_rng(500)
    dfull = rng.standard_normal((PATH_ROWS["grouped"], N)).astype(np.float32)
    bad_rows = {1: -1, 3: N_AS + 5, 5: -1}
    seen = {}
    for path in ("decode", "loop", "grouped"):
        m = PATH_ROWS[path]
        _, a, ids = _inputs(510 + m, m, K)
        for t, v in bad_rows.items():
            ids[t, 1] = v
        d = dfull[:m]
        out = _call(L, pkg, grp, a, ids, 1, PATHS[path], epi=epi, d=d if epi in ("add", "mul", "add_gelu") else None)
        want = _epi_ref(epi, _ref_rows(nso, grp, a, ids[:, 1]), d)
        good = np.array([t for t in range(m) if t not in bad_rows])
        assert nso.rel_l2(out[good], want[good]) < TOL_EPI, (path, epi)
        bad = out[sorted(bad_rows)]
        if epi == "add":
            assert np.array_equal(bad.view(np.uint32), d[sorted(bad_rows)].view(np.uint32)), path
        elif epi == "add_gelu":
            e = nso.rel_l2(bad, _gelu(d[sorted(bad_rows)].astype(np.float64)))
            print("moe invalid ids add_gelu path=%s rel_l2 %.3g" % (path, e))
            assert e < TOL_EPI, (path, e)
        else:
            assert np.all(bad == 0.0), (path, epi)
        seen[path] = bad.copy()
    assert np.array_equal(seen["decode"].view(np.uint32), seen["loop"].view(np.uint32))
    assert np.array_equal(seen["grouped"].view(np.uint32), seen["loop"].view(np.uint32))


@pytest.mark.parametrize("path", ["decode", "loop", "grouped"])
def test_every_id_out_of_range(L, pkg, nso, groups, path):
    """no expert has a row: the grouped path launches no GEMM and its scratch products are never written — the scatter must not read them"""
    grp = groups(S4)
    m = PATH_ROWS[path]
    rng, a, ids = _inputs(520 + m, m, K)
    ids[:, 1] = np.where(np.arange(m) % 2 == 0, -1, N_AS + 5)
    d = rng.standard_normal((m, N)).astype(np.float32)
    out = _call(L, pkg, grp, a, ids, 1, PATHS[path])
    assert np.all(out == 0.0)
    out = _call(L, pkg, grp, a, ids, 1, PATHS[path], epi="add", d=d)
    assert np.array_equal(out.view(np.uint32), d.view(np.uint32))
    out = _call(L, pkg, grp, a, ids, 1, PATHS[path], epi="add_gelu", d=d)
    assert nso.rel_l2(out, _gelu(d.astype(np.float64))) < TOL_EPI


# ---------------------------------------------------------------------------------------------------------------- capture
@pytest.mark.parametrize("fmt", [S4, F8_FORMATS[0]], ids=_fid)
def test_prefill_sized_call_on_a_capturing_stream_takes_the_loop(L, pkg, nso, groups, fmt):
    """40 rows are beyond the decode kernel's count, and grouping them needs the ids on the host, which a capturing stream cannot give:
    the loop kernel is captured (without a grouped attempt) — and a replay follows the ids that are in device memory THEN"""
    import torch
    grp = groups(fmt)
    m = 40
    _, a, ids = _inputs(600, m, K)
    dA, dI = torch.from_numpy(a).cuda(), torch.from_numpy(ids).cuda()
    dC = torch.zeros((m, N), device="cuda")
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    s0 = _stats(L)
    with torch.cuda.graph(gr):
        s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        pkg.check(L.ns_hip_mul_mat_id(dA.data_ptr(), dI.data_ptr(), TOPK, 1, grp.g, dC.data_ptr(), m, K, N, pkg.EPI_NONE, None, 0, s))
    assert tuple(int(v) for v in _stats(L) - s0) == LOOP
    gr.replay()
    torch.cuda.synchronize()
    _check(nso, "capture", "loop", grp, dC.cpu().numpy(), a, ids[:, 1])
    ids2 = ((ids + 1) % N_AS).astype(np.int32)
    dI.copy_(torch.from_numpy(ids2))
    dC.zero_()
    gr.replay()
    torch.cuda.synchronize()
    _check(nso, "capture, new ids", "loop", grp, dC.cpu().numpy(), a, ids2[:, 1])
    assert tuple(int(v) for v in _stats(L) - s0) == LOOP   # replays are not calls


# ---------------------------------------------------------------------------------------------------------------- the grouped path
GN, GK = 272, 512


def _grouped_ids(kind, m, rng):
    ids = np.zeros((m, TOPK), np.int32)
    if kind == "one_row_between":   # expert 1: ONE row, sorted between the rows of experts 0 and 2 (its two-row launch overlaps expert 2's rows)
        ids[:, 1] = np.where(rng.integers(0, 2, size=m) == 0, 0, 2)
        ids[m // 2, 1] = 1
        ids[0, 1], ids[m - 1, 1] = 2, 0
    elif kind == "one_expert":
        ids[:, 1] = 2
    else:
        ids[:, 1] = rng.integers(0, N_AS, size=m)
    ids[:, 0] = (ids[:, 1] + 1) % N_AS
    return ids


@pytest.mark.parametrize("m", [32, 150])
@pytest.mark.parametrize("kind", ["one_row_between", "one_expert", "lda", "ids_stride"])
def test_grouped_path_row_layouts(L, pkg, nso, groups, kind, m):
    grp = groups(S4, n=GN, k=GK)
    rng = np.random.default_rng(700 + m)
    a = rng.standard_normal((m, GK)).astype(np.float32)
    ids = _grouped_ids(kind, m, rng)
    sel = 1
    if kind == "ids_stride":
        ids = np.concatenate([ids, ((ids[:, 1:2] + 2) % N_AS).astype(np.int32)], axis=1)[:, [0, 2, 1]]
        sel = 2
    out = _call(L, pkg, grp, a, ids, sel, GROUPED, pad_a=4 if kind == "lda" else 0)
    if kind == "one_row_between":
        assert int((ids[:, sel] == 1).sum()) == 1
    _check(nso, "grouped " + kind, "grouped", grp, out, a, ids[:, sel])


@pytest.mark.parametrize("m", [32, 150])
def test_grouped_path_refuses_k_not_a_multiple_of_64(L, pkg, nso, groups, m):
    grp = groups(S4, n=GN, k=800)
    _, a, ids = _inputs(710 + m, m, 800)
    out = _call(L, pkg, grp, a, ids, 1, REFUSED_THEN_LOOP)
    _check(nso, "grouped k = 800", "loop", grp, out, a, ids[:, 1])


@pytest.mark.parametrize("fmt", F8_FORMATS, ids=_fid)
def test_grouped_path_fp8_and_an_expert_with_three_rows(L, pkg, nso, groups, fmt):
    """fp8 experts are grouped from 65 rows while every populated expert has at least 17 (the tiled kernel's range for fp8); one expert
    with 3 rows sends the whole call to the loop kernel"""
    grp = groups(fmt, n=GN, k=GK)
    m = 150
    rng, a, ids = _inputs(720, m, GK)
    ids[:, 1] = np.arange(m) % 3          # experts 0..2: 50 rows each, expert 3 none
    out = _call(L, pkg, grp, a, ids, 1, GROUPED)
    _check(nso, "grouped fp8", "grouped", grp, out, a, ids[:, 1])
    ids[[4, 77, 149], 1] = 3              # expert 3: three rows
    out = _call(L, pkg, grp, a, ids, 1, REFUSED_THEN_LOOP)
    _check(nso, "grouped fp8, 3-row expert", "loop", grp, out, a, ids[:, 1])

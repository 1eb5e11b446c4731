#!/usr/bin/env python3
"""Which kernel serves which call: the device-pointer forward / fused entries of libns_hip.so over a fixed case list with seeded inputs.
One line per case: index, name, return code, a hash of every output buffer, ns_hip_last_error().  Two builds of the library (NS_LIB_PATH
selects one) dispatch alike when their listings are identical:

    python scripts/dispatch_listing.py > a.txt;  NS_LIB_PATH=other/libns_hip.so python scripts/dispatch_listing.py > b.txt;  diff a.txt b.txt

Kernel names per case: run it under `rocprofv3 --kernel-trace --output-format csv -d DIR -o t -- python scripts/dispatch_listing.py`
and print the trace with `python scripts/dispatch_listing.py --trace DIR/.../t_kernel_trace.csv` (a one-element silu launch in front of
every case is the separator; the line's index is the listing's; per kernel: name, grid in work-items, LDS bytes).  `--only PREFIX` runs
the cases whose name starts with PREFIX, e.g. `--only attn` (a trace of such a run numbers the cases it ran from 000); NS_ATTN_PIPE=0 in the environment moves the "attn pipelined" cases to the
register-staged 128-row kernel."""
import ctypes as C, csv, hashlib, os, re, sys

if "--trace" in sys.argv:
    rows = list(csv.DictReader(open(sys.argv[sys.argv.index("--trace") + 1])))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    idx, cur = -1, None
    for r in rows:
        n = r["Kernel_Name"].replace("(anonymous namespace)::", "").split("(")[0].replace("void ", "").replace("ns::", "")
        mangled = re.match(r"_ZN2ns(?:12_GLOBAL__N_1)?(\d+)", n)  # kernels that are no templates come without their signature
        if mangled:
            n = n[mangled.end():][:int(mangled.group(1))]
        if "at::" in n or "elementwise" in n or "rocclr" in n:  # torch's own (fills, conversions of the inputs) and the runtime's copies
            continue
        if n.startswith("silu_kernel"):
            if cur is not None:
                print("%03d %s" % (idx, " | ".join(cur)))
            idx, cur = idx + 1, []
        elif cur is not None:  # name, grid and workgroup in work-items (the workgroup tells the wave count), LDS bytes of a workgroup
            cur.append("%s grid %s,%s,%s wg %s,%s,%s lds %s" % (n, r.get("Grid_Size_X"), r.get("Grid_Size_Y"), r.get("Grid_Size_Z"), r.get("Workgroup_Size_X"),
                                                                r.get("Workgroup_Size_Y"), r.get("Workgroup_Size_Z"), r.get("LDS_Block_Size")))
    if cur is not None:
        print("%03d %s" % (idx, " | ".join(cur)))
    sys.exit(0)

import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge
pkg = ge.load_package(); L = pkg.lib()
L.ns_hip_set_compute_mode.argtypes = [C.c_int]
ST = C.c_void_p(0)  # the default stream
rng = np.random.default_rng(1234)
keep = []


def dev(a):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    keep.append(t)
    return t


def make(n, k, qt, sdt, bs, comp):
    w = dev((rng.standard_normal((n, k), dtype=np.float32) * 0.02))
    size = L.ns_BTLAGemmPackBSize(n, k, bs, qt, sdt, False, comp, None)
    blob = torch.zeros(size, dtype=torch.uint8, device="cuda")
    pkg.check(L.ns_hip_quant_pack_device(blob.data_ptr(), w.data_ptr(), n, k, k, bs, qt, sdt, False, comp, True, ST))
    wt = pkg.Weight.from_device_blob(blob.data_ptr(), size, ST)
    torch.cuda.synchronize()
    keep.pop()
    return wt


def make_shuffled(n, k, bs):  # act-order (g_idx) S4 blob, packed on the host
    g_idx = np.repeat(np.arange(k // bs, dtype=np.int32), bs); rng.shuffle(g_idx)
    q = rng.integers(-8, 8, (k, n), dtype=np.int8)
    sc = rng.uniform(0.002, 0.02, (k // bs, n)).astype(np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    L.ns_set_pack_core(1)  # NS_CORE_AVX512F
    try:
        size = L.ns_BTLAGemmPackBSize(n, k, bs, pkg.S4, pkg.F32, False, pkg.COMP_F32, p(g_idx))
        blob = np.zeros(size + 64, np.uint8)
        off = (-blob.ctypes.data) % 64
        ptr = C.c_void_p(blob.ctypes.data + off)
        assert L.ns_BTLAGemmPackB(ptr, p(q), p(sc), None, n, k, n, bs, pkg.S4, pkg.F32, False, pkg.COMP_F32, p(g_idx), None), pkg.last_error()
    finally:
        L.ns_set_pack_core(pkg.CORE_AUTO)
    keep.append(blob)
    return pkg.Weight.from_host_blob(ptr, ST)


S4 = dict(qt=pkg.S4, sdt=pkg.BF16, bs=32, comp=pkg.COMP_INT8)
A, B, Cs, D, E = (256, 256), (4096, 4096), (8192, 4096), (4096, 8192), (14336, 4096)  # (n, k)
W = {}
for name, (n, k) in (("s4_A", A), ("s4_B", B), ("s4_Bk", B), ("s4_Bv", B), ("s4_C", Cs), ("s4_C3", Cs), ("s4_D", D), ("s4_E", E)):
    W[name] = make(n, k, **S4)
W["s8_A"] = make(*A, pkg.S8, pkg.BF16, 32, pkg.COMP_INT8)
W["s8_B"] = make(*B, pkg.S8, pkg.BF16, 32, pkg.COMP_INT8)
W["nf4_A"] = make(*A, pkg.F4_NF4, pkg.BF16, 128, pkg.COMP_BF16)
W["nf4_B"] = make(*B, pkg.F4_NF4, pkg.BF16, 128, pkg.COMP_BF16)
for nm in ("f8_B", "f8_Bk", "f8_Bv"):
    W[nm] = make(*B, pkg.F8_E4M3, pkg.F32, 32, pkg.COMP_F32)
W["s3_B"] = make(*B, pkg.INT_TYPES[3], pkg.BF16, 32, pkg.COMP_INT8)
W["shuf_A"] = make_shuffled(256, 256, 32)

MS = (1, 4, 5, 6, 16, 17, 33, 64, 65)
XMAX = 65
x32 = dev(rng.standard_normal((XMAX, 8192), dtype=np.float32))
X = {}


def acts(m, k, lda=None):
    """fp32 rows and their fp16 shadow, [m][lda]"""
    key = (m, k, lda)
    if key not in X:
        a = torch.zeros((m, lda or k), device="cuda")
        a[:, :k] = x32[:m, :k]
        X[key] = (a, a.half())
    return X[key]


def out32(*shape):
    return torch.full(shape, -7.0, device="cuda")


def out16(*shape):
    return torch.full(shape, -7.0, device="cuda", dtype=torch.float16)


def ptr(t):
    return t.data_ptr() if t is not None else None


mark = torch.zeros(4, device="cuda")
count = [0]


ONLY = sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else ""  # run the cases whose name starts so (the indices stay)


def case(name, fn):
    """fn() -> (rc, output tensors)"""
    if not name.startswith(ONLY):
        count[0] += 1
        return
    L.ns_hip_reset_error()
    L.ns_hip_silu_f32(mark.data_ptr(), mark.data_ptr(), 1, ST)
    try:
        rc, outs = fn()
    except Exception as e:  # a set-up step refused: the line says so
        rc, outs = "EXC " + str(e), []
    torch.cuda.synchronize()
    h = hashlib.sha1()
    for t in outs:
        if t is not None:
            h.update(t.detach().cpu().numpy().tobytes())
    print("%03d %-44s rc %s  out %s  err %r" % (count[0], name, rc, h.hexdigest()[:16], pkg.last_error()), flush=True)
    count[0] += 1


def forward(wn, m, shadow_in=False, shadow_out=False, no32_in=False, no32_out=False, link=None, lda=None, epi=pkg.EPI_NONE):
    w = W[wn]

    def fn():
        a, a16 = acts(m, w.k, lda)
        c = None if no32_out else out32(m, w.n)
        c16 = out16(m, w.n) if (shadow_out or no32_out) else None
        rc = L.ns_hip_f32f32_forward_x(None if no32_in else ptr(a), ptr(a16) if (shadow_in or no32_in) else None, w.h, ptr(c), ptr(c16), m,
                                       lda or w.k, w.n, epi, None, 0, C.byref(link) if link is not None else None, ST)
        return rc, [c, c16]
    return fn


def norm_link(m, k, **kw):
    """the consumer side of a carried RMS norm: sums of squares per 16 columns from ns_hip_norm_prep"""
    parts = (k + 15) // 16
    a, a16 = acts(m, k)
    ssq, n16, gamma = torch.zeros((m, parts), device="cuda"), a16.clone(), torch.ones(k, device="cuda")
    keep.extend((ssq, n16, gamma))
    pkg.check(L.ns_hip_norm_prep(m, k, ptr(a), k, ptr(gamma), ptr(n16), ptr(ssq), parts, ST))
    ln = pkg.NormLink(ptr(ssq), parts, parts, 1e-5, k, None, None, 0)
    for f, v in kw.items():
        setattr(ln, f, v)
    return ln


def qkv(names, m, shadow=False, link=None):
    ws = [W[n] for n in names]

    def fn():
        a, a16 = acts(m, ws[0].k)
        c = out32(3, m, ws[0].n)
        c16 = out16(3, m, ws[0].n) if shadow else None
        rc = L.ns_hip_fusion_qkv_forward_x(ptr(a), ptr(a16) if shadow else None, ws[0].h if ws[0] else None, ws[1].h, ws[2].h, ptr(c), ptr(c16), m,
                                           ws[0].k, ws[0].n, C.byref(link) if link is not None else None, ST)
        return rc, [c, c16]
    return fn


HS, NPAST = 128, 8


def qkv_rope(names, m, mode, flags=0, link=None, no_rope=False, no_shadow=False, hs=HS, n_dims=None):
    ws = [W[n] for n in names]

    def fn():
        k, n = ws[0].k, ws[0].n
        heads = n // hs
        a, a16 = acts(m, k)
        c = out32(3, m, n)
        kc = out16(1, NPAST + m, heads, hs); vc = out16(1, NPAST + m, heads, hs)
        tab = torch.zeros(m, hs // 2, 2, device="cuda")
        if mode in (0, 2):
            pkg.check(L.ns_hip_rope_cos_sin_mode(m, NPAST, hs, mode, 10000.0, 1.0, 1.0, ptr(tab), ST))
        rp = pkg.QkvRope(ptr(kc), ptr(vc), ptr(tab), heads, heads, hs, NPAST, n_dims or hs, mode, heads * hs, hs, flags)
        rc = L.ns_hip_fusion_qkv_rope_forward_x(ptr(a), None if no_shadow else ptr(a16), ws[0].h, ws[1].h, ws[2].h, ptr(c), m, k, n,
                                                C.byref(link) if link is not None else None, None if no_rope else C.byref(rp), ST)
        return rc, [c, kc, vc]
    return fn


def gateup(n1, n3, m, shadow=False, no32_in=False, link=None, act=pkg.EPI_SILU, no_out=False):
    w1, w3 = W[n1], W[n3]

    def fn():
        a, a16 = acts(m, w1.k)
        t1, t2 = out32(m, w1.n), out32(m, w1.n)
        t16 = out16(m, w1.n) if shadow else None
        rc = L.ns_hip_fusion_ffn3_gateup_x(None if no32_in else ptr(a), ptr(a16) if (shadow or no32_in) else None, w1.h, w3.h, ptr(t1),
                                           None if no_out else ptr(t2), ptr(t16), m, act, C.byref(link) if link is not None else None, ST)
        return rc, [t1, t2, t16]
    return fn


def ffn3(n1, n2, n3, m, fp16_mid=False):
    w1, w2, w3 = W[n1], W[n2], W[n3]

    def fn():
        a, a16 = acts(m, w1.k)
        t1, t2, o = out32(m, w1.n), out32(m, w1.n), out32(m, w2.n)
        t16, o16 = out16(m, w1.n), out16(m, w2.n)
        rc = L.ns_hip_fusion_ffn3_forward_h(ptr(a), ptr(a16), w1.h, w2.h, w3.h, ptr(t1), None if fp16_mid else ptr(t2), ptr(t16), ptr(o), ptr(o16), m,
                                            pkg.EPI_SILU, ST)
        return rc, [t1, t2, t16, o, o16]
    return fn


def ffn2(n1, n2, m, no_tmp=False):
    w1, w2 = W[n1], W[n2]

    def fn():
        a, _ = acts(m, w1.k)
        t1, o = out32(m, w1.n), out32(m, w2.n)
        b1, b2 = acts(1, w1.n)[0], acts(1, w2.n)[0]
        rc = L.ns_hip_fusion_ffn2_forward(ptr(a), w1.h, w2.h, ptr(b1), ptr(b2), None if no_tmp else ptr(t1), ptr(o), m, True, ST)
        return rc, [t1, o]
    return fn


def with_mode(mode, fn):
    def g():
        L.ns_hip_set_compute_mode(mode)
        try:
            return fn()
        finally:
            L.ns_hip_set_compute_mode(0)
    return g


def with_tuning(key, value, restore, fn):
    def g():
        L.ns_hip_set_tuning(key, value)
        try:
            return fn()
        finally:
            L.ns_hip_set_tuning(key, restore)
    return g


QB, QF8 = ("s4_B", "s4_Bk", "s4_Bv"), ("f8_B", "f8_Bk", "f8_Bv")
# ---- single forward: every row count on every shape, fp32 rows alone and with both fp16 shadows
for wn in ("s4_A", "s4_B", "s4_C", "s4_D"):
    for m in MS:
        case("fwd %s m%d" % (wn, m), forward(wn, m))
        case("fwd %s m%d +a16 +c16" % (wn, m), forward(wn, m, True, True))
for m in (6, 16, 17):
    case("fwd s4_E m%d" % m, forward("s4_E", m))
    case("fwd s4_E m%d +a16 +c16" % m, forward("s4_E", m, True, True))
for wn in ("s8_A", "s8_B", "nf4_A", "nf4_B", "s3_B", "shuf_A", "f8_B"):
    for m in (1, 5, 17, 65):
        case("fwd %s m%d" % (wn, m), forward(wn, m))
        case("fwd %s m%d +a16 +c16" % (wn, m), forward(wn, m, True, True))
for m in (17, 65):
    case("fwd f8_B m%d g3_f8=0" % m, with_tuning(b"g3_f8", 0, -1, forward("f8_B", m, True, True)))
case("fwd f8_B m65 g3_f8=0, fp32 only", with_tuning(b"g3_f8", 0, -1, forward("f8_B", 65)))
case("fwd s3_B m1 planes_off", with_tuning(b"planes", 0, 1, forward("s3_B", 1)))
case("fwd s4_B m1 gv_rows1=0", with_tuning(b"gv_rows1", 0, 1, forward("s4_B", 1, True)))
case("fwd s4_B m1 epilogue gelu", forward("s4_B", 1, epi=pkg.EPI_GELU))
for wn in ("s4_A", "s4_B", "s8_B", "shuf_A", "nf4_B"):
    for m in (1, 4, 5, 17, 65):
        case("fwd %s m%d ref_int8" % (wn, m), with_mode(1, forward(wn, m)))
for m in (17, 33, 65):
    case("fwd s4_B m%d fp16-only in" % m, forward("s4_B", m, no32_in=True))
    case("fwd s4_B m%d fp16-only out" % m, forward("s4_B", m, True, no32_out=True))
case("fwd f8_B m33 fp16-only in", forward("f8_B", 33, no32_in=True))
case("fwd f8_B m33 fp16-only in g3_f8=0", with_tuning(b"g3_f8", 0, -1, forward("f8_B", 33, no32_in=True)))
for m in (1, 16):
    case("fwd s4_B m%d norm link" % m, lambda m=m: forward("s4_B", m, True, True, link=norm_link(m, 4096))())
# ---- fused QKV
for m in (1, 4, 16, 17, 64, 65):
    case("qkv s4_B m%d" % m, qkv(QB, m))
    case("qkv s4_B m%d +a16 +c16" % m, qkv(QB, m, True))
case("qkv s4_B m4 norm link", lambda: qkv(QB, 4, True, link=norm_link(4, 4096))())
for m in (1, 4, 5, 65):
    case("qkv s4_B m%d ref_int8" % m, with_mode(1, qkv(QB, m)))
for m in (1, 65):
    case("qkv s4/s8/s4 m%d" % m, qkv(("s4_B", "s8_B", "s4_Bv"), m))
    case("qkv s4/s8/s4 m%d ref_int8" % m, with_mode(1, qkv(("s4_B", "s8_B", "s4_Bv"), m)))
for m in (17, 65):
    case("qkv f8_B m%d" % m, qkv(QF8, m, True))
    case("qkv f8_B m%d g3_f8=0" % m, with_tuning(b"g3_f8", 0, -1, qkv(QF8, m, True)))
# ---- fused QKV + RoPE + kv append
for mode, flags in ((0, 0), (2, pkg.QKV_ROPE_NEOX)):
    for m in (1, 32):
        case("qkv+rope s4_B m%d mode %d" % (m, mode), qkv_rope(QB, m, mode, flags))
    case("qkv+rope s4_B m32 mode %d cache-only" % mode, qkv_rope(QB, 32, mode, flags | pkg.QKV_ROPE_KV_CACHE_ONLY))
case("qkv+rope s4_B m4 mode 0 norm link", lambda: qkv_rope(QB, 4, 0, link=norm_link(4, 4096))())
case("qkv+rope f8_B m65 mode 0", qkv_rope(QF8, 65, 0))
# ---- gate / up and the whole FFN
for m in (1, 4, 16, 17, 33, 64, 65):
    case("gateup s4_C m%d" % m, gateup("s4_C", "s4_C3", m))
    case("gateup s4_C m%d +a16 +t16" % m, gateup("s4_C", "s4_C3", m, True))
case("gateup s4_C m65 fp16-only in", gateup("s4_C", "s4_C3", 65, no32_in=True))
case("gateup s4_C m65 fp16-only out", gateup("s4_C", "s4_C3", 65, True, no_out=True))
case("gateup s4_C m4 fp16-only out", gateup("s4_C", "s4_C3", 4, True, no_out=True))
case("gateup s4_B/s8_B m4 (two formats)", gateup("s4_B", "s8_B", 4, True))
case("gateup s4_C m4 norm link", lambda: gateup("s4_C", "s4_C3", 4, True, link=norm_link(4, 4096))())
for m in (1, 4, 5):
    case("gateup s4_C m%d ref_int8" % m, with_mode(1, gateup("s4_C", "s4_C3", m)))
case("gateup f8_B m65", gateup("f8_B", "f8_Bk", 65, True))
case("gateup f8_B m33 fp16-only in", gateup("f8_B", "f8_Bk", 33, no32_in=True))
for m in (1, 17, 65):
    case("ffn3 s4 C/D/C m%d" % m, ffn3("s4_C", "s4_D", "s4_C3", m))
    case("ffn3 s4 C/D/C m%d fp16 intermediate" % m, ffn3("s4_C", "s4_D", "s4_C3", m, True))
case("ffn3 s4 C/D/C m4 ref_int8", with_mode(1, ffn3("s4_C", "s4_D", "s4_C3", 4)))
case("ffn2 s4 C/D m4", ffn2("s4_C", "s4_D", 4))
# ---- refusals: one per error text of the dispatch layer that a caller can reach without exhausting device memory
case("refuse fwd m0", forward("s4_A", 0))
case("refuse fwd fp16-only in, shuffled weight", forward("shuf_A", 33, no32_in=True))
case("refuse fwd fp16-only in, lda not a multiple of 8", forward("s4_A", 33, no32_in=True, lda=260))
case("refuse fwd norm link m17", lambda: forward("s4_B", 17, True, link=norm_link(17, 4096))())
case("refuse fwd norm link in_stride", lambda: forward("s4_B", 4, True, link=norm_link(4, 4096, in_stride=3, in_parts=2))())
case("refuse qkv producer link", lambda: qkv(QB, 4, True, link=norm_link(4, 4096, out_ssq=ptr(mark)))())
case("refuse qkv norm link, two formats", lambda: qkv(("s4_B", "s8_B", "s4_Bv"), 4, True, link=norm_link(4, 4096))())
case("refuse qkv+rope no rope", qkv_rope(QB, 1, 0, no_rope=True))
case("refuse qkv+rope producer link", lambda: qkv_rope(QB, 4, 0, link=norm_link(4, 4096, out_gamma=ptr(mark)))())
case("refuse qkv+rope unknown flag", qkv_rope(QB, 1, 0, 8))
case("refuse qkv+rope NEOX flag with mode 0", qkv_rope(QB, 1, 0, pkg.QKV_ROPE_NEOX))
case("refuse qkv+rope mode 2 without the flag", qkv_rope(QB, 1, 2, 0))
case("refuse qkv+rope NeoX n_dims != head_size", qkv_rope(QB, 1, 2, pkg.QKV_ROPE_NEOX, n_dims=64))
case("refuse qkv+rope NeoX decode head_size 48", qkv_rope(QB, 1, 2, pkg.QKV_ROPE_NEOX, hs=48))
case("refuse qkv+rope NeoX prefill head_size 256", qkv_rope(QB, 32, 2, pkg.QKV_ROPE_NEOX, hs=256))
case("refuse qkv+rope prefill, two formats", qkv_rope(("s4_B", "s8_B", "s4_Bv"), 32, 0))
case("refuse qkv+rope prefill, norm link", lambda: qkv_rope(QB, 32, 0, link=norm_link(32, 4096))())
case("refuse qkv+rope decode, no fp16 shadow", qkv_rope(QB, 4, 0, no_shadow=True))
case("refuse qkv+rope decode, ref_int8", with_mode(1, qkv_rope(QB, 1, 0)))
case("refuse gateup no output", lambda: (L.ns_hip_fusion_ffn3_gateup_x(ptr(mark), None, W["s4_C"].h, W["s4_C3"].h, None, None, None, 1, 0, None, ST), []))
case("refuse gateup fp16-only in at m4", gateup("s4_C", "s4_C3", 4, no32_in=True))
case("refuse gateup producer link", lambda: gateup("s4_C", "s4_C3", 4, True, link=norm_link(4, 4096, out_ssq=ptr(mark)))())
case("refuse gateup norm link m17", lambda: gateup("s4_C", "s4_C3", 17, True, link=norm_link(17, 4096))())
case("refuse gateup norm link, two formats", lambda: gateup("s4_B", "s8_B", 4, True, link=norm_link(4, 4096))())
case("refuse ffn3 w2 does not follow w1", ffn3("s4_C", "s4_C3", "s4_C3", 4))
case("refuse ffn2 no tmp1", ffn2("s4_C", "s4_D", 4, no_tmp=True))
case("refuse compute mode 7", lambda: (L.ns_hip_set_compute_mode(7), []))
case("refuse tuning key", lambda: (L.ns_hip_set_tuning(b"no_such_key", 1), []))
case("refuse tuning gv_nw 3", lambda: (L.ns_hip_set_tuning(b"gv_nw", 3), []))
# ---- attention (ns_hip_attn_fp32_fp16_fp16_fp32_forward_h): two cases or more per row of the path table of docs/kernels/attention.md
arng = np.random.default_rng(77)


def attn(bs, hn, hkv, hs, slq, slkv, flags=0, kt=False, shadow=False, scale=None, head_major=False, q_off=0, tuning=()):
    def fn():
        q = dev(arng.standard_normal(bs * slq * hn * hs + 4, dtype=np.float32))
        k = dev(arng.standard_normal(bs * slkv * hkv * hs, dtype=np.float32).astype(np.float16))
        v = dev(arng.standard_normal(bs * slkv * hkv * hs, dtype=np.float32).astype(np.float16))
        d, d16 = out32(bs * slq * hn * hs), out16(bs * slq * hn * hs) if shadow else None
        a = pkg.attn_args(q.data_ptr() + 4 * q_off, k.data_ptr(), v.data_ptr(), d.data_ptr(), bs, hn, hkv, hs, slq, slkv,
                          hs ** -0.5 if scale is None else scale, flags, kt)
        if head_major:  # K / V [bs][hkv][sl_kv][hs]: one slab per head
            a.step_k_head_num = a.step_v_head_num = slkv * hs
            a.step_k_sl = a.step_v_sl = hs
        for key, value, _ in tuning:
            L.ns_hip_set_tuning(key, value)
        try:
            rc = L.ns_hip_attn_fp32_fp16_fp16_fp32_forward_h(C.byref(a), ptr(d16), ST)
        finally:
            for key, _, restore in tuning:
                L.ns_hip_set_tuning(key, restore)
        del keep[-3:]
        return rc, [d, d16]
    return fn


CAUSAL, ALIBI, TANH = 1, 2, 8
case("attn generic transposed K (1,8,8,128,4,260)", attn(1, 8, 8, 128, 4, 260, kt=True))
case("attn generic head size 20", attn(1, 4, 4, 20, 2, 70, CAUSAL))
case("attn regs head size 32 300 keys", attn(1, 8, 8, 32, 1, 300))
case("attn regs head size 256 520 keys", attn(1, 8, 8, 256, 1, 520, shadow=True))
case("attn regs attn_stream=0 (1,8,2,64,1,600)", attn(1, 8, 2, 64, 1, 600, tuning=((b"attn_stream", 0, 1),)))
case("attn regs unaligned Q", attn(1, 8, 8, 128, 1, 300, q_off=1))
case("attn ring (1,32,32,128,1,2048)", attn(1, 32, 32, 128, 1, 2048, shadow=True))
case("attn ring (1,8,2,64,1,600)", attn(1, 8, 2, 64, 1, 600))
case("attn ring 71 heads on one kv head", attn(1, 71, 1, 64, 1, 520))
case("attn ring alibi 3 rows", attn(1, 8, 4, 128, 3, 300, ALIBI | CAUSAL))
case("attn ring one range (1,4,4,128,3,2)", attn(1, 4, 4, 128, 3, 2))
case("attn ring batch 2 with a head group", attn(2, 8, 2, 128, 1, 700))
case("attn ring attn_inlaunch=1", attn(1, 8, 8, 128, 1, 2048, tuning=((b"attn_inlaunch", 1, 0),)))
case("attn regs attn_inlaunch=1 head size 256", attn(1, 8, 8, 256, 1, 1024, tuning=((b"attn_inlaunch", 1, 0),)))
for hf in (0, 1):
    case("attn ring attn_heads_first=%d" % hf, attn(1, 8, 8, 128, 1, 1024, tuning=((b"attn_heads_first", hf, -1),)))
    case("attn ring head-major cache attn_heads_first=%d" % hf, attn(1, 8, 8, 128, 1, 1024, head_major=True, tuning=((b"attn_heads_first", hf, -1),)))
case("attn ring head-major cache", attn(1, 8, 8, 128, 1, 1024, head_major=True))
case("attn 64-row (1,4,4,64,40,40)", attn(1, 4, 4, 64, 40, 40, CAUSAL))
case("attn 64-row (1,8,8,128,64,64)", attn(1, 8, 8, 128, 64, 64, CAUSAL, shadow=True))
case("attn 64-row negative scale, 150 rows", attn(1, 4, 4, 128, 150, 150, scale=-0.1))
case("attn 128-row biased alibi 16 rows", attn(1, 8, 8, 128, 16, 16, ALIBI | CAUSAL))
case("attn 128-row biased tanh head size 64", attn(1, 4, 2, 64, 40, 200, TANH))
case("attn 128-row padded head size 80", attn(1, 4, 4, 80, 40, 40, CAUSAL))
case("attn 128-row padded head size 160 alibi", attn(1, 4, 4, 160, 130, 130, ALIBI | CAUSAL, shadow=True))
case("attn 128-row head size 256", attn(1, 4, 4, 256, 40, 40, CAUSAL))
case("attn 128-row head size 256 tanh", attn(1, 4, 2, 256, 130, 300, TANH))
case("attn pipelined 40 rows with attn_mfma2_rows=16 (NS_ATTN_PIPE=0: 128-row plain)",attn(1, 8, 8, 128, 40, 40, CAUSAL, tuning=((b"attn_mfma2_rows", 16, 128),)))
case("attn pipelined (1,8,8,128,128,128)", attn(1, 8, 8, 128, 128, 128, CAUSAL, shadow=True))
case("attn pipelined head size 64, 257 rows, batch 2, head group", attn(2, 8, 4, 64, 257, 300, CAUSAL))
case("attn pipelined variant 3 (1,2,2,64,128,3072)", attn(1, 2, 2, 64, 128, 3072))
case("attn pipelined variant 3 causal 3100 keys", attn(1, 2, 1, 128, 130, 3100, CAUSAL))
case("attn refuse causal with more rows than keys", attn(1, 4, 4, 64, 8, 4, CAUSAL))
case("attn refuse head group", attn(1, 6, 4, 64, 1, 64))
L.ns_hip_silu_f32(mark.data_ptr(), mark.data_ptr(), 1, ST)
torch.cuda.synchronize()
for w in W.values():
    w.free()

#!/usr/bin/env python3
"""The fused QKV + NeoX RoPE + kv-append launch (ns_hip_fusion_qkv_rope_forward_x, NS_QKV_ROPE_NEOX) against the two launches it replaces
(fused QKV, then ns_hip_rope_qkv_append(mode 2)), in one process, as dependent launches inside a replayed HIP graph (the method of
scripts/launch_floor.py): K = 4096, 32/32 and 32/8 heads of 128, S4 g32, one row and 2048 rows.  HIP-event time per layer step.
Prints one line per case and a JSON summary; `--out FILE` also writes the text there."""
import ctypes as C, json, os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge
pkg = ge.load_package(); L = pkg.lib()
K, HS, NPAST, BASE = 4096, 128, 512, 10000.0
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def make(n, k, seed):
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    g = torch.Generator(device="cuda").manual_seed(seed)
    w = torch.randn((n, k), generator=g, device="cuda") * 0.02
    size = L.ns_BTLAGemmPackBSize(n, k, 32, pkg.S4, pkg.BF16, False, pkg.COMP_INT8, None)
    blob = torch.zeros(size, dtype=torch.uint8, device="cuda")
    pkg.check(L.ns_hip_quant_pack_device(blob.data_ptr(), w.data_ptr(), n, k, k, 32, pkg.S4, pkg.BF16, False, pkg.COMP_INT8, True, st))
    wt = pkg.Weight.from_device_blob(blob.data_ptr(), size, st)
    torch.cuda.synchronize()
    return wt


def time_us(fn, steps, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    for _ in range(2):
        g.replay()
    torch.cuda.synchronize()
    best = 1e30
    for _ in range(3):  # best of three timed batches
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            g.replay()
        e1.record(); torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) * 1e3 / reps / steps)
    return best


res = {}
for heads, hkv in ((32, 32), (32, 8)):
    d, dkv = heads * HS, hkv * HS
    NW = 4  # weight sets rotated through, so that consecutive steps do not find their weights in L2
    ws = [(make(d, K, 11 + 3 * i), make(dkv, K, 12 + 3 * i), make(dkv, K, 13 + 3 * i)) for i in range(NW)]
    for m in (1, 2048):
        steps, reps = (32, 20) if m == 1 else (4, 5)
        x = torch.randn((m, K), device="cuda"); x16 = x.half()
        ldc = d
        out = torch.zeros(3, m, ldc, device="cuda")
        kc = torch.zeros(1, NPAST + m, hkv, HS, device="cuda", dtype=torch.float16)
        vc = torch.zeros_like(kc)
        tab = torch.zeros(m, HS // 2, 2, device="cuda")
        st0 = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        pkg.check(L.ns_hip_rope_cos_sin_mode(m, NPAST, HS, 2, BASE, 1.0, 1.0, tab.data_ptr(), st0))
        torch.cuda.synchronize()

        def two():
            s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            for i in range(steps):
                wq, wk, wv = ws[i % NW]
                if m <= 16:
                    pkg.check(L.ns_hip_fusion_qkv_forward_x(x.data_ptr(), x16.data_ptr(), wq.h, wk.h, wv.h, out.data_ptr(), None, m, K, ldc, None, s))
                else:
                    pkg.check(L.ns_hip_fusion_qkv_forward_h(x.data_ptr(), x16.data_ptr(), wq.h, wk.h, wv.h, out.data_ptr(), None, m, K, ldc, s))
                pkg.check(L.ns_hip_rope_qkv_append(out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), kc.data_ptr(), vc.data_ptr(), m, heads, hkv, HS,
                                                   NPAST, HS, 2, BASE, 1.0, 0.0, 1.0, hkv * HS, HS, s))

        def fused(flags):
            def fn():
                s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
                rp = pkg.QkvRope(kc.data_ptr(), vc.data_ptr(), tab.data_ptr(), heads, hkv, HS, NPAST, HS, 2, hkv * HS, HS, flags)
                for i in range(steps):
                    wq, wk, wv = ws[i % NW]
                    pkg.check(L.ns_hip_fusion_qkv_rope_forward_x(x.data_ptr(), x16.data_ptr(), wq.h, wk.h, wv.h, out.data_ptr(), m, K, ldc, None, C.byref(rp), s))
            return fn

        # (out[1] / out[2] are [m][ldc] with ldc = d: for 32/8 heads the separate operator reads them as packed [m][dkv] — timing only)
        r = {"two_launches_us": round(time_us(two, steps, reps), 2), "fused_us": round(time_us(fused(pkg.QKV_ROPE_NEOX), steps, reps), 2)}
        if m > 16:
            r["fused_kv_cache_only_us"] = round(time_us(fused(pkg.QKV_ROPE_NEOX | pkg.QKV_ROPE_KV_CACHE_ONLY), steps, reps), 2)
        res["heads_%d_%d_m%d" % (heads, hkv, m)] = r
        say("heads %d/%d of %d, K %d, m %4d: two launches %.2f us, fused %.2f us%s" %
            (heads, hkv, HS, K, m, r["two_launches_us"], r["fused_us"],
             (", fused + KV_CACHE_ONLY %.2f us" % r["fused_kv_cache_only_us"]) if m > 16 else ""))
    for t in ws:
        for w in t:
            w.free()
say(json.dumps(res))
if "--out" in sys.argv:
    path = sys.argv[sys.argv.index("--out") + 1]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    open(path, "w").write("\n".join(lines) + "\n")

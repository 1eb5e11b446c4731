#!/usr/bin/env python3
"""fp8 weights on the tiled prefill GEMM against the path they took before ("g3_f8" 1 / 0), with int8 weights on the same shapes as the
yardstick: the four Llama-2-7B shapes at M = 2048 and M = 128, E4M3 g32 with E8M0 scales, one process, the three legs alternating
round by round after a warm-up, median of the rounds.  Usage: scripts/fp8_gemm_ab.py [rounds]"""
import ctypes as C, json, os, statistics, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge
pkg = ge.load_package(); L = pkg.lib()
torch.cuda.set_device(0)
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
st = C.c_void_p(torch.cuda.current_stream().cuda_stream)


def weight(n, k, qt, sdt, comp):
    w = torch.randn((n, k), device="cuda") * k ** -0.5
    size = L.ns_BTLAGemmPackBSize(n, k, 32, qt, sdt, False, comp, None)
    blob = torch.zeros(size, dtype=torch.uint8, device="cuda")
    pkg.check(L.ns_hip_quant_pack_device(blob.data_ptr(), w.data_ptr(), n, k, k, 32, qt, sdt, False, comp, True, st))
    wt = pkg.Weight.from_device_blob(blob.data_ptr(), size, st)
    torch.cuda.synchronize()
    return wt


for n, k in [(4096, 4096), (11008, 4096), (4096, 11008), (32000, 4096)]:
    w8 = weight(n, k, pkg.F8_E4M3, pkg.F8_E8M0, pkg.COMP_F32)
    wi = weight(n, k, pkg.S8, pkg.BF16, pkg.COMP_INT8)
    for m in (2048, 128):
        a = torch.randn((m, k), device="cuda"); a16 = a.half()
        c = torch.empty((m, n), device="cuda"); c16 = torch.empty((m, n), device="cuda", dtype=torch.float16)
        legs = {"fp8_tiled": (w8, 1, c16), "fp8_before": (w8, 0, None), "int8_tiled": (wi, 1, c16)}   # (the earlier kernel writes no fp16 shadow)

        def timed(wt, sw, o16, reps):
            L.ns_hip_set_tuning(b"g3_f8", sw)
            run = lambda: pkg.check(L.ns_hip_f32f32_forward_h(a.data_ptr(), a16.data_ptr(), wt.h, c.data_ptr(), o16.data_ptr() if o16 is not None else None,
                                                              m, k, n, 0, None, 0, st))
            run(); torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                run()
            e1.record(); torch.cuda.synchronize()
            return e0.elapsed_time(e1) / reps * 1e3

        for name, (wt, sw, o16) in legs.items():
            timed(wt, sw, o16, 5)   # warm-up
        us = {name: [] for name in legs}
        for _ in range(rounds):
            for name, (wt, sw, o16) in legs.items():
                us[name].append(timed(wt, sw, o16, 10))
        L.ns_hip_set_tuning(b"g3_f8", -1)
        out = {"shape": "%dx%d" % (n, k), "m": m}
        for name, v in us.items():
            med = statistics.median(v)
            out[name] = {"us": round(med, 1), "tflops": round(2.0 * m * n * k / med / 1e6, 1), "min_us": round(min(v), 1), "max_us": round(max(v), 1)}
        print(json.dumps(out), flush=True)
        del a, a16, c, c16
    del w8, wi

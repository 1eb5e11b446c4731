#!/usr/bin/env python3
"""Mixture-of-experts FFN at Mixtral-8x7B shapes (8 experts of 14336 x 4096 gate / up and 4096 x 14336 down, 2 experts per token,
int4 g32 bf16): the three expert-indexed matmuls of ffn_id_silu (ne_layers.c:8053-8170: gate with SiLU, up with Mul, down) per
selected expert, ids on the device, one HIP graph; parity of one token's rows against the oracle's fp64 product.  Prints us per
MoE FFN layer, the HBM rate over the expert weights a token really touches, and tokens/s of 32 such layers.
Below 32 tokens a second leg times the whole block through ns_hip_moe_ffn_silu (routing weights and the sum over the selections included)
in the same graph form, on its fused launches and - "moe_ffn_fused" = 0 - on its composition: medians of interleaved replay batches.
From 32 tokens - or from grouped_rows=N tokens, which lowers "moe_ffn_grouped_rows" to N for that leg - a third leg times the block entry as
plain calls (the grouped pass reads the ids on the host: no graph), wall clock around batches that end in a synchronisation, with the
grouped pass on and - "moe_ffn_grouped_rows" negative - off: medians of interleaved batches again.
With device_rows=N (N >= tokens) a fourth leg times the block entry as graph replays - any token count: a captured stream never takes the
grouped pass - on three servers: the composition (every key at its default: the behaviour without the device-grouped pass), the fused
launches stretched to this token count ("moe_gemv_rows" = tokens) and the device-grouped pass ("moe_ffn_device_rows" = N): medians of
interleaved replay batches, median [min ... max] per layer.
usage: moe_bench.py [tokens=1] [act=silu|gelu] [grouped_rows=N] [device_rows=N]      (act: the block entry of the second to fourth leg)"""
import ctypes as C, json, os, sys, time
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge
pkg = ge.load_package(); L = pkg.lib(); nso = ge.load_oracle()
opts = dict(x.split("=", 1) for x in sys.argv[1:] if "=" in x)
pos_args = [x for x in sys.argv[1:] if "=" not in x]
m = int(pos_args[0]) if pos_args else 1
act_name = opts.get("act", "silu")
assert act_name in ("silu", "gelu"), "act=silu or act=gelu"
block_entry = L.ns_hip_moe_ffn_gelu if act_name == "gelu" else L.ns_hip_moe_ffn_silu
act_f64 = (lambda x: 0.5 * x * (1.0 + np.tanh(0.7978845834732056 * (x + 0.044714998453855515 * x ** 3)))) if act_name == "gelu" else \
    (lambda x: x / (1.0 + np.exp(-x)))
grouped_rows = int(opts["grouped_rows"]) if "grouped_rows" in opts else 0   # 0: the library's default threshold
device_rows = int(opts["device_rows"]) if "device_rows" in opts else 0      # 0: no device-grouped leg
n_as, d, ff, topk = 8, 4096, 14336, 2
st = C.c_void_p(torch.cuda.current_stream().cuda_stream)


def make(n, k, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    w = torch.randn((n, k), generator=g, device="cuda") * k ** -0.5
    size = L.ns_BTLAGemmPackBSize(n, k, 32, pkg.S4, pkg.BF16, False, pkg.COMP_INT8, None)
    b = torch.zeros(size, dtype=torch.uint8, device="cuda")
    pkg.check(L.ns_hip_quant_pack_device(b.data_ptr(), w.data_ptr(), n, k, k, 32, pkg.S4, pkg.BF16, False, pkg.COMP_INT8, True, st))
    wt = pkg.Weight.from_device_blob(b.data_ptr(), size, st)
    torch.cuda.synchronize()
    return wt, b


def group(n, k, seed0):
    ws = [make(n, k, seed0 + i) for i in range(n_as)]
    arr = (C.c_void_p * n_as)(*[w[0].h for w in ws])
    g = L.ns_hip_expert_group_create(arr, n_as)
    assert g, pkg.last_error()
    return ws, g


nlay = 2   # two different layers in the graph: 2 x 3 x 8 experts x 33 MB = 1.6 GB resident, a token touches 2 of 8
layers = [(group(ff, d, 100 * i), group(ff, d, 100 * i + 20), group(d, ff, 100 * i + 40)) for i in range(nlay)]
rng = np.random.default_rng(1)
a = torch.randn((m, d), device="cuda")
ids_np = np.stack([rng.permutation(n_as)[:topk] for _ in range(m)]).astype(np.int32)
ids = torch.from_numpy(ids_np).cuda()
gate, act, y = torch.empty((m, ff), device="cuda"), torch.empty((m, ff), device="cuda"), torch.empty((topk, m, d), device="cuda")


def ffn(layer, s):
    (wg, gg), (wu, gu), (wd, gd) = layer
    for sel in range(topk):
        pkg.check(L.ns_hip_mul_mat_id(a.data_ptr(), ids.data_ptr(), topk, sel, gg, gate.data_ptr(), m, d, ff, pkg.EPI_SILU, None, 0, s))
        pkg.check(L.ns_hip_mul_mat_id(a.data_ptr(), ids.data_ptr(), topk, sel, gu, act.data_ptr(), m, d, ff, pkg.EPI_MUL, gate.data_ptr(), ff, s))
        pkg.check(L.ns_hip_mul_mat_id(act.data_ptr(), ids.data_ptr(), topk, sel, gd, y[sel].data_ptr(), m, ff, d, pkg.EPI_NONE, None, 0, s))


def chain(s):
    for layer in layers:
        ffn(layer, s)


for _ in range(3):
    chain(st)
torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
if m >= 32:
    # prefill size (round 5): the grouped form reads the ids on the host, so it is timed as plain calls (NS_MOE_GROUPED_ROWS=0: the per-row kernels)
    reps = 3
    e0.record()
    for _ in range(reps):
        chain(st)
    e1.record(); torch.cuda.synchronize()
else:
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        chain(C.c_void_p(torch.cuda.current_stream().cuda_stream))
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    e0.record()
    reps = 30
    for _ in range(reps):
        g.replay()
    e1.record(); torch.cuda.synchronize()
us = e0.elapsed_time(e1) * 1e3 / reps / nlay
# the fused entry beside that composition, same graph form: out = sum_sel w * down(silu(gate) * up) per layer
block = {}
if m < 32:
    wts = torch.rand((m, topk), device="cuda") + 0.25
    out = torch.empty((m, d), device="cuda")

    def block_chain(s):
        for (wg, gg), (wu, gu), (wd, gd) in layers:
            pkg.check(block_entry(a.data_ptr(), d, m, ids.data_ptr(), topk, wts.data_ptr(), topk, topk, gg, gu, gd, out.data_ptr(), d, s))

    def stats():
        v = (C.c_uint64 * 4)()
        L.ns_hip_moe_ffn_stats(v)
        return [int(x) for x in v]

    graphs = {}
    for name, fused_on in (("fused", 1), ("entry_composition", 0)):
        L.ns_hip_set_tuning(b"moe_ffn_fused", fused_on)
        block_chain(st)
        torch.cuda.synchronize()
        s0 = stats()
        gb = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gb):
            block_chain(C.c_void_p(torch.cuda.current_stream().cuda_stream))
        s1 = stats()
        block[name + "_calls"] = [s1[0] - s0[0], s1[1] - s0[1]]   # [on the fused launches, on the composition] while capturing
        if fused_on:
            block["fused_launches_per_layer"] = (s1[2] - s0[2]) // nlay
        graphs[name] = gb
    L.ns_hip_set_tuning(b"moe_ffn_fused", -1)
    graphs["three_calls"] = g   # the 3 * topk calls timed above (no weighting, no sum)
    times = {k: [] for k in graphs}
    for _ in range(7):
        for k, gb in graphs.items():
            gb.replay(); torch.cuda.synchronize()
            e0.record()
            for _ in range(reps):
                gb.replay()
            e1.record(); torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3 / reps / nlay)
    for k, v in times.items():
        block["us_per_layer_" + k] = {"median": round(float(np.median(v)), 2), "min": round(min(v), 2), "max": round(max(v), 2)}
    # the block's parity: token 0 against the fp64 oracle over both selections
    graphs["fused"].replay(); torch.cuda.synchronize()
    hostb = lambda t: (lambda b: (b.__setitem__(slice(None), t.cpu().numpy()), b)[1])(nso.aligned_bytes(t.numel()))
    a0b, refb = a[:1].cpu().numpy(), np.zeros((1, d))
    for sel in range(topk):
        ex = int(ids_np[0, sel])
        (wg, _), (wu, _), (wd, _) = layers[-1]
        hg, hu = nso.gemm_f64(a0b, hostb(wg[ex][1])), nso.gemm_f64(a0b, hostb(wu[ex][1]))
        refb += float(wts[0, sel]) * nso.gemm_f64((act_f64(hg) * hu).astype(np.float32), hostb(wd[ex][1]))
    block["fused_parity_rel_l2_vs_fp64_oracle_token0"] = float("%.3g" % nso.rel_l2(out[:1].cpu().numpy(), refb))
# the block entry at prompt size, plain calls: the grouped pass against the composition ("moe_ffn_grouped_rows" negative), interleaved batches
prompt = {}
if m >= 32 or (grouped_rows > 0 and m >= grouped_rows):
    wts_p = torch.rand((m, topk), device="cuda") + 0.25
    out_p = torch.empty((m, d), device="cuda")

    def entry_chain():
        for (wg, gg), (wu, gu), (wd, gd) in layers:
            pkg.check(block_entry(a.data_ptr(), d, m, ids.data_ptr(), topk, wts_p.data_ptr(), topk, topk, gg, gu, gd, out_p.data_ptr(), d, st))

    def ffn_stats():
        v = (C.c_uint64 * 4)()
        L.ns_hip_moe_ffn_stats(v)
        return [int(x) for x in v]

    legs = (("grouped", grouped_rows), ("composition", -1))
    reps_p = 5 if m >= 1024 else 15 if m >= 256 else 50
    times_p = {k: [] for k, _ in legs}
    for rnd in range(8):   # (round 0 warms both legs up and is dropped)
        for name, key in legs:
            L.ns_hip_set_tuning(b"moe_ffn_grouped_rows", key)
            s0 = ffn_stats()
            entry_chain(); torch.cuda.synchronize()
            s1 = ffn_stats()
            prompt[name + "_calls"] = [s1[1] - s0[1], s1[3] - s0[3]]   # [on the composition, on the grouped pass] of one chain
            t0 = time.perf_counter()
            for _ in range(reps_p):
                entry_chain()
            torch.cuda.synchronize()
            if rnd:
                times_p[name].append((time.perf_counter() - t0) * 1e6 / reps_p / nlay)
    L.ns_hip_set_tuning(b"moe_ffn_grouped_rows", 0)
    for k, v in times_p.items():
        prompt["us_per_layer_" + k] = {"median": round(float(np.median(v)), 1), "min": round(min(v), 1), "max": round(max(v), 1)}
    prompt["act"], prompt["grouped_rows_key"] = act_name, grouped_rows
    # parity of the grouped leg's token 0 against the fp64 oracle over both selections
    L.ns_hip_set_tuning(b"moe_ffn_grouped_rows", grouped_rows)
    entry_chain(); torch.cuda.synchronize()
    L.ns_hip_set_tuning(b"moe_ffn_grouped_rows", 0)
    hostp = lambda t: (lambda b: (b.__setitem__(slice(None), t.cpu().numpy()), b)[1])(nso.aligned_bytes(t.numel()))
    a0p, refp = a[:1].cpu().numpy(), np.zeros((1, d))
    for sel in range(topk):
        ex = int(ids_np[0, sel])
        (wg, _), (wu, _), (wd, _) = layers[-1]
        hg, hu = nso.gemm_f64(a0p, hostp(wg[ex][1])), nso.gemm_f64(a0p, hostp(wu[ex][1]))
        refp += float(wts_p[0, sel]) * nso.gemm_f64((act_f64(hg) * hu).astype(np.float32), hostp(wd[ex][1]))
    prompt["grouped_parity_rel_l2_vs_fp64_oracle_token0"] = float("%.3g" % nso.rel_l2(out_p[:1].cpu().numpy(), refp))
# the block entry on a captured stream: composition / stretched fused launches / device-grouped pass, interleaved replay batches
device = {}
if device_rows > 0:
    assert m <= device_rows, "device_rows below the token count: the pass would not be tried"
    wts_d = torch.rand((m, topk), device="cuda") + 0.25
    out_d = torch.empty((m, d), device="cuda")

    def device_chain(s):
        for (wg, gg), (wu, gu), (wd, gd) in layers:
            pkg.check(block_entry(a.data_ptr(), d, m, ids.data_ptr(), topk, wts_d.data_ptr(), topk, topk, gg, gu, gd, out_d.data_ptr(), d, s))

    def stats_ex():
        v = (C.c_uint64 * 7)()
        L.ns_hip_moe_ffn_stats_ex(v, 7)
        return [int(x) for x in v]

    legs_d = (("composition", {}), ("fused_stretched", {b"moe_gemv_rows": m}), ("device_grouped", {b"moe_ffn_device_rows": device_rows}))
    graphs_d, outs_d = {}, {}
    for name, keys in legs_d:
        for key, v in keys.items():
            L.ns_hip_set_tuning(key, v)
        device_chain(st)
        torch.cuda.synchronize()
        s0 = stats_ex()
        gd_ = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gd_):
            device_chain(C.c_void_p(torch.cuda.current_stream().cuda_stream))
        s1 = stats_ex()
        device[name + "_calls"] = {"fused": s1[0] - s0[0], "composition": s1[1] - s0[1], "grouped": s1[3] - s0[3], "device_grouped": s1[4] - s0[4]}
        for key in keys:
            L.ns_hip_set_tuning(key, 0)
        gd_.replay(); torch.cuda.synchronize()
        outs_d[name] = out_d.clone()
        graphs_d[name] = gd_
    reps_d = 10
    times_d = {k: [] for k in graphs_d}
    for _ in range(7):
        for k, gb in graphs_d.items():
            gb.replay(); torch.cuda.synchronize()
            e0.record()
            for _ in range(reps_d):
                gb.replay()
            e1.record(); torch.cuda.synchronize()
            times_d[k].append(e0.elapsed_time(e1) * 1e3 / reps_d / nlay)
    for k, v in times_d.items():
        device["us_per_layer_" + k] = {"median": round(float(np.median(v)), 1), "min": round(min(v), 1), "max": round(max(v), 1)}
    device["act"], device["device_rows_key"] = act_name, device_rows
    ref_d = outs_d["composition"].double()
    for k in ("fused_stretched", "device_grouped"):
        device[k + "_rel_l2_vs_composition"] = float("%.3g" % ((outs_d[k].double() - ref_d).norm() / ref_d.norm()).item())
    # parity of the device-grouped leg's token 0 against the fp64 oracle over both selections
    hostd = lambda t: (lambda b: (b.__setitem__(slice(None), t.cpu().numpy()), b)[1])(nso.aligned_bytes(t.numel()))
    a0d, refd = a[:1].cpu().numpy(), np.zeros((1, d))
    for sel in range(topk):
        ex = int(ids_np[0, sel])
        (wg, _), (wu, _), (wd, _) = layers[-1]
        hg, hu = nso.gemm_f64(a0d, hostd(wg[ex][1])), nso.gemm_f64(a0d, hostd(wu[ex][1]))
        refd += float(wts_d[0, sel]) * nso.gemm_f64((act_f64(hg) * hu).astype(np.float32), hostd(wd[ex][1]))
    device["device_grouped_parity_rel_l2_vs_fp64_oracle_token0"] = float("%.3g" % nso.rel_l2(outs_d["device_grouped"][:1].cpu().numpy(), refd))
# parity of the last layer's last selection (token 0): silu(a Wg) * (a Wu) then Wd, fp64 over the oracle's blobs
(wg, _), (wu, _), (wd, _) = layers[-1]
e = int(ids_np[0, topk - 1])
host = lambda t: (lambda b: (b.__setitem__(slice(None), t.cpu().numpy()), b)[1])(nso.aligned_bytes(t.numel()))
a0 = a[:1].cpu().numpy()
hg = nso.gemm_f64(a0, host(wg[e][1])).astype(np.float64)
hu = nso.gemm_f64(a0, host(wu[e][1])).astype(np.float64)
t = (hg / (1.0 + np.exp(-hg)) * hu).astype(np.float32)
ref = nso.gemm_f64(t, host(wd[e][1]))
par = nso.rel_l2(y[topk - 1][:1].cpu().numpy(), ref)
touched = sum(w[0][e2][0].stream_bytes for w in layers[0] for e2 in set(ids_np.reshape(-1).tolist())) if m > 1 else \
    sum(layers[0][j][0][int(ex)][0].stream_bytes for j in range(3) for ex in ids_np[0])
print(json.dumps({"what": "Mixtral-8x7B-shaped MoE FFN (8 x {14336x4096 gate, up; 4096x14336 down}, top-2, int4 g32 bf16), %d token(s)" % m,
                  "us_per_moe_ffn_layer": round(us, 2), "expert_weight_bytes_touched_per_layer": int(touched),
                  "hbm_GBps_over_touched_weights": round(touched / us / 1e3, 1), "tokens_per_s_of_32_moe_ffn_layers": round(m * 1e6 / (32 * us), 1),
                  "parity_rel_l2_vs_fp64_oracle_token0": float("%.3g" % par), "launches_per_layer": 3 * topk,
                  "grouped_by_expert": m >= 32 and os.environ.get("NS_MOE_GROUPED_ROWS", "32") != "0",
                  "tflops": round(m * topk * 3 * 2.0 * d * ff / us / 1e6, 1), "moe_ffn_" + act_name: block, "moe_ffn_prompt": prompt, "moe_ffn_device": device}))

#!/usr/bin/env python3
"""Batched decode over an FP8 (E4M3) paged kv cache against the same step over the fp16 paged cache: one layer's RoPE + kv-cache append + attention for
a batch of independent requests, the twelve shapes and the method of scripts/attn_paged_bench.py —
  (h<bk>)  fp16  ns_hip_rope_qkv_append_paged + ns_hip_attn_decode_paged
  (f<bk>)  FP8   ns_hip_rope_qkv_append_paged_f8 + ns_hip_attn_decode_paged_f8
over blocks of 16 keys in identity order, blocks of 128 keys in identity order, and blocks of 16 keys in a random permutation of the pool (suffix r).
The FP8 pools hold the E4M3 codes of the fp16 pools' values under a scale of 1/8.

Per shape: LAYERS distinct caches, one HIP graph of LAYERS steps per leg, the legs replayed in turn within one process; a leg's figure is the median
over ROUNDS rounds of (event time of REPLAYS replays) / (REPLAYS x LAYERS), its spread the min .. max over the rounds.  The bar of the FP8 entries'
change: at no shape is an FP8 leg's median above its fp16 leg's [min, max]; the script reports every pair and the shapes that miss it.  Needs the GPU.

Usage: scripts/attn_paged_f8_bench.py [--out FILE] [--quick]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402

HEADS = [(32, 32, 128), (32, 8, 128)]  # (head_num, heads_kv, head_size): Llama-2-7B, Llama-3-8B / Mistral-7B
BATCHES = [2, 8, 32]
CAPACITY = 4096
LAYERS, REPLAYS, ROUNDS = 4, 20, 7
SCALE = 0.125
PAIRS = [("16", 16, False), ("128", 128, False), ("16r", 16, True)]  # (suffix, block_keys, permuted)


def lengths(kind, bs):
    if kind == "equal":
        return [2048] * bs
    return [int(round(128 * (4096 / 128) ** (i / (bs - 1)))) for i in range(bs)]  # mixed: spread geometrically from 128 to 4096


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--quick", action="store_true", help="two shapes, two rounds (a rehearsal of the script)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("attn_paged_f8_bench: no GPU")
    pkg = ge.load_package()
    L = pkg.lib()
    s = torch.cuda.Stream()
    shapes = [(h, b, kind) for h in HEADS for b in BATCHES for kind in ("equal", "mixed")]
    rounds = ROUNDS
    if args.quick:
        shapes, rounds = shapes[:2], 2
    results = []
    with torch.cuda.stream(s):
        st = C.c_void_p(s.cuda_stream)
        for (hn, hkv, hs), bs, kind in shapes:
            lens = lengths(kind, bs)
            gen = torch.Generator(device="cuda").manual_seed(bs * 1009 + hkv + len(kind))
            kc = [(torch.randn((bs, CAPACITY, hkv, hs), generator=gen, device="cuda", dtype=torch.float16)) for _ in range(LAYERS)]
            vc = [(torch.randn((bs, CAPACITY, hkv, hs), generator=gen, device="cuda", dtype=torch.float16)) for _ in range(LAYERS)]
            k8 = [(x.float() / SCALE).to(torch.float8_e4m3fn).view(torch.uint8) for x in kc]
            v8 = [(x.float() / SCALE).to(torch.float8_e4m3fn).view(torch.uint8) for x in vc]
            q = torch.randn((bs, 1, hn, hs), generator=gen, device="cuda")
            k = torch.randn((bs, hkv, hs), generator=gen, device="cuda")
            v = torch.randn((bs, hkv, hs), generator=gen, device="cuda")
            pos = torch.tensor([n - 1 for n in lens], dtype=torch.int32, device="cuda")  # the step's own key lands at len - 1; the attention adds 1
            c_sl, c_head = hkv * hs, hs
            scale = hs ** -0.5

            def table(bk, permuted):
                n = bs * (CAPACITY // bk)
                ids = torch.randperm(n, generator=torch.Generator().manual_seed(bk + bs)) if permuted else torch.arange(n)
                return ids.to(torch.int32).reshape(bs, CAPACITY // bk).cuda()

            def leg(f8, qq, outs, bk, tab):
                page = (C.c_void_p(tab.data_ptr()), CAPACITY // bk, bk, bs * (CAPACITY // bk), bk * hkv * hs)
                kp, vp = (k8, v8) if f8 else (kc, vc)
                for il in range(LAYERS):
                    a = pkg.attn_args(qq.data_ptr(), kp[il].data_ptr(), vp[il].data_ptr(), outs[il].data_ptr(), bs, hn, hkv, hs, 1, CAPACITY, scale, pkg.ATTN_CAUSAL)
                    rope = (qq.data_ptr(), k.data_ptr(), v.data_ptr(), kp[il].data_ptr(), vp[il].data_ptr(), bs, hn, hkv, hs, pos.data_ptr(), CAPACITY, hs, 0,
                            10000.0, 1.0, 0.0, 1.0)
                    if f8:
                        a.K_sc = a.V_sc = SCALE
                        pkg.check(L.ns_hip_rope_qkv_append_paged_f8(*rope, *page, c_sl, c_head, SCALE, SCALE, st))
                        pkg.check(L.ns_hip_attn_decode_paged_f8(C.byref(a), C.c_void_p(pos.data_ptr()), 1, *page, None, st))
                    else:
                        pkg.check(L.ns_hip_rope_qkv_append_paged(*rope, *page, c_sl, c_head, st))
                        pkg.check(L.ns_hip_attn_decode_paged(C.byref(a), C.c_void_p(pos.data_ptr()), 1, *page, None, st))

            legs = []  # (name, graph, outputs of the first step, the buffers the graph holds pointers to: kept alive with it)
            for suffix, bk, permuted in PAIRS:
                tab = table(bk, permuted)
                for f8 in (False, True):
                    qq = q.clone()  # (rotated in place by every step: each leg its own)
                    outs = [torch.zeros_like(q) for _ in range(LAYERS)]
                    leg(f8, qq, outs, bk, tab)  # eager: loads code objects, grows the stream's scratch outside the capture
                    s.synchronize()
                    first = [o.clone() for o in outs]
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g, stream=s):
                        leg(f8, qq, outs, bk, tab)
                    for _ in range(3):
                        g.replay()
                    s.synchronize()
                    legs.append((("f" if f8 else "h") + suffix, g, first, (qq, outs, tab)))
            times = {name: [] for name, _, _, _ in legs}
            for _ in range(rounds):
                for name, g, _, _ in legs:  # the legs in turn: drift of the box hits all alike
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(s)
                    for _ in range(REPLAYS):
                        g.replay()
                    e1.record(s)
                    s.synchronize()
                    times[name].append(e0.elapsed_time(e1) / (REPLAYS * LAYERS) * 1e3)
            assert all(bool(torch.all(torch.isfinite(o))) for _, _, first, _ in legs for o in first)
            row = {"heads": hn, "heads_kv": hkv, "head_size": hs, "batch": bs, "lengths": kind, "min_len": min(lens), "max_len": max(lens), "capacity": CAPACITY}
            for n, t in times.items():
                row["%s_us" % n] = round(statistics.median(t), 2)
                row["%s_min_max" % n] = [round(min(t), 2), round(max(t), 2)]
            for suffix, _, _ in PAIRS:
                row["f%s_over_h%s" % (suffix, suffix)] = round(row["f%s_us" % suffix] / row["h%s_us" % suffix], 3)
            row["misses_the_bar"] = [suffix for suffix, _, _ in PAIRS if row["f%s_us" % suffix] > row["h%s_min_max" % suffix][1]]
            results.append(row)
            print(json.dumps(row), flush=True)
            del kc, vc, k8, v8, legs
            torch.cuda.empty_cache()
    summary = {"layers": LAYERS, "replays": REPLAYS, "rounds": rounds, "device": torch.cuda.get_device_name(0),
               "shapes_that_miss_the_bar": sum(1 for r in results if r["misses_the_bar"])}
    print(json.dumps(summary), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("one layer's RoPE + kv-append + decode attention for a batch of requests, us per layer step (median of %d rounds [min, max]); capacity %d;\n"
                    "(h..) fp16 paged pair, (f..) FP8 paged pair; blocks of 16 / 128 keys in identity order, 16r: blocks of 16 in a random permutation\n"
                    % (rounds, CAPACITY))
            names = [x + suffix for suffix, _, _ in PAIRS for x in "hf"]
            f.write("%-8s %5s %-6s %11s | %s | %s\n" % ("heads", "batch", "set", "lengths", " | ".join("%24s" % ("(%s)" % n) for n in names),
                                                    " ".join("%10s" % ("f%s/h%s" % (x, x)) for x, _, _ in PAIRS)))
            cell = lambda r, n: "%8.2f [%6.2f, %6.2f]" % ((r["%s_us" % n],) + tuple(r["%s_min_max" % n]))
            for r in results:
                f.write("%-8s %5d %-6s %11s | %s | %s\n" % ("%d/%d" % (r["heads"], r["heads_kv"]), r["batch"], r["lengths"], "%d..%d" % (r["min_len"], r["max_len"]),
                                                        " | ".join(cell(r, n) for n in names), " ".join("%10.3f" % r["f%s_over_h%s" % (x, x)] for x, _, _ in PAIRS)))
            f.write("\n")
            for r in results:
                f.write(json.dumps(r) + "\n")
            f.write(json.dumps(summary) + "\n")


if __name__ == "__main__":
    main()

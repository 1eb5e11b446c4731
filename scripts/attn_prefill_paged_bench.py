#!/usr/bin/env python3
"""Prompt-sized query blocks over a paged kv cache: one layer's attention of a step whose requests bring many query rows, in the forms the library has
(the method of scripts/attn_block_paged_bench.py) —
  (a) query blocks   ns_hip_attn_block_paged with max_q = the step's longest chunk (context ranges + merge, partials in `tmp`);
  (b) prompt blocks  ns_hip_attn_prefill_paged (one launch of the 128-row kernel's PAGED instantiation);
  (c) uniform        single-request steps only: ns_hip_attn_fp32_fp16_fp16_fp32_forward_h on a contiguous copy of the same keys — (b) / (c) is the
                     price of paging.
Causal, head size 128, 32 / 32 and 32 / 8 heads, pages of 64 keys in a random permutation of the pool, capacity 4096.  Steps: one chunk of 2048 from
position 0; 512 rows over 2048 cached keys; 4 requests x 256 rows at 1024 .. 4096 keys; one chunk of 128 and one of 64 at 2048 keys; 8 x 16 rows at
2048 keys.

Per step: LAYERS distinct caches (a replay does not find its K / V in the Infinity Cache from the layer before), one HIP graph of LAYERS calls per leg,
the legs replayed in turn within one process; a leg's figure is the median over ROUNDS rounds of (event time of REPLAYS replays) / (REPLAYS x LAYERS),
its spread the min .. max over the rounds.  No pass bar: the script reports (a) / (b) and (b) / (c) per step with the spreads, and the rel_l2 between
the legs' outputs.  Needs the GPU; fails without one.

Usage: scripts/attn_prefill_paged_bench.py [--out FILE] [--quick]"""
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
CAPACITY, BLOCK = 4096, 64
LAYERS, REPLAYS, ROUNDS = 4, 10, 7
STEPS = [  # (name, query rows per request, live keys per request — the step's own keys included)
    ("1x2048@2048", [2048], [2048]),
    ("1x512@2560", [512], [2560]),
    ("4x256@1024..4096", [256] * 4, [1024, 2048, 3072, 4096]),
    ("1x128@2048", [128], [2048]),
    ("1x64@2048", [64], [2048]),
    ("8x16@2048", [16] * 8, [2048] * 8),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--quick", action="store_true", help="two steps, two rounds (a rehearsal of the script)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("attn_prefill_paged_bench: no GPU")
    pkg = ge.load_package()
    L = pkg.lib()
    s = torch.cuda.Stream()
    cases = [(h, st) for h in HEADS for st in STEPS]
    rounds = ROUNDS
    if args.quick:
        cases, rounds = cases[3:5], 2
    results = []
    with torch.cuda.stream(s):
        st = C.c_void_p(s.cuda_stream)
        for (hn, hkv, hs), (name, qlens, kvlens) in cases:
            bs, rows, ts, max_q = len(qlens), sum(qlens), CAPACITY // BLOCK, max(qlens)
            gen = torch.Generator(device="cuda").manual_seed(rows * 1009 + hkv)
            kc = [torch.randn((bs * ts, BLOCK, hkv, hs), generator=gen, device="cuda", dtype=torch.float16) for _ in range(LAYERS)]
            vc = [torch.randn((bs * ts, BLOCK, hkv, hs), generator=gen, device="cuda", dtype=torch.float16) for _ in range(LAYERS)]
            q = torch.randn((rows, hn, hs), generator=gen, device="cuda")
            start = [sum(qlens[:b]) for b in range(bs + 1)]
            dstart = torch.tensor(start, dtype=torch.int32, device="cuda")
            dlens = torch.tensor(kvlens, dtype=torch.int32, device="cuda")
            table = torch.randperm(bs * ts, generator=torch.Generator().manual_seed(hkv + rows)).to(torch.int32).reshape(bs, ts).cuda()
            block_step, scale = BLOCK * hkv * hs, hs ** -0.5
            page = (C.c_void_p(table.data_ptr()), ts, BLOCK, bs * ts, block_step)
            ws_bytes = L.ns_hip_attn_block_paged_workspace_size(bs, hn, hkv, hs, max_q, CAPACITY)
            ws = torch.empty(max(ws_bytes, 64), dtype=torch.uint8, device="cuda")
            flat = None
            if bs == 1:  # (c): the request's keys, contiguous, per layer
                nb = -(-kvlens[0] // BLOCK)
                ids = table[0, :nb].long()
                flat = [(kc[il][ids].reshape(nb * BLOCK, hkv, hs)[:kvlens[0]].contiguous(), vc[il][ids].reshape(nb * BLOCK, hkv, hs)[:kvlens[0]].contiguous())
                        for il in range(LAYERS)]

            def paged_args(il, dst):
                return pkg.attn_args(q.data_ptr(), kc[il].data_ptr(), vc[il].data_ptr(), dst.data_ptr(), bs, hn, hkv, hs, max_q, CAPACITY, scale, pkg.ATTN_CAUSAL)

            def leg_query_blocks(outs):
                for il in range(LAYERS):
                    a = paged_args(il, outs[il])
                    a.tmp = ws.data_ptr()
                    pkg.check(L.ns_hip_attn_block_paged(C.byref(a), C.c_void_p(dstart.data_ptr()), C.c_void_p(dlens.data_ptr()), 0, *page, None, st))

            def leg_prompt_blocks(outs):
                for il in range(LAYERS):
                    pkg.check(L.ns_hip_attn_prefill_paged(C.byref(paged_args(il, outs[il])), C.c_void_p(dstart.data_ptr()), C.c_void_p(dlens.data_ptr()), 0, *page,
                                                          None, st))

            def leg_uniform(outs):
                for il in range(LAYERS):
                    a = pkg.attn_args(q.data_ptr(), flat[il][0].data_ptr(), flat[il][1].data_ptr(), outs[il].data_ptr(), 1, hn, hkv, hs, qlens[0], kvlens[0], scale,
                                      pkg.ATTN_CAUSAL)
                    pkg.check(L.ns_hip_attn_fp32_fp16_fp16_fp32_forward_h(C.byref(a), None, st))

            legs = []  # (name, graph, outputs of the first step, the buffers the graph holds pointers to: kept alive with it)
            for leg, fn in (("a", leg_query_blocks), ("b", leg_prompt_blocks)) + ((("c", leg_uniform),) if flat else ()):
                outs = [torch.zeros_like(q) for _ in range(LAYERS)]
                fn(outs)  # eager: loads code objects outside the capture
                s.synchronize()
                first = [o.clone() for o in outs]
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=s):
                    fn(outs)
                for _ in range(3):
                    g.replay()
                s.synchronize()
                legs.append((leg, g, first, outs))
            times = {leg: [] for leg, _, _, _ in legs}
            for _ in range(rounds):
                for leg, g, _, _ in legs:  # the legs in turn: drift of the box hits all alike
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(s)
                    for _ in range(REPLAYS):
                        g.replay()
                    e1.record(s)
                    s.synchronize()
                    times[leg].append(e0.elapsed_time(e1) / (REPLAYS * LAYERS) * 1e3)
            outs_of = {leg: first for leg, _, first, _ in legs}
            rel = lambda x, y: max(float(torch.linalg.norm(b - a) / torch.linalg.norm(a)) for a, b in zip(outs_of[x], outs_of[y]))
            assert all(bool(torch.all(torch.isfinite(o))) for o in outs_of["b"])
            med = {n: statistics.median(t) for n, t in times.items()}
            spread = {n: (min(t), max(t)) for n, t in times.items()}
            row = {"heads": hn, "heads_kv": hkv, "head_size": hs, "step": name, "requests": bs, "rows": rows, "block_keys": BLOCK, "capacity": CAPACITY,
                   "rel_l2_b_vs_a": round(rel("a", "b"), 6)}
            if flat:
                row["rel_l2_b_vs_c"] = round(rel("c", "b"), 6)
            for n in times:
                row["%s_us" % n] = round(med[n], 2)
                row["%s_min_max" % n] = [round(spread[n][0], 2), round(spread[n][1], 2)]
            row["a_over_b"] = round(med["a"] / med["b"], 3)
            if flat:
                row["b_over_c"] = round(med["b"] / med["c"], 3)
            # causal pairs (row, key) the step computes: 4 hs flops each (Q.K and P.V)
            pairs = sum(ql * (kl - ql) + ql * (ql + 1) // 2 for ql, kl in zip(qlens, kvlens))
            row["b_tflops"] = round(4.0 * hs * hn * pairs / (med["b"] * 1e-6) / 1e12, 1)
            results.append(row)
            print(json.dumps(row), flush=True)
            del kc, vc, legs, flat
            torch.cuda.empty_cache()
    summary = {"layers": LAYERS, "replays": REPLAYS, "rounds": rounds, "device": torch.cuda.get_device_name(0)}
    print(json.dumps(summary), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("one layer's causal attention of a step on pages of %d keys in a random permutation, us per call (median of %d rounds [min, max]); capacity %d\n"
                    % (BLOCK, rounds, CAPACITY))
            f.write("(a) ns_hip_attn_block_paged, max_q = the longest chunk   (b) ns_hip_attn_prefill_paged   (c) uniform forward_h on a contiguous copy\n")
            f.write("%-6s %-18s %5s | %28s | %28s | %28s | %7s %7s %7s\n" % ("heads", "step", "rows", "(a)", "(b)", "(c)", "(a)/(b)", "(b)/(c)", "(b) TF"))
            cell = lambda r, n: "%9.2f [%8.2f, %8.2f]" % ((r["%s_us" % n],) + tuple(r["%s_min_max" % n])) if "%s_us" % n in r else "%28s" % "-"
            for r in results:
                f.write("%-6s %-18s %5d | %s | %s | %s | %7.3f %7s %7.1f\n" % ("%d/%d" % (r["heads"], r["heads_kv"]), r["step"], r["rows"], cell(r, "a"), cell(r, "b"),
                                                                          cell(r, "c"), r["a_over_b"], "%.3f" % r["b_over_c"] if "b_over_c" in r else "-", r["b_tflops"]))
            f.write("\n")
            for r in results:
                f.write(json.dumps(r) + "\n")
            f.write(json.dumps(summary) + "\n")


if __name__ == "__main__":
    main()

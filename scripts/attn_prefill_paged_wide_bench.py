#!/usr/bin/env python3
"""Prompt-sized query blocks over a paged kv cache at head size 256: one layer's attention of a step whose requests bring many query rows, in the
forms the library has (the method of scripts/attn_prefill_paged_bench.py) —
  (a) rows as requests  the only form such rows had on pages before ns_hip_attn_prefill_paged_wide: every query row a request of its own to
                        ns_hip_attn_decode_paged, over a table that repeats its request's row (the context is streamed once per row);
  (b) wide prompt blocks  ns_hip_attn_prefill_paged_wide (one launch of attn_wide_paged_kernel);
  (c) uniform           single-request steps only: ns_hip_attn_fp32_fp16_fp16_fp32_forward_h (attn_mfma2_hs256_kernel) on a contiguous copy of the
                        same keys — not a serving alternative: (b) / (c) is the price of paging.
Causal, GPT-J 16 / 16 x 256 and Gemma-2B 8 / 1 x 256, pages of 64 keys in a random permutation of the pool, capacity 4096.  Steps: one chunk of 2048
from position 0; 512 rows over 2048 cached keys; (GPT-J) 4 requests x 256 rows at 1024 .. 4096 keys.

Per step: LAYERS distinct caches (a replay does not find its K / V in the Infinity Cache from the layer before), one HIP graph of LAYERS calls per leg,
the legs replayed in turn within one process; a leg's figure is the median over ROUNDS rounds of (event time of REPLAYS replays) / (REPLAYS x LAYERS),
its spread the min .. max over the rounds.  The claim under test: (b) beats (a) by more than the two legs' combined spread at 512 rows and more —
exit status 1 where (b)'s max is not below (a)'s min.  Reports (b) / (c) and the rel_l2 between the legs' outputs.  Needs the GPU; fails without one.

Usage: scripts/attn_prefill_paged_wide_bench.py [--out FILE] [--quick]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402

HEADS = [(16, 16, 256), (8, 1, 256)]  # (head_num, heads_kv, head_size): GPT-J-6B, Gemma-2B
CAPACITY, BLOCK = 4096, 64
LAYERS, REPLAYS, ROUNDS = 4, 10, 7
STEPS = [  # (name, query rows per request, live keys per request — the step's own keys included)
    ("1x2048@2048", [2048], [2048]),
    ("1x512@2560", [512], [2560]),
    ("4x256@1024..4096", [256] * 4, [1024, 2048, 3072, 4096]),  # (GPT-J only)
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--quick", action="store_true", help="two steps, two rounds (a rehearsal of the script)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("attn_prefill_paged_wide_bench: no GPU")
    pkg = ge.load_package()
    L = pkg.lib()
    s = torch.cuda.Stream()
    cases = [(h, st) for h in HEADS for st in STEPS if h[1] > 1 or len(st[1]) == 1]
    rounds = ROUNDS
    if args.quick:
        cases, rounds = cases[1:3], 2
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
            # (a): row i of request b is a request of kv_len_b - q_len_b + i + 1 keys over request b's table row
            row_req = [b for b in range(bs) for _ in range(qlens[b])]
            row_table = table[torch.tensor(row_req, device="cuda")].contiguous()
            row_lens = torch.tensor([kvlens[b] - qlens[b] + i + 1 for b in range(bs) for i in range(qlens[b])], dtype=torch.int32, device="cuda")
            flat = None
            if bs == 1:  # (c): the request's keys, contiguous, per layer
                nb = -(-kvlens[0] // BLOCK)
                ids = table[0, :nb].long()
                flat = [(kc[il][ids].reshape(nb * BLOCK, hkv, hs)[:kvlens[0]].contiguous(), vc[il][ids].reshape(nb * BLOCK, hkv, hs)[:kvlens[0]].contiguous())
                        for il in range(LAYERS)]

            def paged_args(il, dst):
                return pkg.attn_args(q.data_ptr(), kc[il].data_ptr(), vc[il].data_ptr(), dst.data_ptr(), bs, hn, hkv, hs, max_q, CAPACITY, scale, pkg.ATTN_CAUSAL)

            def leg_rows_as_requests(outs):
                for il in range(LAYERS):
                    a = pkg.attn_args(q.data_ptr(), kc[il].data_ptr(), vc[il].data_ptr(), outs[il].data_ptr(), rows, hn, hkv, hs, 1, CAPACITY, scale, pkg.ATTN_CAUSAL)
                    pkg.check(L.ns_hip_attn_decode_paged(C.byref(a), C.c_void_p(row_lens.data_ptr()), 0, C.c_void_p(row_table.data_ptr()), ts, BLOCK, bs * ts,
                                                         block_step, None, st))

            def leg_prompt_blocks(outs):
                for il in range(LAYERS):
                    pkg.check(L.ns_hip_attn_prefill_paged_wide(C.byref(paged_args(il, outs[il])), C.c_void_p(dstart.data_ptr()), C.c_void_p(dlens.data_ptr()), 0, *page,
                                                          None, st))

            def leg_uniform(outs):
                for il in range(LAYERS):
                    a = pkg.attn_args(q.data_ptr(), flat[il][0].data_ptr(), flat[il][1].data_ptr(), outs[il].data_ptr(), 1, hn, hkv, hs, qlens[0], kvlens[0], scale,
                                      pkg.ATTN_CAUSAL)
                    pkg.check(L.ns_hip_attn_fp32_fp16_fp16_fp32_forward_h(C.byref(a), None, st))

            legs = []  # (name, graph, outputs of the first step, the buffers the graph holds pointers to: kept alive with it)
            for leg, fn in (("a", leg_rows_as_requests), ("b", leg_prompt_blocks)) + ((("c", leg_uniform),) if flat else ()):
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
            row["b_beats_a"] = bool(spread["b"][1] < spread["a"][0])
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
            f.write("(a) every row a request of ns_hip_attn_decode_paged   (b) ns_hip_attn_prefill_paged_wide   (c) uniform forward_h on a contiguous copy\n")
            f.write("%-6s %-18s %5s | %28s | %28s | %28s | %7s %7s %7s\n" % ("heads", "step", "rows", "(a)", "(b)", "(c)", "(a)/(b)", "(b)/(c)", "(b) TF"))
            cell = lambda r, n: "%9.2f [%8.2f, %8.2f]" % ((r["%s_us" % n],) + tuple(r["%s_min_max" % n])) if "%s_us" % n in r else "%28s" % "-"
            for r in results:
                f.write("%-6s %-18s %5d | %s | %s | %s | %7.3f %7s %7.1f\n" % ("%d/%d" % (r["heads"], r["heads_kv"]), r["step"], r["rows"], cell(r, "a"), cell(r, "b"),
                                                                          cell(r, "c"), r["a_over_b"], "%.3f" % r["b_over_c"] if "b_over_c" in r else "-", r["b_tflops"]))
            f.write("\n")
            for r in results:
                f.write(json.dumps(r) + "\n")
            f.write(json.dumps(summary) + "\n")
    if not all(r["b_beats_a"] for r in results if r["rows"] >= 512):
        sys.exit(1)


if __name__ == "__main__":
    main()

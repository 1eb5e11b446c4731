#!/usr/bin/env python3
"""Prompt-sized query blocks over an FP8 (E4M3) paged kv cache at head size 256: one layer's attention of a step whose requests bring many query rows
(the steps and the method of scripts/attn_prefill_paged_wide_bench.py) —
  (a) rows as requests  the only form such rows had on an FP8 pool at this width before ns_hip_attn_prefill_paged_wide_f8: every query row a request
                        of its own to ns_hip_attn_decode_paged_f8, over a table that repeats its request's row;
  (b) fp16 twin         ns_hip_attn_prefill_paged_wide over fp16 pools of the decoded values: what a server had to keep beside the FP8 pool;
  (c) FP8 wide blocks   ns_hip_attn_prefill_paged_wide_f8 (one launch of attn_wide_paged8_kernel).
Causal, GPT-J 16 / 16 x 256 and Gemma-2B 8 / 1 x 256, pages of 64 keys in a random permutation of the pool, capacity 4096.

Per step: LAYERS distinct caches, one HIP graph of LAYERS calls per leg, the legs replayed in turn within one process; a leg's figure is the median
over ROUNDS rounds of (event time of REPLAYS replays) / (REPLAYS x LAYERS), its spread the min .. max over the rounds.  The claim under test: at every
step (c)'s max lies below (a)'s min — exit status 1 otherwise.  (c) / (b) is reported with both spreads and promised nothing; rel_l2 of (c) against
(b) must be 0 (exit status 1 otherwise).  Needs the GPU; fails without one.

Usage: scripts/attn_prefill_paged_wide_f8_bench.py [--out FILE] [--quick] [--ablation]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402
from attn_prefill_paged_wide_bench import BLOCK, CAPACITY, HEADS, LAYERS, REPLAYS, ROUNDS, STEPS  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--quick", action="store_true", help="two steps, two rounds (a rehearsal of the script)")
    ap.add_argument("--ablation", action="store_true", help="times only: for a library built with -DNS_AW8_NODECODE=1, whose (c) is wrong by construction")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("attn_prefill_paged_wide_f8_bench: no GPU")
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
            codes = lambda: torch.randn((bs * ts, BLOCK, hkv, hs), generator=gen, device="cuda").to(torch.float8_e4m3fn)
            k8, v8 = [codes() for _ in range(LAYERS)], [codes() for _ in range(LAYERS)]
            k16, v16 = [x.to(torch.float16) for x in k8], [x.to(torch.float16) for x in v8]  # (exact: every E4M3 value is an fp16 value)
            q = torch.randn((rows, hn, hs), generator=gen, device="cuda")
            dstart = torch.tensor([sum(qlens[:b]) for b in range(bs + 1)], dtype=torch.int32, device="cuda")
            dlens = torch.tensor(kvlens, dtype=torch.int32, device="cuda")
            table = torch.randperm(bs * ts, generator=torch.Generator().manual_seed(hkv + rows)).to(torch.int32).reshape(bs, ts).cuda()
            block_step, scale = BLOCK * hkv * hs, hs ** -0.5
            page = (C.c_void_p(table.data_ptr()), ts, BLOCK, bs * ts, block_step)
            # (a): row i of request b is a request of kv_len_b - q_len_b + i + 1 keys over request b's table row
            row_req = [b for b in range(bs) for _ in range(qlens[b])]
            row_table = table[torch.tensor(row_req, device="cuda")].contiguous()
            row_lens = torch.tensor([kvlens[b] - qlens[b] + i + 1 for b in range(bs) for i in range(qlens[b])], dtype=torch.int32, device="cuda")

            def leg_rows_as_requests(outs):
                for il in range(LAYERS):
                    a = pkg.attn_args(q.data_ptr(), k8[il].data_ptr(), v8[il].data_ptr(), outs[il].data_ptr(), rows, hn, hkv, hs, 1, CAPACITY, scale, pkg.ATTN_CAUSAL)
                    pkg.check(L.ns_hip_attn_decode_paged_f8(C.byref(a), C.c_void_p(row_lens.data_ptr()), 0, C.c_void_p(row_table.data_ptr()), ts, BLOCK, bs * ts,
                                                            block_step, None, st))

            def leg_blocks(entry, kc, vc):
                def run(outs):
                    for il in range(LAYERS):
                        a = pkg.attn_args(q.data_ptr(), kc[il].data_ptr(), vc[il].data_ptr(), outs[il].data_ptr(), bs, hn, hkv, hs, max_q, CAPACITY, scale, pkg.ATTN_CAUSAL)
                        pkg.check(entry(C.byref(a), C.c_void_p(dstart.data_ptr()), C.c_void_p(dlens.data_ptr()), 0, *page, None, st))
                return run

            legs = []  # (name, graph, outputs of the first step, the buffers the graph holds pointers to: kept alive with it)
            for leg, fn in (("a", leg_rows_as_requests), ("b", leg_blocks(L.ns_hip_attn_prefill_paged_wide, k16, v16)),
                            ("c", leg_blocks(L.ns_hip_attn_prefill_paged_wide_f8, k8, v8))):
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
            assert args.ablation or all(bool(torch.all(torch.isfinite(o))) for o in outs_of["c"])
            med = {n: statistics.median(t) for n, t in times.items()}
            spread = {n: (min(t), max(t)) for n, t in times.items()}
            row = {"heads": hn, "heads_kv": hkv, "head_size": hs, "step": name, "requests": bs, "rows": rows, "block_keys": BLOCK, "capacity": CAPACITY,
                   "rel_l2_c_vs_a": round(rel("a", "c"), 6), "rel_l2_c_vs_b": rel("b", "c")}
            for n in times:
                row["%s_us" % n] = round(med[n], 2)
                row["%s_min_max" % n] = [round(spread[n][0], 2), round(spread[n][1], 2)]
            row["a_over_c"], row["c_over_b"] = round(med["a"] / med["c"], 3), round(med["c"] / med["b"], 3)
            pairs = sum(ql * (kl - ql) + ql * (ql + 1) // 2 for ql, kl in zip(qlens, kvlens))  # causal (row, key) pairs: 4 hs flops each
            row["c_tflops"] = round(4.0 * hs * hn * pairs / (med["c"] * 1e-6) / 1e12, 1)
            row["c_beats_a"] = bool(spread["c"][1] < spread["a"][0])
            row["c_median_above_b_max"] = bool(med["c"] > spread["b"][1])
            results.append(row)
            print(json.dumps(row), flush=True)
            del k8, v8, k16, v16, legs
            torch.cuda.empty_cache()
    summary = {"layers": LAYERS, "replays": REPLAYS, "rounds": rounds, "device": torch.cuda.get_device_name(0)}
    print(json.dumps(summary), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("one layer's causal attention of a step on pages of %d keys in a random permutation, us per call (median of %d rounds [min, max]); capacity %d\n"
                    % (BLOCK, rounds, CAPACITY))
            f.write("(a) every row a request of ns_hip_attn_decode_paged_f8   (b) ns_hip_attn_prefill_paged_wide on fp16 pools of the decoded values   "
                    "(c) ns_hip_attn_prefill_paged_wide_f8\n")
            f.write("%-6s %-18s %5s | %28s | %28s | %28s | %7s %7s %7s\n" % ("heads", "step", "rows", "(a)", "(b)", "(c)", "(a)/(c)", "(c)/(b)", "(c) TF"))
            cell = lambda r, n: "%9.2f [%8.2f, %8.2f]" % ((r["%s_us" % n],) + tuple(r["%s_min_max" % n]))
            for r in results:
                f.write("%-6s %-18s %5d | %s | %s | %s | %7.3f %7.3f %7.1f\n" % ("%d/%d" % (r["heads"], r["heads_kv"]), r["step"], r["rows"], cell(r, "a"), cell(r, "b"),
                                                                            cell(r, "c"), r["a_over_c"], r["c_over_b"], r["c_tflops"]))
            f.write("\n")
            for r in results:
                f.write(json.dumps(r) + "\n")
            f.write(json.dumps(summary) + "\n")
    if not args.ablation and not all(r["c_beats_a"] and r["rel_l2_c_vs_b"] == 0.0 for r in results):
        sys.exit(1)


if __name__ == "__main__":
    main()

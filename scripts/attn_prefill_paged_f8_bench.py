#!/usr/bin/env python3
"""Prompt-sized query blocks over an FP8 (E4M3) paged kv cache: one layer's attention of the twelve steps of scripts/attn_prefill_paged_bench.py, by its
method, in three legs —
  (a) ns_hip_attn_block_paged_f8 with max_q = the step's longest chunk (context ranges + merge, partials in `tmp`): what an FP8 pool had;
  (b) ns_hip_attn_prefill_paged on fp16 pools holding the codes' values, the same scales: the 128-row kernel's fp16 form;
  (c) ns_hip_attn_prefill_paged_f8 on the FP8 pools: the new entry.
(a) and (b) are the code the entry was built beside.  Causal, head size 128, 32 / 32 and 32 / 8 heads, pages of 64 keys in a random permutation, capacity
4096; LAYERS distinct caches per step in one HIP graph per leg, the legs replayed in turn; a leg's figure is the median over ROUNDS rounds of (event time
of REPLAYS replays) / (REPLAYS x LAYERS), its spread the min .. max over the rounds.

The bar: at no step may (c)'s median lie above (b)'s [min, max] — byte elements must not make the 128-row kernel slower than its fp16 form.  Exit status
1 if a step misses it.  (c) must hold (b)'s bits.  (a) / (c) per step is reported for the caller's choice between the two FP8 entries.  Needs the GPU.

Usage: scripts/attn_prefill_paged_f8_bench.py [--out FILE] [--quick]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402
from attn_prefill_paged_bench import BLOCK, CAPACITY, HEADS, LAYERS, REPLAYS, ROUNDS, STEPS  # noqa: E402

K_SC, V_SC = 0.125, 0.125


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--quick", action="store_true", help="two steps, two rounds (a rehearsal of the script)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("attn_prefill_paged_f8_bench: no GPU")
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
            draw = lambda: (torch.randn((bs * ts, BLOCK, hkv, hs), generator=gen, device="cuda") * (1.0 / K_SC)).to(torch.float8_e4m3fn)
            k8, v8 = [draw() for _ in range(LAYERS)], [draw() for _ in range(LAYERS)]
            k16, v16 = [x.to(torch.float16) for x in k8], [x.to(torch.float16) for x in v8]  # the codes' values: exact
            q = torch.randn((rows, hn, hs), generator=gen, device="cuda")
            dstart = torch.tensor([sum(qlens[:b]) for b in range(bs + 1)], dtype=torch.int32, device="cuda")
            dlens = torch.tensor(kvlens, dtype=torch.int32, device="cuda")
            table = torch.randperm(bs * ts, generator=torch.Generator().manual_seed(hkv + rows)).to(torch.int32).reshape(bs, ts).cuda()
            page = (C.c_void_p(table.data_ptr()), ts, BLOCK, bs * ts, BLOCK * hkv * hs)
            ws = torch.empty(max(L.ns_hip_attn_block_paged_workspace_size(bs, hn, hkv, hs, max_q, CAPACITY), 64), dtype=torch.uint8, device="cuda")

            def call(entry, kp, vp, dst, tmp=False):
                a = pkg.attn_args(q.data_ptr(), kp.data_ptr(), vp.data_ptr(), dst.data_ptr(), bs, hn, hkv, hs, max_q, CAPACITY, hs ** -0.5, pkg.ATTN_CAUSAL)
                a.K_sc, a.V_sc = K_SC, V_SC
                if tmp:
                    a.tmp = ws.data_ptr()
                pkg.check(entry(C.byref(a), C.c_void_p(dstart.data_ptr()), C.c_void_p(dlens.data_ptr()), 0, *page, None, st))

            fns = {"a": lambda outs: [call(L.ns_hip_attn_block_paged_f8, k8[il], v8[il], outs[il], True) for il in range(LAYERS)],
                   "b": lambda outs: [call(L.ns_hip_attn_prefill_paged, k16[il], v16[il], outs[il]) for il in range(LAYERS)],
                   "c": lambda outs: [call(L.ns_hip_attn_prefill_paged_f8, k8[il], v8[il], outs[il]) for il in range(LAYERS)]}
            legs = []  # (name, graph, outputs of the first step, the buffers the graph holds pointers to: kept alive with it)
            for leg, fn in fns.items():
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
            med = {n: statistics.median(t) for n, t in times.items()}
            row = {"heads": hn, "heads_kv": hkv, "head_size": hs, "step": name, "requests": bs, "rows": rows, "block_keys": BLOCK, "capacity": CAPACITY,
                   "rel_l2_c_vs_a": round(rel("a", "c"), 6), "c_bits_equal_b": all(torch.equal(x, y) for x, y in zip(outs_of["b"], outs_of["c"])),
                   "finite": all(bool(torch.all(torch.isfinite(o))) for o in outs_of["c"])}
            for n, t in times.items():
                row["%s_us" % n] = round(med[n], 2)
                row["%s_min_max" % n] = [round(min(t), 2), round(max(t), 2)]
            row["c_over_b"], row["a_over_c"] = round(med["c"] / med["b"], 3), round(med["a"] / med["c"], 3)
            row["bar_met"] = med["c"] <= max(times["b"])
            results.append(row)
            print(json.dumps(row), flush=True)
            del k8, v8, k16, v16, legs
            torch.cuda.empty_cache()
    summary = {"layers": LAYERS, "replays": REPLAYS, "rounds": rounds, "device": torch.cuda.get_device_name(0),
               "bar_met_at_every_step": all(r["bar_met"] for r in results), "bits_equal_at_every_step": all(r["c_bits_equal_b"] and r["finite"] for r in results)}
    print(json.dumps(summary), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("one layer's causal attention of a step on pages of %d keys in a random permutation, us per call (median of %d rounds [min, max]); capacity %d\n"
                    % (BLOCK, rounds, CAPACITY))
            f.write("(a) ns_hip_attn_block_paged_f8, max_q = the longest chunk   (b) ns_hip_attn_prefill_paged, fp16 pools of the codes' values   "
                    "(c) ns_hip_attn_prefill_paged_f8\nbar: (c)'s median not above (b)'s max\n")
            f.write("%-6s %-18s %5s | %28s | %28s | %28s | %7s %7s %4s\n" % ("heads", "step", "rows", "(a)", "(b)", "(c)", "(c)/(b)", "(a)/(c)", "bar"))
            cell = lambda r, n: "%9.2f [%8.2f, %8.2f]" % ((r["%s_us" % n],) + tuple(r["%s_min_max" % n]))
            for r in results:
                f.write("%-6s %-18s %5d | %s | %s | %s | %7.3f %7.3f %4s\n" % ("%d/%d" % (r["heads"], r["heads_kv"]), r["step"], r["rows"], cell(r, "a"), cell(r, "b"),
                                                                         cell(r, "c"), r["c_over_b"], r["a_over_c"], "met" if r["bar_met"] else "MISS"))
            f.write("\n")
            for r in results:
                f.write(json.dumps(r) + "\n")
            f.write(json.dumps(summary) + "\n")
    sys.exit(0 if summary["bar_met_at_every_step"] and summary["bits_equal_at_every_step"] else 1)


if __name__ == "__main__":
    main()

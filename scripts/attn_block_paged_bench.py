#!/usr/bin/env python3
"""Ragged query blocks over a paged kv cache: one layer's RoPE + kv-cache append + attention of a step in which requests bring several query rows, in
the two forms the library has (the method of scripts/attn_paged_bench.py) —
  (a) rows as requests  ns_hip_rope_qkv_append_paged + ns_hip_attn_decode_paged with every query row a request of its own: its request's table row
                        duplicated, its own length kv_len - q_len + i + 1;
  (b) query blocks      ns_hip_rope_qkv_append_paged_seq + ns_hip_attn_block_paged on the requests as they are.
Head size 128, blocks of 64 keys in identity order, capacity 4096.  Steps: 8 requests x 4 rows and x 16 rows at 2048 keys; a mixed step of 7 decode
rows and one 64-row chunk, the requests' lengths spread geometrically from 128 to 4096 (the chunk belongs to the request of 927 keys); 1 x 64 rows at
2048 keys.

Per step: LAYERS distinct caches (a replay does not find its K / V in the Infinity Cache from the layer before), one HIP graph of LAYERS steps per leg,
the legs replayed in turn within one process; a leg's figure is the median over ROUNDS rounds of (event time of REPLAYS replays) / (REPLAYS x LAYERS),
its spread the min .. max over the rounds.  No pass bar: the script reports (a) / (b) per step with the spreads.  Needs the GPU; fails without one.

Usage: scripts/attn_block_paged_bench.py [--out FILE] [--quick]"""
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
LAYERS, REPLAYS, ROUNDS = 4, 20, 7
MIXED = [int(round(128 * (4096 / 128) ** (i / 7))) for i in range(8)]
STEPS = [  # (name, query rows per request, live keys per request — the step's own keys included)
    ("8x4@2048", [4] * 8, [2048] * 8),
    ("8x16@2048", [16] * 8, [2048] * 8),
    ("7x1+1x64@128..4096", [1, 1, 1, 1, 64, 1, 1, 1], MIXED),
    ("1x64@2048", [64], [2048]),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--quick", action="store_true", help="two steps, two rounds (a rehearsal of the script)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("attn_block_paged_bench: no GPU")
    pkg = ge.load_package()
    L = pkg.lib()
    s = torch.cuda.Stream()
    cases = [(h, st) for h in HEADS for st in STEPS]
    rounds = ROUNDS
    if args.quick:
        cases, rounds = cases[:2], 2
    results = []
    with torch.cuda.stream(s):
        st = C.c_void_p(s.cuda_stream)
        for (hn, hkv, hs), (name, qlens, kvlens) in cases:
            bs, rows, ts = len(qlens), sum(qlens), CAPACITY // BLOCK
            gen = torch.Generator(device="cuda").manual_seed(rows * 1009 + hkv)
            kc = [torch.randn((bs * ts, BLOCK, hkv, hs), generator=gen, device="cuda", dtype=torch.float16) for _ in range(LAYERS)]
            vc = [torch.randn((bs * ts, BLOCK, hkv, hs), generator=gen, device="cuda", dtype=torch.float16) for _ in range(LAYERS)]
            q = torch.randn((rows, hn, hs), generator=gen, device="cuda")
            k = torch.randn((rows, hkv, hs), generator=gen, device="cuda")
            v = torch.randn((rows, hkv, hs), generator=gen, device="cuda")
            req = [b for b in range(bs) for _ in range(qlens[b])]
            pos = [kvlens[b] - qlens[b] + i for b in range(bs) for i in range(qlens[b])]  # a row's own key; it sees pos + 1 keys
            start = [sum(qlens[:b]) for b in range(bs + 1)]
            dpos = torch.tensor(pos, dtype=torch.int32, device="cuda")
            dreq = torch.tensor(req, dtype=torch.int32, device="cuda")
            dstart = torch.tensor(start, dtype=torch.int32, device="cuda")
            dlens = torch.tensor(kvlens, dtype=torch.int32, device="cuda")
            table = torch.arange(bs * ts, dtype=torch.int32).reshape(bs, ts).cuda()
            table_rows = table[dreq.long()].contiguous()  # (a): one table row per query row
            c_sl, c_head, block_step, scale = hkv * hs, hs, BLOCK * hkv * hs, hs ** -0.5
            ws_bytes = L.ns_hip_attn_block_paged_workspace_size(bs, hn, hkv, hs, max(qlens), CAPACITY)
            ws = torch.empty(max(ws_bytes, 64), dtype=torch.uint8, device="cuda")

            def args_of(qq, il, dst, batch, sl_q):
                return pkg.attn_args(qq.data_ptr(), kc[il].data_ptr(), vc[il].data_ptr(), dst.data_ptr(), batch, hn, hkv, hs, sl_q, CAPACITY, scale, pkg.ATTN_CAUSAL)

            def leg_rows_as_requests(qq, outs):
                page = (C.c_void_p(table_rows.data_ptr()), ts, BLOCK, bs * ts, block_step)
                for il in range(LAYERS):
                    pkg.check(L.ns_hip_rope_qkv_append_paged(qq.data_ptr(), k.data_ptr(), v.data_ptr(), kc[il].data_ptr(), vc[il].data_ptr(), rows, hn, hkv, hs,
                                                             dpos.data_ptr(), CAPACITY, hs, 0, 10000.0, 1.0, 0.0, 1.0, *page, c_sl, c_head, st))
                    pkg.check(L.ns_hip_attn_decode_paged(C.byref(args_of(qq, il, outs[il], rows, 1)), C.c_void_p(dpos.data_ptr()), 1, *page, None, st))

            def leg_query_blocks(qq, outs):
                page = (C.c_void_p(table.data_ptr()), ts, BLOCK, bs * ts, block_step)
                for il in range(LAYERS):
                    pkg.check(L.ns_hip_rope_qkv_append_paged_seq(qq.data_ptr(), k.data_ptr(), v.data_ptr(), kc[il].data_ptr(), vc[il].data_ptr(), rows, hn, hkv, hs,
                                                                 dpos.data_ptr(), CAPACITY, hs, 0, 10000.0, 1.0, 0.0, 1.0, dreq.data_ptr(), bs, *page, c_sl, c_head, st))
                    a = args_of(qq, il, outs[il], bs, max(qlens))
                    a.tmp = ws.data_ptr()
                    pkg.check(L.ns_hip_attn_block_paged(C.byref(a), C.c_void_p(dstart.data_ptr()), C.c_void_p(dlens.data_ptr()), 0, *page, None, st))

            legs = []  # (name, graph, outputs of the first step, the buffers the graph holds pointers to: kept alive with it)
            for leg, fn in (("a", leg_rows_as_requests), ("b", leg_query_blocks)):
                qq = q.clone()  # (rotated in place by every step: each leg its own)
                outs = [torch.zeros_like(q) for _ in range(LAYERS)]
                fn(qq, outs)  # eager: loads code objects, grows the stream's scratch outside the capture
                s.synchronize()
                first = [o.clone() for o in outs]
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=s):
                    fn(qq, outs)
                for _ in range(3):
                    g.replay()
                s.synchronize()
                legs.append((leg, g, first, (qq, outs)))
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
            # the two forms compute the same step (different operand rounding: the project's figure for the pair is rel_l2 2e-4 .. 3e-4)
            rel = max(float(torch.linalg.norm(b - a) / torch.linalg.norm(a)) for a, b in zip(legs[0][2], legs[1][2]))
            assert all(bool(torch.all(torch.isfinite(o))) for o in legs[1][2]) and rel < 1e-3, rel
            med = {n: statistics.median(t) for n, t in times.items()}
            spread = {n: (min(t), max(t)) for n, t in times.items()}
            row = {"heads": hn, "heads_kv": hkv, "head_size": hs, "step": name, "requests": bs, "rows": rows, "block_keys": BLOCK, "capacity": CAPACITY,
                   "rel_l2_b_vs_a": round(rel, 6)}
            for n in times:
                row["%s_us" % n] = round(med[n], 2)
                row["%s_min_max" % n] = [round(spread[n][0], 2), round(spread[n][1], 2)]
            row["a_over_b"] = round(med["a"] / med["b"], 3)
            row["widest_spread_us"] = round(max(hi - lo for lo, hi in spread.values()), 2)
            row["a_minus_b_us"] = round(med["a"] - med["b"], 2)
            results.append(row)
            print(json.dumps(row), flush=True)
            del kc, vc, legs
            torch.cuda.empty_cache()
    summary = {"layers": LAYERS, "replays": REPLAYS, "rounds": rounds, "device": torch.cuda.get_device_name(0)}
    print(json.dumps(summary), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("one layer's RoPE + kv-append + attention of a ragged step on pages of %d keys, us per layer step (median of %d rounds [min, max]); capacity %d\n"
                    % (BLOCK, rounds, CAPACITY))
            f.write("(a) every query row a request of ns_hip_attn_decode_paged   (b) ns_hip_rope_qkv_append_paged_seq + ns_hip_attn_block_paged\n")
            f.write("%-8s %-20s %5s | %26s | %26s | %7s %9s\n" % ("heads", "step", "rows", "(a)", "(b)", "(a)/(b)", "(a)-(b)"))
            cell = lambda r, n: "%8.2f [%7.2f, %7.2f]" % ((r["%s_us" % n],) + tuple(r["%s_min_max" % n]))
            for r in results:
                f.write("%-8s %-20s %5d | %s | %s | %7.3f %9.2f\n" % ("%d/%d" % (r["heads"], r["heads_kv"]), r["step"], r["rows"], cell(r, "a"), cell(r, "b"),
                                                                  r["a_over_b"], r["a_minus_b_us"]))
            f.write("\n")
            for r in results:
                f.write(json.dumps(r) + "\n")
            f.write(json.dumps(summary) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Batched decode over a paged kv cache against the same step on slabs: one layer's RoPE + kv-cache append + attention for a batch of independent
requests (the shapes and the method of scripts/attn_rows_bench.py) —
  (b)     rows   ns_hip_rope_qkv_append_rows + ns_hip_attn_decode_rows on one slab of CAPACITY rows per request;
  (p16)   paged  ns_hip_rope_qkv_append_paged + ns_hip_attn_decode_paged, blocks of 16 keys in identity order (request b's block j is physical block
                 b * table_stride + j);
  (p64)   ... blocks of 64 keys, (p128) ... of 128 keys;
  (p16r)  blocks of 16 keys in a random permutation of the pool.
A pool of position-major blocks in identity order IS the slab array, byte for byte, so (b) and the identity legs read the same memory and their outputs
must hold the same bits (asserted).  (p16r) walks the same pool through a permuted table: the same bytes per step, scattered in 16-key pieces.

Per shape: LAYERS distinct caches (a replay does not find its K / V in the Infinity Cache from the layer before), one HIP graph of LAYERS steps per leg,
the legs replayed in turn within one process; a leg's figure is the median over ROUNDS rounds of (event time of REPLAYS replays) / (REPLAYS x LAYERS),
its spread the min .. max over the rounds.  No pass bar: the script reports (p) / (b) per shape with the spreads.  Needs the GPU; fails without one.

Usage: scripts/attn_paged_bench.py [--out FILE] [--quick]"""
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
LEGS = [("rows", 0, False), ("p16", 16, False), ("p64", 64, False), ("p128", 128, False), ("p16r", 16, True)]  # (name, block_keys, permuted)


def lengths(kind, bs):
    if kind == "equal":
        return [2048] * bs
    return [int(round(128 * (4096 / 128) ** (i / (bs - 1)))) for i in range(bs)]  # mixed: spread geometrically from 128 to 4096


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--quick", action="store_true", help="one shape, two rounds (a rehearsal of the script)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("attn_paged_bench: no GPU")
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
            q = torch.randn((bs, 1, hn, hs), generator=gen, device="cuda")
            k = torch.randn((bs, hkv, hs), generator=gen, device="cuda")
            v = torch.randn((bs, hkv, hs), generator=gen, device="cuda")
            pos = torch.tensor([n - 1 for n in lens], dtype=torch.int32, device="cuda")  # the step's own key lands at len - 1; the attention adds 1
            c_bs, c_sl, c_head = CAPACITY * hkv * hs, hkv * hs, hs
            scale = hs ** -0.5

            def table(bk, permuted):
                n = bs * (CAPACITY // bk)
                ids = torch.randperm(n, generator=torch.Generator().manual_seed(bk + bs)) if permuted else torch.arange(n)
                return ids.to(torch.int32).reshape(bs, CAPACITY // bk).cuda()

            def attn_args(qq, il, dst):
                a = pkg.attn_args(qq.data_ptr(), kc[il].data_ptr(), vc[il].data_ptr(), dst.data_ptr(), bs, hn, hkv, hs, 1, CAPACITY, scale, pkg.ATTN_CAUSAL)
                a.step_k_bs = a.step_v_bs = c_bs
                return a

            def leg_rows(qq, outs, bk, tab):
                for il in range(LAYERS):
                    pkg.check(L.ns_hip_rope_qkv_append_rows(qq.data_ptr(), k.data_ptr(), v.data_ptr(), kc[il].data_ptr(), vc[il].data_ptr(), bs, hn, hkv, hs,
                                                            pos.data_ptr(), CAPACITY, hs, 0, 10000.0, 1.0, 0.0, 1.0, c_bs, c_sl, c_head, st))
                    pkg.check(L.ns_hip_attn_decode_rows(C.byref(attn_args(qq, il, outs[il])), C.c_void_p(pos.data_ptr()), 1, None, st))

            def leg_paged(qq, outs, bk, tab):
                page = (C.c_void_p(tab.data_ptr()), CAPACITY // bk, bk, bs * (CAPACITY // bk), bk * hkv * hs)
                for il in range(LAYERS):
                    pkg.check(L.ns_hip_rope_qkv_append_paged(qq.data_ptr(), k.data_ptr(), v.data_ptr(), kc[il].data_ptr(), vc[il].data_ptr(), bs, hn, hkv, hs,
                                                             pos.data_ptr(), CAPACITY, hs, 0, 10000.0, 1.0, 0.0, 1.0, *page, c_sl, c_head, st))
                    pkg.check(L.ns_hip_attn_decode_paged(C.byref(attn_args(qq, il, outs[il])), C.c_void_p(pos.data_ptr()), 1, *page, None, st))

            legs = []  # (name, graph, outputs of the first step, the buffers the graph holds pointers to: kept alive with it)
            for name, bk, permuted in LEGS:
                fn = leg_paged if bk else leg_rows
                tab = table(bk, permuted) if bk else None
                qq = q.clone()  # (rotated in place by every step: each leg its own)
                outs = [torch.zeros_like(q) for _ in range(LAYERS)]
                fn(qq, outs, bk, tab)  # eager: loads code objects, grows the stream's scratch outside the capture
                s.synchronize()
                first = [o.clone() for o in outs]
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=s):
                    fn(qq, outs, bk, tab)
                for _ in range(3):
                    g.replay()
                s.synchronize()
                legs.append((name, g, first, (qq, outs, tab)))
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
            for name, _, first, _ in legs[1:4]:  # identity order: the slabs' own bytes, so the rows entry's bits
                assert all(torch.equal(o, b) for o, b in zip(first, legs[0][2])), name
            assert all(bool(torch.all(torch.isfinite(o))) for o in legs[4][2])
            med = {n: statistics.median(t) for n, t in times.items()}
            spread = {n: (min(t), max(t)) for n, t in times.items()}
            row = {"heads": hn, "heads_kv": hkv, "head_size": hs, "batch": bs, "lengths": kind, "min_len": min(lens), "max_len": max(lens), "capacity": CAPACITY}
            for n in times:
                row["%s_us" % n] = round(med[n], 2)
                row["%s_min_max" % n] = [round(spread[n][0], 2), round(spread[n][1], 2)]
            for n in times:
                if n != "rows":
                    row["%s_over_rows" % n] = round(med[n] / med["rows"], 3)
            row["widest_spread_us"] = round(max(hi - lo for lo, hi in spread.values()), 2)
            row["p128_minus_rows_us"] = round(med["p128"] - med["rows"], 2)
            results.append(row)
            print(json.dumps(row), flush=True)
            del kc, vc, legs
            torch.cuda.empty_cache()
    summary = {"layers": LAYERS, "replays": REPLAYS, "rounds": rounds, "device": torch.cuda.get_device_name(0),
               "identity_legs_bit_equal_to_rows": True}
    print(json.dumps(summary), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("one layer's RoPE + kv-append + decode attention for a batch of requests, us per layer step (median of %d rounds [min, max]); capacity %d\n"
                    % (rounds, CAPACITY))
            names = [n for n, _, _ in LEGS]
            f.write("%-8s %5s %-6s %11s | %s | %s\n" % ("heads", "batch", "set", "lengths", " | ".join("%24s" % ("(%s)" % n) for n in names),
                                                    " ".join("%10s" % ("%s/(b)" % n) for n in names[1:])))
            cell = lambda r, n: "%8.2f [%6.2f, %6.2f]" % ((r["%s_us" % n],) + tuple(r["%s_min_max" % n]))
            for r in results:
                f.write("%-8s %5d %-6s %11s | %s | %s\n" % ("%d/%d" % (r["heads"], r["heads_kv"]), r["batch"], r["lengths"], "%d..%d" % (r["min_len"], r["max_len"]),
                                                        " | ".join(cell(r, n) for n in names), " ".join("%10.3f" % r["%s_over_rows" % n] for n in names[1:])))
            f.write("\n")
            for r in results:
                f.write(json.dumps(r) + "\n")
            f.write(json.dumps(summary) + "\n")


if __name__ == "__main__":
    main()

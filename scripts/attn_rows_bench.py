#!/usr/bin/env python3
"""Batched decode over per-request context lengths: one layer's RoPE + kv-cache append + attention for a batch of independent requests, three ways —
  (a) loop    the only form without the per-request entries: per request one ns_hip_rope_qkv_append(seq 1) and one
              ns_hip_attn_fp32_fp16_fp16_fp32_forward_h(batch 1, sl_kv = its length) on its slab;
  (b) rows    ns_hip_rope_qkv_append_rows + ns_hip_attn_decode_rows: two calls, one positions array;
  (c) uniform equal-length sets only: ns_hip_rope_qkv_append_rows + the uniform entry with batch_size = B and sl_kv = the length — a grid laid out for
              the live length instead of the capacity; it cannot express the mixed sets.
Every request's slab has CAPACITY rows (a server sizes a slab for the longest context it admits), position-major.

Per shape: LAYERS distinct caches (as the layers of a model are: a replay does not find its K / V in the Infinity Cache from the layer before), one HIP
graph of LAYERS steps per leg, the legs replayed in turn within one process; a leg's figure is the median over ROUNDS rounds of (event time of REPLAYS
replays) / (REPLAYS x LAYERS), its spread the min .. max over the rounds.  (b)'s output is compared with (a)'s on the same inputs.  The verdict per
shape: (b) is not slower than (a) by more than the spread the legs show (b's median <= a's maximum, or the medians within the larger spread).
Needs the GPU; fails without one.

Usage: scripts/attn_rows_bench.py [--out FILE] [--quick]"""
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
        sys.exit("attn_rows_bench: no GPU")
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

            def attn_args(qq, il, dst, batch, b0, sl_kv):
                a = pkg.attn_args(qq.data_ptr(), kc[il][b0].data_ptr(), vc[il][b0].data_ptr(), dst.data_ptr(), batch, hn, hkv, hs, 1, sl_kv, scale, pkg.ATTN_CAUSAL)
                a.step_k_bs = a.step_v_bs = c_bs
                return a

            def rope_rows(qq, il):
                pkg.check(L.ns_hip_rope_qkv_append_rows(qq.data_ptr(), k.data_ptr(), v.data_ptr(), kc[il].data_ptr(), vc[il].data_ptr(), bs, hn, hkv, hs, pos.data_ptr(),
                                                        CAPACITY, hs, 0, 10000.0, 1.0, 0.0, 1.0, c_bs, c_sl, c_head, st))

            def leg_loop(qq, outs):
                for il in range(LAYERS):
                    for b, n in enumerate(lens):
                        pkg.check(L.ns_hip_rope_qkv_append(qq[b].data_ptr(), k[b].data_ptr(), v[b].data_ptr(), kc[il][b].data_ptr(), vc[il][b].data_ptr(), 1, hn, hkv, hs,
                                                           n - 1, hs, 0, 10000.0, 1.0, 0.0, 1.0, c_sl, c_head, st))
                        pkg.check(L.ns_hip_attn_fp32_fp16_fp16_fp32_forward_h(C.byref(attn_args(qq[b], il, outs[il][b], 1, b, n)), None, st))

            def leg_rows(qq, outs):
                for il in range(LAYERS):
                    rope_rows(qq, il)
                    pkg.check(L.ns_hip_attn_decode_rows(C.byref(attn_args(qq, il, outs[il], bs, 0, CAPACITY)), C.c_void_p(pos.data_ptr()), 1, None, st))

            def leg_uniform(qq, outs):
                for il in range(LAYERS):
                    rope_rows(qq, il)
                    pkg.check(L.ns_hip_attn_fp32_fp16_fp16_fp32_forward_h(C.byref(attn_args(qq, il, outs[il], bs, 0, lens[0])), None, st))

            legs = []  # (name, graph, outputs of the first step, the buffers the graph holds pointers to: kept alive with it)
            for name, fn in [("loop", leg_loop), ("rows", leg_rows)] + ([("uniform", leg_uniform)] if kind == "equal" else []):
                qq = q.clone()  # (rotated in place by every step: each leg its own)
                outs = [torch.zeros_like(q) for _ in range(LAYERS)]
                fn(qq, outs)  # eager: loads code objects, grows the stream's scratch outside the capture
                s.synchronize()
                first = [o.clone() for o in outs]  # one rotation of q: what the legs' outputs are compared on
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=s):
                    fn(qq, outs)
                for _ in range(3):
                    g.replay()
                s.synchronize()
                legs.append((name, g, first, (qq, outs)))
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
            err = max(float((o - b).norm() / b.norm()) for o, b in zip(legs[1][2], legs[0][2]))
            per = [["%.2g" % float((o[b] - r[b]).norm() / r[b].norm()) for b in range(bs)] for o, r in zip(legs[1][2], legs[0][2])]
            assert err < 2e-6, (err, per)  # two one-row launches that split a context differently (tests/test_gpu_attn_rows.py)
            med = {n: statistics.median(t) for n, t in times.items()}
            spread = {n: (min(t), max(t)) for n, t in times.items()}
            widest = max(hi - lo for lo, hi in spread.values())
            row = {"heads": hn, "heads_kv": hkv, "head_size": hs, "batch": bs, "lengths": kind, "min_len": min(lens), "max_len": max(lens), "capacity": CAPACITY}
            for n in times:
                row["%s_us" % n] = round(med[n], 2)
                row["%s_min_max" % n] = [round(spread[n][0], 2), round(spread[n][1], 2)]
            row["rows_over_loop"] = round(med["rows"] / med["loop"], 3)
            row["rows_over_uniform"] = round(med["rows"] / med["uniform"], 3) if "uniform" in med else None
            row["rows_not_slower_than_loop"] = bool(med["rows"] <= spread["loop"][1] or med["rows"] - med["loop"] <= widest)
            row["rel_l2_rows_vs_loop"] = float("%.2g" % err)
            results.append(row)
            print(json.dumps(row), flush=True)
            del kc, vc, legs
            torch.cuda.empty_cache()
    summary = {"layers": LAYERS, "replays": REPLAYS, "rounds": rounds, "device": torch.cuda.get_device_name(0),
               "rows_not_slower_than_loop_everywhere": all(r["rows_not_slower_than_loop"] for r in results)}
    print(json.dumps(summary), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("one layer's RoPE + kv-append + decode attention for a batch of requests, us per layer step (median of %d rounds [min, max]); capacity %d\n"
                    % (rounds, CAPACITY))
            f.write("%-8s %5s %-6s %11s | %24s | %24s | %24s | %9s %12s\n" % ("heads", "batch", "set", "lengths", "(a) loop", "(b) rows", "(c) uniform", "(b) / (a)", "(b) / (c)"))
            cell = lambda r, n: "%8.2f [%6.2f, %6.2f]" % ((r["%s_us" % n],) + tuple(r["%s_min_max" % n])) if "%s_us" % n in r else "-"
            for r in results:
                f.write("%-8s %5d %-6s %11s | %24s | %24s | %24s | %9.3f %12s\n" % (
                    "%d/%d" % (r["heads"], r["heads_kv"]), r["batch"], r["lengths"], "%d..%d" % (r["min_len"], r["max_len"]), cell(r, "loop"), cell(r, "rows"),
                    cell(r, "uniform"), r["rows_over_loop"], "%.3f" % r["rows_over_uniform"] if r["rows_over_uniform"] else "-"))
            f.write("\n")
            for r in results:
                f.write(json.dumps(r) + "\n")
            f.write(json.dumps(summary) + "\n")


if __name__ == "__main__":
    main()

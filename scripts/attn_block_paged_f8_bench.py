#!/usr/bin/env python3
"""Ragged query blocks over an FP8 (E4M3) paged kv cache: one layer's RoPE + kv-cache append + attention of a step in which requests bring several
query rows, on fp16 pools and on FP8 pools of the same values (the method and the eight steps of scripts/attn_block_paged_bench.py) —
  (b)  fp16 pools  ns_hip_rope_qkv_append_paged_seq + ns_hip_attn_block_paged (leg (b) of that script);
  (f8) FP8 pools   ns_hip_rope_qkv_append_paged_seq_f8 + ns_hip_attn_block_paged_f8: the same plan, half the K / V bytes.
Head size 128, blocks of 64 keys in identity order, capacity 4096.  The FP8 pools hold random finite codes under a scale of 1/8, the fp16 pools their
decoded values; the step's own rows are appended by each leg in its own format, so the two outputs differ by those rows' quantisation (reported).

Per step: LAYERS distinct caches (a replay does not find its K / V in the Infinity Cache from the layer before), one HIP graph of LAYERS steps per leg,
the legs replayed in turn within one process; a leg's figure is the median over ROUNDS rounds of (event time of REPLAYS replays) / (REPLAYS x LAYERS),
its spread the min .. max over the rounds.  Bar: at no step may the FP8 median lie above the fp16 leg's max — half the bytes must never cost time.
Exit status 1 if a step misses it.  Needs the GPU; fails without one.

Usage: scripts/attn_block_paged_f8_bench.py [--out FILE] [--quick]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402
from attn_block_paged_bench import BLOCK, CAPACITY, HEADS, LAYERS, REPLAYS, ROUNDS, STEPS  # noqa: E402

SCALE8 = 0.125  # both pools' scale


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--quick", action="store_true", help="two steps, two rounds (a rehearsal of the script)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("attn_block_paged_f8_bench: no GPU")
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

            def codes():  # finite codes of either sign: exponent and mantissa below 0x78 (|value| <= 240 * scale)
                shape = (bs * ts, BLOCK, hkv, hs)
                return torch.randint(0, 0x78, shape, generator=gen, device="cuda", dtype=torch.uint8) | (torch.randint(0, 2, shape, generator=gen, device="cuda", dtype=torch.uint8) << 7)

            k8, v8 = [codes() for _ in range(LAYERS)], [codes() for _ in range(LAYERS)]
            k16, v16 = ([(x.view(torch.float8_e4m3fn).to(torch.float16) * SCALE8) for x in pool] for pool in (k8, v8))
            q = torch.randn((rows, hn, hs), generator=gen, device="cuda")
            k = torch.randn((rows, hkv, hs), generator=gen, device="cuda")
            v = torch.randn((rows, hkv, hs), generator=gen, device="cuda")
            req = [b for b in range(bs) for _ in range(qlens[b])]
            pos = [kvlens[b] - qlens[b] + i for b in range(bs) for i in range(qlens[b])]  # a row's own key; it sees pos + 1 keys
            dpos = torch.tensor(pos, dtype=torch.int32, device="cuda")
            dreq = torch.tensor(req, dtype=torch.int32, device="cuda")
            dstart = torch.tensor([sum(qlens[:b]) for b in range(bs + 1)], dtype=torch.int32, device="cuda")
            dlens = torch.tensor(kvlens, dtype=torch.int32, device="cuda")
            table = torch.arange(bs * ts, dtype=torch.int32).reshape(bs, ts).cuda()
            c_sl, c_head, block_step, scale = hkv * hs, hs, BLOCK * hkv * hs, hs ** -0.5
            page = (C.c_void_p(table.data_ptr()), ts, BLOCK, bs * ts, block_step)
            ws = torch.empty(max(L.ns_hip_attn_block_paged_workspace_size(bs, hn, hkv, hs, max(qlens), CAPACITY), 64), dtype=torch.uint8, device="cuda")

            def leg(f8, qq, outs):
                kc, vc = (k8, v8) if f8 else (k16, v16)
                for il in range(LAYERS):
                    rope = (qq.data_ptr(), k.data_ptr(), v.data_ptr(), kc[il].data_ptr(), vc[il].data_ptr(), rows, hn, hkv, hs, dpos.data_ptr(), CAPACITY, hs, 0,
                            10000.0, 1.0, 0.0, 1.0, dreq.data_ptr(), bs, *page, c_sl, c_head)
                    a = pkg.attn_args(qq.data_ptr(), kc[il].data_ptr(), vc[il].data_ptr(), outs[il].data_ptr(), bs, hn, hkv, hs, max(qlens), CAPACITY, scale,
                                      pkg.ATTN_CAUSAL)
                    a.tmp = ws.data_ptr()
                    tail = (C.byref(a), C.c_void_p(dstart.data_ptr()), C.c_void_p(dlens.data_ptr()), 0, *page, None, st)
                    if f8:
                        a.K_sc = a.V_sc = SCALE8
                        pkg.check(L.ns_hip_rope_qkv_append_paged_seq_f8(*rope, SCALE8, SCALE8, st))
                        pkg.check(L.ns_hip_attn_block_paged_f8(*tail))
                    else:
                        pkg.check(L.ns_hip_rope_qkv_append_paged_seq(*rope, st))
                        pkg.check(L.ns_hip_attn_block_paged(*tail))

            legs = []  # (name, graph, outputs of the first step, the buffers the graph holds pointers to: kept alive with it)
            for tag, f8 in (("b", False), ("f8", True)):
                qq = q.clone()  # (rotated in place by every step: each leg its own)
                outs = [torch.zeros_like(q) for _ in range(LAYERS)]
                leg(f8, qq, outs)  # eager: loads code objects, grows the stream's scratch outside the capture
                s.synchronize()
                first = [o.clone() for o in outs]
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=s):
                    leg(f8, qq, outs)
                for _ in range(3):
                    g.replay()
                s.synchronize()
                legs.append((tag, g, first, (qq, outs)))
            times = {tag: [] for tag, _, _, _ in legs}
            for _ in range(rounds):
                for tag, g, _, _ in legs:  # the legs in turn: drift of the box hits all alike
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(s)
                    for _ in range(REPLAYS):
                        g.replay()
                    e1.record(s)
                    s.synchronize()
                    times[tag].append(e0.elapsed_time(e1) / (REPLAYS * LAYERS) * 1e3)
            rel = max(float(torch.linalg.norm(b - a) / torch.linalg.norm(a)) for a, b in zip(legs[0][2], legs[1][2]))
            assert all(bool(torch.all(torch.isfinite(o))) for o in legs[1][2]) and rel < 5e-2, rel  # (the step's own rows: E4M3 against fp16)
            med = {n: statistics.median(t) for n, t in times.items()}
            spread = {n: (min(t), max(t)) for n, t in times.items()}
            row = {"heads": hn, "heads_kv": hkv, "head_size": hs, "step": name, "requests": bs, "rows": rows, "block_keys": BLOCK, "capacity": CAPACITY,
                   "rel_l2_f8_vs_b": round(rel, 6)}
            for n in times:
                row["%s_us" % n] = round(med[n], 2)
                row["%s_min_max" % n] = [round(spread[n][0], 2), round(spread[n][1], 2)]
            row["f8_over_b"] = round(med["f8"] / med["b"], 3)
            row["bar_f8_median_within_b_max"] = med["f8"] <= spread["b"][1]
            results.append(row)
            print(json.dumps(row), flush=True)
            del k8, v8, k16, v16, legs
            torch.cuda.empty_cache()
    summary = {"layers": LAYERS, "replays": REPLAYS, "rounds": rounds, "device": torch.cuda.get_device_name(0),
               "steps_missing_the_bar": [r["step"] + " %d/%d" % (r["heads"], r["heads_kv"]) for r in results if not r["bar_f8_median_within_b_max"]]}
    print(json.dumps(summary), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("one layer's RoPE + kv-append + attention of a ragged step on pages of %d keys, us per layer step (median of %d rounds [min, max]); capacity %d\n"
                    % (BLOCK, rounds, CAPACITY))
            f.write("(b) fp16 pools: ns_hip_rope_qkv_append_paged_seq + ns_hip_attn_block_paged   (f8) FP8 pools: the _f8 pair\n")
            f.write("%-8s %-20s %5s | %26s | %26s | %8s %s\n" % ("heads", "step", "rows", "(b)", "(f8)", "(f8)/(b)", "bar"))
            cell = lambda r, n: "%8.2f [%7.2f, %7.2f]" % ((r["%s_us" % n],) + tuple(r["%s_min_max" % n]))
            for r in results:
                f.write("%-8s %-20s %5d | %s | %s | %8.3f %s\n" % ("%d/%d" % (r["heads"], r["heads_kv"]), r["step"], r["rows"], cell(r, "b"), cell(r, "f8"),
                                                                 r["f8_over_b"], "ok" if r["bar_f8_median_within_b_max"] else "MISSED"))
            f.write("\n")
            for r in results:
                f.write(json.dumps(r) + "\n")
            f.write(json.dumps(summary) + "\n")
    sys.exit(1 if summary["steps_missing_the_bar"] else 0)


if __name__ == "__main__":
    main()

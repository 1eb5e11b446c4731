#!/usr/bin/env python3
"""Shared-prefix decode over an FP8 (E4M3) paged kv cache: one layer's attention of a decode step whose requests share prompt prefixes (the steps and
the method of scripts/attn_shared_paged_bench.py), in three forms —
  (a) FP8 paged decode     ns_hip_attn_decode_paged_f8 over the aliased tables: every request streams its whole context through its own table row —
                           all an FP8 pool had for such a step before the shared FP8 entry;
  (b) FP8 shared prefix    ns_hip_attn_decode_paged_shared_f8 with the groups named: a group's prefix is streamed once per 64 (member, head) slots;
  (c) fp16 shared prefix   ns_hip_attn_decode_paged_shared over fp16 pools of the decoded values (twice the bytes of (b)).
Head size 128, pages of 64 keys, capacity 4096.  K / V are drawn, then rounded to E4M3 of x / 0.125, so (c)'s pools hold (b)'s values exactly.

Per step: LAYERS distinct caches (a replay does not find its K / V in the Infinity Cache from the layer before), one HIP graph of LAYERS calls per leg,
the legs replayed in turn within one process; a leg's figure is the median over ROUNDS rounds of (event time of REPLAYS replays) / (REPLAYS x LAYERS),
its spread the min .. max over the rounds.  The K / V bytes a leg must read follow from the shapes and are printed beside the times.  Two claims are
reported per step, neither is a pass bar: (a) - (b) above the two legs' combined spread, and (b) - (c) not above theirs.  Needs the GPU; fails without one.

Usage: scripts/attn_shared_paged_f8_bench.py [--out FILE] [--quick]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402
from attn_shared_paged_bench import BLOCK, CAPACITY, HEADS, LAYERS, REPLAYS, ROUNDS, STEPS, SUFFIX  # noqa: E402

SCALE = 0.125  # of both pools
LEGS = {"a": "ns_hip_attn_decode_paged_f8 over the aliased tables", "b": "ns_hip_attn_decode_paged_shared_f8",
        "c": "ns_hip_attn_decode_paged_shared over fp16 pools of the decoded values"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--quick", action="store_true", help="two steps, two rounds (a rehearsal of the script)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("attn_shared_paged_f8_bench: no GPU")
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
        for (hn, hkv, hs), (name, groups, per, prefix) in cases:
            bs, ts = groups * per, CAPACITY // BLOCK
            lens = [(prefix if prefix else 2048) + SUFFIX[b % 8] for b in range(bs)]
            gen = torch.Generator(device="cuda").manual_seed(bs * 1009 + hkv + prefix)
            draw = lambda: (torch.randn((bs * ts, BLOCK, hkv, hs), generator=gen, device="cuda") * (1.0 / SCALE)).clamp_(-448, 448).to(torch.float8_e4m3fn)
            k8, v8 = [draw() for _ in range(LAYERS)], [draw() for _ in range(LAYERS)]
            k16, v16 = ([x.to(torch.float16) * SCALE for x in pools] for pools in (k8, v8))  # exact: every E4M3 value times 2^-3 is an fp16 value
            q = torch.randn((bs, 1, hn, hs), generator=gen, device="cuda")
            table = torch.arange(bs * ts, dtype=torch.int32).reshape(bs, ts)
            for b in range(bs):
                table[b, :prefix // BLOCK] = table[b // per * per, :prefix // BLOCK]  # the leader's blocks below the prefix
            table = table.cuda()
            dstart = torch.tensor([g * per for g in range(groups + 1)], dtype=torch.int32, device="cuda")
            dprefix = torch.tensor([prefix] * groups, dtype=torch.int32, device="cuda")
            dlens = torch.tensor(lens, dtype=torch.int32, device="cuda")
            page = (C.c_void_p(table.data_ptr()), ts, BLOCK, bs * ts, BLOCK * hkv * hs)
            ws = torch.empty(max(L.ns_hip_attn_decode_paged_shared_workspace_size(bs, hn, hkv, hs, per, CAPACITY), 64), dtype=torch.uint8, device="cuda")
            row_bytes = 2 * hkv * hs  # one key's K and V rows of every kv head, in codes
            slot_blocks = -(-per * (hn // hkv) // 64)
            shared_rows = groups * slot_blocks * prefix + sum(n - prefix for n in lens)
            mib = {"a": sum(lens) * row_bytes / 2 ** 20, "b": shared_rows * row_bytes / 2 ** 20, "c": shared_rows * row_bytes * 2 / 2 ** 20}

            def args_of(kp, vp, il, dst, scale):
                a = pkg.attn_args(q.data_ptr(), kp[il].data_ptr(), vp[il].data_ptr(), dst.data_ptr(), bs, hn, hkv, hs, 1, CAPACITY, hs ** -0.5, pkg.ATTN_CAUSAL)
                a.K_sc = a.V_sc = scale
                a.tmp = ws.data_ptr()
                return a

            def leg_a(outs):
                for il in range(LAYERS):
                    a = args_of(k8, v8, il, outs[il], SCALE)
                    a.tmp = None  # (the decode entry's partials: the stream's scratch)
                    pkg.check(L.ns_hip_attn_decode_paged_f8(C.byref(a), C.c_void_p(dlens.data_ptr()), 0, *page, None, st))

            def shared(fn, kp, vp, scale):
                def leg(outs):
                    for il in range(LAYERS):
                        pkg.check(fn(C.byref(args_of(kp, vp, il, outs[il], scale)), C.c_void_p(dstart.data_ptr()), groups, per, C.c_void_p(dprefix.data_ptr()),
                                     C.c_void_p(dlens.data_ptr()), 0, *page, None, st))
                return leg

            legs = []  # (name, graph, outputs of the first step, the buffers the graph holds pointers to: kept alive with it)
            for leg, fn in (("a", leg_a), ("b", shared(L.ns_hip_attn_decode_paged_shared_f8, k8, v8, SCALE)),
                            ("c", shared(L.ns_hip_attn_decode_paged_shared, k16, v16, 1.0))):
                outs = [torch.zeros_like(q) for _ in range(LAYERS)]
                fn(outs)  # eager: loads code objects, grows the stream's scratch outside the capture
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
            # the three forms compute the same step: (b) and (c) share their operand rounding, (a) is another kernel family
            rel = lambda x, y: max(float(torch.linalg.norm(u - w) / torch.linalg.norm(w)) for w, u in zip(legs[x][2], legs[y][2]))
            rel_a, rel_c = rel(0, 1), rel(2, 1)
            assert all(torch.equal(o, f) for _, _, first, outs in legs[1:] for o, f in zip(outs, first))  # every replay of a shared entry: the eager call's bits
            assert all(bool(torch.all(torch.isfinite(o))) for o in legs[1][2]) and rel_a < 1e-3 and rel_c < 2e-4, (rel_a, rel_c)
            med = {n: statistics.median(t) for n, t in times.items()}
            spread = {n: (min(t), max(t)) for n, t in times.items()}
            width = lambda *names: sum(spread[n][1] - spread[n][0] for n in names)
            row = {"heads": hn, "heads_kv": hkv, "head_size": hs, "step": name, "requests": bs, "block_keys": BLOCK, "capacity": CAPACITY,
                   "rel_l2_b_vs_a": round(rel_a, 7), "rel_l2_b_vs_c": round(rel_c, 9)}
            for n in times:
                row["kv_mib_%s" % n] = round(mib[n], 2)
                row["%s_us" % n] = round(med[n], 2)
                row["%s_min_max" % n] = [round(spread[n][0], 2), round(spread[n][1], 2)]
            row["a_over_b"], row["b_over_c"] = round(med["a"] / med["b"], 3), round(med["b"] / med["c"], 3)
            row["a_minus_b_us"], row["spread_ab_us"] = round(med["a"] - med["b"], 2), round(width("a", "b"), 2)
            row["b_minus_c_us"], row["spread_bc_us"] = round(med["b"] - med["c"], 2), round(width("b", "c"), 2)
            row["b_beats_a"], row["b_not_above_c"] = med["a"] - med["b"] > width("a", "b"), med["b"] - med["c"] <= width("b", "c")
            results.append(row)
            print(json.dumps(row), flush=True)
            del k8, v8, k16, v16, legs
            torch.cuda.empty_cache()
    summary = {"layers": LAYERS, "replays": REPLAYS, "rounds": rounds, "device": torch.cuda.get_device_name(0)}
    print(json.dumps(summary), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("one layer's attention of a shared-prefix decode step on FP8 pages of %d keys, us per layer step (median of %d rounds [min, max]); capacity %d\n"
                    % (BLOCK, rounds, CAPACITY))
            for n, text in LEGS.items():
                f.write("(%s) %s\n" % (n, text))
            f.write("MiB: the K / V bytes the leg must read; spreads: the two legs' max - min, summed\n")
            f.write("%-6s %-12s | %7s %26s | %7s %26s | %7s %26s | %7s %8s %8s | %7s %8s %8s\n" % (
                "heads", "step", "MiB", "(a)", "MiB", "(b)", "MiB", "(c)", "(a)/(b)", "(a)-(b)", "spreads", "(b)/(c)", "(b)-(c)", "spreads"))
            cell = lambda r, n: "%7.2f %8.2f [%7.2f, %7.2f]" % ((r["kv_mib_%s" % n], r["%s_us" % n]) + tuple(r["%s_min_max" % n]))
            for r in results:
                f.write("%-6s %-12s | %s | %s | %s | %7.3f %8.2f %8.2f | %7.3f %8.2f %8.2f\n" % (
                    "%d/%d" % (r["heads"], r["heads_kv"]), r["step"], cell(r, "a"), cell(r, "b"), cell(r, "c"), r["a_over_b"], r["a_minus_b_us"],
                    r["spread_ab_us"], r["b_over_c"], r["b_minus_c_us"], r["spread_bc_us"]))
            f.write("\n")
            for r in results:
                f.write(json.dumps(r) + "\n")
            f.write(json.dumps(summary) + "\n")


if __name__ == "__main__":
    main()

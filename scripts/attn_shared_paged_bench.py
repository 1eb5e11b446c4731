#!/usr/bin/env python3
"""Shared-prefix decode over a paged kv cache: one layer's attention of a decode step whose requests share prompt prefixes, in the two forms the library
has (the method of scripts/attn_block_paged_bench.py) —
  (a) paged decode    ns_hip_attn_decode_paged over the aliased tables: every request streams its whole context through its own table row;
  (b) shared prefix   ns_hip_attn_decode_paged_shared with the groups named: a group's prefix is streamed once per 64 (member, head) slots.
Head size 128, pages of 64 keys, capacity 4096; a member's row names its own blocks behind the prefix and the leader's below it.  Steps: one group of 8
and of 32 over prefixes of 1024 and 2048 keys, 32 requests as four groups of 8, 32 groups of one with prefix 0 (nothing shared: the price of the entry
where it cannot win), a group of 32 with a prefix of 256.  Suffixes of 64 .. 512 keys, mixed.

Per step: LAYERS distinct caches (a replay does not find its K / V in the Infinity Cache from the layer before), one HIP graph of LAYERS calls per leg,
the legs replayed in turn within one process; a leg's figure is the median over ROUNDS rounds of (event time of REPLAYS replays) / (REPLAYS x LAYERS),
its spread the min .. max over the rounds.  The K / V bytes a leg must read follow from the shapes and are printed beside the times.  No pass bar: the
script reports (a) / (b) per step with the spreads.  Needs the GPU; fails without one.

Usage: scripts/attn_shared_paged_bench.py [--out FILE] [--quick]"""
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
SUFFIX = [64, 512, 128, 448, 256, 96, 384, 192]  # of member i % 8
STEPS = [  # (name, groups, requests per group, prefix keys)
    ("1x8@1024", 1, 8, 1024),
    ("1x8@2048", 1, 8, 2048),
    ("1x32@1024", 1, 32, 1024),
    ("1x32@2048", 1, 32, 2048),
    ("4x8@2048", 4, 8, 2048),
    ("32x1@0+2048", 32, 1, 0),  # nothing shared: every request's 2048 + suffix keys are its own
    ("1x32@256", 1, 32, 256),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--quick", action="store_true", help="two steps, two rounds (a rehearsal of the script)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("attn_shared_paged_bench: no GPU")
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
            kc = [torch.randn((bs * ts, BLOCK, hkv, hs), generator=gen, device="cuda", dtype=torch.float16) for _ in range(LAYERS)]
            vc = [torch.randn((bs * ts, BLOCK, hkv, hs), generator=gen, device="cuda", dtype=torch.float16) for _ in range(LAYERS)]
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
            row_bytes = 2 * hkv * hs * 2  # one key's K and V rows of every kv head
            slot_blocks = -(-per * (hn // hkv) // 64)
            bytes_a = sum(lens) * row_bytes
            bytes_b = (groups * slot_blocks * prefix + sum(n - prefix for n in lens)) * row_bytes

            def args_of(il, dst):
                return pkg.attn_args(q.data_ptr(), kc[il].data_ptr(), vc[il].data_ptr(), dst.data_ptr(), bs, hn, hkv, hs, 1, CAPACITY, hs ** -0.5, pkg.ATTN_CAUSAL)

            def leg_paged_decode(outs):
                for il in range(LAYERS):
                    pkg.check(L.ns_hip_attn_decode_paged(C.byref(args_of(il, outs[il])), C.c_void_p(dlens.data_ptr()), 0, *page, None, st))

            def leg_shared_prefix(outs):
                for il in range(LAYERS):
                    a = args_of(il, outs[il])
                    a.tmp = ws.data_ptr()
                    pkg.check(L.ns_hip_attn_decode_paged_shared(C.byref(a), C.c_void_p(dstart.data_ptr()), groups, per, C.c_void_p(dprefix.data_ptr()),
                                                                C.c_void_p(dlens.data_ptr()), 0, *page, None, st))

            legs = []  # (name, graph, outputs of the first step, the buffers the graph holds pointers to: kept alive with it)
            for leg, fn in (("a", leg_paged_decode), ("b", leg_shared_prefix)):
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
            # the two forms compute the same step (different operand rounding: the project's figure for the pair of families is rel_l2 2e-4 .. 3e-4)
            rel = max(float(torch.linalg.norm(b - a) / torch.linalg.norm(a)) for a, b in zip(legs[0][2], legs[1][2]))
            assert all(bool(torch.all(torch.isfinite(o))) for o in legs[1][2]) and rel < 1e-3, rel
            med = {n: statistics.median(t) for n, t in times.items()}
            spread = {n: (min(t), max(t)) for n, t in times.items()}
            row = {"heads": hn, "heads_kv": hkv, "head_size": hs, "step": name, "requests": bs, "block_keys": BLOCK, "capacity": CAPACITY,
                   "kv_mib_a": round(bytes_a / 2 ** 20, 2), "kv_mib_b": round(bytes_b / 2 ** 20, 2), "rel_l2_b_vs_a": round(rel, 6)}
            for n in times:
                row["%s_us" % n] = round(med[n], 2)
                row["%s_min_max" % n] = [round(spread[n][0], 2), round(spread[n][1], 2)]
            row["a_over_b"] = round(med["a"] / med["b"], 3)
            row["a_minus_b_us"] = round(med["a"] - med["b"], 2)
            row["combined_spread_us"] = round(sum(hi - lo for lo, hi in spread.values()), 2)
            results.append(row)
            print(json.dumps(row), flush=True)
            del kc, vc, legs
            torch.cuda.empty_cache()
    summary = {"layers": LAYERS, "replays": REPLAYS, "rounds": rounds, "device": torch.cuda.get_device_name(0)}
    print(json.dumps(summary), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("one layer's attention of a shared-prefix decode step on pages of %d keys, us per layer step (median of %d rounds [min, max]); capacity %d\n"
                    % (BLOCK, rounds, CAPACITY))
            f.write("(a) ns_hip_attn_decode_paged over the aliased tables   (b) ns_hip_attn_decode_paged_shared; MiB: the K / V bytes the leg must read\n")
            f.write("%-6s %-12s | %7s %26s | %7s %26s | %7s %8s %8s\n" % ("heads", "step", "MiB", "(a)", "MiB", "(b)", "(a)/(b)", "(a)-(b)", "spreads"))
            cell = lambda r, n: "%8.2f [%7.2f, %7.2f]" % ((r["%s_us" % n],) + tuple(r["%s_min_max" % n]))
            for r in results:
                f.write("%-6s %-12s | %7.2f %s | %7.2f %s | %7.3f %8.2f %8.2f\n" % ("%d/%d" % (r["heads"], r["heads_kv"]), r["step"], r["kv_mib_a"], cell(r, "a"),
                                                                                  r["kv_mib_b"], cell(r, "b"), r["a_over_b"], r["a_minus_b_us"],
                                                                                  r["combined_spread_us"]))
            f.write("\n")
            for r in results:
                f.write(json.dumps(r) + "\n")
            f.write(json.dumps(summary) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""A short block of query rows over a long cache: one attention call with ns_hip_set_tuning("attn_block_split") off — exactly the kernels the default
dispatch launches, the baseline — and on (attn_block_split_kernel + attn_merge_kernel), for a sweep of the path's range rule
("attn_block_wg_target" x "attn_block_min_keys").

Per shape: LAYERS distinct position-major fp16 caches (more bytes than the Infinity Cache holds at the long context, as the layers of a model are),
one HIP graph of LAYERS calls per variant, all variants replayed in turn within one process, REPS rounds; a variant's figure is the median over the
rounds of (event time of REPLAYS replays) / (REPLAYS x LAYERS), its spread the min .. max over the rounds.  The outputs of every variant are
compared with the baseline's on the same inputs.  Needs the GPU; fails without one.

Usage: scripts/attn_block_split_bench.py [--out FILE] [--quick]"""
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
ROWS, KEYS = [4, 16, 64], [2048, 8192]
SWEEP = [(t, m) for t in (128, 256, 512) for m in (128, 256)]
DEFAULT = (512, 128)  # what ships (AttnKnobs::block_target / block_min_keys): put back at the end
LAYERS, REPLAYS, REPS = 8, 25, 7
PATHS = ["refused", "generic", "split_regs", "ring", "rows64", "rows128", "pipelined", "block_split"]


def ranges(hn, hkv, sl_q, sl_kv, target, min_keys):
    """the range rule of ns_attn_plan.cpp, for the table's "ranges" column"""
    cd = lambda a, b: -(-a // b)
    base = hkv * cd(sl_q * (hn // hkv), 64)
    n = min(cd(target, base), max(1, cd(sl_kv, min_keys)), 64)
    kps = cd(cd(sl_kv, n), 64) * 64
    return cd(sl_kv, kps), kps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--quick", action="store_true", help="one shape, two rounds (a rehearsal of the script)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("attn_block_split_bench: no GPU")
    pkg = ge.load_package()
    L = pkg.lib()

    def stats():
        out = (C.c_uint64 * 8)()
        L.ns_hip_attn_stats(out)
        return list(out)

    s = torch.cuda.Stream()
    results = []
    shapes = [(h, r, k) for h in HEADS for r in ROWS for k in KEYS]
    reps = REPS
    if args.quick:
        shapes, reps = shapes[:1], 2
    with torch.cuda.stream(s):
        for (hn, hkv, hs), sl_q, sl_kv in shapes:
            gen = torch.Generator(device="cuda").manual_seed(sl_q * 100003 + sl_kv + hkv)
            kc = [torch.randn((1, sl_kv, hkv, hs), generator=gen, device="cuda").half() for _ in range(LAYERS)]
            vc = [torch.randn((1, sl_kv, hkv, hs), generator=gen, device="cuda").half() for _ in range(LAYERS)]
            q = torch.randn((1, sl_q, hn, hs), generator=gen, device="cuda")
            st = C.c_void_p(s.cuda_stream)

            def step(outs):
                for il in range(LAYERS):
                    a = pkg.attn_args(q.data_ptr(), kc[il].data_ptr(), vc[il].data_ptr(), outs[il].data_ptr(), 1, hn, hkv, hs, sl_q, sl_kv, hs ** -0.5, pkg.ATTN_CAUSAL)
                    pkg.check(L.ns_hip_attn_fp32_fp16_fp16_fp32_forward(C.byref(a), st))

            variants = []  # (name, key value, target, min_keys, graph, outputs, path)
            for name, key, target, mk in [("off", 0) + DEFAULT] + [("on %d/%d" % tm, 1, tm[0], tm[1]) for tm in SWEEP]:
                L.ns_hip_set_tuning(b"attn_block_split", key)
                L.ns_hip_set_tuning(b"attn_block_wg_target", target)
                L.ns_hip_set_tuning(b"attn_block_min_keys", mk)
                outs = [torch.zeros_like(q) for _ in range(LAYERS)]
                before = stats()
                step(outs)  # eager: loads code objects, grows the stream's scratch outside the capture
                s.synchronize()
                moved = [b - a for a, b in zip(before, stats())]
                path = PATHS[moved.index(max(moved))]
                assert sum(moved) == LAYERS and max(moved) == LAYERS, moved
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=s):
                    step(outs)
                for _ in range(3):
                    g.replay()
                s.synchronize()
                variants.append((name, key, target, mk, g, outs, path))
            L.ns_hip_set_tuning(b"attn_block_split", 0)
            L.ns_hip_set_tuning(b"attn_block_wg_target", DEFAULT[0])
            L.ns_hip_set_tuning(b"attn_block_min_keys", DEFAULT[1])
            times = {v[0]: [] for v in variants}
            for _ in range(reps):
                for name, _, _, _, g, _, _ in variants:  # the variants in turn: drift of the box hits all alike
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(s)
                    for _ in range(REPLAYS):
                        g.replay()
                    e1.record(s)
                    s.synchronize()
                    times[name].append(e0.elapsed_time(e1) / (REPLAYS * LAYERS) * 1e3)
            base_outs = variants[0][5]
            base_us = statistics.median(times["off"])
            for name, key, target, mk, _, outs, path in variants:
                err = max(float((o - b).norm() / b.norm()) for o, b in zip(outs, base_outs))
                assert err < 1e-3, (name, err)  # the project's tensor bound: the one-row kernels keep Q and the probabilities in fp32, the matrix cores take fp16
                t = times[name]
                n, kps = ranges(hn, hkv, sl_q, sl_kv, target, mk) if key else (0, 0)
                row = {"heads": hn, "heads_kv": hkv, "head_size": hs, "sl_q": sl_q, "sl_kv": sl_kv, "variant": name, "path": path, "ranges": n, "keys_per_range": kps,
                       "us_per_call": round(statistics.median(t), 2), "us_min": round(min(t), 2), "us_max": round(max(t), 2),
                       "speedup_vs_off": round(base_us / statistics.median(t), 3), "rel_l2_vs_off": float("%.2g" % err)}
                results.append(row)
                print(json.dumps(row), flush=True)
            del kc, vc, variants
            torch.cuda.empty_cache()
    # the best pair: the largest geometric mean of the speed-ups over all shapes
    best = {}
    for name in ["on %d/%d" % tm for tm in SWEEP]:
        sp = [r["speedup_vs_off"] for r in results if r["variant"] == name]
        best[name] = round(float(torch.tensor(sp).log().mean().exp()), 3)
    summary = {"geomean_speedup_vs_off": best, "layers": LAYERS, "replays": REPLAYS, "rounds": reps, "device": torch.cuda.get_device_name(0)}
    print(json.dumps(summary), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for r in results:
                f.write(json.dumps(r) + "\n")
            f.write(json.dumps(summary) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""bench.py — decode throughput of the Llama-2-7B "Q4_0" (BesTLA: int4 sym, group 32, bf16 scales) GEMM chain on MI355X.

A *step* is one pass of the hot path over one token (batch 1): for each of the 32 layers
    QKV  (fused, 3 x 4096->4096)  ->  WO (4096->4096)  ->  FFN gate/up (fused W1,W3 4096->11008, SiLU*mul)
    ->  FFN down (W2 11008->4096)
then lm_head (4096->32000) — 6 607 077 376 weights, 3 716 481 024 algorithmic bytes, all through the
device-resident C ABI of libns_hip.so (include/ns_bestla.h part 3), captured once in a HIP graph and replayed.
Every layer reads the token's seeded input vector (the chain has no norms; see Chain.__init__) and writes its own
output row.  Inputs are resident in HBM when the timed region starts.  Weights are synthetic (seeded torch.randn, quantized and
packed ON THE GPU by the product quantizer into reference-format blobs, then loaded like any reference blob).

N > 1: 1-D tensor parallel exactly as the reference shards Llama (models/model_utils/model_files.h:145-190):
wq/wk/wv/w1/w3 split on N, wo/w2 split on K + one fp32 all-reduce each (RCCL), lm_head replicated; one process per
GPU under torch.distributed.  Total work is fixed -> "scaling": "strong".

Prints ONE JSON line on rank 0.  A plain run sets up, warms up, times exactly --steps steps and reports them
(`ms_per_step`, `value` = tokens/s); --full adds five more timed batches (`value` = their median), the `roofline` and
`cpu_baseline` objects and the other legs (parity, whole token, prefill, int8 semantics, config 4 / 5, reference route).
--dump-outputs DIR writes the last timed step's logits (DIR/logits.npy) and every layer's output (DIR/hidden.npy), float32.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec (MI355X_MICROARCH.md); ~6300 GB/s measured achievable

CFG = dict(name="llama-2-7b", n_embd=4096, n_ff=11008, n_layer=32, n_vocab=32000, group=32, n_head=32)


def REDUCE(t):
    """ne_all_reduce: the TP communication layer's reduce_add (one-shot peer-memory kernel or RCCL, parallel.py)"""
    from neural_speed_amd import parallel as par
    return par.reduce_add(t)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--layers", type=int, default=CFG["n_layer"], help="debug only: fewer layers => INVALID number")
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--chain-only", action="store_true", help="diagnostics: skip the roofline / prefill / CPU legs")
    ap.add_argument("--no-secondary", action="store_true", help="skip the BASELINE config 4 / config 5 legs")
    ap.add_argument("--secondary-only", action="store_true", help="diagnostics: print the config 4 / config 5 legs alone and exit")
    ap.add_argument("--full-token-only", action="store_true", help="diagnostics: print the whole-token leg alone and exit")
    ap.add_argument("--no-reference-route", action="store_true", help="skip the leg that runs the reference's unchanged model_eval on the device route")
    ap.add_argument("--reference-route-only", action="store_true", help="diagnostics: print the reference_route leg alone and exit")
    ap.add_argument("--full", action="store_true",
                    help="also run everything beside the headline: five more timed batches (value = their median), parity "
                         "against the oracle, roofline, whole token / prefill / int8 / config 4-5 legs, CPU baseline, "
                         "reference route, all-reduce latency (TP)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last step computed (rank 0's logits and every layer's "
                         "output) as DIR/<name>.npy")
    return ap.parse_args()


class Chain:
    """Builds the per-rank weights and runs the decode GEMM chain through the C ABI."""

    KEEP_HOST_LAYERS = 4  # host copies for the oracle legs: 4 x 114 MB + lm_head 74 MB = 0.53 GB working set (> any LLC)

    def __init__(self, pkg, n_layers, rank, world, keep_host_layer=False):
        self.pkg, self.L = pkg, pkg.lib()
        self.rank, self.world = rank, world
        self.st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        d, ff, V = CFG["n_embd"], CFG["n_ff"], CFG["n_vocab"]
        assert d % world == 0 and ff % world == 0
        self.d, self.ff, self.V = d, ff, V
        self.dl, self.ffl = d // world, ff // world
        self.layers = []
        self.host_blobs = None
        self.host_layers = []
        self.stream_bytes = 0
        t0 = time.time()
        for il in range(n_layers):
            seed = 1000 + il * 8
            lw = {}
            kh = keep_host_layer and il < self.KEEP_HOST_LAYERS
            # norm-preserving synthetic init: one layer maps an O(1) input to an O(1) output (random data, no zeros)
            lw["q"] = self._make(self.dl, d, seed + 0, d ** -0.5, kh)
            lw["k"] = self._make(self.dl, d, seed + 1, d ** -0.5, kh)
            lw["v"] = self._make(self.dl, d, seed + 2, d ** -0.5, kh)
            lw["o"] = self._make(d, self.dl, seed + 3, d ** -0.5, kh)
            lw["w1"] = self._make(self.ffl, d, seed + 4, d ** -0.5, kh)
            lw["w3"] = self._make(self.ffl, d, seed + 5, d ** -0.5, kh)
            lw["w2"] = self._make(d, self.ffl, seed + 6, (ff ** -0.5) / 0.6, kh)
            if kh:
                if self.host_blobs is None:
                    self.host_blobs = {}
                    self.host_layers = []
                self.host_layers.append({k: v[1] for k, v in lw.items()})
                if il == 0:
                    self.host_blobs = dict(self.host_layers[0])
            self.layers.append({k: v[0] for k, v in lw.items()})
        head = self._make(V, d, 999, d ** -0.5, keep_host_layer)
        if keep_host_layer:
            self.host_blobs["head"] = head[1]
        self.head = head[0]
        torch.cuda.synchronize()
        self.setup_s = time.time() - t0
        dev = "cuda"
        g = torch.Generator(device=dev).manual_seed(7)
        self.x0 = torch.randn((1, d), generator=g, device=dev, dtype=torch.float32)
        # every layer reads the token's input x0 and writes its own row of `hidden`.  The chain has no norms, and without
        # them the gated FFN squares the activations' scale layer after layer: fed from one layer to the next, the fp16
        # shadows overflowed partway through the 32 layers and every logit came out NaN.  Launches, shapes and bytes are the same.
        self.hidden = torch.empty((n_layers, 1, d), device=dev, dtype=torch.float32)
        self.x = self.hidden[n_layers - 1]
        self.qkv = torch.empty((3, 1, self.dl), device=dev, dtype=torch.float32)
        self.attn = torch.empty((1, d), device=dev, dtype=torch.float32)
        self.t2 = torch.empty((1, self.ffl), device=dev, dtype=torch.float32)
        self.logits = torch.empty((1, V), device=dev, dtype=torch.float32)
        # fp16 shadows of the activations (written by the producing GEMM's epilogue, read by the next GEMM's staging)
        self.use_h = os.environ.get("NS_BENCH_NO_SHADOW", "0") != "1"
        # opt-in experiment: "workgroups:fraction" of every weight prefetched beside the previous GEMM run
        pf = os.environ.get("NS_BENCH_PREFETCH", "")
        self.prefetch = (int(pf.split(":")[0]), float(pf.split(":")[1]), pf.split(":")[2:] == ["fine"]) if pf else None
        self.pf_stream = None
        h = torch.float16
        self.x0h = self.x0.to(h)
        self.xh = torch.empty((1, d), device=dev, dtype=h)
        self.qkvh = torch.empty((3, 1, self.dl), device=dev, dtype=h)
        self.attnh = torch.empty((1, d), device=dev, dtype=h)
        self.t2h = torch.empty((1, self.ffl), device=dev, dtype=h)

    def _make(self, n, k, seed, std, keep_host=False):
        pkg, L = self.pkg, self.L
        g = torch.Generator(device="cuda").manual_seed(seed * 64 + self.rank)
        w = torch.randn((n, k), generator=g, device="cuda", dtype=torch.float32) * std
        size = L.ns_BTLAGemmPackBSize(n, k, CFG["group"], pkg.S4, pkg.BF16, False, pkg.COMP_INT8, None)
        blob = torch.zeros(size, dtype=torch.uint8, device="cuda")
        pkg.check(L.ns_hip_quant_pack_device(blob.data_ptr(), w.data_ptr(), n, k, k, CFG["group"], pkg.S4, pkg.BF16,
                                             False, pkg.COMP_INT8, True, self.st), "quant_pack_device")
        wt = pkg.Weight.from_device_blob(blob.data_ptr(), size, self.st)
        torch.cuda.synchronize()
        self.stream_bytes += wt.stream_bytes
        host = blob.cpu().numpy() if keep_host else None
        del w, blob
        return wt, host

    def segments(self):
        """The token step as a list of ("gemm", callable) / ("reduce", tensor) items: the GEMM runs between two
        all-reduces are graph-capturable on their own, the collectives stay outside (TP only)."""
        L, pkg = self.L, self.pkg
        d = self.d
        H = self.use_h
        p = lambda t: t.data_ptr() if H else None
        tp_ = self.world > 1  # after an all-reduce the fp16 shadow of the summed vector is stale: fall back to fp32 A
        items = []
        x_in, x_in_h = self.x0, self.x0h
        for il, lw in enumerate(self.layers):
            x_out = self.hidden[il]

            def attn_block(lw=lw, x_in=x_in, x_in_h=x_in_h):
                st = self.st
                pkg.check(L.ns_hip_fusion_qkv_forward_h(x_in.data_ptr(), p(x_in_h) if x_in_h is not None else None,
                                                        lw["q"].h, lw["k"].h, lw["v"].h, self.qkv.data_ptr(),
                                                        p(self.qkvh), 1, d, self.dl, st))
                # attention itself is outside this chain (its own operator, ns_attn.hip); its output stands in as the
                # Q slice
                pkg.check(L.ns_hip_f32f32_forward_h(self.qkv.data_ptr(), p(self.qkvh), lw["o"].h, self.attn.data_ptr(),
                                                    None if tp_ else p(self.attnh), 1, self.dl, d, pkg.EPI_NONE, None,
                                                    0, st))
            items.append(("gemm", attn_block))
            if tp_:
                items.append(("reduce", self.attn))  # ne_all_reduce after attn-out (llama.cpp:590-593)

            def ffn_block(lw=lw, x_out=x_out):
                st = self.st
                pkg.check(L.ns_hip_fusion_ffn3_forward_h(self.attn.data_ptr(), None if tp_ else p(self.attnh),
                                                         lw["w1"].h, lw["w2"].h, lw["w3"].h, None, self.t2.data_ptr(),
                                                         p(self.t2h), x_out.data_ptr(), None if tp_ else p(self.xh), 1,
                                                         pkg.EPI_SILU, st))
            items.append(("gemm", ffn_block))
            if tp_:
                items.append(("reduce", x_out))  # ne_all_reduce after FFN (llama.cpp:690-694)
            # (layers >= 1 read x0 like layer 0; under TP as fp32 A, the path they took before)
            x_in, x_in_h = self.x0, (None if tp_ else self.x0h)
        x_in, x_in_h = self.x, (None if tp_ else self.xh)

        def head_block(x_in=x_in, x_in_h=x_in_h):
            st = self.st
            pkg.check(L.ns_hip_f32f32_forward_h(x_in.data_ptr(), p(x_in_h) if x_in_h is not None else None, self.head.h,
                                                self.logits.data_ptr(), None, 1, d, self.V, pkg.EPI_NONE, None, 0, st))
        items.append(("gemm", head_block))
        return items

    def step(self):
        if self.prefetch and self.world == 1:
            return self.step_prefetch()
        for kind, it in self.segments():
            if kind == "gemm":
                it()
            else:
                REDUCE(it)

    def block_weights(self):
        """weights streamed by each GEMM run of segments(), in launch order (tp1)"""
        out = []
        for lw in self.layers:
            out.append([lw["q"], lw["k"], lw["v"], lw["o"]])
            out.append([lw["w1"], lw["w3"], lw["w2"]])
        out.append([self.head])
        return out

    def launches(self):
        """tp1 only: the chain as single kernel launches, each with the weights it streams (the same C calls
        segments() makes; the fused FFN entry is its gate/up entry + the down projection, ns_api.cpp)."""
        L, pkg = self.L, self.pkg
        d = self.d
        H = self.use_h
        p = lambda t: t.data_ptr() if H else None
        out = []
        x_in, x_in_h = self.x0, self.x0h
        for il, lw in enumerate(self.layers):
            out.append((lambda lw=lw, x_in=x_in, x_in_h=x_in_h: pkg.check(L.ns_hip_fusion_qkv_forward_h(
                x_in.data_ptr(), p(x_in_h), lw["q"].h, lw["k"].h, lw["v"].h, self.qkv.data_ptr(), p(self.qkvh), 1, d,
                self.dl, self.st)), [lw["q"], lw["k"], lw["v"]]))
            out.append((lambda lw=lw: pkg.check(L.ns_hip_f32f32_forward_h(
                self.qkv.data_ptr(), p(self.qkvh), lw["o"].h, self.attn.data_ptr(), p(self.attnh), 1, self.dl, d,
                pkg.EPI_NONE, None, 0, self.st)), [lw["o"]]))
            out.append((lambda lw=lw: pkg.check(L.ns_hip_fusion_ffn3_gateup_h(
                self.attn.data_ptr(), p(self.attnh), lw["w1"].h, lw["w3"].h, None, self.t2.data_ptr(), p(self.t2h), 1,
                pkg.EPI_SILU, self.st)), [lw["w1"], lw["w3"]]))
            out.append((lambda lw=lw, x_out=self.hidden[il]: pkg.check(L.ns_hip_f32f32_forward_h(
                self.t2.data_ptr(), p(self.t2h), lw["w2"].h, x_out.data_ptr(), p(self.xh), 1, self.ffl, d,
                pkg.EPI_NONE, None, 0, self.st)), [lw["w2"]]))
        x_in, x_in_h = self.x, self.xh
        out.append((lambda x_in=x_in, x_in_h=x_in_h: pkg.check(L.ns_hip_f32f32_forward_h(
            x_in.data_ptr(), p(x_in_h), self.head.h, self.logits.data_ptr(), None, 1, d, self.V, pkg.EPI_NONE, None, 0,
            self.st)), [self.head]))
        return out

    def step_prefetch(self):
        """The same chain with a second stream (a parallel graph branch under capture) that pulls the NEXT GEMM run's
        weights into the Infinity Cache (ns_hip_weight_prefetch) while the current run streams its own: the ramp-up
        and tail of every launch leave HBM idle.  Each prefetch waits for the start of the run
        it runs beside, so it is never more than one run (<= 76 MB) ahead.  NS_BENCH_PREFETCH="workgroups:fraction[:fine]"."""
        L, pkg = self.L, self.pkg
        grid, frac, fine = self.prefetch
        cur = torch.cuda.current_stream()
        if self.pf_stream is None:
            self.pf_stream = torch.cuda.Stream()
        pf = self.pf_stream
        pfh = C.c_void_p(pf.cuda_stream)
        if fine:  # one prefetch per kernel launch instead of one per GEMM run
            blocks, wl = zip(*self.launches())
        else:
            blocks = [it for kind, it in self.segments() if kind == "gemm"]
            wl = self.block_weights()
        assert len(wl) == len(blocks)
        pf.wait_stream(cur)  # fork
        for b, blk in enumerate(blocks):
            if True:  # the last run (lm_head) prefetches layer 0 for the next token: weights are static
                ev = torch.cuda.Event()
                ev.record(cur)
                pf.wait_event(ev)
                for w in wl[(b + 1) % len(blocks)]:
                    pkg.check(L.ns_hip_weight_prefetch(w.h, 0, int(frac * w.stream_bytes), grid, pfh), "prefetch")
            blk()
        cur.wait_stream(pf)  # join


def capture(fn):
    """fn() captured into a CUDAGraph on a side stream; `with torch.cuda.stream` restores the current stream even when
    the capture is invalidated half way (torch.cuda.graph's own __exit__ does not)."""
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        graph.capture_begin()
        try:
            fn()
        except Exception:
            try:
                graph.capture_end()
            except Exception:
                pass
            raise
        graph.capture_end()
    torch.cuda.current_stream().wait_stream(side)
    return graph


def agree_failed(failed, world):
    """max over ranks of a failure flag (collective on every rank when world > 1)"""
    if world == 1:
        return bool(failed)
    flag = torch.tensor([1 if failed else 0], device="cuda", dtype=torch.int32)
    torch.distributed.all_reduce(flag, op=torch.distributed.ReduceOp.MAX)
    return bool(int(flag.item()))


EXTRA_BATCH_MS = []  # time_graph(..., extra_batches=n): wall ms of n further batches of `steps` steps (the spread beside the one reading)


def time_graph(fn, steps, warmup, use_graph, world, extra_batches=0):
    """W warm-up steps, then EXACTLY `steps` timed steps bracketed by barrier + synchronize on both sides."""
    if world > 1:
        torch.distributed.barrier()  # ranks enter their first all-reduce together (the peer-memory kernel's wait is bounded)
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    err = None
    try:
        if use_graph == "segments":
            # TP: one graph per GEMM run between two all-reduces; the collectives are launched eagerly in between, so
            # nothing depends on RCCL being capturable
            plan = [(k, capture(it) if k == "gemm" else it) for k, it in fn.segments()]

            def run():
                for k, it in plan:
                    if k == "gemm":
                        it.replay()
                    else:
                        REDUCE(it)
        elif use_graph:
            run = capture(fn).replay
        else:
            run = fn
    except Exception as e:  # noqa: BLE001 - any capture failure selects the next launch mode
        err = e
        try:
            torch.cuda.synchronize()
        except Exception:  # noqa: BLE001
            pass
        ge.load_package().lib().ns_hip_reset_error()  # an invalidated capture leaves a sticky error behind
    # every rank learns about a failed capture BEFORE any rank replays a captured collective: a rank that went on to
    # its warm-up all-reduces while another one had already given up would pair mismatched collectives
    if agree_failed(err is not None, world):
        raise err if err is not None else RuntimeError("capture failed on another rank")
    for _ in range(warmup):
        run()
    torch.cuda.synchronize()
    if world > 1:
        torch.distributed.barrier()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(steps):
        run()
    e1.record()
    torch.cuda.synchronize()
    if world > 1:
        torch.distributed.barrier()
    torch.cuda.synchronize()
    wall_ms = (time.perf_counter() - t0) * 1e3
    ev_ms = e0.elapsed_time(e1)
    del EXTRA_BATCH_MS[:]
    for _ in range(extra_batches):  # (outside the reported region: VERDICT r04 #9, box-to-box and run-to-run spread)
        tb = time.perf_counter()
        for _ in range(steps):
            run()
        torch.cuda.synchronize()
        EXTRA_BATCH_MS.append((time.perf_counter() - tb) * 1e3)
    return wall_ms, ev_ms


def main():
    args = parse()
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus and world > 1:
        raise SystemExit("--gpus must equal WORLD_SIZE")
    torch.cuda.set_device(local % max(1, torch.cuda.device_count()))
    pkg = ge.load_package()
    from neural_speed_amd import parallel as par  # the replacement of parallel_context.{h,cpp}
    # "nccl" = RCCL over xGMI on ROCm.  NS_DIST_BACKEND=gloo lets the TP code path be smoke-tested with several ranks
    # on ONE GPU (RCCL refuses two ranks per device); numbers from such a run are not bench results.
    backend = os.environ.get("NS_DIST_BACKEND", "nccl")
    pctx = par.init_parallel_context(backend if world > 1 else None)
    # decode-sized all-reduces: one-shot kernel over peer-mapped HBM (xGMI), RCCL otherwise.  NS_P2P=0 keeps RCCL.
    use_p2p = world > 1 and os.environ.get("NS_P2P", "1") != "0" and pctx.enable_p2p(1 << 20)
    # the collectives themselves go through the library's native layer (ns_tp_*: RCCL / the peer-memory kernel behind a
    # C ABI); torch.distributed only bootstraps it (128-byte unique id) and carries the failure flags.  NS_TP_NATIVE=0
    # keeps torch's ProcessGroup all-reduce instead.
    # (NS_TP_RCCL_LIB: a named collective library — with a non-RCCL process group that is the tests' shared-memory stand-in,
    # which lets two ranks share one GPU; such a line is marked INVALID below)
    use_native = (world > 1 and os.environ.get("NS_TP_NATIVE", "1") != "0" and
                  (backend == "nccl" or bool(os.environ.get("NS_TP_RCCL_LIB"))) and pctx.enable_native())
    chain = Chain(pkg, args.layers, rank, world,
                  keep_host_layer=(args.full and rank == 0 and world == 1 and not args.no_cpu_baseline))
    # the chain object itself carries the captured stream handle; under graph capture torch switches the current
    # stream, so the stream pointer handed to the C ABI must be re-read inside the capture.
    class Step:
        """callable token step; segments() re-reads the current stream for every GEMM run (capture switches it)"""

        def __call__(self):
            chain.st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            chain.step()

        def segments(self):
            def wrap(f):
                def g():
                    chain.st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
                    f()
                return g
            return [(k, wrap(it) if k == "gemm" else it) for k, it in chain.segments()]

    step = Step()

    # launch modes, most to least ambitious: True = the whole token in one HIP graph (TP: all-reduces captured too — the
    # peer-memory kernel is an ordinary kernel node, RCCL is capturable through torch's ProcessGroupNCCL), "segments" =
    # one graph per GEMM run + eager all-reduces (TP only), False = eager launches.  With the peer-memory all-reduce
    # enabled the list is walked with it first and, if every mode fails or a flag wait times out, again over RCCL.
    # A failed attempt falls through to the next one; every rank takes the same decisions (failure flags are reduced).
    def launch_modes(p2p_on):
        if args.no_graph:
            return [False]
        if world == 1:
            return [True, False]
        fg = os.environ.get("NS_BENCH_FULL_GRAPH", "1")  # "0": start at "segments"; "force": try True on any backend
        full = fg == "force" or (fg == "1" and (backend == "nccl" or p2p_on))
        return ([True] if full else []) + ["segments", False]

    if args.secondary_only and world == 1:
        print(json.dumps(secondary_configs(pkg)))
        return
    if args.reference_route_only and world == 1:
        print(json.dumps({"reference_route": reference_route()}))
        return
    if args.full_token_only and world == 1:
        ft, _ = full_token(chain, pkg, 2048, fused=True)
        print(json.dumps({"full_token": ft, "full_prefill": full_prefill(chain, pkg, 2048)}))
        return
    attempts = ([(m, True) for m in launch_modes(True)] if use_p2p else []) + [(m, False) for m in launch_modes(False)]
    wall_ms = ev_ms = None
    p2p_dead = False
    for idx, (use_graph, with_p2p) in enumerate(attempts):
        if with_p2p and p2p_dead:
            continue
        if not with_p2p and pctx.p2p_enabled():
            pctx.disable_p2p()  # collective; reduce_add is RCCL from here on
        failed, err = 0, None
        try:
            wall_ms, ev_ms = time_graph(step, args.steps, args.warmup, use_graph, world,
                                        extra_batches=5 if (world == 1 and args.full) else 0)
        except Exception as e:
            failed, err = 1, e
            try:
                torch.cuda.synchronize()
            except Exception:
                pass
            pkg.lib().ns_hip_reset_error()  # an invalidated capture leaves a sticky error behind
        if with_p2p:
            try:
                p2p_dead = pctx.p2p_error()  # collective: a flag wait timed out on some rank -> numbers are void
            except Exception as e:  # noqa: BLE001
                p2p_dead, err = True, err or e
            if p2p_dead and err is None:
                err = RuntimeError("peer-memory all-reduce: a flag wait timed out")
        failed = agree_failed(failed or (with_p2p and p2p_dead), world)
        if not failed:
            break
        if idx == len(attempts) - 1:
            raise err if err is not None else RuntimeError("another rank failed")
        sys.stderr.write("launch mode %r (%s all-reduce) failed (%s); trying the next one\n" %
                         (use_graph, "peer-memory" if with_p2p else "RCCL",
                          str(err).splitlines()[0] if err else "on another rank"))
    if args.dump_outputs and rank == 0:
        # the last timed step's result (every step recomputes it from the same seeded input; lm_head is replicated under TP)
        os.makedirs(args.dump_outputs, exist_ok=True)
        np.save(os.path.join(args.dump_outputs, "logits.npy"), chain.logits.detach().cpu().numpy().astype(np.float32))
        np.save(os.path.join(args.dump_outputs, "hidden.npy"), chain.hidden.detach().cpu().numpy().astype(np.float32))
    comm = (all_reduce_latency(chain, world, pctx.p2p_enabled() or backend == "nccl")
            if (world > 1 and args.full) else None)  # collective
    t = torch.tensor([wall_ms], device="cuda", dtype=torch.float64)
    if world > 1:
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
    wall_ms = float(t.item())
    first_batch_ms = wall_ms
    # N = 1: the line's value is the MEDIAN of six batches of exactly `steps` steps each (the bracketed one + five more, every one between
    # synchronisations) — the single reading moves +-1.5 % between identical runs; the first batch is kept beside it
    if world == 1 and EXTRA_BATCH_MS:
        batches = sorted([wall_ms] + list(EXTRA_BATCH_MS))
        wall_ms = 0.5 * (batches[(len(batches) - 1) // 2] + batches[len(batches) // 2])
    ms_per_step = wall_ms / args.steps
    value = 1000.0 / ms_per_step  # tokens/s of the whole TP group (batch 1: one token per step)

    if rank == 0:
        out = {
            "metric": "decode_tokens_per_sec",
            "value": round(value, 2),
            "unit": "tokens/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 5),
            "higher_is_better": True,
            "scaling": "strong",
            "vs_baseline": None,
            "dtype": "f16",  # int4 codes dequantized to fp16 MFMA operands, fp16 activations, fp32 accumulate/scales
            "data": "synthetic (seeded torch.randn weights quantized on the GPU by the product quantizer; randn activations)",
            "config": {
                "workload": "Llama-2-7B Q4_0 (BesTLA int4 sym g32 bf16-scale) batch=1 decode GEMM chain: %d layers x "
                            "{QKV, WO, FFN gate/up, FFN down} + lm_head" % args.layers,
                "parallelism": "tp%d" % world,
                "launch": ("hipGraph replay" if use_graph is True else
                           "hipGraph per GEMM run + eager all-reduce" if use_graph == "segments" else "eager"),
                "weights_bytes_per_gpu": chain.stream_bytes,
                "value_is": ("median of six timed batches of %d steps" % args.steps) if (world == 1 and EXTRA_BATCH_MS) else "the one timed batch (max over ranks)",
                "tokens_per_s_first_batch": round(1000.0 * args.steps / first_batch_ms, 2),
                "tokens_per_s_5_more_batches": [round(1000.0 * args.steps / b, 1) for b in EXTRA_BATCH_MS],
                "all_reduce": (None if world == 1 else
                               ("ns_tp_reduce_add (native C ABI): " if pctx.native_enabled() else "") +
                               ("one-shot kernel over peer-mapped HBM (HIP IPC, xGMI)" if pctx.p2p_enabled() else
                                ("RCCL all-reduce" if not os.environ.get("NS_TP_RCCL_LIB") else
                                 "collective library %s" % os.path.basename(os.environ["NS_TP_RCCL_LIB"]))
                                if pctx.native_enabled() else "torch.distributed all_reduce (%s)" % backend)),
                "event_ms_per_step": round(ev_ms / args.steps, 5),
            },
        }
        if chain.prefetch and world == 1:
            out["config"]["weight_prefetch"] = "second graph branch, %d workgroups, first %.2f of the next %s's weights" % (chain.prefetch[0], chain.prefetch[1], "launch" if chain.prefetch[2] else "GEMM run")
        if args.layers != CFG["n_layer"]:
            out["config"]["INVALID"] = "debug run with %d layers" % args.layers
        if world > 1 and backend != "nccl":
            out["config"]["INVALID"] = "smoke run of the TP path over %s, not RCCL" % backend
        alg_bytes = chain.stream_bytes + 4 * sum(
            [(CFG["n_embd"] + 3 * chain.dl), (chain.dl + CFG["n_embd"]), (CFG["n_embd"] + chain.ffl),
             (chain.ffl + CFG["n_embd"])]) * args.layers + 4 * (CFG["n_embd"] + CFG["n_vocab"])
        out["config"]["algorithmic_bytes_per_step_per_gpu"] = alg_bytes
        out["config"]["chain_hbm_GBps"] = round(alg_bytes / (ms_per_step * 1e-3) / 1e9, 1)
        if args.chain_only and world == 1:
            out["config"]["INVALID"] = "chain-only diagnostic run (no roofline / cpu_baseline legs)"
            print(json.dumps(out))
            return
        if world == 1 and chain.host_blobs:
            # the number only counts if the GPU path agrees with the oracle on the layer it times
            par = parity_vs_oracle(chain, pkg)
            out["config"]["parity_rel_l2_vs_oracle"] = par
            worst = max(par.values())
            if not worst <= 1e-3:
                out["config"]["INVALID"] = "GPU chain disagrees with the oracle (rel-L2 %.3g > 1e-3)" % worst
        if args.full:
            out["roofline"] = roofline(chain, pkg)
        # (stable keys: null at one GPU)
        out["config"]["all_reduce_us"] = comm["us"] if (world > 1 and comm is not None) else None
        out["config"]["all_reduces_per_step"] = comm["per_step"] if (world > 1 and comm is not None) else (None if world > 1 else 0)
        out["config"]["comm_fraction"] = round(comm["us"] * comm["per_step"] / (ms_per_step * 1e3), 4) if (world > 1 and comm is not None) else None
        if world == 1 and args.full:
            # the whole token (attention over a 2048-position fp16 kv-cache, norms, RoPE, residuals) on the same weights
            ft, lg = full_token(chain, pkg, 2048, fused=True)
            fu, lgu = full_token(chain, pkg, 2048, fused=False, iters=10)
            rel = float((lg.double() - lgu.double()).norm() / lgu.double().norm())
            out["config"]["full_token_tokens_per_s"] = ft["tokens_per_s"]
            out["config"]["full_token"] = {"fused": ft, "one_launch_per_operator": fu,
                                           "logits_rel_l2_fused_vs_unfused": round(rel, 6)}
            out["config"]["full_prefill"] = full_prefill(chain, pkg, 2048)
            out["config"]["prefill_m2048_tflops"] = prefill_tflops(chain, pkg)
            out["config"]["prefill_m2048_tflops_int8w"] = prefill_tflops_int8w(chain, pkg)
            out["config"]["prefill_m2048_tflops_ref_int8_semantics"] = prefill_tflops_ref_int8(chain, pkg)
            out["config"]["prefill_m2048_detail"] = PREFILL_DETAIL
            out["config"]["decode_tokens_per_s_ref_int8_semantics"] = decode_ref_int8(step, pkg)
            if not args.no_secondary:
                sec = secondary_configs(pkg)
                out["config"]["config4_tokens_per_s"] = sec["config4"]["tokens_per_s"]
                out["config"]["config5_rank_ms"] = sec["config5"]["ms_per_step"]
                out["config"]["config4"] = sec["config4"]
                out["config"]["config5"] = sec["config5"]
        if world == 1 and args.full and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(chain, args.layers)
        if world == 1 and args.full and not args.no_reference_route:
            # (last: the chain's weights are released first — the leg's worker processes load their own model)
            del chain
            torch.cuda.empty_cache()
            out["config"]["reference_route"] = reference_route()
        print(json.dumps(out))
    if world > 1:
        pctx.disable_native()
        pctx.disable_p2p()  # collective: unmap peers, barrier, free
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


def reference_route():
    """What an unchanged Model.generate() user gets: the reference's OWN llama code built with its device switch
    (-DNS_SYCL: loader, graph builder models/llama/llama.cpp:148, graph executor core/ne_layers.c:11915-12028 — oracle/_ref/libne_llama_dev_ref.so,
    compiled from /root/reference as the CALLER only) generating greedily on libns_hip.so's bestla_device_* set (csrc/ns_device.hip, ns_route.cpp) from
    a Llama-2-7B-shaped synthetic Q4_0 file.  Fresh interpreter per run (scripts/dev_llama7b.py leg ...: the provider library must be loaded before
    the reference's); outside every timed region of the headline.  Keys are stable: a value that could not be measured is null and
    `skipped` says why."""
    import subprocess
    out = {"what": "reference's unchanged model_eval (its -DNS_SYCL build as the caller) on libns_hip.so's device route; Llama-2-7B-shaped synthetic "
                   "Q4_0 g32 bf16-scale model, n_ctx 2048, greedy, batch 1; decode = median over the single-token evals of one generation",
           "decode_tokens_per_s_ctx64": None, "decode_us_median_ctx64": None, "decode_tokens_per_s_ctx1500": None, "decode_us_median_ctx1500": None,
           "prompt_1500_ms": None, "prompt_1500_tokens_per_s": None, "prompt_1500_ms_second_evaluation": None, "prompt_64_ms": None, "single_token_evals": None,
           "replay_ctx64": None, "replay_ctx1500": None, "tokens_equal_host_route": None, "tokens_compared": None,
           "host_route_tokens_per_s": None, "model_file": None, "seconds": None, "skipped": None}
    dev_lib = os.path.join(ROOT, "oracle", "_ref", "libne_llama_dev_ref.so")
    host_lib = os.path.join(ROOT, "oracle", "_ref", "libne_llama_ref.so")
    if not os.path.exists(dev_lib):
        out["skipped"] = "oracle/_ref/libne_llama_dev_ref.so is absent (built from /root/reference by `make -C oracle nellamadev`)"
        return out
    worker = os.path.join(ROOT, "scripts", "dev_llama7b.py")
    t0 = time.time()
    path = None

    def run(mode, n_prompt, n_new, timeout):
        cmd = [sys.executable, worker, "leg", mode, str(n_prompt), str(n_new), "2048"] + ([path] if path else [])
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout, cwd=ROOT)
        lines = [ln for ln in r.stdout.decode(errors="replace").splitlines() if ln.startswith("{")]
        if r.returncode != 0 or not lines:
            raise RuntimeError("%s run (prompt %d) failed, rc %d: %s" % (mode, n_prompt, r.returncode, r.stderr.decode(errors="replace")[-400:]))
        return json.loads(lines[-1])
    try:
        a = run("device", 64, 64, 420)   # (builds the model file when there is none: ~1 minute)
        path = a["model_file"]["path"]
        out["model_file"] = a["model_file"]
        out["decode_tokens_per_s_ctx64"], out["decode_us_median_ctx64"] = a["tokens_per_s_median"], a["us_median"]
        out["prompt_64_ms"], out["single_token_evals"], out["replay_ctx64"] = a["prompt_ms"], a["single_token_evals"], a["replay"]
        os.environ["NS_HARNESS_PROMPT_REPEAT"] = "1"   # (the 1500-token prompt is evaluated twice in its context: the first evaluation of a process, then a warm one)
        b = run("device", 1500, 64, 300)
        os.environ.pop("NS_HARNESS_PROMPT_REPEAT", None)
        out["prompt_1500_ms_second_evaluation"] = b.get("prompt_ms_second_evaluation")
        out["decode_tokens_per_s_ctx1500"], out["decode_us_median_ctx1500"] = b["tokens_per_s_median"], b["us_median"]
        out["prompt_1500_ms"], out["prompt_1500_tokens_per_s"], out["replay_ctx1500"] = b["prompt_ms"], b["prompt_tokens_per_s"], b["replay"]
        if os.path.exists(host_lib):
            # the same file through the reference's DEFAULT build (host pointers, its library-managed fp16 cache): same greedy tokens
            h = run("host", 64, 16, 300)
            n = min(len(h["tokens"]), len(a["tokens"]))
            out["tokens_compared"] = n
            out["tokens_equal_host_route"] = h["tokens"][:n] == a["tokens"][:n]
            out["host_route_tokens_per_s"] = h["tokens_per_s"]
            if not out["tokens_equal_host_route"]:
                out["tokens_device_route"], out["tokens_host_route"] = a["tokens"][:n], h["tokens"][:n]
    except Exception as e:  # noqa: BLE001 - the leg never takes the headline down
        out["skipped"] = str(e)[:600]
    finally:
        if path and os.path.exists(path) and not os.environ.get("NS_BENCH_KEEP_MODEL_FILE"):
            os.remove(path)   # (3.9 GB, possibly held in memory under /dev/shm)
    out["seconds"] = round(time.time() - t0, 1)
    return out


def full_token(chain, pkg, ctx=2048, fused=True, iters=30, keep=None):
    """A WHOLE decode token of the same model on the same weights, device resident in one HIP graph (SURVEY 8f rows on
    top of the GEMM chain): rms norm . gamma, fused QKV, RoPE(q, k), kv-cache append, fused attention over `ctx` cached
    positions (fp16 cache), WO + residual, rms norm . gamma, fused gate/up, down + residual; final norm + lm_head.
    fused=True: the norms are carried across the GEMMs (ns_norm_link) and RoPE + the cache append are the QKV launch's
    epilogue (ns_qkv_rope) -> 5 launches per layer + the attention split merge; fused=False: one launch per operator."""
    L = pkg.lib()
    d, ff, V = chain.d, chain.ff, chain.V
    heads, hs = CFG["n_head"], CFG["n_embd"] // CFG["n_head"]
    nl = len(chain.layers)
    dev, h16 = "cuda", torch.float16
    ctx_max = ctx + 8
    n_past = ctx - 1
    g = torch.Generator(device=dev).manual_seed(11)
    kc = [torch.randn((1, ctx_max, heads, hs), generator=g, device=dev).to(h16) for _ in range(nl)]
    vc = [torch.randn((1, ctx_max, heads, hs), generator=g, device=dev).to(h16) for _ in range(nl)]
    gam = [(torch.ones(d, device=dev), torch.ones(d, device=dev)) for _ in range(nl)]
    gf = torch.ones(d, device=dev)
    shape = pkg.AttnShape(1, heads, heads, hs, 1, ctx_max)
    attn_ws = torch.empty(L.bestla_fusion_attn_workspace_size(C.byref(shape)), dtype=torch.uint8, device=dev)
    f32 = lambda *sh: torch.empty(*sh, device=dev)
    f16 = lambda *sh: torch.empty(*sh, device=dev, dtype=h16)
    parts = d // 16
    b = dict(h=f32(1, d), qkv=f32(3, 1, d), att=f32(1, d), r1=f32(1, d), h2=f32(1, d), t2=f32(1, ff), x=f32(1, d),
             logits=f32(1, V), ssq_a=torch.zeros(1, parts, device=dev), ssq_b=torch.zeros(1, parts, device=dev))
    sh = dict(h=f16(1, d), att=f16(1, d), r1=f16(1, d), t2=f16(1, ff), x=f16(1, d), x0=f16(1, d))
    x0 = chain.x0
    rope_tab = torch.zeros(1, hs // 2, 2, device=dev)
    launches = [0]

    def step():
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        ck = pkg.check
        n = 0
        if fused:
            ck(L.ns_hip_norm_prep(1, d, x0.data_ptr(), d, gam[0][0].data_ptr(), sh["x0"].data_ptr(), b["ssq_a"].data_ptr(), parts, st))
            ck(L.ns_hip_rope_cos_sin(1, n_past, hs, 10000.0, 1.0, 1.0, rope_tab.data_ptr(), st))  # once per token, all layers
            n += 2
        xin, xin16 = x0, sh["x0"]
        for il, lw in enumerate(chain.layers):
            if fused:
                lk = pkg.NormLink(b["ssq_a"].data_ptr(), parts, parts, 1e-5, d, None, None, 0)
                rp = pkg.QkvRope(kc[il].data_ptr(), vc[il].data_ptr(), rope_tab.data_ptr(), heads, heads, hs, n_past, hs, 0,
                                 heads * hs, hs)
                ck(L.ns_hip_fusion_qkv_rope_forward_x(xin.data_ptr(), xin16.data_ptr(), lw["q"].h, lw["k"].h, lw["v"].h,
                                                      b["qkv"].data_ptr(), 1, d, d, C.byref(lk), C.byref(rp), st))
                n += 1
            else:
                ck(L.ns_hip_norm_mul_h(1, d, True, 1e-5, xin.data_ptr(), gam[il][0].data_ptr(), b["h"].data_ptr(), sh["h"].data_ptr(), st))
                ck(L.ns_hip_fusion_qkv_forward_h(b["h"].data_ptr(), sh["h"].data_ptr(), lw["q"].h, lw["k"].h, lw["v"].h,
                                                 b["qkv"].data_ptr(), None, 1, d, d, st))
                ck(L.ns_hip_rope_qkv_append(b["qkv"][0].data_ptr(), b["qkv"][1].data_ptr(), b["qkv"][2].data_ptr(),
                                            kc[il].data_ptr(), vc[il].data_ptr(), 1, heads, heads, hs, n_past, hs, 0, 10000.0,
                                            1.0, 0.0, 1.0, heads * hs, hs, st))
                n += 3
            a = pkg.attn_args(b["qkv"][0].data_ptr(), kc[il].data_ptr(), vc[il].data_ptr(), b["att"].data_ptr(), 1, heads,
                              heads, hs, 1, n_past + 1, hs ** -0.5, pkg.ATTN_CAUSAL)
            a.step_k_bs = a.step_v_bs = ctx_max * heads * hs
            a.tmp = attn_ws.data_ptr()
            # the attention kernel also writes the fp16 shadow of its output (the WO projection's A operand)
            ck(L.ns_hip_attn_fp32_fp16_fp16_fp32_forward_h(C.byref(a), sh["att"].data_ptr() if fused else None, st))
            n += 2  # context splits + merge
            xin_next_gamma = gam[il + 1][0] if il + 1 < nl else gf
            if fused:
                lk = pkg.NormLink(None, 0, 0, 0.0, 0, gam[il][1].data_ptr(), b["ssq_b"].data_ptr(), parts)
                ck(L.ns_hip_f32f32_forward_x(b["att"].data_ptr(), sh["att"].data_ptr(), lw["o"].h, b["r1"].data_ptr(),
                                             sh["r1"].data_ptr(), 1, d, d, pkg.EPI_ADD, xin.data_ptr(), d, C.byref(lk), st))
                lk = pkg.NormLink(b["ssq_b"].data_ptr(), parts, parts, 1e-5, d, None, None, 0)
                ck(L.ns_hip_fusion_ffn3_gateup_x(b["r1"].data_ptr(), sh["r1"].data_ptr(), lw["w1"].h, lw["w3"].h, None,
                                                 b["t2"].data_ptr(), sh["t2"].data_ptr(), 1, pkg.EPI_SILU, C.byref(lk), st))
                lk = pkg.NormLink(None, 0, 0, 0.0, 0, xin_next_gamma.data_ptr(), b["ssq_a"].data_ptr(), parts)
                ck(L.ns_hip_f32f32_forward_x(b["t2"].data_ptr(), sh["t2"].data_ptr(), lw["w2"].h, b["x"].data_ptr(),
                                             sh["x"].data_ptr(), 1, ff, d, pkg.EPI_ADD, b["r1"].data_ptr(), d, C.byref(lk), st))
                n += 3
            else:
                ck(L.ns_hip_f32f32_forward(b["att"].data_ptr(), lw["o"].h, b["r1"].data_ptr(), 1, d, d, pkg.EPI_ADD, xin.data_ptr(), d, st))
                ck(L.ns_hip_norm_mul_h(1, d, True, 1e-5, b["r1"].data_ptr(), gam[il][1].data_ptr(), b["h2"].data_ptr(), sh["h"].data_ptr(), st))
                ck(L.ns_hip_fusion_ffn3_gateup_h(b["h2"].data_ptr(), sh["h"].data_ptr(), lw["w1"].h, lw["w3"].h, None,
                                                 b["t2"].data_ptr(), sh["t2"].data_ptr(), 1, pkg.EPI_SILU, st))
                ck(L.ns_hip_f32f32_forward_h(b["t2"].data_ptr(), sh["t2"].data_ptr(), lw["w2"].h, b["x"].data_ptr(), None, 1, ff, d,
                                             pkg.EPI_ADD, b["r1"].data_ptr(), d, st))
                n += 4
            xin, xin16 = b["x"], sh["x"]
        if fused:
            lk = pkg.NormLink(b["ssq_a"].data_ptr(), parts, parts, 1e-5, d, None, None, 0)
            ck(L.ns_hip_f32f32_forward_x(xin.data_ptr(), xin16.data_ptr(), chain.head.h, b["logits"].data_ptr(), None, 1, d, V,
                                         pkg.EPI_NONE, None, 0, C.byref(lk), st))
            n += 1
        else:
            ck(L.ns_hip_norm_mul_h(1, d, True, 1e-5, xin.data_ptr(), gf.data_ptr(), b["h"].data_ptr(), sh["h"].data_ptr(), st))
            ck(L.ns_hip_f32f32_forward_h(b["h"].data_ptr(), sh["h"].data_ptr(), chain.head.h, b["logits"].data_ptr(), None, 1, d, V,
                                         pkg.EPI_NONE, None, 0, st))
            n += 2
        launches[0] = n

    for _ in range(2):
        step()
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        step()
    for _ in range(3):
        gr.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        gr.replay()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / iters
    logits = b["logits"].clone()
    if keep is not None:  # scripts/full_token_oracle.py: the kv caches (incl. the rows this token appended) for the fp64 model
        keep.update(kc=kc, vc=vc, n_past=n_past, x0=x0)
    return {"ctx": ctx, "ms_per_token": round(ms, 4), "tokens_per_s": round(1000.0 / ms, 1),
            "launches_per_token": launches[0], "launches_per_layer": round((launches[0] - (3 if fused else 2)) / nl, 2),
            "finite": bool(torch.isfinite(logits).all().item())}, logits


PREFILL_ROPE_IN_QKV = os.environ.get("NS_BENCH_PREFILL_ROPE_IN_QKV", "1") != "0"  # 0: RoPE + cache append as a launch of its own (rounds 2-4; A/B)


def full_prefill(chain, pkg, m=2048, iters=5):
    """A WHOLE prompt of m tokens through the same model on the same weights, one launch per operator: rms norm . gamma, fused
    QKV (tiled MFMA GEMM) with RoPE(q, k) + kv-cache append as its epilogue (round 5; before: a launch of their own), causal attention over the prompt (the 128-row matrix-core kernel, fp16 K / V
    just appended), WO + residual, norm, gate/up . SiLU, down + residual — every layer — then the final norm and the lm_head row of
    the LAST position (what a first token needs).  tflops = 2 x weights x m + 4 x heads x head_size x m^2 / 2 per layer (causal half)."""
    L = pkg.lib()
    d, ff, V = chain.d, chain.ff, chain.V
    heads, hs = CFG["n_head"], CFG["n_embd"] // CFG["n_head"]
    nl = len(chain.layers)
    dev, h16 = "cuda", torch.float16
    g = torch.Generator(device=dev).manual_seed(13)
    kc = [torch.zeros((1, m, heads, hs), device=dev, dtype=h16) for _ in range(nl)]
    vc = [torch.zeros((1, m, heads, hs), device=dev, dtype=h16) for _ in range(nl)]
    gam = torch.ones(d, device=dev)
    f32 = lambda *sh: torch.empty(*sh, device=dev)
    f16 = lambda *sh: torch.empty(*sh, device=dev, dtype=h16)
    x0 = torch.randn((m, d), generator=g, device=dev)
    b = dict(h=f32(m, d), qkv=f32(3, m, d), att=f32(m, d), r1=f32(m, d), h2=f32(m, d), x=f32(m, d), logits=f32(1, V))
    sh = dict(h=f16(m, d), att=f16(m, d), t2=f16(m, ff))

    rope_tab = torch.zeros((m, hs // 2, 2), device=dev)  # (cos, sin) per (position, pair): the same for every layer, filled once per prompt

    def step():
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        ck = pkg.check
        xin = x0
        if PREFILL_ROPE_IN_QKV:
            ck(L.ns_hip_rope_cos_sin(m, 0, hs, 10000.0, 1.0, 1.0, rope_tab.data_ptr(), st))
        for il, lw in enumerate(chain.layers):
            # (the norms write their fp16 result only where the tiled GEMM behind them multiplies fp16 activations as they are: PREFILL_ROPE_IN_QKV)
            ck(L.ns_hip_norm_mul_h(m, d, True, 1e-5, xin.data_ptr(), gam.data_ptr(), None if PREFILL_ROPE_IN_QKV else b["h"].data_ptr(), sh["h"].data_ptr(), st))
            if PREFILL_ROPE_IN_QKV:
                # one launch: the fused-QKV GEMM rotates q / k and appends k, v to the fp16 cache in its epilogue; k and v are never fp32 tensors
                rp = pkg.QkvRope(kc[il].data_ptr(), vc[il].data_ptr(), rope_tab.data_ptr(), heads, heads, hs, 0, hs, 0, heads * hs, hs, 1)
                ck(L.ns_hip_fusion_qkv_rope_forward_x(None, sh["h"].data_ptr(), lw["q"].h, lw["k"].h, lw["v"].h,
                                                      b["qkv"].data_ptr(), m, d, d, None, C.byref(rp), st))
            else:
                ck(L.ns_hip_fusion_qkv_forward_h(b["h"].data_ptr(), sh["h"].data_ptr(), lw["q"].h, lw["k"].h, lw["v"].h,
                                                 b["qkv"].data_ptr(), None, m, d, d, st))
                ck(L.ns_hip_rope_qkv_append(b["qkv"][0].data_ptr(), b["qkv"][1].data_ptr(), b["qkv"][2].data_ptr(), kc[il].data_ptr(),
                                            vc[il].data_ptr(), m, heads, heads, hs, 0, hs, 0, 10000.0, 1.0, 0.0, 1.0, heads * hs, hs, st))
            a = pkg.attn_args(b["qkv"][0].data_ptr(), kc[il].data_ptr(), vc[il].data_ptr(), b["att"].data_ptr(), 1, heads, heads, hs,
                              m, m, hs ** -0.5, pkg.ATTN_CAUSAL)
            ck(L.ns_hip_attn_fp32_fp16_fp16_fp32_forward_h(C.byref(a), sh["att"].data_ptr(), st))
            ck(L.ns_hip_f32f32_forward_h(b["att"].data_ptr(), sh["att"].data_ptr(), lw["o"].h, b["r1"].data_ptr(), None, m, d, d,
                                         pkg.EPI_ADD, xin.data_ptr(), d, st))
            ck(L.ns_hip_norm_mul_h(m, d, True, 1e-5, b["r1"].data_ptr(), gam.data_ptr(), None if PREFILL_ROPE_IN_QKV else b["h2"].data_ptr(), sh["h"].data_ptr(), st))
            # gate / up tile pairs, one launch, the product in fp16 only; the down projection (+ residual) multiplies it as it is
            ck(L.ns_hip_fusion_ffn3_gateup_h(None if PREFILL_ROPE_IN_QKV else b["h2"].data_ptr(), sh["h"].data_ptr(), lw["w1"].h, lw["w3"].h, None, None, sh["t2"].data_ptr(),
                                             m, pkg.EPI_SILU, st))
            ck(L.ns_hip_f32f32_forward_h(None, sh["t2"].data_ptr(), lw["w2"].h, b["x"].data_ptr(), None, m, ff, d,
                                         pkg.EPI_ADD, b["r1"].data_ptr(), d, st))
            xin = b["x"]
        last = xin[m - 1:m]
        ck(L.ns_hip_norm_mul_h(1, d, True, 1e-5, last.data_ptr(), gam.data_ptr(), b["h"].data_ptr(), sh["h"].data_ptr(), st))
        ck(L.ns_hip_f32f32_forward_h(b["h"].data_ptr(), sh["h"].data_ptr(), chain.head.h, b["logits"].data_ptr(), None, 1, d, V,
                                     pkg.EPI_NONE, None, 0, st))

    ms = _timed(step, 2, iters)
    wflops = sum(2.0 * m * lw[k].n * lw[k].k for lw in chain.layers for k in ("q", "k", "v", "o", "w1", "w3", "w2"))
    aflops = nl * 4.0 * heads * hs * m * m / 2
    return {"prompt_tokens": m, "ms": round(ms, 3), "prompt_tokens_per_s": round(m / ms * 1e3, 0),
            "tflops_gemm_plus_causal_attention": round((wflops + aflops) / ms / 1e9, 1),
            "attention_share_of_flops": round(aflops / (wflops + aflops), 3), "launches": (7 * nl + 3) if PREFILL_ROPE_IN_QKV else (8 * nl + 2),
            "rope_and_cache_append": "QKV GEMM epilogue" if PREFILL_ROPE_IN_QKV else "own launch",
            "finite": bool(torch.isfinite(b["logits"]).all().item())}


ROOFLINE_KERNEL = "gemv_kernel<INT4,SPS4,BF16,sym,DUAL>"  # demangled: ns::gemv_kernel<0, 4, 0, false, 1, false>


def all_reduce_latency(chain, world, try_graph):
    """per-all-reduce time of the decode-sized buffer ([1][n_embd] fp32) on the path the timed step used: 64 back-to-back
    calls in one HIP graph when that captures, eager otherwise; max over ranks."""
    x = torch.zeros((1, chain.d), device="cuda", dtype=torch.float32)
    n = 64

    def body():
        for _ in range(n):
            REDUCE(x)

    torch.distributed.barrier()
    body()
    torch.cuda.synchronize()
    run = body
    try:
        if not try_graph:  # a process-group all-reduce that is not capturable (gloo) must not be called under capture
            raise RuntimeError("eager")
        g = capture(body)
        run = g.replay
        failed = 0
    except Exception:  # noqa: BLE001
        failed = 1
        try:
            torch.cuda.synchronize()
        except Exception:  # noqa: BLE001
            pass
        ge.load_package().lib().ns_hip_reset_error()
    if agree_failed(failed, world):
        run = body
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    torch.distributed.barrier()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reps = 10
    e0.record()
    for _ in range(reps):
        run()
    e1.record()
    torch.cuda.synchronize()
    us = torch.tensor([e0.elapsed_time(e1) * 1e3 / (reps * n)], device="cuda", dtype=torch.float64)
    torch.distributed.all_reduce(us, op=torch.distributed.ReduceOp.MAX)
    return {"us": round(float(us.item()), 2), "per_step": 2 * len(chain.layers)}


def pmc_traffic(chain):
    """HBM bytes per gate/up launch from the TCC FETCH_SIZE counter.  PMC collection needs its own rocprofv3 pass
    (scripts/pmc_traffic.sh; the driver runs bench.py bare), so the measured per-launch figure is read back from the
    committed summary (the newest profiles/*_pmc_fetch_size.json) — only when that summary was taken on the SAME kernel sources
    (a hash of ns_gemv.hip + ns_dev.h recorded in it), kernel name and grid this run launches; any change makes the figure null
    until the counters are collected again."""
    prof = os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles")
    paths = sorted((p for p in os.listdir(prof) if p.endswith("_pmc_fetch_size.json")), reverse=True) if os.path.isdir(prof) else []
    if chain.world != 1 or not paths:
        return None
    try:
        import hashlib
        src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "neural-speed_amd", "csrc")
        h = hashlib.sha256()
        for f in ("ns_gemv.hip", "ns_dev.h"):
            h.update(open(os.path.join(src, f), "rb").read())
        d = json.load(open(os.path.join(prof, paths[0])))
        g = d["gate_up"]
        lw = chain.layers[0]
        # only a summary taken on THIS kernel: same sources (hash), same kernel name, same launch grid
        if d.get("kernel_source_sha16") != h.hexdigest()[:16] or g.get("kernel") != "gemv_kernel" or g.get("grid") != (lw["w1"].n + 15) // 16:
            return None
        return g["hbm_bytes_corrected"]
    except Exception:
        return None


def roofline(chain, pkg):
    """Dominant kernel = the fused FFN gate/up weight-streaming GEMV (gemv_kernel, dual mode): 2 x 4096 x
    11008/tp int4 weights + bf16 group scales per launch = 27.6 % x 3 of every layer's bytes.  Average launch duration is
    measured live with HIP events on the launch stream around a hipGraph that holds one gate/up launch per layer (each
    layer's own weights, so nothing is cache resident), divided by the number of launches."""
    L = pkg.lib()
    d = chain.d
    nl = len(chain.layers)
    t2 = chain.t2

    def body():
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        for lw in chain.layers:
            pkg.check(L.ns_hip_fusion_ffn3_gateup_h(chain.x0.data_ptr(), chain.x0h.data_ptr() if chain.use_h else None,
                                                    lw["w1"].h, lw["w3"].h, None, t2.data_ptr(),
                                                    chain.t2h.data_ptr() if chain.use_h else None, 1, pkg.EPI_SILU, st))

    for _ in range(3):
        body()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        body()
    for _ in range(40):  # steady state, like every other leg: ~15 ms under this load before the timed region
        g.replay()
    torch.cuda.synchronize()
    reps = 100
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / (reps * nl)
    lw = chain.layers[0]
    bytes_per_launch = lw["w1"].stream_bytes + lw["w3"].stream_bytes + 4 * (d + chain.ffl)
    achieved = bytes_per_launch / (us * 1e-6) / 1e9
    return {
        "kernel": ROOFLINE_KERNEL + " (FFN gate/up GEMV)",
        "bound": "hbm",
        "achieved": round(achieved, 1),
        "peak": HBM_PEAK_GBS,
        "unit": "GB/s",
        "frac": round(achieved / HBM_PEAK_GBS, 4),
        "traffic": pmc_traffic(chain),
        "traffic_source": "rocprofv3 --pmc FETCH_SIZE (own pass, scripts/pmc_traffic.sh), x2 gfx950 correction, "
                          "bytes per gate/up launch at tp=1: the newest profiles/*_pmc_fetch_size.json whose kernel-source hash "
                          "matches this build (null otherwise)",
        "bytes_per_launch": bytes_per_launch,
        "avg_launch_us": round(us, 3),
        "note": "avg over %d back-to-back graph launches incl. ~1.2us inter-kernel boundary each" % (reps * nl),
    }


def decode_ref_int8(step, pkg, steps=60, warmup=10):
    """the SAME decode chain in the reference's DEFAULT numerics for this model (Q4_0: compute_dtype = int8 —
    quantize_fp_u8_colblock on every GEMV input + gemv_4bit_u8s8_fp32's integer dots, kernel_ref.h:1824-1883, :2371-2429):
    NS_COMPUTE_REF_INT8 routes the same entry points to the streaming kernel's int8 variant (one activation quantization
    launch per distinct input + the fused QKV / gate-up / plain launches); one HIP graph, tokens/s"""
    L = pkg.lib()
    prev = L.ns_hip_set_compute_mode(1)
    try:
        wall_ms, _ = time_graph(step, steps, warmup, True, 1)
        return round(1000.0 / (wall_ms / steps), 2)
    finally:
        L.ns_hip_set_compute_mode(prev if prev in (0, 1) else 0)


# Prefill legs: steady state.  Round 2 timed 5 passes (5 ms) after 2 warm-ups and read 790-820 TFLOPS; the same kernels on
# the same box read 975-993 once the chip has been under this load for a few tens of milliseconds (scripts/prefill_ab.py,
# profiles/r03w_prefill_ab.txt: consecutive measurements 793, 896, 954, ... 992 — the clock settles, nothing is cached:
# a layer's GEMMs stream 100 MB of weights and 50 MB of activations per pass).  A 2048-token prompt runs 32 such layers
# back to back (> 30 ms), so the steady state is the regime that counts: 80 warm-up passes (the reading still climbs after 10), 60 timed ones.
PREFILL_WARMUP, PREFILL_REPS = 80, 60
PREFILL_DETAIL = {}      # leg -> {"steady_tflops", "cold_tflops_after_2_warmup_passes", "parity_rel_l2_vs_oracle"}
PREFILL_LEG = ["int4"]   # which leg prefill_tflops() is timing (the int8-reference leg re-enters it)


def _timed(run, warmup, reps):
    for _ in range(warmup):
        run()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        run()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def _prefill_layer_run(pkg, L, st, m, d, dl, a_d, a_d16, wq, wk, wv, wo, w1, w3, w2, qkv_out, qkv_out16, out_big, out_big16):
    """one layer's seven GEMMs as the reference's graphs issue them: Q, K, V through bestla_fusion_QKV_f32f32_forward's device form
    (ip_fusion_qkv.cpp:84-86: one launch of the tiled kernel with the three matrices side by side), the attention-output projection as
    a plain forward, and the FFN through bestla_fusion_FFN_SiLu_f32f32_forward's device form (ip_fusion_ffn.cpp:364-406; round 5: gate / up
    tile pairs in ONE launch with act(gate) * up formed in registers, the intermediate kept in fp16 only — the reference treats tmp1 / tmp2
    as scratch — and the down projection on it).  Every GEMM writes fp32 C plus the fp16 shadow for its consumer."""
    def run():
        pkg.check(L.ns_hip_fusion_qkv_forward_h(a_d.data_ptr(), a_d16.data_ptr(), wq.h, wk.h, wv.h, qkv_out.data_ptr(),
                                                qkv_out16.data_ptr(), m, d, dl, st))
        pkg.check(L.ns_hip_f32f32_forward_h(a_d.data_ptr(), a_d16.data_ptr(), wo.h, out_big.data_ptr(), out_big16.data_ptr(), m, wo.k, wo.n,
                                            pkg.EPI_NONE, None, 0, st))
        pkg.check(L.ns_hip_fusion_ffn3_forward_h(a_d.data_ptr(), a_d16.data_ptr(), w1.h, w2.h, w3.h, None, None, None, out_big.data_ptr(),
                                                 out_big16.data_ptr(), m, pkg.EPI_SILU, st))
    return run


def _prefill_parity(a_w2, out_w2, blob_w2, a_q, out_q, blob_q, nrows=6, int8_ref=False):
    """the prefill legs' own outputs (what the timed run() left behind) against the oracle's fp64 GEMM on the same blobs: a few
    rows, every column (bar 1e-3; the kernels are covered row by row in tests/test_gpu_fullsize.py).  blob_w2 = (w1, w3, w2): the
    FFN chain silu(a W1) * (a W3) -> W2 of the oracle (round 5: the FFN runs through the fused entry)"""
    nso = ge.load_oracle()
    m = a_w2.shape[0]
    rows = np.unique(np.linspace(0, m - 1, nrows).astype(np.int64))
    ridx = torch.from_numpy(rows).cuda()

    def blob(v):
        b = nso.aligned_bytes(v.size)
        b[:] = v
        return b
    out = {}
    gemm = nso.gemm_u8s8 if int8_ref else nso.gemm_f64
    for name, a, o, b in (("ffn_silu_out", a_w2, out_w2, blob_w2), ("wq_of_fused_qkv", a_q, out_q, blob_q)):
        # (the int8-reference leg computes u8 x s8 integer dots: its oracle is the reference's own arithmetic, not the fp64 product)
        rows_a = np.ascontiguousarray(a[ridx].cpu().numpy())
        if isinstance(b, tuple):
            g, u = gemm(rows_a, blob(b[0])).astype(np.float64), gemm(rows_a, blob(b[1])).astype(np.float64)
            ref = gemm(np.ascontiguousarray((g / (1.0 + np.exp(-g)) * u).astype(np.float32)), blob(b[2]))
        else:
            ref = gemm(rows_a, blob(b))
        n = ref.shape[1]
        got = o.reshape(-1)[:m * n].view(m, n)  # the GEMM wrote [m][ldc = n] at the start of the (larger, shared) output buffer
        out[name] = float("%.3g" % nso.rel_l2(got[ridx].cpu().numpy(), ref))
    if int8_ref:
        out["oracle"] = "nso.gemm_u8s8 (quantize_fp_u8_colblock + integer dots per k-block)"
    return out


def prefill_tflops_ref_int8(chain, pkg, m=2048):
    """the same seven GEMMs (int4 g32 weights) in the reference's DEFAULT int8-compute semantics (NS_COMPUTE_REF_INT8: u8
    activation quantization per k-block + exact integer dots per 32-deep slice on the matrix cores — ns_i8ref.hip
    i8mfma2_kernel: fp16 operands holding the integers a - za and u - zb, so one MFMA returns float(isum) exactly); the
    activation quantizer is inside the timed region.  TFLOPS-equivalent (2 m n k)."""
    L = pkg.lib()
    prev = L.ns_hip_set_compute_mode(1)
    PREFILL_LEG[0] = "ref_int8_semantics"
    try:
        return prefill_tflops(chain, pkg, m)
    finally:
        PREFILL_LEG[0] = "int4"
        L.ns_hip_set_compute_mode(prev if prev in (0, 1) else 0)


def prefill_tflops(chain, pkg, m=2048):
    """second half of BASELINE.json's metric: prefill TFLOPS of one layer's GEMMs (same int4 g32 weights) at M = 2048
    through the tiled MFMA GEMM kernel; 2*M*N*K flops per GEMM, HIP events on the launch stream."""
    L = pkg.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    lw = chain.layers[0]
    d, ff = chain.d, chain.ffl
    a_d = torch.randn((m, d), device="cuda", dtype=torch.float32)
    # device-resident chain: every GEMM reads the fp16 shadow its producer wrote and writes fp32 C plus the fp16 shadow
    # for its consumer (the "_h" entry points), exactly like the decode chain above
    a_d16 = a_d.half()
    out_big = torch.empty((m, max(d, ff)), device="cuda", dtype=torch.float32)
    out_big16 = torch.empty((m, max(d, ff)), device="cuda", dtype=torch.float16)
    qkv_out = torch.empty((3, m, d), device="cuda", dtype=torch.float32)
    qkv_out16 = torch.empty((3, m, d), device="cuda", dtype=torch.float16)
    run = _prefill_layer_run(pkg, L, st, m, d, chain.dl, a_d, a_d16, lw["q"], lw["k"], lw["v"], lw["o"], lw["w1"], lw["w3"], lw["w2"],
                             qkv_out, qkv_out16, out_big, out_big16)
    flops = sum(2.0 * m * lw[k].n * lw[k].k for k in ("q", "k", "v", "o", "w1", "w3", "w2"))
    cold = _timed(run, 2, 4)     # a first prompt: two passes of warm-up only (clocks and caches as a cold start finds them)
    ms = _timed(run, PREFILL_WARMUP, PREFILL_REPS)
    detail = {"steady_tflops": round(flops / ms / 1e9, 1), "cold_tflops_after_2_warmup_passes": round(flops / cold / 1e9, 1)}
    if chain.host_layers:  # parity of the timed kernels: sampled rows of the FFN's output and of the fused QKV's q against the oracle's fp64 GEMMs
        hl = chain.host_layers[0]
        detail["parity_rel_l2_vs_oracle"] = _prefill_parity(a_d, out_big, (hl["w1"], hl["w3"], hl["w2"]), a_d, qkv_out[0], hl["q"],
                                                            int8_ref=PREFILL_LEG[0] != "int4")
    PREFILL_DETAIL[PREFILL_LEG[0]] = detail
    return detail["steady_tflops"]


def prefill_tflops_int8w(chain, pkg, m=2048):
    """BASELINE config 3: prefill on INT8 weights (S8 sym g32, bf16 scales), fp16 compute, M = 2048, one layer's seven
    GEMMs of the Llama-2-7B shapes through the tiled MFMA GEMM; same timing as prefill_tflops."""
    L = pkg.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    d, ff = chain.d, chain.ffl
    ws, host_ffn = [], []
    for i, (n, k) in enumerate([(d, d)] * 4 + [(ff, d)] * 2 + [(d, ff)]):
        g = torch.Generator(device="cuda").manual_seed(4242 + i)
        w = torch.randn((n, k), generator=g, device="cuda", dtype=torch.float32) * (k ** -0.5)
        size = L.ns_BTLAGemmPackBSize(n, k, CFG["group"], pkg.S8, pkg.BF16, False, pkg.COMP_INT8, None)
        blob = torch.zeros(size, dtype=torch.uint8, device="cuda")
        pkg.check(L.ns_hip_quant_pack_device(blob.data_ptr(), w.data_ptr(), n, k, k, CFG["group"], pkg.S8, pkg.BF16, False,
                                             pkg.COMP_INT8, True, st), "quant_pack_device(int8)")
        ws.append(pkg.Weight.from_device_blob(blob.data_ptr(), size, st))
        torch.cuda.synchronize()
        if i == 0:
            host_q = blob.cpu().numpy()
        if i >= 4:
            host_ffn.append(blob.cpu().numpy())
        del w, blob
    a_d = torch.randn((m, d), device="cuda", dtype=torch.float32)
    a_d16 = a_d.half()
    out_big = torch.empty((m, max(d, ff)), device="cuda", dtype=torch.float32)
    out_big16 = torch.empty((m, max(d, ff)), device="cuda", dtype=torch.float16)

    qkv_out = torch.empty((3, m, d), device="cuda", dtype=torch.float32)
    qkv_out16 = torch.empty((3, m, d), device="cuda", dtype=torch.float16)
    run = _prefill_layer_run(pkg, L, st, m, d, d, a_d, a_d16, ws[0], ws[1], ws[2], ws[3], ws[4], ws[5], ws[6], qkv_out, qkv_out16, out_big,
                             out_big16)

    flops = sum(2.0 * m * wt.n * wt.k for wt in ws)
    cold = _timed(run, 2, 4)
    ms = _timed(run, PREFILL_WARMUP, PREFILL_REPS)
    detail = {"steady_tflops": round(flops / ms / 1e9, 1), "cold_tflops_after_2_warmup_passes": round(flops / cold / 1e9, 1),
              "parity_rel_l2_vs_oracle": _prefill_parity(a_d, out_big, (host_ffn[0], host_ffn[1], host_ffn[2]), a_d, qkv_out[0], host_q)}
    PREFILL_DETAIL["int8w"] = detail
    del ws
    return detail["steady_tflops"]


def parity_vs_oracle(chain, pkg):
    """Every GEMV of layer 0 + lm_head, as the timed chain launches it (fp16 shadow in, gemv_kernel), against the
    oracle's sequential-fp32 GEMV (kernel_ref.h gemv_4bit_fp32_fp32 semantics) on the SAME inputs: relative L2 per
    operator (the reference's cmpData.diff2); the north-star bar is 1e-3."""
    nso = ge.load_oracle()
    L = pkg.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    hb, lw = chain.host_layers[0], chain.layers[0]
    d, dl, ffl = chain.d, chain.dl, chain.ffl
    ncores = min(64, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1))

    def blob(v):
        b = nso.aligned_bytes(v.size)
        b[:] = v
        return b

    def gpu(wt, a, epi=pkg.EPI_NONE):
        a16 = a.to(torch.float16)
        c = torch.empty((1, wt.n), device="cuda", dtype=torch.float32)
        pkg.check(L.ns_hip_f32f32_forward_h(a.data_ptr(), a16.data_ptr(), wt.h, c.data_ptr(), None, 1, wt.k, wt.n, epi, None, 0, st))
        torch.cuda.synchronize()
        return c

    out = {}
    x0 = chain.x0
    x0n = x0.cpu().numpy()
    # fused QKV launch (what the chain runs) vs three oracle GEMVs
    qkv = torch.empty((3, 1, dl), device="cuda", dtype=torch.float32)
    pkg.check(L.ns_hip_fusion_qkv_forward_h(x0.data_ptr(), chain.x0h.data_ptr(), lw["q"].h, lw["k"].h, lw["v"].h, qkv.data_ptr(), None,
                                            1, d, dl, st))
    torch.cuda.synchronize()
    for i, nm in enumerate("qkv"):
        out["w" + nm] = nso.rel_l2(qkv[i].cpu().numpy(), nso.gemv_f32(x0n, blob(hb[nm]), ncores))
    q_in = qkv[0]
    o = gpu(lw["o"], q_in)
    out["wo"] = nso.rel_l2(o.cpu().numpy(), nso.gemv_f32(q_in.cpu().numpy(), blob(hb["o"]), ncores))
    # fused gate/up launch vs silu(x W1) * (x W3) from the oracle
    t2 = torch.empty((1, ffl), device="cuda", dtype=torch.float32)
    pkg.check(L.ns_hip_fusion_ffn3_gateup_h(o.data_ptr(), o.to(torch.float16).data_ptr(), lw["w1"].h, lw["w3"].h, None, t2.data_ptr(),
                                            None, 1, pkg.EPI_SILU, st))
    torch.cuda.synchronize()
    on = o.cpu().numpy()
    h1 = nso.gemv_f32(on, blob(hb["w1"]), ncores).astype(np.float64)
    h3 = nso.gemv_f32(on, blob(hb["w3"]), ncores).astype(np.float64)
    out["ffn_gate_up"] = nso.rel_l2(t2.cpu().numpy(), (h1 / (1.0 + np.exp(-h1))) * h3)
    x = gpu(lw["w2"], t2)
    out["ffn_down"] = nso.rel_l2(x.cpu().numpy(), nso.gemv_f32(t2.cpu().numpy(), blob(hb["w2"]), ncores))
    lg = gpu(chain.head, x)
    out["lm_head"] = nso.rel_l2(lg.cpu().numpy(), nso.gemv_f32(x.cpu().numpy(), blob(chain.host_blobs["head"]), ncores))
    return {k: float("%.3g" % v) for k, v in out.items()}


def secondary_configs(pkg):
    """BASELINE.json configs 4 and 5 on this GPU, each with a parity value against the oracle:
      config 4  Mistral-7B NF4 g128 (bf16 scales), batch 8 decode: tokens/s of the GEMM chain (fused QKV with GQA widths, WO, fused
                gate/up, down) — enough DIFFERENT layers in one HIP graph to exceed the 256 MB Infinity Cache several times, x 32
                layers + lm_head; the small-batch kernel (ns_gemvs.hip) serves every launch
      config 5  Llama-2-70B Q4_0 g32, batch 1, ONE rank's shards of TP = 8 (model_files.h:145-190 split rules): ms per token of
                that rank's GEMMs (160 all-reduces of 32 KB per token come on top)
    Same protocol as scripts/config_bench.py (kept as the per-shape breakdown).  Parity: one layer's launches against the
    oracle's fp64 GEMM on the same blobs (relative L2, bar 1e-3)."""
    nso = ge.load_oracle()
    L = pkg.lib()

    def make(n, k, qt, st_dt, bs, comp, seed):
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        g = torch.Generator(device="cuda").manual_seed(seed)
        w = torch.randn((n, k), generator=g, device="cuda") * 0.02
        size = L.ns_BTLAGemmPackBSize(n, k, bs, qt, st_dt, False, comp, None)
        blob = torch.zeros(size, dtype=torch.uint8, device="cuda")
        pkg.check(L.ns_hip_quant_pack_device(blob.data_ptr(), w.data_ptr(), n, k, k, bs, qt, st_dt, False, comp, True, st))
        wt = pkg.Weight.from_device_blob(blob.data_ptr(), size, st)
        torch.cuda.synchronize()
        return wt, blob

    def graph_us(fn, reps=20):
        for _ in range(3):
            fn(C.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            fn(C.c_void_p(torch.cuda.current_stream().cuda_stream))
        for _ in range(3):
            g.replay()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            g.replay()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps

    def host(blob):
        b = nso.aligned_bytes(blob.numel())
        b[:] = blob.cpu().numpy()
        return b

    def run(d_in, qn, kvn, o_k, ff_n, vocab, fmt, m, n_layers, min_bytes=700e6):
        qt, st_dt, bs, comp = fmt
        layers = []
        while True:
            i = len(layers)
            lw = {nm: make(n, k, qt, st_dt, bs, comp, 100 + 8 * i + j) for j, (nm, n, k) in enumerate(
                [("q", qn, d_in), ("k", kvn, d_in), ("v", kvn, d_in), ("o", d_in, o_k), ("w1", ff_n, d_in), ("w3", ff_n, d_in), ("w2", d_in, ff_n)])}
            layers.append(lw)
            per_layer = sum(w[0].stream_bytes for w in lw.values())
            if per_layer * len(layers) >= min_bytes or len(layers) >= n_layers:
                break
        ldq = max(qn, kvn)
        g = torch.Generator(device="cuda").manual_seed(5)
        x = torch.randn((m, d_in), generator=g, device="cuda")
        xh = x.half()
        qkv = torch.empty((3, m, ldq), device="cuda"); qkvh = torch.empty((3, m, ldq), device="cuda", dtype=torch.float16)
        att = torch.empty((m, d_in), device="cuda"); atth = torch.empty((m, d_in), device="cuda", dtype=torch.float16)
        t2 = torch.empty((m, ff_n), device="cuda"); t2h = torch.empty((m, ff_n), device="cuda", dtype=torch.float16)
        y = torch.empty((m, d_in), device="cuda"); yh = torch.empty((m, d_in), device="cuda", dtype=torch.float16)

        def layer(lw, xi, xih, s):
            pkg.check(L.ns_hip_fusion_qkv_forward_h(xi.data_ptr(), xih.data_ptr(), lw["q"][0].h, lw["k"][0].h, lw["v"][0].h, qkv.data_ptr(),
                                                    qkvh.data_ptr(), m, d_in, ldq, s))
            # attention is its own operator: the first o_k columns of the q slice stand in for its output
            pkg.check(L.ns_hip_f32f32_forward_h(qkv.data_ptr(), qkvh.data_ptr(), lw["o"][0].h, att.data_ptr(), atth.data_ptr(), m, ldq, d_in,
                                                pkg.EPI_NONE, None, 0, s))
            pkg.check(L.ns_hip_fusion_ffn3_forward_h(att.data_ptr(), atth.data_ptr(), lw["w1"][0].h, lw["w2"][0].h, lw["w3"][0].h, None,
                                                     t2.data_ptr(), t2h.data_ptr(), y.data_ptr(), yh.data_ptr(), m, pkg.EPI_SILU, s))

        def chain(s):
            xi, xih = x, xh
            for lw in layers:
                layer(lw, xi, xih, s)
                xi, xih = y, yh
        us_layer = graph_us(chain) / len(layers)
        head, head_blob = make(vocab, d_in, qt, st_dt, bs, comp, 99)
        lg = torch.empty((m, vocab), device="cuda")
        us_head = graph_us(lambda s: pkg.check(L.ns_hip_f32f32_forward_h(y.data_ptr(), yh.data_ptr(), head.h, lg.data_ptr(), None, m, d_in, vocab,
                                                                         pkg.EPI_NONE, None, 0, s)), reps=10)
        # ---- parity of layer 0's launches (they ran last inside graph_us with xi = x only for layer 0: run it again alone) ----
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        layer(layers[0], x, xh, st)
        torch.cuda.synchronize()
        lw = layers[0]
        par = {}
        xn = x.cpu().numpy()
        qn_ = qkv.cpu().numpy()
        for i, nm in enumerate("qkv"):
            n = qn if nm == "q" else kvn
            par["w" + nm] = nso.rel_l2(qn_[i][:, :n], nso.gemm_f64(xn, host(lw[nm][1])))
        par["wo"] = nso.rel_l2(att.cpu().numpy(), nso.gemm_f64(np.ascontiguousarray(qkv[0][:, :o_k].cpu().numpy()), host(lw["o"][1])))
        an = att.cpu().numpy()
        h1 = nso.gemm_f64(an, host(lw["w1"][1])).astype(np.float64)
        h3 = nso.gemm_f64(an, host(lw["w3"][1])).astype(np.float64)
        par["ffn_gate_up"] = nso.rel_l2(t2.cpu().numpy(), (h1 / (1.0 + np.exp(-h1))) * h3)
        par["ffn_down"] = nso.rel_l2(y.cpu().numpy(), nso.gemm_f64(t2.cpu().numpy(), host(lw["w2"][1])))
        byt_layer = sum(w[0].stream_bytes for w in lw.values())
        tot_us = us_layer * n_layers + us_head
        tot_b = byt_layer * n_layers + head.stream_bytes
        for l_ in layers:
            for w in l_.values():
                w[0].free()
        head.free()
        return {"layers_in_graph": len(layers), "us_per_layer": round(us_layer, 2), "us_lm_head": round(us_head, 2),
                "ms_per_step": round(tot_us / 1e3, 4), "weight_bytes_per_step": int(tot_b), "weight_bytes_per_layer": int(byt_layer),
                "hbm_GBps": round(tot_b / tot_us / 1e3, 1), "frac_of_8TBps": round(tot_b / tot_us / 8e6, 3),
                "parity_rel_l2_vs_oracle": {k: float("%.3g" % v) for k, v in par.items()}}, tot_us

    out = {}
    c4, us4 = run(4096, 4096, 1024, 4096, 14336, 32000, (pkg.F4_NF4, pkg.BF16, 128, pkg.COMP_BF16), 8, 32)
    c4["tokens_per_s"] = round(8 * 1e6 / us4, 1)
    c4["workload"] = "Mistral-7B NF4 g128 bf16-scale, batch 8 decode GEMM chain, 32 layers x {QKV (GQA 4096/1024/1024), WO, gate/up, down} + lm_head"
    out["config4"] = c4
    d, ff, kvd = 8192, 28672, 1024
    c5, us5 = run(d, d // 8, kvd // 8, d // 8, ff // 8, 32000, (pkg.S4, pkg.BF16, 32, pkg.COMP_INT8), 1, 80)
    c5["workload"] = "Llama-2-70B Q4_0 g32, batch 1, one rank's shards of TP = 8 (N or K / 8), 80 layers + lm_head; all-reduces not included"
    # (stable keys: one rank's shards timed on one GPU carry no collective — null here, filled by a TP = 8 run's headline keys of the same names)
    c5["all_reduce_us"], c5["all_reduces_per_step"], c5["comm_fraction"] = None, 160, None
    out["config5"] = c5
    return out


def _cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except Exception:
        pass
    return "unknown"


def cpu_baseline(chain, n_layers):
    """The oracle's ports of the reference's two decode paths, timed on this box's host cores (SURVEY 8d / BASELINE.md
    section 3): `fp32` = gemv_4bit_fp32_fp32 (kernel_ref.h:2489-2531), `u8s8` = the DEFAULT int8-compute path
    (quantize_fp_u8_colblock + gemv_4bit_u8s8_fp32, kernel_ref.h:1824-1883, :2371-2429), both streamed from the packed
    blobs with OpenMP over the column tiles, and — when the host has AVX512-VNNI — the reference's OWN kernels built from
    its tree (oracle/_ref/libkernel_avx_ref.so), swept over {64, 128, 256} threads; `value` = the steady-state MEDIAN at the
    best thread count, the minimum beside it (`value_min`), plus the packed-weight GB/s that median corresponds to next to
    the host's nominal DRAM rate.  Protocol: warm-ups, then >= 30-50 timed layer passes (7 GEMVs each) cycling
    through 4 DIFFERENT layers' weights + lm_head = 0.53 GB working set, larger than any last-level cache (the reference
    benchmark cycles its weights the same way, ut/bestla_ut.h:69-76); steady-state MIN and median; tokens/s = 1 / (32 x
    layer + lm_head).  A reported baseline (kernel_ref restatement, NOT the BesTLA JIT), not the target."""
    nso = ge.load_oracle()
    if not chain.host_layers:
        return None
    avail = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    # 64 threads: the port parallelises over 85..667 column tiles per GEMV with one OpenMP region each; on the 256-thread
    # GPU hosts it runs 100x SLOWER at 256 threads than at 64 (0.04 vs 6 tokens/s, profiles/r02m_bench.json: fork/join and
    # dynamic-schedule contention dominate 50 us of work per thread), so the baseline uses the setting that favours the CPU
    ncores = min(avail, 64)
    rng = np.random.default_rng(7)

    def aligned(v):
        b = nso.aligned_bytes(v.size)
        b[:] = v
        return b

    layers = [{k: aligned(v) for k, v in hl.items()} for hl in chain.host_layers]
    head = aligned(chain.host_blobs["head"])
    x = rng.standard_normal((1, CFG["n_embd"])).astype(np.float32)
    xf = rng.standard_normal((1, chain.ffl)).astype(np.float32)

    def layer_pass(gemv, lw):
        t0 = time.perf_counter()
        for nm in ("q", "k", "v", "o", "w1", "w3"):
            gemv(x, lw[nm], ncores)
        gemv(xf, lw["w2"], ncores)
        return time.perf_counter() - t0

    def head_pass(gemv):
        t0 = time.perf_counter()
        gemv(x, head, ncores)
        return time.perf_counter() - t0

    res = {}
    t_begin = time.perf_counter()
    legs = [("fp32", nso.gemv_f32), ("u8s8", nso.gemv_u8s8)]
    # the reference's OWN decode kernels (avx512f::vnni::gemv_4bit_u8s8_fp32 + its AVX512 activation quantizer, built from the
    # reference tree into oracle/_ref/libkernel_avx_ref.so) when this host has AVX512-VNNI: the CPU path the reference
    # actually runs for one row, timed on the same blobs
    have_ref = nso.avxref() is not None
    if have_ref:
        try:  # one checked call before it is trusted with the timing loop
            probe = nso.gemv_u8s8_avx512vnni(rng.standard_normal((1, CFG["n_embd"])).astype(np.float32), layers[0]["q"], ncores).copy()
            have_ref = bool(np.all(np.isfinite(probe)))
        except Exception:
            have_ref = False
    if have_ref:
        legs.append(("u8s8_ref_avx512vnni", nso.gemv_u8s8_avx512vnni))
    layer_bytes = sum(v.size for v in layers[0].values())

    def run_leg(gemv, nthreads, min_passes, budget_s):
        nonlocal ncores
        saved, ncores = ncores, nthreads
        try:
            for it in range(3 if min_passes > 4 else 1):
                layer_pass(gemv, layers[it % len(layers)])
            head_pass(gemv)
            tl, th = [], []
            t_start = time.perf_counter()
            it = 0
            while it < min_passes or (time.perf_counter() - t_start < budget_s and it < 400):
                tl.append(layer_pass(gemv, layers[it % len(layers)]))
                if it % 4 == 0:
                    th.append(head_pass(gemv))
                it += 1
        finally:
            ncores = saved
        med_l, med_h = float(np.median(tl)), float(np.median(th))
        return {
            "threads": nthreads,
            "tokens_per_s_median": round(1.0 / (med_l * CFG["n_layer"] + med_h), 3),
            "tokens_per_s_min": round(1.0 / (min(tl) * CFG["n_layer"] + min(th)), 3),
            "layer_ms_min": round(min(tl) * 1e3, 3), "layer_ms_median": round(med_l * 1e3, 3),
            "lm_head_ms_min": round(min(th) * 1e3, 3), "iterations": it,
            "weights_GBps_median": round(layer_bytes / med_l / 1e9, 1),
        }

    for name, gemv in legs:
        if name == "u8s8_ref_avx512vnni":
            # the reference's own kernels: thread counts swept (the tiles of one GEMV are spread with one OpenMP region each;
            # which team size wins depends on the host), the best MEDIAN is the reported value
            # {64, 128, 256}; above 128 threads a pass can cost ~1 s (fork/join dominated), so fewer of them
            # (round 5: team sizes up to HALF the logical CPUs only — 256 threads on 64 cores / 256 logical CPUs read 0.037 tok/s,
            # an oversubscription artefact that cost seconds of every run)
            cap = max(1, (os.cpu_count() or avail) // 2)
            sweep = [run_leg(gemv, t, 30, 2.0) for t in sorted({t for t in (64, 128) if t <= min(avail, cap)} or {min(avail, cap)})]
            best_run = max(sweep, key=lambda r: r["tokens_per_s_median"])
            res[name] = dict(best_run, threads_sweep=[{k: r[k] for k in ("threads", "tokens_per_s_median", "tokens_per_s_min", "weights_GBps_median")}
                                                      for r in sweep])
        else:
            res[name] = run_leg(gemv, ncores, 50, 3.0)
    wall = time.perf_counter() - t_begin
    best = "u8s8_ref_avx512vnni" if have_ref else "u8s8"
    return {
        # the MEDIAN of the steady state (the minimum flattered the CPU by 20 %); the minimum is beside it
        "value": res[best]["tokens_per_s_median"],
        "value_min": res[best]["tokens_per_s_min"],
        "unit": "tokens/s",
        "cores": res[best]["threads"],
        "nproc": os.cpu_count(),
        "affinity_cpus": avail,
        "cpu_model": _cpu_model(),
        "kind": "reference" if have_ref else "port",
        # how far from the host's memory rate: packed weights streamed per second at the median vs the nominal DRAM rate of
        # the GPU hosts' CPU (EPYC 9575F: 12 channels DDR5-6000 = 576 GB/s; a STREAM triad reaches ~80 % of that)
        "weights_GBps_median": res[best]["weights_GBps_median"],
        "host_dram_nominal_GBps": 576 if "9575F" in _cpu_model() else None,
        "reference_kernel": ("bestla::kernel::avx512f::vnni::gemv_4bit_u8s8_fp32<bf16, 48, 1> + avx512f::quantize_fp_u8_colblock "
                             "(kernel_avx512_vnni.h:31-133, kernel_avx512f.h:1252-1377) per 48-column tile, tiles over OpenMP threads; "
                             "`value`") if have_ref else None,
        "sample": ("the reference's own AVX512-VNNI decode kernels (`value` = median at the best of the swept thread counts, see "
                   "reference_kernel) next to " if have_ref else "") +
                  "oracle ports of kernel_ref gemv_4bit_u8s8_fp32 (the reference's default compute_dtype=int8 path%s) and "
                  "gemv_4bit_fp32_fp32, OpenMP over column tiles; >= 30-50 layer passes (7 GEMVs) per leg cycling through %d "
                  "layers' weights + lm_head (%.2f GB working set), warm-ups, steady-state median / min, layer x 32 + lm_head; "
                  "%.1f s wall; kernel_ref restatement, not the BesTLA JIT"
                  % ("" if have_ref else "; `value`", len(layers),
                     (sum(sum(v.size for v in l.values()) for l in layers) + head.size) / 1e9, wall),
        "u8s8": res["u8s8"],
        "fp32": res["fp32"],
        "u8s8_ref_avx512vnni": res.get("u8s8_ref_avx512vnni"),
    }


if __name__ == "__main__":
    main()

"""csrc/ns_route.cpp, the transitions test_gpu_route_replay.py does not walk: an evaluation that is run AGAIN (fp16 overflow) at a token the plan replayed,
results fetched by bestla_device_memcpy + bestla_device_sync instead of _memcpy_sync, device memory freed while ops are handed over and not launched yet, a
first evaluation behind a loader's copies, a synchronisation behind bestla_device_load_storage.  Each of them returned wrong or non-finite results without
an error when it was wrong (round 6: all five were).

The expected value is an fp64 numpy model of the stream (tests/tools/route_stream_f64.py, checked on the CPU by test_route_stream_f64.py), not the same
kernels launched plainly.  Tolerance against it, measured on the MI355X with the PLAIN launches (replay=0: round 6's kernels, no part of the route under
test): d0 = largest per-token rel-l2 = 4.27e-4 for the ordinary inputs (seed 12) and 3.90e-4 for the overflow inputs at token 5 with device_kv_f16=0.  A
route-on run rounds activations to fp16 once at a different point (fused / carried-norm forms), which can double the rounding, not multiply it:
BAR = 2 x d0 rounded up to one digit = 9e-4.  The two other input sets are worse conditioned (test_route_stream_f64.py prints their sensitivity to fp16
activations: 6.3e-4 and 9.3e-4 against 4.0e-4) and have a d0 of their own by the same measurement — overflow at token 3: 6.48e-4, the existing overflow
case's first-token inputs: 9.58e-4 — and by the same rule BAR_WIDE = 2e-3 (both under the 4e-3 that twice the project's bar for one 7B-width layer against
fp64 allows).  Against the run with the fp16 shortcuts off from the start: 2e-3, caches 2e-3 (the existing overflow case's bars).  Largest values reached
are in each case's docstring."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from test_gpu_route_replay import DELTA, D, FF, HEADS, HS, NL, _api, _blobs, _ll, _run_layers  # noqa: F401

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import route_stream_f64 as rs  # noqa: E402

pytestmark = pytest.mark.gpu

BAR = 9e-4       # route-on run against the fp64 model: the ordinary inputs and the overflow inputs at token 5 (see above)
BAR_WIDE = 2e-3  # ... the overflow inputs at token 3 and the first-token overflow inputs
BAR_F32 = 2e-3   # against the device_kv_f16=0 run, and the caches
assert (D, FF, HEADS, HS, NL) == (rs.D, rs.FF, rs.HEADS, rs.HS, rs.NL)


def _stats(L):
    st = (C.c_uint64 * 8)()
    L.ns_hip_route_stats(st)
    return list(st)


def _against_model(model, outs, caches, what, bar=BAR):
    """every token finite and within the bar of the fp64 model, the caches within BAR_F32; prints each figure in front of its assertion, returns the largest"""
    worst = 0.0
    for t, (want, got) in enumerate(zip(model["outs"], outs)):
        assert np.all(np.isfinite(got)), (what, t)
        e = rs.rel_l2(got, want)
        worst = max(worst, e)
        print("%s: token %d rel-l2 against the fp64 model %.3g (bar %.1g)" % (what, t, e, bar))
        assert e < bar, (what, t, e)
    assert len(outs) == len(model["outs"])
    for i, (want, got) in enumerate(zip(model["caches"], caches)):
        assert np.all(np.isfinite(got)) and np.count_nonzero(got) > 0, (what, i)
        assert np.array_equal(want, got) or rs.rel_l2(got, want) < BAR_F32, (what, "cache", i, rs.rel_l2(got, want))
    print("%s: largest per-token rel-l2 against the fp64 model %.3g (bar %.1g)" % (what, worst, bar))
    return worst


def _overflow_run(L, nso, capfd, inputs, t_ov, **kw):
    """the stream with the fp16 shortcuts off from the start (replay=5) and with them on (replay=3); returns (fp32 run's outputs, route run's outputs and caches,
    stderr of the route run, tokens replayed before token t_ov ended, route statistics' differences over the route run)"""
    blobs, gam, xs = inputs
    _api(L)
    L.ns_hip_set_tuning.argtypes = [C.c_char_p, C.c_int]
    seen = []
    try:
        assert L.ns_hip_set_tuning(b"device_kv_f16", 0) == 0
        ref_out, _, _ = _run_layers(L, nso, blobs, gam, xs, replay=5)
        capfd.readouterr()
        assert L.ns_hip_set_tuning(b"device_kv_f16", 1) == 0
        st1 = _stats(L)
        got_out, got_c, st2 = _run_layers(L, nso, blobs, gam, xs, replay=3, hook=(t_ov, "end", lambda L_, q: seen.append(_stats(L_))), **kw)
        err = capfd.readouterr().err
    finally:
        L.ns_hip_set_tuning(b"device_kv_f16", -1)
        L.ns_hip_route_set_enabled(1)
    return ref_out, got_out, got_c, err, seen[0][0] - st1[0], [st2[i] - st1[i] for i in range(4)]


def _check_overflow_run(nso, inputs, t_ov, run, what, bar=BAR):
    ref_out, got_out, got_c, err, replayed_before, _ = run
    blobs, gam, xs = inputs
    assert err.count("beyond the fp16 range") == 1, err[-1500:]
    assert "could not be run again" not in err, err[-1500:]
    if t_ov >= 2:
        assert replayed_before >= 1, replayed_before   # (the overflowing token is one the plan replays, not the plan's first)
    model = rs.run(rs.unpack(nso, blobs), gam, xs)
    assert model["max_k"][t_ov][0] >= 2 * rs.F16_MAX
    worst = _against_model(model, got_out, got_c, what, bar)
    for t, (a, b) in enumerate(zip(ref_out, got_out)):
        assert nso.rel_l2(b, a) < BAR_F32, (what, t, nso.rel_l2(b, a))
    return worst


@pytest.mark.parametrize("t_ov", [rs.T_OV, 3])
def test_overflow_at_a_replayed_token_is_evaluated_again_from_its_own_input(L, pkg, nso, capfd, t_ov):
    """K leaves the fp16 range at token 5 of 10 (rs.overflow_inputs: one large direction, well conditioned — test_route_stream_f64.py) — a token that is
    REPLAYED: it ran on the plan's activations, its own input sits DELTA * k bytes above the plan's, inside memory the plan's segments have written.  Run again
    on the fp32 forms it must start from ITS input (the route's stash): that token and every later token equal the fp64 model, one message on stderr.
    Round 6: the stash was declared stale when the evaluation ended, in front of the overflow check, and nothing was restored.  Whether that shows depends on
    where DELTA * k lands: token 5 (k = 4) lands on the second norm's two tensors, which a plan with carried norms never writes — round 6 passed it by
    that accident (3.95e-4) —, token 3 (k = 2) on the V and Q rows: round 6 returned finite, wrong logits there (rel-l2 1.36 at token 3).
    Reached with the fix: 3.95e-4 (token 5, bar 9e-4), 6.45e-4 (token 3, bar 2e-3)."""
    inputs = rs.overflow_inputs(nso, t_ov=t_ov)
    run = _overflow_run(L, nso, capfd, inputs, t_ov)
    _check_overflow_run(nso, inputs, t_ov, run, "overflow at replayed token %d" % t_ov, BAR if t_ov == rs.T_OV else BAR_WIDE)


@pytest.mark.parametrize("where", ["first", "replayed"])
def test_overflow_with_results_fetched_by_memcpy_and_sync(L, pkg, nso, capfd, where):
    """The same, the token's output fetched by bestla_device_memcpy + bestla_device_sync (both exported) instead of bestla_device_memcpy_sync: at the first
    token (the existing overflow case's inputs) and at replayed token 5.  Round 6: only _memcpy_sync copied again behind a re-evaluation; this caller kept
    the first pass (round 6: non-finite at the first token; rel-l2 0.25 at token 5).  Now a copy from device memory waits and lets the route look first.
    Reached with the fix: 9.58e-4 (first token, bar 2e-3), 3.95e-4 (token 5, bar 9e-4)."""
    inputs, t_ov = (rs.first_token_overflow_inputs(nso), 0) if where == "first" else (rs.overflow_inputs(nso), rs.T_OV)
    run = _overflow_run(L, nso, capfd, inputs, t_ov, fetch="memcpy+sync")
    _check_overflow_run(nso, inputs, t_ov, run, "overflow at the %s token, memcpy + sync" % where, BAR_WIDE if where == "first" else BAR)


@pytest.mark.parametrize("call", ["device_free", "storage_release"])
@pytest.mark.parametrize("tok", [1, 6])
@pytest.mark.parametrize("where", ["mid", "end"])
def test_a_free_between_hand_over_and_sync_loses_no_launch(L, pkg, nso, where, tok, call):
    """Device memory that has nothing to do with the stream is freed while a token's ops are handed over and not launched: token 1 (in the window) and token 6
    (replayed: its first segments have run on the plan's activations), between the two layers and behind the last forward, by bestla_device_free of a 1 MB
    allocation and by ns_hip_device_storage_release of a weight the stream does not use.  Dropping the plan on a free is allowed, dropping work is not:
    every token equals the fp64 model and counts once.  Round 6: route_invalidate cleared the window without launching it, and dropped the plan under a token
    half of which had run on the plan's addresses (rel-l2 1.0 .. 1.3 at the token of the free in all eight cases).
    Reached with the fix: 4.50e-4 (token 1), 4.54e-4 (token 6), bar 9e-4."""
    import torch
    blobs, gam, xs = rs.ordinary_inputs(nso, 12, 10)
    model = rs.run(rs.unpack(nso, blobs), gam, xs)
    _api(L)
    dev2 = L.bestla_create_device(False)
    q2 = L.bestla_get_device_queue(dev2)
    if call == "device_free":
        buf = L.bestla_device_malloc(1 << 20, q2)
        hook = lambda L_, q: L_.bestla_device_free(buf, q)
    else:
        blob = rs._pack(nso, np.random.default_rng(3).standard_normal((D, D)) * D ** -0.5)
        size = int(np.frombuffer(blob[:8].tobytes(), np.uint64)[0])
        buf = L.bestla_device_malloc((size + 255) // 256 * 256, q2)
        stor = np.zeros(int(L.bestla_device_storage_size()), np.uint8)
        L.bestla_device_load_storage(nso.ptr(blob), nso.ptr(stor), buf, q2)
        L.bestla_device_sync(q2)
        torch.cuda.synchronize()   # (the load is complete whatever the sync above waited for)
        hook = lambda L_, q: L_.ns_hip_device_storage_release(nso.ptr(stor))
    try:
        st1 = _stats(L)
        got_out, got_c, st2 = _run_layers(L, nso, blobs, gam, xs, replay=3, hook=(tok, where, hook))
    finally:
        if call == "storage_release":
            L.ns_hip_device_storage_release(nso.ptr(stor))   # (twice is harmless: the storage area is marked empty)
            L.bestla_device_free(buf, q2)
        L.bestla_release_device(dev2)
        L.ns_hip_route_set_enabled(1)
    replayed, eager = st2[0] - st1[0], st2[1] - st1[1]
    _against_model(model, got_out, got_c, "free (%s) at token %d, %s" % (call, tok, where))
    assert replayed + eager == len(xs), (replayed, eager)
    if tok == 6:
        assert replayed >= 4, replayed   # (tokens 2 .. 5 were replayed: the free met a plan)


@pytest.mark.parametrize("preload_mb", [300, 420])
def test_first_evaluation_after_a_large_load_can_still_be_run_again(L, pkg, nso, capfd, preload_mb):
    """300 MB of copies into device memory in front of the first token, as a loader makes them (60 MB at a time), then the existing overflow case: the first
    evaluation overflows and must be run again.  Round 6: the route kept EVERY copy since the process began as "the evaluation's input", gave up once that
    needed more than 512 MB, and then refused to run the evaluation again — its results kept the overflow.  It grew by doubling at 60, 120 and 180 MB (to
    360 MB of device memory), so 300 MB of 60 MB pieces still fitted and round 6 passed that case; the 420 MB case it failed ("could not be run again").
    Reached with the fix: 9.58e-4 in both (bar 2e-3)."""
    inputs = rs.first_token_overflow_inputs(nso)
    run = _overflow_run(L, nso, capfd, inputs, 0, preload_mb=preload_mb)
    _check_overflow_run(nso, inputs, 0, run, "first-token overflow behind a %d MB load" % preload_mb, BAR_WIDE)


def _hip_runtime():
    """the HIP runtime this process has loaded already (dlopen of a loaded file returns the handle that exists)"""
    with open("/proc/self/maps") as f:
        paths = sorted({line.split()[-1] for line in f if "libamdhip64" in line})
    assert paths, "no HIP runtime loaded"
    return C.CDLL(paths[0])


def test_sync_after_load_storage_waits_for_the_load(L, pkg, nso):
    """bestla_device_sync is a queue wait (the reference's is): behind bestla_device_load_storage of an 11008 x 4096 S4 g32 blob — 24 MB uploaded and
    re-laid-out by kernels on the queue — the queue must be idle when it returns: hipStreamQuery == hipSuccess.  Round 6: the load was not counted as
    pending work, the wait was left "to the next copy" and the call returned with the queue at work.
    ONE-SIDED: a load that happens to have finished by the time of the query passes either way; the case is not repeated to catch the other side."""
    import torch  # (its HIP runtime first: one runtime per process)
    _api(L)
    hip = _hip_runtime()
    hip.hipStreamQuery.argtypes = [C.c_void_p]
    hip.hipStreamQuery.restype = C.c_int
    rng = np.random.default_rng(2)
    blob = rs._pack(nso, rng.standard_normal((11008, 4096), dtype=np.float32) * np.float32(4096 ** -0.5))
    size = int(np.frombuffer(blob[:8].tobytes(), np.uint64)[0])
    dev = L.bestla_create_device(False)
    q = L.bestla_get_device_queue(dev)
    dptr = L.bestla_device_malloc((size + 255) // 256 * 256, q)
    stor = np.zeros(int(L.bestla_device_storage_size()), np.uint8)
    try:
        torch.cuda.synchronize()   # (idle in front of the load: the context's warm-up work is done)
        assert hip.hipStreamQuery(q) == 0
        L.bestla_device_load_storage(nso.ptr(blob), nso.ptr(stor), dptr, q)
        L.bestla_device_sync(q)
        busy = hip.hipStreamQuery(q)
        assert busy == 0, "the queue is still working behind bestla_device_sync (hipStreamQuery = %d; 600 = hipErrorNotReady)" % busy
    finally:
        L.ns_hip_device_storage_release(nso.ptr(stor))
        L.bestla_device_free(dptr, q)
        L.bestla_release_device(dev)

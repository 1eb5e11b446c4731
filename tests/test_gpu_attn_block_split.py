"""attn_block_split_kernel (neural-speed_amd/csrc/ns_attn_block.hip) behind ns_hip_set_tuning("attn_block_split", v): 2 .. 127 query rows over a long
cache, the context split into ranges, one matrix-core workgroup per (64 slots of a kv head, range), attn_merge_kernel behind it.  Opt-in: every
test turns the key on itself and a fixture puts it back to 0 (the key is process-wide, other tests pin paths).

Reference and bounds are the project's (tests/test_gpu_attention_paths.py): nso.attn_ref, rel_l2 < 1e-3 over the tensor and, per (batch, row, head),
max(2^-11, 4 d) with d the row's distance between the fp64 rounding model and the reference.  ns_hip_attn_stats tells which kernel family served a
call: index 7 is this path's."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_attention_paths import case_against_the_reference, check, rounding_model, run, worker
from test_gpu_kvcache import forward as cache_forward, kv_info, update

pytestmark = pytest.mark.gpu
BLOCK_SPLIT = 7  # AttnPath::AP_BLOCK_SPLIT (neural-speed_amd/csrc/ns_attn.h), the index of ns_hip_attn_stats
KEY = b"attn_block_split"


@pytest.fixture(autouse=True)
def key_back_to_zero(L):
    # the host entries take K / V for a library-managed cache when a device mirror exists at their host addresses (ns_kvcache.hip): none of an earlier
    # test's cache, whose memory numpy may hand out again, survives into a test here
    L.ns_hip_cache_clear()
    yield
    L.ns_hip_set_tuning(KEY, 0)


def stats(L):
    out = (C.c_uint64 * 8)()
    L.ns_hip_attn_stats(out)
    return np.array(out[:], np.int64)


def only_the_new_path_moved(before, after, calls=1):
    d = after - before
    return d[BLOCK_SPLIT] == calls and d.sum() == calls


# ---- the main cases -------------------------------------------------------------------------------------------------------------------------
CASES = [  # bs, heads, heads_kv, head_size, sl_q, sl_kv, flags
    (1, 4, 4, 128, 16, 512, 1),    # one full wave, MHA
    (1, 4, 4, 64, 2, 300, 1),      # smallest block, last range not a multiple of 64
    (2, 8, 2, 64, 5, 333, 1),      # GQA slots, 20 of 64 live, batch 2
    (1, 8, 1, 128, 9, 257, 1),     # 72 slots: two slot blocks, the second with 8 live slots, a last range of one key
    (1, 2, 2, 64, 100, 260, 1),    # the first slot block's kv_end lies in front of the last range: the empty-record exit
    (1, 4, 2, 128, 127, 1000, 0),  # not causal, four slot blocks
    (1, 4, 4, 128, 33, 2065, 1),   # many ranges
]


@pytest.mark.parametrize("case", CASES)
def test_block_split_against_the_reference(L, pkg, nso, case):
    assert L.ns_hip_set_tuning(KEY, 1) == 0
    before = stats(L)
    case_against_the_reference(L, pkg, nso, "block split %s" % (case,), case, 71)
    assert only_the_new_path_moved(before, stats(L)), (before, stats(L))


def test_negative_score_scale(L, pkg, nso):
    assert L.ns_hip_set_tuning(KEY, 1) == 0
    case = (1, 4, 2, 64, 20, 400, 1)
    before = stats(L)
    case_against_the_reference(L, pkg, nso, "block split, negative QK_scale %s" % (case,), case, 72, qk_scale=-float(1.0 / np.sqrt(case[3])))
    assert only_the_new_path_moved(before, stats(L))


def test_tensor_scales_are_applied_once(L, pkg, nso):
    """Q_sc and K_sc scale the scores, V_sc / dst_sc the output: the range kernel leaves out_scale to the merge"""
    assert L.ns_hip_set_tuning(KEY, 1) == 0
    case = (1, 4, 2, 128, 40, 600, 1)
    before = stats(L)
    case_against_the_reference(L, pkg, nso, "block split, tensor scales %s" % (case,), case, 73, scales=(0.5, 2.0, 3.0, 1.5))
    assert only_the_new_path_moved(before, stats(L))


# ---- the device entry: strided output, the fp16 shadow, the caller's workspace, capture ---------------------------------------------------------
def device_call(L, pkg, q, k, v, flags, dst_ptr, dst16_ptr=None, tmp_ptr=None, dst_row=None, stream=None):
    import torch
    bs, sl_q, hn, hs = q.shape
    a = pkg.attn_args(q.data_ptr(), k.data_ptr(), v.data_ptr(), dst_ptr, bs, hn, k.shape[2], hs, sl_q, k.shape[1], float(1.0 / np.sqrt(hs)), flags)
    if dst_row is not None:
        a.step_dst_sl, a.step_dst_bs = dst_row, sl_q * dst_row
    a.tmp = tmp_ptr
    st = C.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
    pkg.check(L.ns_hip_attn_fp32_fp16_fp16_fp32_forward_h(C.byref(a), dst16_ptr, st))
    return a


def test_strided_unaligned_output_and_the_fp16_shadow(L, pkg, nso):
    """dst one float off a 16-byte boundary with rows 4 floats longer than heads x head_size, dst16 with the same element strides: written by the
    merge, the bytes between the rows untouched"""
    import torch
    assert L.ns_hip_set_tuning(KEY, 1) == 0
    bs, hn, hkv, hs, sl_q, sl_kv = 1, 4, 2, 128, 19, 400
    q, k, v = worker.inputs(bs, hn, hkv, hs, sl_q, sl_kv, 74)
    scale = float(1.0 / np.sqrt(hs))
    ref = nso.attn_ref(q, k, v, scale, 1)
    dq, dk, dv = torch.from_numpy(q).cuda(), torch.from_numpy(k).cuda(), torch.from_numpy(v).cuda()
    row = hn * hs + 4
    buf = torch.full((1 + sl_q * row,), 7.0, device="cuda")
    buf16 = torch.full((1 + sl_q * row,), 7.0, device="cuda", dtype=torch.float16)
    before = stats(L)
    device_call(L, pkg, dq, dk, dv, 1, buf.data_ptr() + 4, C.c_void_p(buf16.data_ptr() + 2), dst_row=row)
    torch.cuda.synchronize()
    assert only_the_new_path_moved(before, stats(L))
    rows = buf[1:].cpu().numpy().reshape(sl_q, row)
    rows16 = buf16[1:].float().cpu().numpy().reshape(sl_q, row)
    out = rows[:, :hn * hs].reshape(q.shape)
    check(nso, "block split, strided dst", out, ref, rounding_model(q, k, v, scale, 1))
    assert np.array_equal(rows16[:, :hn * hs].reshape(q.shape), out.astype(np.float16).astype(np.float32))
    assert np.all(rows[:, hn * hs:] == 7.0) and np.all(rows16[:, hn * hs:] == 7.0) and float(buf[0]) == 7.0 and float(buf16[0]) == 7.0


@pytest.mark.parametrize("case,fits", [((1, 4, 4, 128, 16, 512, 1), True), ((1, 4, 2, 128, 127, 1000, 0), False)])
def test_the_callers_workspace_serves_only_where_it_is_large_enough(L, pkg, nso, case, fits):
    """bestla_fusion_attn_workspace_size does not know the path: partials that fit its answer go to the caller's tmp, larger ones to the stream's
    scratch — tmp (0xff bytes, with as many behind it) is then not touched at all"""
    import torch
    assert L.ns_hip_set_tuning(KEY, 1) == 0
    bs, hn, hkv, hs, sl_q, sl_kv, flags = case
    q, k, v = worker.inputs(bs, hn, hkv, hs, sl_q, sl_kv, 75)
    scale = float(1.0 / np.sqrt(hs))
    size = L.bestla_fusion_attn_workspace_size(C.byref(pkg.AttnShape(bs, hn, hkv, hs, sl_q, sl_kv)))
    ws = torch.full((2 * size,), 0xff, dtype=torch.uint8, device="cuda")
    dq, dk, dv = torch.from_numpy(q).cuda(), torch.from_numpy(k).cuda(), torch.from_numpy(v).cuda()
    dd = torch.full_like(dq, 7.0)
    before = stats(L)
    device_call(L, pkg, dq, dk, dv, flags, dd.data_ptr(), tmp_ptr=ws.data_ptr())
    torch.cuda.synchronize()
    assert only_the_new_path_moved(before, stats(L))
    check(nso, "block split, caller's tmp %s" % (case,), dd.cpu().numpy(), nso.attn_ref(q, k, v, scale, flags), rounding_model(q, k, v, scale, flags))
    got = ws.cpu().numpy()
    assert np.all(got[size:] == 0xff)
    assert bool(np.any(got[:size] != 0xff)) == fits


def test_captured_and_replayed_on_new_cache_contents(L, pkg, nso):
    """one eager call on the stream grows its scratch; the call is then captured, K / V rows are overwritten, and the replay gives what an eager
    call gives on the new contents"""
    import torch
    assert L.ns_hip_set_tuning(KEY, 1) == 0
    bs, hn, hkv, hs, sl_q, sl_kv = 1, 8, 2, 128, 12, 700
    q, k, v = worker.inputs(bs, hn, hkv, hs, sl_q, sl_kv, 76)
    _, k2, v2 = worker.inputs(bs, hn, hkv, hs, sl_q, sl_kv, 77)
    dq, dk, dv = torch.from_numpy(q).cuda(), torch.from_numpy(k).cuda(), torch.from_numpy(v).cuda()
    dd = torch.full_like(dq, 7.0)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    before = stats(L)
    with torch.cuda.stream(s):
        device_call(L, pkg, dq, dk, dv, 1, dd.data_ptr(), stream=s)
        s.synchronize()
        first = dd.clone()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            device_call(L, pkg, dq, dk, dv, 1, dd.data_ptr(), stream=s)
        assert only_the_new_path_moved(before, stats(L), calls=2)
        dd.fill_(7.0)
        g.replay()
        s.synchronize()
        assert torch.equal(dd, first)
        dk[:, 100:400].copy_(torch.from_numpy(k2[:, 100:400]).cuda())
        dv[:, 650:].copy_(torch.from_numpy(v2[:, 650:]).cuda())
        dd.fill_(7.0)
        g.replay()
        s.synchronize()
        replayed = dd.clone()
        dd.fill_(7.0)
        device_call(L, pkg, dq, dk, dv, 1, dd.data_ptr(), stream=s)
        s.synchronize()
    assert torch.equal(replayed, dd) and not torch.equal(replayed, first)
    kn, vn = dk.cpu().numpy(), dv.cpu().numpy()
    scale = float(1.0 / np.sqrt(hs))
    check(nso, "block split, replayed", replayed.cpu().numpy(), nso.attn_ref(q, kn, vn, scale, 1), rounding_model(q, kn, vn, scale, 1))


# ---- the library-managed cache ---------------------------------------------------------------------------------------------------------------
def test_a_chunk_appended_to_the_library_managed_cache(L, pkg, nso):
    """head-major slabs of 1024 rows with 0x7f bytes (fp16 NaNs) behind the appended rows: a 12-row chunk at position 500.  The last block of the
    last range reaches past row 511 into those bytes: the fetch clamps and V^T's zero fill are tied to sl_kv"""
    assert L.ns_hip_set_tuning(KEY, 1) == 0
    bs, hn, hkv, hs, n_ctx, past, n = 1, 4, 2, 128, 1024, 500, 12
    rng = np.random.default_rng(78)
    info = kv_info(L, pkg, hkv, hs, n_ctx)
    kc = np.full(bs * info.k_bytes, 0x7f, np.uint8)
    vc = np.full(bs * info.v_bytes, 0x7f, np.uint8)
    kf = rng.standard_normal((bs, past + n, hkv, hs)).astype(np.float32)
    vf = rng.standard_normal((bs, past + n, hkv, hs)).astype(np.float32)
    q = rng.standard_normal((bs, n, hn, hs)).astype(np.float32)
    scale = float(hs ** -0.5)
    for off, rows in ((0, past), (past, n)):
        update(L, pkg, "bestla_reordered_attn_fp32_update_k", kc, kf[:, off:off + rows], off, n_ctx)
        update(L, pkg, "bestla_reordered_attn_fp32_update_v", vc, vf[:, off:off + rows], off, n_ctx)
    before = stats(L)
    try:
        out = cache_forward(L, pkg, q, kc, vc, info, bs, hn, hkv, hs, n, past + n, scale, 1)
    finally:
        L.ns_hip_cache_clear()  # ... and none of this one for a later test whose K / V land at these host addresses
    assert only_the_new_path_moved(before, stats(L))
    k16, v16 = kf.astype(np.float16), vf.astype(np.float16)
    check(nso, "block split over the library-managed cache", out, nso.attn_ref(q, k16, v16, scale, 1), rounding_model(q, k16, v16, scale, 1))
    assert np.all(kc.reshape(bs, hkv, n_ctx, hs * 2)[:, :, past + n:] == 0x7f) and np.all(vc.reshape(bs, hkv, n_ctx, hs * 2)[:, :, past + n:] == 0x7f)


# ---- outside the envelope, determinism -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [
    (1, 8, 8, 128, 16, 512, 3),    # ALiBi
    (1, 4, 4, 80, 16, 512, 1),     # head size 80
    (1, 4, 4, 128, 1, 512, 1),     # one query row
    (1, 4, 4, 128, 128, 512, 1),   # 128 query rows
    (1, 4, 4, 128, 16, 200, 1),    # fewer than 256 keys
])
def test_calls_outside_the_envelope_are_served_as_with_the_key_at_zero(L, pkg, nso, case):
    assert L.ns_hip_set_tuning(KEY, 1) == 0
    bs, hn, hkv, hs, sl_q, sl_kv, flags = case
    q, k, v = worker.inputs(bs, hn, hkv, hs, sl_q, sl_kv, 79)
    before = stats(L)
    on = run(L, pkg, q, k, v, flags)
    mid = stats(L)
    assert L.ns_hip_set_tuning(KEY, 0) == 0
    off = run(L, pkg, q, k, v, flags)
    after = stats(L)
    assert (mid - before)[BLOCK_SPLIT] == 0 and (mid - before).sum() == 1 and np.array_equal(mid - before, after - mid)
    assert np.all(np.isfinite(off)), "the call with the key at 0"
    assert np.array_equal(on.view(np.uint32), off.view(np.uint32))


def test_the_key_is_a_threshold_and_zero_is_off(L, pkg, nso):
    assert L.ns_hip_set_tuning(KEY, 1) == 0
    q, k, v = worker.inputs(1, 4, 4, 128, 16, 512, 80)
    paths = []
    for value in (1, 512, 513, 0, -3):
        assert L.ns_hip_set_tuning(KEY, value) == 0
        before = stats(L)
        run(L, pkg, q, k, v, 1)
        paths.append(int(np.argmax(stats(L) - before)))
    assert paths == [BLOCK_SPLIT, BLOCK_SPLIT, 4, 4, 4]  # (4: the 64-row matrix-core kernel)


def test_the_same_call_twice_gives_the_same_bits(L, pkg, nso):
    assert L.ns_hip_set_tuning(KEY, 1) == 0
    q, k, v = worker.inputs(2, 8, 2, 64, 5, 333, 81)
    before = stats(L)
    a, b = run(L, pkg, q, k, v, 1), run(L, pkg, q, k, v, 1)
    assert only_the_new_path_moved(before, stats(L), calls=2)
    assert np.all(np.isfinite(a)) and np.array_equal(a.view(np.uint32), b.view(np.uint32))

"""The branches of launch_attn (neural-speed_amd/csrc/ns_attn.cpp) that no other attention test lands on, each against nso.attn_ref:
the long-key schedule of attn_mfma3_kernel (sl_kv >= 3072: the next tile requested behind K.Q^T, idle waves requesting in a branch of
their own) and its bit-equality with the short-key schedule, the 128-row kernels over the library-managed head-major cache with NaN
bytes behind the appended rows, tensor scales and a non-positive score scale on the matrix-core kernels, unmasked attention with more
queries than keys, head-major (permuted) Q / dst, and the XCD remap of workgroups with a head group above one.
docs/kernels/attention.md ("What tests which launch path") maps every path to its test.

Two bounds per case.  The project's tensor bound, rel_l2 < 1e-3 — and one PER ROW, because a single wrong row among heads x rows
weighs 1 / sqrt(rows) in the tensor metric and passes it (test_one_wrong_row_passes_the_tensor_metric_and_fails_the_row_check shows
that on the reference alone, without a GPU).  The per-row bound is not taken from the kernels: rounding_model() is an fp64 attention of
the same inputs with the two roundings the matrix cores are fed — Q to fp16, every unnormalised softmax weight exp(s - rowmax) to
fp16 in front of the P.V sum — and a row may be off by max(2^-11, 4 x that row's distance between the model and the reference):
one fp16 unit as the floor, the factor 4 for accumulation order, the hardware exp2 and the rescale by the running maximum.

Every test but the last needs the GPU and carries the gpu mark itself, so that the last one runs without one."""
import ctypes as C
import importlib.util
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from test_gpu_kvcache import forward as cache_forward, kv_info, update

gpu = pytest.mark.gpu
TOL = 1e-3
ROW_FLOOR, ROW_FACTOR = 2.0 ** -11, 4.0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "tools", "attn_variant_worker.py")
_spec = importlib.util.spec_from_file_location("attn_variant_worker", WORKER)
worker = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(worker)


# ---- the per-row check --------------------------------------------------------------------------------------------------------
def attn_row_errors(out, ref):
    """||out - ref|| / ||ref|| over the head dimension, for every (batch, row, head) of [bs][sl_q][heads][hs] tensors"""
    out, ref = np.asarray(out, np.float64), np.asarray(ref, np.float64)
    return np.linalg.norm(out - ref, axis=-1) / np.maximum(np.linalg.norm(ref, axis=-1), 1e-30)


def rounding_model(q, k, v, qk_scale, flags, scales=(1.0, 1.0, 1.0, 1.0)):
    """fp64 attention of q fp32 [bs][sl_q][heads][hs], k / v fp16 [bs][sl_kv][heads_kv][hs] with the operand roundings of the
    matrix-core kernels: Q rounded to fp16, each unnormalised weight exp(s - rowmax) rounded to fp16 before P.V (the row sum keeps
    the unrounded weights).  flags: 0 or 1 (causal: row i sees keys 0 .. i + sl_kv - sl_q)."""
    assert flags in (0, 1)
    bs, sl_q, hn, hs = q.shape
    sl_kv, hkv = k.shape[1], k.shape[2]
    q_sc, k_sc, v_sc, dst_sc = scales
    sc = float(np.float32(qk_scale)) * q_sc * k_sc
    q16 = q.astype(np.float16).astype(np.float64)
    out = np.zeros(q.shape, np.float64)
    hidden = np.arange(sl_kv)[None, :] > (np.arange(sl_q)[:, None] + (sl_kv - sl_q)) if flags & 1 else None
    for b in range(bs):
        for h in range(hn):
            kk, vv = k[b, :, h // (hn // hkv)].astype(np.float64), v[b, :, h // (hn // hkv)].astype(np.float64)
            s = (q16[b, :, h] @ kk.T) * sc
            if hidden is not None:
                s[hidden] = -np.inf
            p = np.exp(s - s.max(axis=1, keepdims=True))
            out[b, :, h] = (p.astype(np.float16).astype(np.float64) @ vv) / p.sum(axis=1, keepdims=True) * (v_sc / dst_sc)
    return out


def row_bounds(model, ref):
    return np.maximum(ROW_FLOOR, ROW_FACTOR * attn_row_errors(model, ref))


def failing_rows(out, ref, bounds):
    """(batch, row, head) of every row whose error exceeds its bound"""
    return [tuple(int(x) for x in w) for w in np.argwhere(attn_row_errors(out, ref) > bounds)]


def check(nso, tag, out, ref, model):
    """finite, tensor bound, per-row bound; prints both figures (the table in docs/kernels/attention.md is made of these lines)"""
    assert np.all(np.isfinite(out)), tag
    e = nso.rel_l2(out, ref)
    bounds = row_bounds(model, ref)
    ratio = attn_row_errors(out, ref) / bounds
    w = tuple(int(x) for x in np.unravel_index(np.argmax(ratio), ratio.shape))
    print("ATTN_PATHS %s: rel_l2 %.3g, worst row_err / bound %.3f at (batch, row, head) %s (bound %.3g)" % (tag, e, float(ratio[w]), w, float(bounds[w])))
    assert e < TOL, (tag, e)
    bad = failing_rows(out, ref, bounds)
    assert not bad, (tag, len(bad), bad[:8], float(ratio.max()))


def run(L, pkg, q, k, v, flags, qk_scale=None, scales=None, q_perm=False, dst_perm=False):
    """the host-tensor entry; q_perm / dst_perm: Q / dst handed over head-major, as [bs][heads][sl_q][hs] buffers (the reference's
    graph passes Q as such a permuted view).  The output buffer starts as 7.0; returned position-major."""
    bs, sl_q, hn, hs = q.shape
    sl_kv, hkv = k.shape[1], k.shape[2]
    qb = np.ascontiguousarray(q.transpose(0, 2, 1, 3)) if q_perm else q
    out = np.full((bs, hn, sl_q, hs) if dst_perm else q.shape, 7.0, np.float32)
    a = pkg.attn_args(qb.ctypes.data, k.ctypes.data, v.ctypes.data, out.ctypes.data, bs, hn, hkv, hs, sl_q, sl_kv,
                      float(1.0 / np.sqrt(hs)) if qk_scale is None else qk_scale, flags)
    if scales is not None:
        a.Q_sc, a.K_sc, a.V_sc, a.dst_sc = scales
    if q_perm:
        a.step_q_head_num, a.step_q_sl = sl_q * hs, hs
    if dst_perm:
        a.step_dst_head_num, a.step_dst_sl = sl_q * hs, hs
    L.bestla_fusion_attn_fp32_fp16_fp16_fp32_forward(C.byref(a))
    return out.transpose(0, 2, 1, 3) if dst_perm else out


def case_against_the_reference(L, pkg, nso, tag, case, seed, qk_scale=None, scales=(1.0, 1.0, 1.0, 1.0), **layout):
    bs, hn, hkv, hs, sl_q, sl_kv, flags = case
    q, k, v = worker.inputs(bs, hn, hkv, hs, sl_q, sl_kv, seed)
    scale = float(1.0 / np.sqrt(hs)) if qk_scale is None else qk_scale
    out = run(L, pkg, q, k, v, flags, scale, scales, **layout)
    ref = nso.attn_ref(q, k, v, scale, flags, scales=scales)
    check(nso, tag, out, ref, rounding_model(q, k, v, scale, flags, scales))
    return out


# ---- 1 / 7: the long-key schedule of attn_mfma3_kernel (pvar = 3 from 3072 keys on), the XCD remap with a head group -------------
LONG_CASES = [  # bs, heads, heads_kv, head_size, sl_q, sl_kv, flags
    (1, 2, 2, 128, 128, 3072, 1),   # exactly at the threshold: one query block behind 2944 cached positions
    (1, 2, 2, 128, 128, 3071, 1),   # the same seed one key below it (variant 0): both schedules side by side
    (1, 4, 2, 64, 130, 3100, 1),    # hs 64, GQA; the second block has 2 rows (one wave nearly empty, three idle: the idle-wave request branch); ragged last tile (48 * 64 + 28)
    (1, 8, 8, 128, 200, 3135, 0),   # unmasked, ragged, workgroups remapped over the XCDs
    (2, 8, 4, 64, 257, 3073, 1),    # batch 2 x 4 kv heads: the remap with G = 2, three query blocks (the last with one row), heavy-first reversal on half the units
    (1, 2, 1, 64, 3072, 3072, 1),   # a whole prompt: every diagonal position under the schedule, 24 blocks
]
LONG_SEED = 3072
_long = {}


def long_case(L, pkg, nso, idx):
    """inputs, the default schedule's output and the reference of LONG_CASES[idx]: computed once, shared, never written to"""
    if idx not in _long:
        bs, hn, hkv, hs, sl_q, sl_kv, flags = LONG_CASES[idx]
        q, k, v = worker.inputs(bs, hn, hkv, hs, sl_q, sl_kv, LONG_SEED)
        scale = float(1.0 / np.sqrt(hs))
        out = worker.forward(L, pkg, q, k, v, flags)
        ref = nso.attn_ref(q, k, v, scale, flags)
        model = rounding_model(q, k, v, scale, flags)
        for x in (q, k, v, out, ref, model):
            x.setflags(write=False)
        _long[idx] = (q, k, v, out, ref, model)
    return _long[idx]


@gpu
@pytest.mark.parametrize("idx", range(len(LONG_CASES)))
def test_long_key_schedule(L, pkg, nso, idx):
    assert "NS_ATTN_PVAR" not in os.environ and "NS_ATTN_PIPE" not in os.environ  # the default dispatch is what is tested
    q, k, v, out, ref, model = long_case(L, pkg, nso, idx)
    check(nso, "long %s" % (LONG_CASES[idx],), out, ref, model)


_child_failed = []


def run_child(case, env_add):
    """the worker in a fresh process under a time limit of its own; after one child failed no other is started"""
    if _child_failed:
        pytest.fail("not started: an earlier child process failed (%s)" % _child_failed[0])
    env = dict(os.environ)
    env.update(env_add)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "out.npz")
        cmd = ["timeout", "-k", "10", "120", sys.executable, WORKER] + [str(x) for x in case] + [str(LONG_SEED), path]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, cwd=ROOT)
        if r.returncode != 0:
            _child_failed.append("%s %s: exit %d" % (env_add, case, r.returncode))
            pytest.fail("worker %s %s: exit %d\n%s\n%s" % (env_add, case, r.returncode, r.stdout[-2000:], r.stderr[-2000:]))
        return np.load(path)["out"]


@gpu
@pytest.mark.parametrize("idx", [1, 2, 4])
def test_short_key_schedule_gives_the_bits_of_the_long_key_schedule(L, pkg, nso, idx):
    """the variant moves the tile requests, not the arithmetic: NS_ATTN_PVAR=0 (read once per process, hence the child) and the default
    dispatch give identical bits (LONG_CASES[1] sits below the threshold and runs variant 0 either way; [2] and [4] switch schedule, [2] with
    idle waves, [4] with three query blocks per head and the workgroups remapped over the XCDs with G = 2)"""
    q, k, v, out, ref, model = long_case(L, pkg, nso, idx)
    got = run_child(LONG_CASES[idx], {"NS_ATTN_PVAR": "0"})
    assert got.shape == out.shape and got.dtype == np.float32
    assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(out).view(np.uint32)), int((got.view(np.uint32) != np.ascontiguousarray(out).view(np.uint32)).sum())


@gpu
def test_register_staged_128_row_kernel_at_exact_head_sizes(L, pkg, nso):
    """NS_ATTN_PIPE=0: attn_mfma2_kernel<64> without padding or bias, which the default dispatch never launches — parity only (its
    operands travel through registers; same arithmetic, but nothing here depends on that)"""
    q, k, v, out, ref, model = long_case(L, pkg, nso, 2)
    got = run_child(LONG_CASES[2], {"NS_ATTN_PIPE": "0"})
    check(nso, "NS_ATTN_PIPE=0 %s" % (LONG_CASES[2],), got, ref, model)


# ---- 2: the 128-row kernels over the library-managed cache -----------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("hn,hkv,hs,n_ctx,chunks", [
    (4, 2, 128, 320, (160,)),
    (4, 2, 128, 320, (130, 140)),      # a 140-row block behind 130 cached rows, on the head-major slab
    (4, 4, 64, 320, (160,)),
    (4, 4, 64, 320, (130, 140)),
    (4, 2, 128, 3200, (2950, 130)),    # the slab read under the long-key schedule (3080 keys)
])
def test_prefill_over_the_library_managed_cache(L, pkg, nso, hn, hkv, hs, n_ctx, chunks):
    """The cache is a head-major slab with capacity beyond sl_kv, filled with 0x7f bytes (fp16 NaNs) behind the appended rows:
    attn_mfma3_kernel's buffer descriptor must end at the last key, a probability of 0 times a stale NaN row of V is NaN."""
    bs = 1
    L.ns_hip_cache_clear()  # no mirror of an earlier test's cache at the same host address
    rng = np.random.default_rng(hs + n_ctx + len(chunks))
    info = kv_info(L, pkg, hkv, hs, n_ctx)
    kc = np.full(bs * info.k_bytes, 0x7f, np.uint8)
    vc = np.full(bs * info.v_bytes, 0x7f, np.uint8)
    total = sum(chunks)
    assert total < n_ctx
    kf = rng.standard_normal((bs, total, hkv, hs)).astype(np.float32)
    vf = rng.standard_normal((bs, total, hkv, hs)).astype(np.float32)
    k16, v16 = kf.astype(np.float16), vf.astype(np.float16)
    scale = float(hs ** -0.5)
    off = 0
    for i, n in enumerate(chunks):
        update(L, pkg, "bestla_reordered_attn_fp32_update_k", kc, kf[:, off:off + n], off, n_ctx)
        update(L, pkg, "bestla_reordered_attn_fp32_update_v", vc, vf[:, off:off + n], off, n_ctx)
        off += n
        q = rng.standard_normal((bs, n, hn, hs)).astype(np.float32)
        out = cache_forward(L, pkg, q, kc, vc, info, bs, hn, hkv, hs, n, off, scale, 1)
        assert np.all(np.isfinite(out)), i
        rows = slice(n - 64, n) if n > 1000 else slice(0, n)  # the long first chunk: its last 64 rows only, to keep the oracle short
        ref = nso.attn_ref(q[:, rows], k16[:, :off], v16[:, :off], scale, 1)
        check(nso, "cache hs %d n_ctx %d chunk %d of %s" % (hs, n_ctx, i, chunks), out[:, rows], ref,
              rounding_model(q[:, rows], k16[:, :off], v16[:, :off], scale, 1))
    for c, f16 in ((kc, k16), (vc, v16)):
        rows16 = c.view(np.float16).reshape(bs, hkv, n_ctx, hs)
        assert np.array_equal(rows16[:, :, :total].view(np.uint16), f16.transpose(0, 2, 1, 3).view(np.uint16))
        assert np.all(c.reshape(bs, hkv, n_ctx, hs * 2)[:, :, total:] == 0x7f)


# ---- 3: tensor scales on the matrix-core kernels ---------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("case", [
    (1, 4, 2, 128, 40, 200, 0),     # the 64-row kernel
    (1, 4, 2, 64, 200, 333, 1),     # the DMA-fed 128-row kernel, causal
    (1, 4, 4, 80, 150, 150, 1),     # padded on the 128-row kernel
    (1, 2, 2, 256, 129, 129, 1),    # head size 256
])
def test_tensor_scales_on_the_matrix_core_kernels(L, pkg, nso, case):
    case_against_the_reference(L, pkg, nso, "scales %s" % (case,), case, 31, scales=(0.5, 2.0, 3.0, 1.5))


# ---- 4: a non-positive QK_scale * Q_sc * K_sc --------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("door", ["QK_scale", "K_sc"])
@pytest.mark.parametrize("case", [
    (1, 4, 4, 128, 200, 333, 1),
    (1, 4, 2, 64, 130, 130, 0),
    (1, 4, 4, 80, 150, 200, 1),     # a padded size: leaves the matrix cores
])
def test_negative_score_scale_stays_off_the_raw_maximum_kernels(L, pkg, nso, case, door):
    """the 128-row kernels take the running maximum of RAW scores and scale afterwards, which is only a maximum for a positive scale:
    launch_attn keeps them for qk_scale > 0.  Without that gate the maximum would be the minimum and the weights overflow."""
    hs = case[3]
    if door == "QK_scale":
        case_against_the_reference(L, pkg, nso, "negative QK_scale %s" % (case,), case, 41, qk_scale=-float(1.0 / np.sqrt(hs)))
    else:
        case_against_the_reference(L, pkg, nso, "negative K_sc %s" % (case,), case, 41, scales=(1.0, -1.0, 1.0, 1.0))


@gpu
def test_zero_score_scale_is_the_mean_of_the_visible_rows(L, pkg, nso):
    case = (1, 2, 2, 128, 130, 200, 1)
    bs, hn, hkv, hs, sl_q, sl_kv, flags = case
    out = case_against_the_reference(L, pkg, nso, "zero QK_scale %s" % (case,), case, 43, qk_scale=0.0)
    q, k, v = worker.inputs(bs, hn, hkv, hs, sl_q, sl_kv, 43)
    mean = np.zeros(q.shape, np.float64)
    for i in range(sl_q):
        vis = i + (sl_kv - sl_q) + 1
        mean[0, i] = v[0, :vis].astype(np.float64).mean(axis=0)[np.arange(hn) // (hn // hkv)]
    assert nso.rel_l2(out, mean) < TOL
    assert float(attn_row_errors(out, mean).max()) <= ROW_FLOOR


# ---- 5: unmasked, more queries than keys -------------------------------------------------------------------------------------------
MORE_QUERIES = [
    (1, 4, 4, 128, 200, 50, 0),
    (1, 4, 2, 64, 130, 7, 0),
    (2, 2, 2, 80, 150, 33, 0),
    (1, 4, 4, 128, 3, 2, 0),        # the decode kernels
]


@gpu
@pytest.mark.parametrize("case", MORE_QUERIES)
def test_unmasked_attention_with_more_queries_than_keys(L, pkg, nso, case):
    """the cross-attention shape: sl_kv - sl_q is negative and must stay out of every address and count"""
    case_against_the_reference(L, pkg, nso, "sl_q > sl_kv %s" % (case,), case, 51)


@gpu
@pytest.mark.parametrize("case", MORE_QUERIES)
def test_causal_attention_with_more_queries_than_keys_is_refused(L, pkg, nso, case):
    bs, hn, hkv, hs, sl_q, sl_kv, _ = case
    q, k, v = worker.inputs(bs, hn, hkv, hs, sl_q, sl_kv, 51)
    out = run(L, pkg, q, k, v, 1)
    assert np.all(out == 7.0)
    assert b"causal" in L.ns_hip_last_error()


# ---- 6: head-major Q / dst -----------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("case,dst_perm", [
    ((1, 4, 2, 128, 200, 333, 1), True),
    ((2, 4, 4, 64, 129, 129, 1), True),
    ((1, 4, 4, 128, 40, 200, 1), True),     # the 64-row kernel
    ((1, 4, 4, 96, 130, 130, 1), True),     # padded
    ((1, 4, 2, 128, 200, 333, 1), False),   # Q head-major, dst position-major (what the reference's graph does)
])
def test_head_major_q_and_dst(L, pkg, nso, case, dst_perm):
    """Q and dst as [bs][heads][sl_q][hs] buffers (step_*_head_num = sl_q * hs, step_*_sl = hs): the vectorised output store of the
    128-row kernels with head-major steps, compared on the un-permuted view"""
    case_against_the_reference(L, pkg, nso, "head-major Q%s %s" % (" and dst" if dst_perm else "", case), case, 61, q_perm=True, dst_perm=dst_perm)


# ---- the per-row check has teeth (no GPU) -------------------------------------------------------------------------------------------
def test_one_wrong_row_passes_the_tensor_metric_and_fails_the_row_check(nso):
    """A causal off-by-one on ONE row of ONE head of a 16-head, 300-row prompt — the row sees one key too many — made from the reference
    alone: the tensor metric stays under the project's 1e-3, the per-row check names exactly that row."""
    bs, hn, hkv, hs, sl_q, sl_kv = 1, 16, 16, 128, 300, 300
    row, head = 219, 5  # the extra key carries about 1 / 220 of the row's weight
    q, k, v = worker.inputs(bs, hn, hkv, hs, sl_q, sl_kv, 300)
    scale = float(1.0 / np.sqrt(hs))
    ref = nso.attn_ref(q, k, v, scale, 1)
    bounds = row_bounds(rounding_model(q, k, v, scale, 1), ref)
    assert failing_rows(ref, ref, bounds) == []
    wrong = ref.copy()
    # the row as the last of a chunk behind row + 1 cached keys: it sees keys 0 .. row + 1
    wrong[0, row, head] = nso.attn_ref(q[:, row:row + 1, head:head + 1], k[:, :row + 2, head:head + 1], v[:, :row + 2, head:head + 1], scale, 1)[0, 0, 0]
    assert not np.array_equal(wrong[0, row, head], ref[0, row, head])
    e = nso.rel_l2(wrong, ref)
    r = float(attn_row_errors(wrong, ref)[0, row, head])
    print("ATTN_PATHS one wrong row: rel_l2 %.3g, row error %.3g against a bound of %.3g" % (e, r, float(bounds[0, row, head])))
    assert e < TOL, e
    assert failing_rows(wrong, ref, bounds) == [(0, row, head)]

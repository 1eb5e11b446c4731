"""The grouped pass of ns_hip_moe_ffn_silu (csrc/ns_moe.cpp ffn_grouped, csrc/ns_moe_plan.cpp): from "moe_ffn_grouped_rows" rows a call
outside a capture sorts all (row, selection) pairs by expert on the host, gathers their rows once, runs one fused gate / up and one down
launch of the tiled GEMM per populated expert and combines the products with the routing weights in one launch.  Checked against the
oracle's fp64 products and against the composition on the same inputs (the same entry with the tuning key negative); which path served a
call is read from ns_hip_moe_ffn_stats ([1] the composition, [3] the grouped pass).  Those counters are process-wide sums that nothing resets,
and tests/test_gpu_moe_ffn.py holds slot [3] at 0 for its calls of up to 8 rows: the files that run the grouped pass (this one,
test_gpu_moe_gelu.py) sort behind it, so in the suite's order that assertion holds; they compare differences only."""
import numpy as np
import pytest

from test_gpu_moe import FORMATS
from test_gpu_moe_ffn import BAR, D, N_AS, block, stats, stream

pytestmark = pytest.mark.gpu

KEY = b"moe_ffn_grouped_rows"
SENTINEL = 7.0


@pytest.fixture(autouse=True)
def default_tuning(L):
    for key, v in ((b"moe_ffn_fused", -1), (b"moe_gemv_rows", 0), (b"moe_grouped_rows", 0), (KEY, 0)):
        L.ns_hip_set_tuning(key, v)
    yield
    for key, v in ((b"moe_ffn_fused", -1), (KEY, 0)):
        L.ns_hip_set_tuning(key, v)


def act_silu(x):
    return x / (1 + np.exp(-x))


def act_gelu(x):  # the tanh form (kernel_ref.h:1570-1572)
    return 0.5 * x * (1 + np.tanh(0.7978845834732056 * (x + 0.044714998453855515 * x ** 3)))


def reference(nso, a, ids, wts, blk, act=act_silu):
    """fp64 over the oracle's blobs, one product per expert over the rows that selected it"""
    bg, _, bu, _, bd, _ = blk
    m, n_used = ids.shape
    out = np.zeros((m, D), np.float64)
    for e in range(N_AS):
        for i in range(n_used):
            rows = np.nonzero(ids[:, i] == e)[0]
            if len(rows) == 0:
                continue
            ar = np.ascontiguousarray(a[rows])
            gate, up = nso.gemm_f64(ar, bg[e]), nso.gemm_f64(ar, bu[e])
            h = (act(gate) * up).astype(np.float32)
            out[rows] += wts[rows, i:i + 1].astype(np.float64) * nso.gemm_f64(h, bd[e])
    return out


def padded(x, stride, fill, dtype):
    """device tensor [rows][stride] with x in its first columns and `fill` behind them"""
    import torch
    full = np.full((x.shape[0], stride), fill, dtype)
    full[:, :x.shape[1]] = x
    return torch.from_numpy(full).cuda()


def route(L, pkg, m, n_used, rng, ids_stride, w_stride):
    """ids and weights as ns_hip_moe_route leaves them, in rows longer than n_used"""
    import torch
    logits = rng.standard_normal((m, N_AS)).astype(np.float32)
    dL = torch.from_numpy(logits).cuda()
    dI = torch.full((m, ids_stride), -77, dtype=torch.int32, device="cuda")
    dW = torch.full((m, w_stride), float("nan"), dtype=torch.float32, device="cuda")
    pkg.check(L.ns_hip_moe_route(dL.data_ptr(), N_AS, m, N_AS, n_used, dI.data_ptr(), ids_stride, dW.data_ptr(), w_stride, None, stream()))
    torch.cuda.synchronize()
    return dI, dW, dI.cpu().numpy()[:, :n_used], dW.cpu().numpy()[:, :n_used]


def run(L, pkg, dA, dI, dW, m, n_used, blk, ldo=D, entry=None):
    """one call of the block entry on [m][lda] activations; (out [m][D], the padding columns)"""
    import torch
    _, gg, _, gu, _, gd = blk
    out = torch.full((m, ldo), SENTINEL, device="cuda")
    fn = entry or L.ns_hip_moe_ffn_silu
    pkg.check(fn(dA.data_ptr(), dA.shape[1], m, dI.data_ptr(), dI.shape[1], dW.data_ptr() if dW is not None else None,
                 dW.shape[1] if dW is not None else 0, n_used, gg, gu, gd, out.data_ptr(), ldo, stream()))
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    return o[:, :D], o[:, D:]


def inputs(L, pkg, m, n_used, seed, strided=True):
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((m, D)).astype(np.float32)
    dA = padded(a, D + 8 if strided else D, np.nan, np.float32)   # (a kernel that read the padding would return NaN)
    dI, dW, ids, wts = route(L, pkg, m, n_used, rng, n_used + 1 if strided else n_used, n_used + 3 if strided else n_used)
    return a, dA, dI, dW, ids, wts


@pytest.mark.parametrize("m,n_used", [(33, 1), (40, 2), (64, 2)])
@pytest.mark.parametrize("fmt", FORMATS, ids=[f[0] + "_" + f[1] for f in FORMATS])
def test_grouped_pass_against_fp64_and_the_composition(L, pkg, nso, fmt, m, n_used):
    ff = 512
    blk = block(L, pkg, nso, fmt, ff)
    a, dA, dI, dW, ids, wts = inputs(L, pkg, m, n_used, 100 * m + n_used)
    ref = reference(nso, a, ids, wts, blk)
    s0 = stats(L)
    out, pad = run(L, pkg, dA, dI, dW, m, n_used, blk, ldo=D + 5)
    s1 = stats(L)
    assert L.ns_hip_set_tuning(KEY, -1) == 0
    comp, _ = run(L, pkg, dA, dI, dW, m, n_used, blk, ldo=D + 5)
    s2 = stats(L)
    e_grouped, e_comp = nso.rel_l2(out, ref), nso.rel_l2(comp, ref)
    print("moe_ffn grouped %s m=%d n_used=%d: grouped %.3e composition %.3e" % (fmt[0] + "/" + fmt[1], m, n_used, e_grouped, e_comp))
    assert np.all(pad == SENTINEL)
    assert s1[3] - s0[3] == 1 and s1[0] == s0[0] and s1[1] == s0[1]
    assert s2[1] - s1[1] == 1 and s2[3] == s1[3]           # (the comparison really ran on the composition)
    assert e_grouped < BAR
    assert e_grouped <= 1.5 * e_comp


@pytest.mark.parametrize("lone", [0, 3])
def test_engineered_ids_row_by_row(L, pkg, nso, lone):
    """m = 40, top-2: one expert with exactly one pair (the first group, then the last), one with none, ids -1 and 9, a row with both ids
    bad, a row [1, 1]"""
    import torch
    ff, m, n_used = 512, 40, 2
    blk = block(L, pkg, nso, FORMATS[0], ff)
    rng = np.random.default_rng(40 + lone)
    a = rng.standard_normal((m, D)).astype(np.float32)
    ids = np.array([[1, 2] if rng.integers(2) else [2, 1] for _ in range(m)], np.int32)
    ids[5] = [lone, 1]
    ids[7] = [-1, 2]
    ids[9] = [1, 9]
    ids[11] = [-1, 9]
    ids[13] = [1, 1]
    assert np.sum(ids == lone) == 1 and np.sum(ids == 3 - lone) == 0
    wts = rng.uniform(0.2, 0.8, (m, n_used)).astype(np.float32)
    dA = padded(a, D + 8, np.nan, np.float32)
    dI, dW = padded(ids, n_used + 1, -77, np.int32), padded(wts, n_used + 3, np.nan, np.float32)
    ref = reference(nso, a, ids, wts, blk)
    s0 = stats(L)
    out, pad = run(L, pkg, dA, dI, dW, m, n_used, blk, ldo=D + 5)
    s1 = stats(L)
    assert s1[3] - s0[3] == 1 and s1[1] == s0[1]
    assert np.all(pad == SENTINEL)
    assert np.all(out[11] == 0.0) and not np.any(np.signbit(out[11]))      # every id of the row is bad: exactly 0.0f
    worst = 0.0
    for t in range(m):
        if t == 11:
            continue
        assert np.any(ref[t] != 0.0)
        e = nso.rel_l2(out[t:t + 1], ref[t:t + 1])
        worst = max(worst, e)
        assert e < BAR, (t, ids[t].tolist(), e)
    print("moe_ffn grouped, engineered ids (lone expert %d): worst row %.3e" % (lone, worst))


def test_null_weights_mean_one(L, pkg, nso):
    ff, m, n_used = 512, 40, 2
    blk = block(L, pkg, nso, FORMATS[0], ff)
    a, dA, dI, _, ids, _ = inputs(L, pkg, m, n_used, 77)
    ref = reference(nso, a, ids, np.ones((m, n_used), np.float32), blk)
    s0 = stats(L)
    out, _ = run(L, pkg, dA, dI, None, m, n_used, blk)
    assert stats(L)[3] - s0[3] == 1
    assert nso.rel_l2(out, ref) < BAR


def test_two_runs_of_one_call_are_bit_equal(L, pkg, nso):
    ff, m, n_used = 512, 40, 2
    blk = block(L, pkg, nso, FORMATS[0], ff)
    a, dA, dI, dW, _, _ = inputs(L, pkg, m, n_used, 78)
    s0 = stats(L)
    first, _ = run(L, pkg, dA, dI, dW, m, n_used, blk)
    second, _ = run(L, pkg, dA, dI, dW, m, n_used, blk)
    # ... and so are the same rows at a stride that rules out the gather's 16-byte loads, written at a stride that rules out 16-byte stores
    third, _ = run(L, pkg, padded(a, D + 3, np.nan, np.float32), dI, dW, m, n_used, blk, ldo=D + 1)
    assert stats(L)[3] - s0[3] == 3
    assert np.array_equal(first.view(np.uint32), second.view(np.uint32))
    assert np.array_equal(first.view(np.uint32), third.view(np.uint32))


@pytest.mark.parametrize("case", ["ff528", "fp8", "mixed_formats", "key_negative", "m31"])
def test_the_composition_serves_what_the_grouped_pass_does_not(L, pkg, nso, case):
    ff, n_used = (528 if case == "ff528" else 512), 2
    m = 31 if case == "m31" else 40
    if case == "fp8":
        blk = block(L, pkg, nso, ("F8_E4M3", "F32", False, 32, "CORE_AVX512F"), ff)
    elif case == "mixed_formats":   # S4 gate, S8 up
        blk = block(L, pkg, nso, FORMATS[0], ff, fmt_up=FORMATS[2])
    else:
        blk = block(L, pkg, nso, FORMATS[0], ff)
    if case == "key_negative":
        assert L.ns_hip_set_tuning(KEY, -1) == 0
    a, dA, dI, dW, ids, wts = inputs(L, pkg, m, n_used, len(case))
    ref = reference(nso, a, ids, wts, blk)
    s0 = stats(L)
    out, pad = run(L, pkg, dA, dI, dW, m, n_used, blk, ldo=D + 5)
    s1 = stats(L)
    assert s1[1] - s0[1] == 1 and s1[3] == s0[3] and s1[0] == s0[0]
    assert np.all(pad == SENTINEL)
    assert nso.rel_l2(out, ref) < BAR


def test_a_captured_call_stays_on_the_composition_and_follows_new_ids(L, pkg, nso):
    import torch
    ff, m, n_used = 512, 40, 2
    blk = block(L, pkg, nso, FORMATS[0], ff)
    _, gg, _, gu, _, gd = blk
    rng = np.random.default_rng(21)
    a = rng.standard_normal((m, D)).astype(np.float32)
    dA = torch.from_numpy(a).cuda()
    lg1 = rng.standard_normal((m, N_AS)).astype(np.float32)
    lg2 = np.ascontiguousarray(lg1[:, ::-1])
    dL = torch.from_numpy(lg1).cuda()
    dI = torch.zeros((m, n_used), dtype=torch.int32, device="cuda")
    dW = torch.zeros((m, n_used), dtype=torch.float32, device="cuda")
    out = torch.zeros((m, D), device="cuda")
    pkg.check(L.ns_hip_moe_route(dL.data_ptr(), N_AS, m, N_AS, n_used, dI.data_ptr(), n_used, dW.data_ptr(), n_used, None, stream()))
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    s0 = stats(L)
    with torch.cuda.graph(gr):
        s = stream()
        pkg.check(L.ns_hip_moe_route(dL.data_ptr(), N_AS, m, N_AS, n_used, dI.data_ptr(), n_used, dW.data_ptr(), n_used, None, s))
        pkg.check(L.ns_hip_moe_ffn_silu(dA.data_ptr(), D, m, dI.data_ptr(), n_used, dW.data_ptr(), n_used, n_used, gg, gu, gd,
                                        out.data_ptr(), D, s))
    s1 = stats(L)
    assert s1[1] - s0[1] == 1 and s1[3] == s0[3]
    results = []
    for lg in (lg1, lg2):
        dL.copy_(torch.from_numpy(lg))
        gr.replay()
        torch.cuda.synchronize()
        ids, wts = dI.cpu().numpy(), dW.cpu().numpy()
        results.append(out.cpu().numpy())
        assert nso.rel_l2(results[-1], reference(nso, a, ids, wts, blk)) < BAR
    assert not np.array_equal(results[0], results[1])


def test_the_tuning_key_moves_the_threshold(L, pkg, nso):
    ff, m, n_used = 512, 12, 2
    blk = block(L, pkg, nso, FORMATS[0], ff)
    a, dA, dI, dW, ids, wts = inputs(L, pkg, m, n_used, 12)
    ref = reference(nso, a, ids, wts, blk)
    s0 = stats(L)
    run(L, pkg, dA, dI, dW, m, n_used, blk)
    s1 = stats(L)
    assert s1[1] - s0[1] == 1 and s1[3] == s0[3]          # 12 rows at the default: the composition
    assert L.ns_hip_set_tuning(KEY, 10) == 0
    out, _ = run(L, pkg, dA, dI, dW, m, n_used, blk)
    s2 = stats(L)
    assert s2[3] - s1[3] == 1 and s2[1] == s1[1]
    assert nso.rel_l2(out, ref) < BAR

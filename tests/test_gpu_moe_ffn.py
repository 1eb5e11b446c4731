"""ns_hip_moe_ffn_silu (csrc/ns_moe.cpp, gemv_kernel XV = 4): out[t] = sum_i w[t][i] * down_e(silu(gate_e(a_t)) * up_e(a_t)), e = ids[t][i] —
n_used x { ne_mul_id_ffn_silu ; mul(weights) ; add } of the reference (llama.cpp:641-679) — against the oracle's fp64 products per row
and against the three-call ns_hip_mul_mat_id composition on the same inputs; which path served a call is read from
ns_hip_moe_ffn_stats."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_moe import FORMATS, _group

pytestmark = pytest.mark.gpu

N_AS, D = 4, 256
BAR = 2e-3          # the bar test_ffn_id_composition_in_a_graph_and_bad_ids holds for this composition
_BLOCKS = {}


@pytest.fixture(autouse=True)
def default_tuning(L):
    L.ns_hip_set_tuning(b"moe_ffn_fused", -1)
    L.ns_hip_set_tuning(b"moe_gemv_rows", 0)
    yield
    L.ns_hip_set_tuning(b"moe_ffn_fused", -1)


def block(L, pkg, nso, fmt, ff, fmt_up=None):
    """gate / up / down expert groups of one format (cached for the module): (blobs, group handle) x 3"""
    key = (fmt, ff, fmt_up)
    if key not in _BLOCKS:
        rng = np.random.default_rng(1000 + len(_BLOCKS))
        bg, wg, gg = _group(L, pkg, nso, rng, N_AS, ff, D, *fmt)
        bu, wu, gu = _group(L, pkg, nso, rng, N_AS, ff, D, *(fmt_up or fmt))
        bd, wd, gd = _group(L, pkg, nso, rng, N_AS, D, ff, *fmt)
        _BLOCKS[key] = (bg, gg, bu, gu, bd, gd, (wg, wu, wd))
    return _BLOCKS[key][:6]


def stats(L):
    out = (C.c_uint64 * 4)()
    L.ns_hip_moe_ffn_stats(out)
    return [int(v) for v in out]


def stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def route(L, pkg, m, n_used, rng):
    """ids and weights as ns_hip_moe_route leaves them (device tensors + host copies)"""
    import torch
    logits = rng.standard_normal((m, N_AS)).astype(np.float32)
    dL = torch.from_numpy(logits).cuda()
    dI = torch.zeros((m, n_used), dtype=torch.int32, device="cuda")
    dW = torch.zeros((m, n_used), dtype=torch.float32, device="cuda")
    pkg.check(L.ns_hip_moe_route(dL.data_ptr(), N_AS, m, N_AS, n_used, dI.data_ptr(), n_used, dW.data_ptr(), n_used, None, stream()))
    torch.cuda.synchronize()
    return dI, dW, dI.cpu().numpy(), dW.cpu().numpy()


def expert_out(nso, a_row, bg, bu, bd, e):
    gate = nso.gemm_f64(a_row, bg[e])
    up = nso.gemm_f64(a_row, bu[e])
    h = (gate / (1 + np.exp(-gate)) * up).astype(np.float32)
    return nso.gemm_f64(h, bd[e])[0]


def reference(nso, a, ids, wts, blk):
    bg, _, bu, _, bd, _ = blk
    m, n_used = ids.shape
    out = np.zeros((m, D), np.float64)
    for t in range(m):
        for i in range(n_used):
            e = int(ids[t, i])
            if 0 <= e < N_AS:
                out[t] += float(wts[t, i]) * expert_out(nso, a[t:t + 1], bg, bu, bd, e)
    return out


def fused(L, pkg, dA, dI, dW, m, n_used, blk, ff, ldo=D):
    import torch
    _, gg, _, gu, _, gd = blk
    out = torch.full((m, ldo), 7.0, device="cuda")
    pkg.check(L.ns_hip_moe_ffn_silu(dA.data_ptr(), D, m, dI.data_ptr(), dI.shape[1], dW.data_ptr() if dW is not None else None,
                                    dW.shape[1] if dW is not None else 0, n_used, gg, gu, gd, out.data_ptr(), ldo, stream()))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def three_calls(L, pkg, dA, dI, dW, m, n_used, blk, ff):
    """the composition as a caller writes it today: three ns_hip_mul_mat_id calls per selection, weighting and sum by the caller"""
    import torch
    _, gg, _, gu, _, gd = blk
    t1 = torch.zeros((m, ff), device="cuda")
    t2 = torch.zeros((m, ff), device="cuda")
    t3 = torch.zeros((m, D), device="cuda")
    out = torch.zeros((m, D), device="cuda")
    s = stream()
    for i in range(n_used):
        pkg.check(L.ns_hip_mul_mat_id(dA.data_ptr(), dI.data_ptr(), dI.shape[1], i, gg, t1.data_ptr(), m, D, ff, pkg.EPI_SILU, None, 0, s))
        pkg.check(L.ns_hip_mul_mat_id(dA.data_ptr(), dI.data_ptr(), dI.shape[1], i, gu, t2.data_ptr(), m, D, ff, pkg.EPI_MUL, t1.data_ptr(), ff, s))
        pkg.check(L.ns_hip_mul_mat_id(t2.data_ptr(), dI.data_ptr(), dI.shape[1], i, gd, t3.data_ptr(), m, ff, D, pkg.EPI_NONE, None, 0, s))
        out += t3 * (dW[:, i:i + 1] if dW is not None else 1.0)
    torch.cuda.synchronize()
    return out.cpu().numpy()


SHAPES = [(512, m, k) for m in (1, 3, 8) for k in (1, 2)] + [(528, 1, 2), (528, 3, 2)]  # 528: 33 tiles; down's K is not a whole k-step


@pytest.mark.parametrize("ff,m,n_used", SHAPES)
@pytest.mark.parametrize("fmt", FORMATS, ids=[f[0] + "_" + f[1] for f in FORMATS])
def test_fused_block_against_fp64_and_the_three_call_composition(L, pkg, nso, fmt, ff, m, n_used):
    import torch
    blk = block(L, pkg, nso, fmt, ff)
    rng = np.random.default_rng(ff + 10 * m + n_used)
    a = rng.standard_normal((m, D)).astype(np.float32)
    dA = torch.from_numpy(a).cuda()
    dI, dW, ids, wts = route(L, pkg, m, n_used, rng)
    ref = reference(nso, a, ids, wts, blk)
    s0 = stats(L)
    out = fused(L, pkg, dA, dI, dW, m, n_used, blk, ff, ldo=D + 5)
    s1 = stats(L)
    assert np.all(out[:, D:] == 7.0)
    comp = three_calls(L, pkg, dA, dI, dW, m, n_used, blk, ff)
    e_fused, e_comp = nso.rel_l2(out[:, :D], ref), nso.rel_l2(comp, ref)
    print("moe_ffn %s ff=%d m=%d n_used=%d: fused %.3e composition %.3e" % (fmt[0] + "/" + fmt[1], ff, m, n_used, e_fused, e_comp))
    assert s1[0] - s0[0] == 1 and s1[1] == s0[1] and s1[2] - s0[2] == 1 + n_used and s1[3] == 0
    assert e_fused < BAR
    assert e_fused <= 1.5 * e_comp


def test_null_weights_mean_one(L, pkg, nso):
    import torch
    ff, m, n_used = 512, 3, 2
    blk = block(L, pkg, nso, FORMATS[0], ff)
    rng = np.random.default_rng(77)
    a = rng.standard_normal((m, D)).astype(np.float32)
    dA = torch.from_numpy(a).cuda()
    dI, _, ids, _ = route(L, pkg, m, n_used, rng)
    ref = reference(nso, a, ids, np.ones((m, n_used), np.float32), blk)
    s0 = stats(L)
    out = fused(L, pkg, dA, dI, None, m, n_used, blk, ff)
    assert stats(L)[0] - s0[0] == 1
    assert nso.rel_l2(out, ref) < BAR


@pytest.mark.parametrize("case", ["m9", "fp8", "tuning_off", "mixed_formats"])
def test_the_composition_serves_what_the_fused_launches_do_not(L, pkg, nso, case):
    import torch
    ff, n_used = 512, 2
    m = {"m9": 9, "fp8": 2, "tuning_off": 3, "mixed_formats": 3}[case]
    if case == "fp8":
        blk = block(L, pkg, nso, ("F8_E4M3", "F32", False, 32, "CORE_AVX512F"), ff)
    elif case == "mixed_formats":   # S4 gate, S8 up: served, not refused
        blk = block(L, pkg, nso, FORMATS[0], ff, fmt_up=FORMATS[2])
    else:
        blk = block(L, pkg, nso, FORMATS[0], ff)
    if case == "tuning_off":
        assert L.ns_hip_set_tuning(b"moe_ffn_fused", 0) == 0
    rng = np.random.default_rng(len(case))
    a = rng.standard_normal((m, D)).astype(np.float32)
    dA = torch.from_numpy(a).cuda()
    dI, dW, ids, wts = route(L, pkg, m, n_used, rng)
    ref = reference(nso, a, ids, wts, blk)
    s0 = stats(L)
    out = fused(L, pkg, dA, dI, dW, m, n_used, blk, ff)
    s1 = stats(L)
    assert s1[1] - s0[1] == 1 and s1[0] == s0[0]
    assert nso.rel_l2(out, ref) < BAR


@pytest.mark.parametrize("fused_on", [1, 0])
def test_out_of_range_ids_contribute_zero(L, pkg, nso, fused_on):
    import torch
    ff, m, n_used = 512, 4, 2
    blk = block(L, pkg, nso, FORMATS[0], ff)
    L.ns_hip_set_tuning(b"moe_ffn_fused", fused_on)
    rng = np.random.default_rng(9)
    a = rng.standard_normal((m, D)).astype(np.float32)
    dA = torch.from_numpy(a).cuda()
    ids = np.array([[0, 9], [-1, 2], [9, -1], [1, 3]], np.int32)
    wts = rng.uniform(0.2, 0.8, (m, n_used)).astype(np.float32)
    dI, dW = torch.from_numpy(ids).cuda(), torch.from_numpy(wts).cuda()
    out = fused(L, pkg, dA, dI, dW, m, n_used, blk, ff)
    assert np.all(out[2] == 0.0)                     # every id of the row is bad: exactly zero
    assert nso.rel_l2(out, reference(nso, a, ids, wts, blk)) < BAR
    # rows 0 and 1 equal their good selection's contribution alone: a run with n_used = 1 on that selection
    for t, good in ((0, 0), (1, 1)):
        dI1 = torch.from_numpy(np.ascontiguousarray(ids[t:t + 1, good:good + 1])).cuda()
        dW1 = torch.from_numpy(np.ascontiguousarray(wts[t:t + 1, good:good + 1])).cuda()
        one = fused(L, pkg, dA[t:t + 1], dI1, dW1, 1, 1, blk, ff)
        # (0 + w x on one side, w x on the other: at most the rounding of the weight multiply apart)
        assert np.allclose(out[t], one[0], rtol=2.0 ** -22, atol=1e-30)
        assert np.any(out[t] != 0.0)


def test_router_and_block_in_one_graph_follow_new_logits(L, pkg, nso):
    import torch
    ff, m, n_used = 512, 4, 2
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
    gr = torch.cuda.CUDAGraph()
    s0 = stats(L)
    with torch.cuda.graph(gr):
        s = stream()
        pkg.check(L.ns_hip_moe_route(dL.data_ptr(), N_AS, m, N_AS, n_used, dI.data_ptr(), n_used, dW.data_ptr(), n_used, None, s))
        pkg.check(L.ns_hip_moe_ffn_silu(dA.data_ptr(), D, m, dI.data_ptr(), n_used, dW.data_ptr(), n_used, n_used, gg, gu, gd,
                                        out.data_ptr(), D, s))
    assert stats(L)[0] - s0[0] == 1
    results = []
    for lg in (lg1, lg2):
        dL.copy_(torch.from_numpy(lg))
        gr.replay()
        torch.cuda.synchronize()
        ids, wts = dI.cpu().numpy(), dW.cpu().numpy()
        results.append(out.cpu().numpy())
        assert nso.rel_l2(results[-1], reference(nso, a, ids, wts, blk)) < BAR
    assert not np.array_equal(results[0], results[1])

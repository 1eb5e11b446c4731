"""ns_hip_moe_route (csrc/ns_moe_router.hip): the router's tail soft_max -> top_k -> get_rows -> sum_rows -> div of the reference graph
(models/llama/llama.cpp:631-638) in one launch, against the reference's arithmetic restated in numpy operation by operation
(ne_compute_forward_soft_max_f32, ne_layers.c:8887-8954; table fill :745; sum_rows :5972; ne_vec_div_f32): x - max in fp32, rounded to
fp16, table_exp_f16 (built here from the C library's expf - the host libm the library used), double sum, float(1 / sum), fp32 multiply;
selected values summed in double in selection order, stored as float, fp32 divide.  Every step is an IEEE operation or a table lookup,
so ids, probabilities and weights are compared bit for bit."""
import ctypes as C
import ctypes.util

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_TABLE = []


def exp_table():
    """fp16(expf(fp32(code))) for all 65 536 fp16 codes, with the host's expf"""
    if not _TABLE:
        libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
        libm.expf.restype = C.c_float
        libm.expf.argtypes = [C.c_float]
        x = np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16).astype(np.float32)
        v = np.array([libm.expf(float(t)) for t in x], dtype=np.float32)
        with np.errstate(over="ignore", invalid="ignore"):
            _TABLE.append(v.astype(np.float16))
    return _TABLE[0]


def ref_route(logits, n_used):
    """(ids [m][n_used], weights [m][n_used] f32, probs [m][n_expert] f32, table values [m][n_expert] f32); ties: lower index first"""
    tab = exp_table()
    m, n = logits.shape
    ids = np.zeros((m, n_used), np.int32)
    wts = np.zeros((m, n_used), np.float32)
    probs = np.zeros((m, n), np.float32)
    vals = np.zeros((m, n), np.float32)
    for t in range(m):
        x = logits[t].astype(np.float32)
        mx = np.float32(x.max())
        with np.errstate(invalid="ignore", over="ignore"):
            h = (x - mx).astype(np.float32).astype(np.float16)
        val = tab[h.view(np.uint16)].astype(np.float32)
        val[np.isneginf(x)] = 0.0
        s = float(val.astype(np.float64).sum())      # <= 64 fp16 values: exact in double, any order
        inv = np.float32(1.0 / s)
        p = (val * inv).astype(np.float32)
        order = sorted(range(n), key=lambda e: (-float(p[e]), e))[:n_used]
        wsum = np.float64(0.0)
        for e in order:
            wsum += np.float64(p[e])
        wsf = np.float32(wsum)
        ids[t] = order
        wts[t] = (p[order] / wsf).astype(np.float32)
        probs[t], vals[t] = p, val
    return ids, wts, probs, vals


def unambiguous_logits(rng, m, n_expert):
    """a random permutation of -0.3 j + U(-0.05, 0.05) per row"""
    rows = []
    for _ in range(m):
        base = -0.3 * np.arange(n_expert) + rng.uniform(-0.05, 0.05, n_expert)
        rows.append(rng.permutation(base))
    return np.stack(rows).astype(np.float32)


def run_route(L, pkg, logits_pad, m, n_expert, n_used, ids_stride, w_stride, want_probs):
    import torch
    ld = logits_pad.shape[1]
    dL = torch.from_numpy(logits_pad).cuda()
    dI = torch.full((m, ids_stride), -77, dtype=torch.int32, device="cuda")
    dW = torch.full((m, w_stride), 7.0, dtype=torch.float32, device="cuda")
    dP = torch.full((m, ld), 7.0, dtype=torch.float32, device="cuda") if want_probs else None
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = L.ns_hip_moe_route(dL.data_ptr(), ld, m, n_expert, n_used, dI.data_ptr(), ids_stride, dW.data_ptr(), w_stride,
                            dP.data_ptr() if want_probs else None, st)
    torch.cuda.synchronize()
    return rc, dI.cpu().numpy(), dW.cpu().numpy(), (dP.cpu().numpy() if want_probs else None)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("want_probs", [False, True])
@pytest.mark.parametrize("m,n_expert,n_used,ld", [(1, 8, 2, 8), (5, 8, 1, 12), (3, 60, 8, 64), (70, 64, 4, 64)])
def test_route_is_bit_equal_to_the_reference_arithmetic(L, pkg, m, n_expert, n_used, ld, want_probs):
    rng = np.random.default_rng(m * 100 + n_expert + n_used)
    logits = unambiguous_logits(rng, m, n_expert)
    pad = np.full((m, ld), 3.0, np.float32)      # columns beyond n_expert are not the router's: larger than every logit on purpose
    pad[:, :n_expert] = logits
    ids, wts, probs, vals = ref_route(logits, n_used)
    top = -np.sort(-vals, axis=1)[:, :n_used + 1]
    assert np.all(top[:, :-1] > top[:, 1:]), "the inputs must make the reference's answer unambiguous"
    ids_stride, w_stride = n_used + 3, n_used + 1   # strides larger than the rows
    rc, gi, gw, gp = run_route(L, pkg, pad, m, n_expert, n_used, ids_stride, w_stride, want_probs)
    assert rc == 0, pkg.last_error()
    assert np.array_equal(gi[:, :n_used], ids)
    assert np.all(gi[:, n_used:] == -77) and np.all(gw[:, n_used:] == 7.0)
    assert np.array_equal(bits(gw[:, :n_used]), bits(wts))
    if want_probs:
        assert np.array_equal(bits(gp[:, :n_expert]), bits(probs))
        assert np.all(gp[:, n_expert:] == 7.0)


def test_ties_go_to_the_lower_expert_index(L, pkg):
    m, n_expert, n_used = 2, 8, 3
    logits = np.full((m, n_expert), 0.25, np.float32)
    logits[1, :] = -4.0
    ids, wts, probs, _ = ref_route(logits, n_used)
    rc, gi, gw, gp = run_route(L, pkg, logits, m, n_expert, n_used, n_used, n_used, True)
    assert rc == 0, pkg.last_error()
    assert np.array_equal(gi, np.tile(np.arange(n_used, dtype=np.int32), (m, 1)))
    assert np.array_equal(gi, ids)
    assert np.all(gw == gw[:, :1]) and np.array_equal(bits(gw), bits(wts)) and np.array_equal(bits(gp), bits(probs))


def test_minus_infinity_logits_get_probability_zero(L, pkg):
    rng = np.random.default_rng(11)
    m, n_expert, n_used = 3, 8, 2
    logits = unambiguous_logits(rng, m, n_expert)
    logits[0, [1, 5]] = -np.inf
    logits[1, :5] = -np.inf
    logits[2, 7] = -np.inf
    ids, wts, probs, _ = ref_route(logits, n_used)
    rc, gi, gw, gp = run_route(L, pkg, logits, m, n_expert, n_used, n_used, n_used, True)
    assert rc == 0, pkg.last_error()
    assert np.all(gp[np.isneginf(logits)] == 0.0)
    assert np.array_equal(gi, ids) and np.array_equal(bits(gw), bits(wts)) and np.array_equal(bits(gp), bits(probs))
    assert not np.any(np.isneginf(logits[np.arange(m)[:, None], gi]))


def test_rows_outside_the_contract_still_get_distinct_ids_in_range(L, pkg):
    m, n_expert, n_used = 3, 6, 4
    logits = np.zeros((m, 8), np.float32)
    logits[0, :] = -np.inf
    logits[1, 2] = np.nan
    logits[2, :] = np.nan
    rc, gi, gw, _ = run_route(L, pkg, logits, m, n_expert, n_used, n_used, n_used, False)
    assert rc == 0, pkg.last_error()
    for t in range(m):
        assert len(set(gi[t].tolist())) == n_used and gi[t].min() >= 0 and gi[t].max() < n_expert


@pytest.mark.parametrize("n_expert,n_used", [(65, 2), (16, 9), (3, 4), (8, 0)])
def test_route_refuses_what_is_outside_its_envelope(L, pkg, n_expert, n_used):
    logits = np.zeros((2, 72), np.float32)
    rc, gi, gw, gp = run_route(L, pkg, logits, 2, n_expert, n_used, 12, 12, True)
    assert rc == -1 and "moe_route" in pkg.last_error()
    assert np.all(gi == -77) and np.all(gw == 7.0) and np.all(gp == 7.0)
    L.ns_hip_reset_error()


def test_a_replayed_graph_follows_the_logits(L, pkg):
    import torch
    rng = np.random.default_rng(5)
    m, n_expert, n_used = 4, 8, 2
    l1, l2 = unambiguous_logits(rng, m, n_expert), unambiguous_logits(rng, m, n_expert)
    assert run_route(L, pkg, l1, m, n_expert, n_used, n_used, n_used, False)[0] == 0    # (the exponential table exists before the capture)
    dL = torch.from_numpy(l1).cuda()
    dI = torch.zeros((m, n_used), dtype=torch.int32, device="cuda")
    dW = torch.zeros((m, n_used), dtype=torch.float32, device="cuda")
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        pkg.check(L.ns_hip_moe_route(dL.data_ptr(), n_expert, m, n_expert, n_used, dI.data_ptr(), n_used, dW.data_ptr(), n_used, None, s))
    for lg in (l1, l2):
        dL.copy_(torch.from_numpy(lg))
        gr.replay()
        torch.cuda.synchronize()
        ids, wts, _, _ = ref_route(lg, n_used)
        assert np.array_equal(dI.cpu().numpy(), ids) and np.array_equal(bits(dW.cpu().numpy()), bits(wts))
    assert not np.array_equal(ref_route(l1, n_used)[0], ref_route(l2, n_used)[0])

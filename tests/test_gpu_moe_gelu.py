"""The Grok form of the MoE block (models/grok/grok.cpp:292-343): ns_hip_moe_ffn_gelu - gelu(gate) * up experts, the tanh-form GeLU of
kernel_ref.h:1570-1572, on all three paths of the block entry (fused decode launches, composition, grouped pass) against the oracle's fp64
products - and ns_hip_moe_route_f, whose NS_MOE_ROUTE_RAW_WEIGHTS flag leaves the selected soft_max values themselves as the weights
(grok.cpp:293-299: no sum_rows, no div)."""
import numpy as np
import pytest

from test_gpu_moe import FORMATS
from test_gpu_moe_ffn import BAR, D, N_AS, block, stats, stream
from test_gpu_moe_ffn_grouped import act_gelu, act_silu, inputs, reference, run
from test_gpu_moe_route import bits, unambiguous_logits

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def default_tuning(L):
    for key, v in ((b"moe_ffn_fused", -1), (b"moe_gemv_rows", 0), (b"moe_grouped_rows", 0), (b"moe_ffn_grouped_rows", 0)):
        L.ns_hip_set_tuning(key, v)
    yield


# (m, n_used, counter that serves the call: [0] fused launches, [1] composition, [3] grouped pass)
CASES = [(m, k, 0) for m in (1, 3, 8) for k in (1, 2)] + [(9, 2, 1), (40, 2, 3)]


@pytest.mark.parametrize("m,n_used,served", CASES)
def test_gelu_block_against_fp64_on_every_path(L, pkg, nso, m, n_used, served):
    ff = 512
    blk = block(L, pkg, nso, FORMATS[0], ff)
    a, dA, dI, dW, ids, wts = inputs(L, pkg, m, n_used, 500 + 10 * m + n_used)
    ref = reference(nso, a, ids, wts, blk, act_gelu)
    s0 = stats(L)
    out, pad = run(L, pkg, dA, dI, dW, m, n_used, blk, ldo=D + 5, entry=L.ns_hip_moe_ffn_gelu)
    s1 = stats(L)
    d = [s1[i] - s0[i] for i in range(4)]
    assert d[served] == 1 and all(d[i] == 0 for i in (0, 1, 3) if i != served)
    assert d[2] == (1 + n_used if served == 0 else 0)
    assert np.all(pad == 7.0)
    e = nso.rel_l2(out, ref)
    print("moe_ffn_gelu m=%d n_used=%d path [%d]: %.3e" % (m, n_used, served, e))
    assert e < BAR
    # the activation is not ignored: the SiLU entry on the same inputs gives something else, and that is the SiLU reference
    silu, _ = run(L, pkg, dA, dI, dW, m, n_used, blk, ldo=D + 5)
    assert nso.rel_l2(silu, reference(nso, a, ids, wts, blk, act_silu)) < BAR
    assert nso.rel_l2(silu, ref) > 10 * BAR and not np.array_equal(silu, out)


@pytest.mark.parametrize("m", [3, 9, 40])
def test_gelu_out_of_range_ids_contribute_zero(L, pkg, nso, m):
    import torch
    ff, n_used = 512, 2
    blk = block(L, pkg, nso, FORMATS[0], ff)
    rng = np.random.default_rng(m)
    a = rng.standard_normal((m, D)).astype(np.float32)
    ids = np.stack([rng.permutation(N_AS)[:n_used] for _ in range(m)]).astype(np.int32)
    ids[0] = [0, 9]
    ids[1] = [-1, 2]
    ids[2] = [9, -1]
    wts = rng.uniform(0.2, 0.8, (m, n_used)).astype(np.float32)
    out, _ = run(L, pkg, torch.from_numpy(a).cuda(), torch.from_numpy(ids).cuda(), torch.from_numpy(wts).cuda(), m, n_used, blk,
                 entry=L.ns_hip_moe_ffn_gelu)
    assert np.all(out[2] == 0.0)
    assert nso.rel_l2(out, reference(nso, a, ids, wts, blk, act_gelu)) < BAR


def route_f(L, dL, m, n_expert, n_used, ids_stride, w_stride, flags, want_probs=True):
    import torch
    ld = dL.shape[1]
    dI = torch.full((m, ids_stride), -77, dtype=torch.int32, device="cuda")
    dW = torch.full((m, w_stride), 7.0, dtype=torch.float32, device="cuda")
    dP = torch.full((m, ld), 7.0, dtype=torch.float32, device="cuda") if want_probs else None
    args = [dL.data_ptr(), ld, m, n_expert, n_used, dI.data_ptr(), ids_stride, dW.data_ptr(), w_stride, dP.data_ptr() if want_probs else None]
    rc = L.ns_hip_moe_route(*args, stream()) if flags is None else L.ns_hip_moe_route_f(*args, flags, stream())
    torch.cuda.synchronize()
    return rc, dI.cpu().numpy(), dW.cpu().numpy(), (dP.cpu().numpy() if want_probs else None)


@pytest.mark.parametrize("m,n_expert,n_used,ld", [(1, 8, 2, 8), (5, 8, 1, 12), (3, 60, 8, 64), (70, 64, 4, 64)])
def test_route_f_flag_0_is_the_old_entry_and_the_raw_flag_leaves_the_probabilities(L, pkg, m, n_expert, n_used, ld):
    import torch
    rng = np.random.default_rng(m * 100 + n_expert + n_used)
    pad = np.full((m, ld), 3.0, np.float32)
    pad[:, :n_expert] = unambiguous_logits(rng, m, n_expert)
    dL = torch.from_numpy(pad).cuda()
    ids_stride, w_stride = n_used + 3, n_used + 1
    rc, oi, ow, op = route_f(L, dL, m, n_expert, n_used, ids_stride, w_stride, None)
    assert rc == 0, pkg.last_error()
    rc, zi, zw, zp = route_f(L, dL, m, n_expert, n_used, ids_stride, w_stride, 0)
    assert rc == 0, pkg.last_error()
    assert np.array_equal(zi, oi) and np.array_equal(bits(zw), bits(ow)) and np.array_equal(bits(zp), bits(op))
    rc, ri, rw, rp = route_f(L, dL, m, n_expert, n_used, ids_stride, w_stride, pkg.MOE_ROUTE_RAW_WEIGHTS)
    assert rc == 0, pkg.last_error()
    assert np.array_equal(ri, oi) and np.array_equal(bits(rp), bits(op))
    picked = np.take_along_axis(op, oi[:, :n_used].astype(np.int64), axis=1)
    assert np.array_equal(bits(rw[:, :n_used]), bits(picked))
    assert np.all(rw[:, n_used:] == 7.0) and np.all(ri[:, n_used:] == -77)
    assert not np.array_equal(bits(rw[:, :n_used]), bits(ow[:, :n_used]))     # (un-normalised: really another answer)
    # without the probabilities as an output the weights are the same
    rc, _, rw2, _ = route_f(L, dL, m, n_expert, n_used, ids_stride, w_stride, pkg.MOE_ROUTE_RAW_WEIGHTS, want_probs=False)
    assert rc == 0 and np.array_equal(bits(rw2), bits(rw))


def test_route_f_unknown_bits_write_nothing(L, pkg):
    import torch
    dL = torch.zeros((2, 8), device="cuda")
    rc, gi, gw, gp = route_f(L, dL, 2, 8, 2, 4, 4, 2)
    assert rc == -1 and "moe_route" in pkg.last_error()
    assert np.all(gi == -77) and np.all(gw == 7.0) and np.all(gp == 7.0)
    L.ns_hip_reset_error()


def test_a_replayed_graph_with_the_raw_flag_follows_the_logits(L, pkg):
    import torch
    rng = np.random.default_rng(5)
    m, n_expert, n_used = 4, 8, 2
    l1, l2 = unambiguous_logits(rng, m, n_expert), unambiguous_logits(rng, m, n_expert)
    dL = torch.from_numpy(l1).cuda()
    eager = {}
    for name, lg in (("l1", l1), ("l2", l2)):      # (also: the exponential table exists before the capture)
        rc, gi, gw, _ = route_f(L, torch.from_numpy(lg).cuda(), m, n_expert, n_used, n_used, n_used, pkg.MOE_ROUTE_RAW_WEIGHTS)
        assert rc == 0, pkg.last_error()
        eager[name] = (gi, gw)
    dI = torch.zeros((m, n_used), dtype=torch.int32, device="cuda")
    dW = torch.zeros((m, n_used), dtype=torch.float32, device="cuda")
    dP = torch.zeros((m, n_expert), dtype=torch.float32, device="cuda")
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        pkg.check(L.ns_hip_moe_route_f(dL.data_ptr(), n_expert, m, n_expert, n_used, dI.data_ptr(), n_used, dW.data_ptr(), n_used, dP.data_ptr(),
                                       pkg.MOE_ROUTE_RAW_WEIGHTS, stream()))
    for name, lg in (("l1", l1), ("l2", l2)):
        dL.copy_(torch.from_numpy(lg))
        gr.replay()
        torch.cuda.synchronize()
        gi, gw, gp = dI.cpu().numpy(), dW.cpu().numpy(), dP.cpu().numpy()
        assert np.array_equal(gi, eager[name][0]) and np.array_equal(bits(gw), bits(eager[name][1]))
        assert np.array_equal(bits(gw), bits(np.take_along_axis(gp, gi.astype(np.int64), axis=1)))
    assert not np.array_equal(eager["l1"][0], eager["l2"][0])

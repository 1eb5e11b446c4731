"""The device-grouped pass of ns_hip_moe_ffn_silu / _gelu (csrc/ns_moe.cpp ffn_device_grouped, csrc/ns_moe_group.hip, gemv_kernel XV = 6):
up to "moe_ffn_device_rows" rows (opt-in, default 0) a call - captured or not - sorts its (row, selection) pairs by expert ON THE DEVICE,
gathers their rows once, streams every expert once per chunk of its pairs (one fused gate / up launch, one down launch of the decode
kernel) and combines the products with the routing weights: five launches, nothing read on the host.  Checked against the oracle's fp64
products, against the composition on the same inputs (the same entry with the key at 0), and - the layout the sort leaves on the device -
against the rule of moe_chunk_plan as tests/test_moe_device_plan.py restates it (and pins to the C++ function on the CPU).  Which server
took a call is read from ns_hip_moe_ffn_stats_ex ([4] calls the pass served, [5] its launches, [6] calls it was tried for and handed on).
Both keys are put back to 0 behind every test: other files assert the counters of the default paths."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_moe import FORMATS
from test_gpu_moe_ffn import BAR, D, N_AS, block, reference, route, stream
from test_gpu_moe_ffn_grouped import act_gelu, reference as reference_act
from test_moe_device_plan import restate

pytestmark = pytest.mark.gpu

KEY, CHUNK = b"moe_ffn_device_rows", b"moe_ffn_chunk_rows"
SENTINEL = 7.0
FF = 512


@pytest.fixture(autouse=True)
def tuning(L):
    for key, v in ((b"moe_ffn_fused", -1), (b"moe_gemv_rows", 0), (b"moe_grouped_rows", 0), (b"moe_ffn_grouped_rows", 0), (KEY, 0), (CHUNK, 0)):
        assert L.ns_hip_set_tuning(key, v) == 0, key
    yield
    for key in (KEY, CHUNK):
        L.ns_hip_set_tuning(key, 0)


def stats_ex(L):
    out = (C.c_uint64 * 7)()
    L.ns_hip_moe_ffn_stats_ex(out, 7)
    return [int(v) for v in out]


def moved(s0, s1):
    return [b - a for a, b in zip(s0, s1)]


def served_by_the_pass(d):
    return d[4] == 1 and d[5] == 5 and d[0] == d[1] == d[3] == d[6] == 0


def call(L, pkg, dA, dI, dW, m, n_used, blk, ldo=D, entry=None, out=None):
    """one call of a block entry; (out [m][D], the padding columns)"""
    import torch
    _, gg, _, gu, _, gd = blk
    if out is None:
        out = torch.full((m, ldo), SENTINEL, device="cuda")
    fn = entry or L.ns_hip_moe_ffn_silu
    pkg.check(fn(dA.data_ptr(), dA.shape[1], m, dI.data_ptr(), dI.shape[1], dW.data_ptr(), dW.shape[1], n_used, gg, gu, gd, out.data_ptr(), ldo, stream()))
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    return o[:, :D], o[:, D:]


def on_device(a, ids, wts):
    import torch
    return torch.from_numpy(a).cuda(), torch.from_numpy(np.ascontiguousarray(ids, np.int32)).cuda(), torch.from_numpy(np.ascontiguousarray(wts, np.float32)).cuda()


# ---- numerics --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", ["silu", "gelu"])
@pytest.mark.parametrize("m,n_used", [(m, k) for m in (9, 16, 17, 31) for k in (1, 2)])
@pytest.mark.parametrize("fmt", FORMATS, ids=[f[0] + "_" + f[1] for f in FORMATS])
def test_device_grouped_pass_against_fp64_and_the_composition(L, pkg, nso, fmt, m, n_used, act):
    import torch
    blk = block(L, pkg, nso, fmt, FF)
    rng = np.random.default_rng(7000 + 10 * m + n_used)
    a = rng.standard_normal((m, D)).astype(np.float32)
    dA = torch.from_numpy(a).cuda()
    dI, dW, ids, wts = route(L, pkg, m, n_used, rng)
    ref = reference(nso, a, ids, wts, blk) if act == "silu" else reference_act(nso, a, ids, wts, blk, act_gelu)
    entry = L.ns_hip_moe_ffn_silu if act == "silu" else L.ns_hip_moe_ffn_gelu
    assert L.ns_hip_set_tuning(KEY, 31) == 0, "the key is unknown: the device-grouped pass is missing"
    s0 = stats_ex(L)
    out, pad = call(L, pkg, dA, dI, dW, m, n_used, blk, ldo=D + 5, entry=entry)
    s1 = stats_ex(L)
    assert L.ns_hip_set_tuning(KEY, 0) == 0
    comp, _ = call(L, pkg, dA, dI, dW, m, n_used, blk, ldo=D + 5, entry=entry)
    s2 = stats_ex(L)
    e_dev, e_comp = nso.rel_l2(out, ref), nso.rel_l2(comp, ref)
    print("moe_ffn device-grouped %s %s m=%d n_used=%d: device %.3e composition %.3e" % (fmt[0] + "/" + fmt[1], act, m, n_used, e_dev, e_comp))
    assert served_by_the_pass(moved(s0, s1)), moved(s0, s1)
    assert moved(s1, s2)[1] == 1 and moved(s1, s2)[4] == 0 and moved(s1, s2)[6] == 0       # key at 0: the composition, the pass not even tried
    assert np.all(pad == SENTINEL)
    assert e_dev < BAR
    assert e_dev <= 1.5 * e_comp


# ---- chunk boundaries ------------------------------------------------------------------------------------------------------------------------
def column(counts, rng):
    col = np.asarray([e for e, c in enumerate(counts) for _ in range(c)], np.int32)
    rng.shuffle(col)
    return col.reshape(-1, 1)


def boundary_tables():
    rng = np.random.default_rng(5)
    return {"groups_of_3_4_16_17": column([3, 4, 16, 17], rng),            # 40 rows: served with the key at 64
            "an_expert_with_none": column([5, 0, 9, 3], rng),
            "all_on_one_expert": np.full((9, 2), 2, np.int32)}              # 18 pairs of expert 2, every row names it twice


@pytest.mark.parametrize("cap", [1, 3, 16])
@pytest.mark.parametrize("table", sorted(boundary_tables()))
def test_chunk_boundaries(L, pkg, nso, table, cap):
    ids = boundary_tables()[table]
    m, n_used = ids.shape
    blk = block(L, pkg, nso, FORMATS[0], FF)
    rng = np.random.default_rng(len(table) + cap)
    a = rng.standard_normal((m, D)).astype(np.float32)
    wts = rng.uniform(0.2, 0.8, (m, n_used)).astype(np.float32)
    dA, dI, dW = on_device(a, ids, wts)
    assert L.ns_hip_set_tuning(KEY, 64) == 0 and L.ns_hip_set_tuning(CHUNK, cap) == 0
    s0 = stats_ex(L)
    out, pad = call(L, pkg, dA, dI, dW, m, n_used, blk, ldo=D + 5)
    assert served_by_the_pass(moved(s0, stats_ex(L)))
    assert np.all(pad == SENTINEL)
    assert nso.rel_l2(out, reference_act(nso, a, ids, wts, blk)) < BAR
    # the chunk size does not change a row's arithmetic: the same bits as with the chunks sized by LDS fit
    assert L.ns_hip_set_tuning(CHUNK, 0) == 0
    fit, _ = call(L, pkg, dA, dI, dW, m, n_used, blk, ldo=D + 5)
    assert np.array_equal(out, fit)


# ---- the layout the sort leaves on the device ------------------------------------------------------------------------------------------------
def device_layout(L, pkg, ids, n_as, r_gu, r_dn, ids_stride=None):
    import torch
    m, n_used = ids.shape
    stride = ids_stride or n_used
    full = np.full((m, stride), 1 << 20, np.int32)
    full[:, :n_used] = ids
    dI = torch.from_numpy(full).cuda()
    P = m * n_used
    slots = [(P + min(n_as, P) * (r - 1)) // r for r in (r_gu, r_dn)]
    n = 2 * P + 2 + 3 * sum(slots)
    out = np.full(n + 4, -99, np.int32)
    got = L.ns_hip_moe_ffn_device_layout(dI.data_ptr(), stride, m, n_used, n_as, r_gu, r_dn, out.ctypes.data, n, stream())
    assert got == n, pkg.last_error()
    assert np.all(out[n:] == -99)
    lists, at = [], 2 * P
    for s in slots:
        count = int(out[at])
        assert 0 <= count <= s
        body = out[at + 1:at + 1 + 3 * s].reshape(s, 3)
        assert np.all(body[count:] == np.array([-1, 0, 0]))
        lists.append([tuple(int(x) for x in row) for row in body[:count]])
        at += 1 + 3 * s
    return [int(x) for x in out[:P]], [int(x) for x in out[P:2 * P]], lists


def test_the_device_layout_is_the_pure_functions(L, pkg):
    assert L.ns_hip_set_tuning(KEY, 31) == 0
    rng = np.random.default_rng(3)
    tables = [(np.stack([rng.permutation(4)[:2] for _ in range(12)]), 4, 2), (np.stack([rng.permutation(8)[:2] for _ in range(31)]), 8, 3),
              (rng.integers(-1, 6, (17, 3)), 5, 3), (np.full((9, 2), 2), 4, 2), (np.array([[1, 1], [0, 1], [1, 1], [3, 3]]), 4, 2),
              (np.array([[-1, 9], [9, -1]]), 4, 2), (column([3, 4, 16, 17], rng), 4, 1), (column([16, 17, 32, 1], rng), 4, 1),
              (np.array([[3]]), 4, 1), (np.stack([rng.permutation(64)[:2] for _ in range(512)]), 64, 2), (rng.integers(0, 3, (1024, 1)), 3, 1)]
    for ids, n_as, stride in tables:
        ids = np.asarray(ids, np.int64)
        for r_gu, r_dn in ((16, 7), (1, 2), (3, 16)):
            src_row, pos, lists = device_layout(L, pkg, ids, n_as, r_gu, r_dn, stride)
            for R, chunks in zip((r_gu, r_dn), lists):
                want = restate(ids, n_as, R)
                assert src_row == want["src_row"] and pos == want["pos"], (ids.shape, n_as, R)
                assert chunks == want["chunks"], (ids.shape, n_as, R)
    # what the entry refuses: too many pairs, a chunk size outside 1 .. 16, a short output
    import torch
    dI = torch.zeros((1025, 1), dtype=torch.int32, device="cuda")
    out = np.zeros(1 << 14, np.int32)
    assert L.ns_hip_moe_ffn_device_layout(dI.data_ptr(), 1, 1025, 1, 4, 4, 4, out.ctypes.data, len(out), stream()) == -1
    assert L.ns_hip_moe_ffn_device_layout(dI.data_ptr(), 1, 8, 1, 4, 17, 4, out.ctypes.data, len(out), stream()) == -1
    assert L.ns_hip_moe_ffn_device_layout(dI.data_ptr(), 1, 8, 1, 4, 4, 4, out.ctypes.data, 16, stream()) == -1
    L.ns_hip_reset_error()


# ---- bad ids ---------------------------------------------------------------------------------------------------------------------------------
def test_bad_ids_and_a_row_naming_one_expert_twice(L, pkg, nso):
    m, n_used = 10, 2
    blk = block(L, pkg, nso, FORMATS[0], FF)
    rng = np.random.default_rng(9)
    a = rng.standard_normal((m, D)).astype(np.float32)
    ids = np.stack([rng.permutation(N_AS)[:n_used] for _ in range(m)]).astype(np.int32)
    ids[0] = [0, N_AS]
    ids[1] = [-1, 2]
    ids[2] = [N_AS, -1]
    ids[3] = [1, 1]
    wts = rng.uniform(0.2, 0.8, (m, n_used)).astype(np.float32)
    dA, dI, dW = on_device(a, ids, wts)
    assert L.ns_hip_set_tuning(KEY, 31) == 0
    s0 = stats_ex(L)
    out, _ = call(L, pkg, dA, dI, dW, m, n_used, blk)
    assert served_by_the_pass(moved(s0, stats_ex(L)))
    assert np.all(out[2] == 0.0) and not np.any(np.signbit(out[2]))          # every id of the row is bad: exactly 0.0f
    ref = reference(nso, a, ids, wts, blk)
    assert nso.rel_l2(out, ref) < BAR
    assert nso.rel_l2(out[3:4], ref[3:4]) < BAR and np.any(out[3] != 0.0)     # the expert named twice counts twice
    # rows 0 and 1 are their good selection's contribution alone: the same call with the bad selection's weight changed gives the same bits
    wts2 = wts.copy()
    wts2[0, 1], wts2[1, 0] = 123.0, -55.0
    out2, _ = call(L, pkg, dA, dI, on_device(a, ids, wts2)[2], m, n_used, blk)
    assert np.array_equal(out, out2)


# ---- row independence ------------------------------------------------------------------------------------------------------------------------
def test_rows_do_not_depend_on_their_neighbours(L, pkg, nso):
    m, n_used = 23, 2
    blk = block(L, pkg, nso, FORMATS[1], FF)
    rng = np.random.default_rng(31)
    a = rng.standard_normal((m, D)).astype(np.float32)
    ids = np.stack([rng.permutation(N_AS)[:n_used] for _ in range(m)]).astype(np.int32)
    wts = rng.uniform(0.2, 0.8, (m, n_used)).astype(np.float32)
    assert L.ns_hip_set_tuning(KEY, 31) == 0 and L.ns_hip_set_tuning(CHUNK, 3) == 0
    s0 = stats_ex(L)
    out, _ = call(L, pkg, *on_device(a, ids, wts), m, n_used, blk)
    again, _ = call(L, pkg, *on_device(a, ids, wts), m, n_used, blk)
    perm = rng.permutation(m)
    shuffled, _ = call(L, pkg, *on_device(a[perm], ids[perm], wts[perm]), m, n_used, blk)
    assert moved(s0, stats_ex(L))[4] == 3 and moved(s0, stats_ex(L))[1] == 0
    assert np.array_equal(out, again)
    assert np.array_equal(shuffled, out[perm])
    assert nso.rel_l2(out, reference(nso, a, ids, wts, blk)) < BAR


# ---- capture ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,key", [(12, 31), (40, 64)])
def test_router_and_block_in_one_graph_follow_new_logits(L, pkg, nso, m, key):
    import torch
    n_used = 2
    blk = block(L, pkg, nso, FORMATS[0], FF)
    _, gg, _, gu, _, gd = blk
    rng = np.random.default_rng(21 + m)
    a = rng.standard_normal((m, D)).astype(np.float32)
    dA = torch.from_numpy(a).cuda()
    lg1 = rng.standard_normal((m, N_AS)).astype(np.float32)
    lg2 = np.ascontiguousarray(lg1[:, ::-1])
    dL = torch.from_numpy(lg1).cuda()
    dI = torch.zeros((m, n_used), dtype=torch.int32, device="cuda")
    dW = torch.zeros((m, n_used), dtype=torch.float32, device="cuda")
    out = torch.zeros((m, D), device="cuda")
    assert L.ns_hip_set_tuning(KEY, key) == 0
    # scratch and code objects before the capture, as a served call leaves them
    call(L, pkg, dA, dI, dW, m, n_used, blk)
    gr = torch.cuda.CUDAGraph()
    s0 = stats_ex(L)
    with torch.cuda.graph(gr):
        s = stream()
        pkg.check(L.ns_hip_moe_route(dL.data_ptr(), N_AS, m, N_AS, n_used, dI.data_ptr(), n_used, dW.data_ptr(), n_used, None, s))
        pkg.check(L.ns_hip_moe_ffn_silu(dA.data_ptr(), D, m, dI.data_ptr(), n_used, dW.data_ptr(), n_used, n_used, gg, gu, gd, out.data_ptr(), D, s))
    assert served_by_the_pass(moved(s0, stats_ex(L))), moved(s0, stats_ex(L))      # (m = 40: the composition's before this pass)
    results = []
    for lg in (lg1, lg2):
        dL.copy_(torch.from_numpy(lg))
        gr.replay()
        torch.cuda.synchronize()
        ids, wts = dI.cpu().numpy(), dW.cpu().numpy()
        results.append(out.cpu().numpy())
        assert nso.rel_l2(results[-1], reference(nso, a, ids, wts, blk)) < BAR
        eager, _ = call(L, pkg, dA, dI, dW, m, n_used, blk)                         # the same ids and weights, outside the graph
        assert np.array_equal(results[-1], eager)
    assert not np.array_equal(results[0], results[1])


# ---- what the pass hands on ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["ff_528", "fp8", "m_32"])
def test_the_pass_hands_on_what_it_does_not_serve(L, pkg, nso, case):
    import torch
    n_used = 2
    ff = 528 if case == "ff_528" else FF                                            # 528: the down launch's K is not whole k-steps
    m = 32 if case == "m_32" else 12
    blk = block(L, pkg, nso, ("F8_E4M3", "F32", False, 32, "CORE_AVX512F") if case == "fp8" else FORMATS[0], ff)
    rng = np.random.default_rng(len(case))
    a = rng.standard_normal((m, D)).astype(np.float32)
    dA = torch.from_numpy(a).cuda()
    dI, dW, ids, wts = route(L, pkg, m, n_used, rng)
    assert L.ns_hip_set_tuning(KEY, 31) == 0
    s0 = stats_ex(L)
    out, pad = call(L, pkg, dA, dI, dW, m, n_used, blk, ldo=D + 5)
    d = moved(s0, stats_ex(L))
    assert d[4] == 0 and d[5] == 0 and d[0] == 0
    if case == "m_32":
        assert d[3] == 1 and d[1] == 0 and d[6] == 0          # above the key: not tried, the grouped pass as before
    else:
        assert d[1] == 1 and d[3] == 0 and d[6] == 1          # tried, handed on, the composition serves
    assert np.all(pad == SENTINEL)
    assert nso.rel_l2(out, reference(nso, a, ids, wts, blk)) < BAR

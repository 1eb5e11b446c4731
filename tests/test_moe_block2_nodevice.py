"""Without a HIP device the MoE block's second pair of entries (ns_hip_moe_route_f, ns_hip_moe_ffn_gelu) refuse like every compute entry:
-1, "no HIP device" in the error text, nothing written - there is no CPU fallback.  ns_hip_moe_route_f refuses an unknown flag bit with or
without a device.  With a device the rest of this file is a no-op (the GPU tests cover the entries)."""
import ctypes as C

import numpy as np

vp = lambda x: x.ctypes.data_as(C.c_void_p)


def route_buffers(m=2, n_expert=8, n_used=2):
    return (np.zeros((m, n_expert), np.float32), np.full((m, n_used), -77, np.int32), np.full((m, n_used), 7.0, np.float32),
            np.full((m, n_expert), 7.0, np.float32))


def test_the_new_entries_refuse_without_a_device(L, pkg):
    if L.ns_hip_device_count() > 0:
        return
    m, n_expert, n_used, d = 2, 8, 2, 64
    logits, ids, wts, probs = route_buffers(m, n_expert, n_used)
    for flags in (0, pkg.MOE_ROUTE_RAW_WEIGHTS):
        L.ns_hip_reset_error()
        assert L.ns_hip_moe_route_f(vp(logits), n_expert, m, n_expert, n_used, vp(ids), n_used, vp(wts), n_used, vp(probs), flags, None) == -1
        assert "no HIP device" in pkg.last_error()
        assert np.all(ids == -77) and np.all(wts == 7.0) and np.all(probs == 7.0)
    L.ns_hip_reset_error()
    a = np.zeros((m, d), np.float32)
    out = np.full((m, d), 7.0, np.float32)
    # (no expert group can exist without a device: the entry must refuse before it looks at one)
    assert L.ns_hip_moe_ffn_gelu(vp(a), d, m, vp(ids), n_used, vp(wts), n_used, n_used, None, None, None, vp(out), d, None) == -1
    assert "no HIP device" in pkg.last_error()
    assert np.all(out == 7.0)
    stats = (C.c_uint64 * 4)()
    L.ns_hip_moe_ffn_stats(stats)
    assert list(stats) == [0, 0, 0, 0]
    L.ns_hip_reset_error()


def test_route_f_refuses_an_unknown_flag_bit(L, pkg):
    import ctypes as C
    if L.ns_hip_device_count() > 0:
        import torch
        m, n_expert, n_used = 2, 8, 2
        dL = torch.zeros((m, n_expert), device="cuda")
        dI = torch.full((m, n_used), -77, dtype=torch.int32, device="cuda")
        dW = torch.full((m, n_used), 7.0, device="cuda")
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        for flags in (2, 3, 1 << 30):
            assert L.ns_hip_moe_route_f(dL.data_ptr(), n_expert, m, n_expert, n_used, dI.data_ptr(), n_used, dW.data_ptr(), n_used, None, flags, st) == -1
            assert "flag" in pkg.last_error()
        torch.cuda.synchronize()
        assert bool((dI == -77).all()) and bool((dW == 7.0).all())
    else:
        logits, ids, wts, probs = route_buffers()
        for flags in (2, 3, 1 << 30):
            assert L.ns_hip_moe_route_f(vp(logits), 8, 2, 8, 2, vp(ids), 2, vp(wts), 2, vp(probs), flags, None) == -1
        assert np.all(ids == -77) and np.all(wts == 7.0) and np.all(probs == 7.0)
    L.ns_hip_reset_error()


def test_the_new_tuning_key_is_accepted(L):
    for v in (10, -1, 0):
        assert L.ns_hip_set_tuning(b"moe_ffn_grouped_rows", v) == 0

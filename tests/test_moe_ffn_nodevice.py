"""Without a HIP device the MoE decode block's entries (ns_hip_moe_route, ns_hip_moe_ffn_silu) refuse like every compute entry: -1,
"no HIP device" in the error text, nothing written — there is no CPU fallback.  With a device this file is a no-op (the GPU tests
cover the entries)."""
import ctypes as C

import numpy as np


def test_moe_entries_refuse_without_a_device(L, pkg):
    if L.ns_hip_device_count() > 0:
        return
    m, n_expert, n_used, d = 2, 8, 2, 64
    logits = np.zeros((m, n_expert), np.float32)
    ids = np.full((m, n_used), -77, np.int32)
    wts = np.full((m, n_used), 7.0, np.float32)
    probs = np.full((m, n_expert), 7.0, np.float32)
    vp = lambda x: x.ctypes.data_as(C.c_void_p)
    L.ns_hip_reset_error()
    assert L.ns_hip_moe_route(vp(logits), n_expert, m, n_expert, n_used, vp(ids), n_used, vp(wts), n_used, vp(probs), None) == -1
    assert "no HIP device" in pkg.last_error()
    assert np.all(ids == -77) and np.all(wts == 7.0) and np.all(probs == 7.0)
    L.ns_hip_reset_error()
    a = np.zeros((m, d), np.float32)
    out = np.full((m, d), 7.0, np.float32)
    # (no expert group can exist without a device: the entry must refuse before it looks at one)
    assert L.ns_hip_moe_ffn_silu(vp(a), d, m, vp(ids), n_used, vp(wts), n_used, n_used, None, None, None, vp(out), d, None) == -1
    assert "no HIP device" in pkg.last_error()
    assert np.all(out == 7.0)
    stats = (C.c_uint64 * 4)()
    L.ns_hip_moe_ffn_stats(stats)
    assert list(stats) == [0, 0, 0, 0]
    L.ns_hip_reset_error()

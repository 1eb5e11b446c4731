"""ns_hip_rope_cos_sin_mode checks its arguments before it looks for a device: a refusal needs no GPU."""
import numpy as np


def test_rope_cos_sin_mode_refuses_bad_arguments_without_a_device(L, pkg):
    buf = np.full(64, 7.0, np.float32)
    p = buf.ctypes.data
    for mode in (1, 3, 4, -1):
        assert L.ns_hip_rope_cos_sin_mode(1, 0, 16, mode, 10000.0, 1.0, 1.0, p, None) == -1
        assert "modes 0" in pkg.last_error()
        L.ns_hip_reset_error()
    for mode in (0, 2):
        for n_dims in (15, 1, 0):
            assert L.ns_hip_rope_cos_sin_mode(1, 0, n_dims, mode, 10000.0, 1.0, 1.0, p, None) == -1
            assert "invalid argument" in pkg.last_error()
            L.ns_hip_reset_error()
        assert L.ns_hip_rope_cos_sin_mode(1, 0, 16, mode, 10000.0, 1.0, 1.0, None, None) == -1
        L.ns_hip_reset_error()
    assert np.all(buf == 7.0)

"""CPU part of tests/test_gpu_gemm3_fp8.py: the fp8 blobs its GPU cases multiply parse with the oracle alone and their fp64
reference is finite, the wide-scale-range ones included."""
import numpy as np
import pytest

F8 = [("F8_E4M3", "F8_E8M0"), ("F8_E4M3", "F32"), ("F8_E5M2", "F8_E8M0"), ("F8_E5M2", "F32")]


def _blob(nso, w, f8, st, bs=32, core="CORE_AVX512F"):
    return nso.quant_pack(w, bs, getattr(nso, f8), getattr(nso, st), False, getattr(nso, core))


def _spread(rng, n, k, log2):
    w = (rng.standard_normal((n, k)) * 0.05).astype(np.float32)
    w[0::3] *= np.float32(2.0 ** log2)
    w[1::3] *= np.float32(2.0 ** -log2)
    return w


@pytest.mark.parametrize("f8,st", F8)
def test_oracle_alone_loads_the_blobs(nso, f8, st):
    """CPU part of case 1: the blobs the GPU cases use parse, and their fp64 reference is finite"""
    rng = np.random.default_rng(5)
    for w in ((rng.standard_normal((144, 512)) * 0.05).astype(np.float32), _spread(rng, 144, 512, 10), _spread(rng, 144, 512, 3)):
        blob = _blob(nso, w, f8, st)
        assert nso.parse(blob).q_bytes > 0
        ref = nso.gemm_f64(rng.standard_normal((5, 512)).astype(np.float32), blob)
        assert np.all(np.isfinite(ref)) and np.any(ref != 0)

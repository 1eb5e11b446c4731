"""Worker of tests/test_gpu_attention_paths.py: one attention call in a process of its own.

  attn_variant_worker.py <bs> <heads> <heads_kv> <head_size> <sl_q> <sl_kv> <flags> <seed> <out.npz>

launch_attn reads NS_ATTN_PVAR (when the next K / V tile of attn_mfma3_kernel is requested) and NS_ATTN_PIPE (0: attn_mfma2_kernel for
the exact head sizes) once per process, so a schedule other than the default can only be had from a fresh process with the variable
set by the parent.  The inputs are a function of (case, seed) alone: the parent draws the same ones with inputs()."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def inputs(bs, hn, hkv, hs, sl_q, sl_kv, seed):
    """q fp32 [bs][sl_q][heads][hs]; k, v fp16 [bs][sl_kv][heads_kv][hs].  K and V are drawn key by key, so two cases that differ in
    sl_kv only share Q and every key they both have."""
    rng = np.random.default_rng(seed)
    q = rng.standard_normal((bs, sl_q, hn, hs)).astype(np.float32)
    kv = rng.standard_normal((sl_kv, bs, 2, hkv, hs)).astype(np.float16)
    k = np.ascontiguousarray(kv[:, :, 0].transpose(1, 0, 2, 3))
    v = np.ascontiguousarray(kv[:, :, 1].transpose(1, 0, 2, 3))
    return q, k, v


def forward(L, pkg, q, k, v, flags):
    """the host-tensor entry on position-major tensors, QK_scale = 1 / sqrt(hs); the output buffer starts as 7.0"""
    bs, sl_q, hn, hs = q.shape
    sl_kv, hkv = k.shape[1], k.shape[2]
    out = np.full(q.shape, 7.0, np.float32)
    a = pkg.attn_args(q.ctypes.data, k.ctypes.data, v.ctypes.data, out.ctypes.data, bs, hn, hkv, hs, sl_q, sl_kv,
                      float(1.0 / np.sqrt(hs)), flags)
    L.bestla_fusion_attn_fp32_fp16_fp16_fp32_forward(C.byref(a))
    return out


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    case = [int(x) for x in sys.argv[1:8]]
    pkg = ge.load_package()
    q, k, v = inputs(*case[:6], int(sys.argv[8]))
    out = forward(pkg.lib(), pkg, q, k, v, case[6])
    assert np.all(np.isfinite(out)) and not np.any(out == 7.0), "the entry left rows unwritten: %s" % pkg.lib().ns_hip_last_error()
    np.savez(sys.argv[9], out=out)
    print("ATTN_VARIANT_WORKER_OK PVAR=%s PIPE=%s" % (os.environ.get("NS_ATTN_PVAR"), os.environ.get("NS_ATTN_PIPE")))

"""Worker of tests/test_gpu_launch_order.py: two launches of kernels that need more than the default dynamic LDS limit, in a given
order, in a process of its own — whichever runs first is the first kernel of its launcher that this process launches.

  launch_order_worker.py gemm3 sym,asym <out.npz>     gemm3_kernel<..., ASYM, 256>, symmetric / asymmetric S4 weights
  launch_order_worker.py attn 64,128 <out.npz>        attn_mfma3_kernel<head size>, causal prefill of 128 rows

Every call goes through an entry that returns a status, and the worker fails on the first that is not 0.  The outputs land in the
.npz under the names of the order.  The inputs are functions of the name alone: the parent draws the same ones."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

GEMM_N, GEMM_K, GEMM_M, GEMM_GROUP = 256, 512, 256, 32
ATTN_ROWS, ATTN_HEADS = 128, 2


def gemm_inputs(name):
    """w fp32 [n][k], a fp32 [m][k], asym"""
    asym = {"sym": False, "asym": True}[name]
    rng = np.random.default_rng(11 + asym)
    w = (rng.standard_normal((GEMM_N, GEMM_K)) * 0.05).astype(np.float32)
    a = rng.standard_normal((GEMM_M, GEMM_K)).astype(np.float32)
    return w, a, asym


def gemm_blob(nso, w, asym):
    return nso.quant_pack(w, GEMM_GROUP, nso.S4, nso.BF16, asym, nso.CORE_AVX512_VNNI_KB)


def attn_inputs(name):
    """q fp32 [1][rows][heads][hs]; k, v fp16 [1][rows][heads][hs]"""
    hs = int(name)
    rng = np.random.default_rng(hs)
    q = rng.standard_normal((1, ATTN_ROWS, ATTN_HEADS, hs)).astype(np.float32)
    k = rng.standard_normal((1, ATTN_ROWS, ATTN_HEADS, hs)).astype(np.float16)
    v = rng.standard_normal((1, ATTN_ROWS, ATTN_HEADS, hs)).astype(np.float16)
    return q, k, v


def run_gemm3(pkg, nso, torch, name):
    L = pkg.lib()
    w, a, asym = gemm_inputs(name)
    blob = gemm_blob(nso, w, asym)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    wt = pkg.Weight.from_host_blob(nso.ptr(blob), st)
    da = torch.from_numpy(a).cuda()
    dc = torch.full((GEMM_M, GEMM_N), 7.0, device="cuda")
    pkg.check(L.ns_hip_f32f32_forward(da.data_ptr(), wt.h, dc.data_ptr(), GEMM_M, GEMM_K, GEMM_N, 0, None, 0, st))
    torch.cuda.synchronize()
    return dc.cpu().numpy()


def run_attn(pkg, nso, torch, name):
    L = pkg.lib()
    q, k, v = attn_inputs(name)
    hs = q.shape[-1]
    dq, dk, dv = torch.from_numpy(q).cuda(), torch.from_numpy(k).cuda(), torch.from_numpy(v).cuda()
    dd = torch.full(q.shape, 7.0, device="cuda")
    a = pkg.attn_args(dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), dd.data_ptr(), 1, ATTN_HEADS, ATTN_HEADS, hs, ATTN_ROWS, ATTN_ROWS,
                      float(1.0 / np.sqrt(hs)), 1)
    pkg.check(L.ns_hip_attn_fp32_fp16_fp16_fp32_forward(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return dd.cpu().numpy()


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    import torch

    import __graft_entry__ as ge
    pkg, nso = ge.load_package(), ge.load_oracle()
    kind, order, path = sys.argv[1], sys.argv[2].split(","), sys.argv[3]
    outs = {}
    if kind == "gemm3":
        assert pkg.lib().ns_hip_set_tuning(b"g3_bm", 256) == 0
    for name in order:
        outs[name] = (run_gemm3 if kind == "gemm3" else run_attn)(pkg, nso, torch, name)
        assert np.all(np.isfinite(outs[name])) and not np.any(outs[name] == 7.0), "%s %s left outputs unwritten" % (kind, name)
    np.savez(path, **outs)
    print("LAUNCH_ORDER_WORKER_OK %s %s" % (kind, ",".join(order)))

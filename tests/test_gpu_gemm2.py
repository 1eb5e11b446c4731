"""gemm2_kernel (prefill GEMM, second generation; ns_gemm2.hip) serves single matrices only below "g3_min_m" rows or with NS_GEMM3=0, so the
suite reaches it by raising that threshold above the call's rows: device-pointer forward against the fp64 product of the dequantised
weight, at the bar of tests/test_gpu_gemm3.py::test_gemm3_host_api.  Shapes: one partial row block (33 rows) and two with a partial one
(150); a partial column block with a partial k-step (144 x 192) and a K split (128 x 1024: two splits of 8 chunks + the reduction pass)."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

_spec = importlib.util.spec_from_file_location("gemm_blocks", os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools", "gemm_blocks.py"))
gb = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gb)

pytestmark = pytest.mark.gpu
TOL = 1e-3  # test_gpu_gemm3.py::test_gemm3_host_api


@pytest.fixture(scope="module")
def problems(nso):
    """(activations, blob, fp64 reference) per (format, shape, rows), computed once"""
    out = {}
    for qt, core in (("S4", "CORE_AVX512_VNNI_KB"), ("S8", "CORE_AVX512F")):
        for n, k in ((144, 192), (128, 1024)):
            rng = np.random.default_rng(n + k + len(qt))
            w = (rng.standard_normal((n, k)) * 0.05).astype(np.float32)
            blob = nso.quant_pack(w, 32, getattr(nso, qt), nso.BF16, False, getattr(nso, core))
            for m in (33, 150):
                a = rng.standard_normal((m, k)).astype(np.float32)
                out[qt, n, k, m] = (a, blob, nso.gemm_f64(a, blob))
    return out


# f32: fp32 activations in, fp32 out (the conversion pass).  shadow: fp32 + fp16 activations in, fp32 + fp16 out.  f16only: fp16 activations alone
# — the entry that hands a call of 33 rows to the tiled kernels whatever the output's width (fp32 calls of up to 64 rows on a narrow
# output stay on the streaming kernel, ns_dispatch.cpp)
@pytest.mark.parametrize("form", ["f32", "shadow", "f16only"])
@pytest.mark.parametrize("m", [33, 150])
@pytest.mark.parametrize("n,k", [(144, 192), (128, 1024)])
@pytest.mark.parametrize("qt", ["S4", "S8"])
def test_gemm2_kernel_device_forward(L, pkg, nso, problems, qt, n, k, m, form):
    import torch
    a, blob, ref = problems[qt, n, k, m]
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    wt = pkg.Weight.from_host_blob(nso.ptr(blob), st)
    da = torch.from_numpy(a).cuda()
    da16 = da.half()
    if form == "f16only":  # the reference of what the kernel is given: the fp16-rounded activations
        ref = nso.gemm_f64(da16.float().cpu().numpy(), blob)
    dc = torch.full((m, n), -7.0, device="cuda")
    dc16 = torch.full((m, n), -7.0, device="cuda", dtype=torch.float16)
    assert L.ns_hip_set_tuning(b"g3_min_m", 1 << 20) == 0
    try:
        pkg.check(L.ns_hip_f32f32_forward_h(None if form == "f16only" else da.data_ptr(), None if form == "f32" else da16.data_ptr(), wt.h, dc.data_ptr(),
                                            None if form == "f32" else dc16.data_ptr(), m, k, n, pkg.EPI_NONE, None, n, st))
        torch.cuda.synchronize()
    finally:
        L.ns_hip_set_tuning(b"g3_min_m", 0)
        wt.free()
    out = dc.cpu().numpy()
    err = nso.rel_l2(out, ref)
    print("gemm2_kernel %s %dx%d m=%d %s: rel_l2 %.3g" % (qt, n, k, m, form, err))
    assert err < TOL
    # rows, 16-column tiles, (tile x 64-row block) and term errors as well (tests/tools/gemm_blocks.py); the fp16-only form against the
    # references of what the kernel is given, the fp16-rounded activations
    gb.check_blocks(nso, out, da16.float().cpu().numpy() if form == "f16only" else a, blob, "tiled", what="gemm2_kernel %s %s" % (qt, form))
    if form == "f32":
        assert torch.all(dc16 == -7.0)
    else:
        assert np.allclose(dc16.float().cpu().numpy(), out, rtol=2e-3, atol=2e-3)

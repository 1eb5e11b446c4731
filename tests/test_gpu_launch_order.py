"""Kernels that need more dynamic LDS than the 64 KiB default have their limit raised at their first launch (launch_lds,
neural-speed_amd/csrc/ns_launch.h).  That has to hold per KERNEL, whichever kernel of a launcher a process happens to launch first:
    gemm3_kernel<..., ASYM = false, 256> and <..., ASYM = true, 256>          both above 64 KiB
    attn_mfma3_kernel<64> (33 KiB) and attn_mfma3_kernel<128> (66 KiB)
Each order runs in a fresh process (tests/tools/launch_order_worker.py), every call must succeed, and every output is compared with
the oracle at the tolerance the kernel's own test file uses (test_gpu_gemm3.py / test_gpu_attention.py: 1e-3 relative L2)."""
import importlib.util
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
TOL = 1e-3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "tools", "launch_order_worker.py")
_spec = importlib.util.spec_from_file_location("launch_order_worker", WORKER)
worker = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(worker)

_child_failed = []


def run_child(kind, order):
    """the worker in a fresh process under a time limit; after one child failed no other is started"""
    if _child_failed:
        pytest.fail("not started: an earlier child process failed (%s)" % _child_failed[0])
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "out.npz")
        cmd = [sys.executable, WORKER, kind, ",".join(order), path]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=120)
        except subprocess.TimeoutExpired:
            _child_failed.append("%s %s: time limit" % (kind, order))
            raise
        if r.returncode != 0:
            _child_failed.append("%s %s: exit %d" % (kind, order, r.returncode))
            pytest.fail("worker %s %s: exit %d\n%s\n%s" % (kind, order, r.returncode, r.stdout[-2000:], r.stderr[-2000:]))
        with np.load(path) as z:
            return {name: z[name] for name in order}


@pytest.fixture(scope="module")
def gemm_refs(nso):
    refs = {}
    for name in ("sym", "asym"):
        w, a, asym = worker.gemm_inputs(name)
        refs[name] = nso.gemm_f64(a, worker.gemm_blob(nso, w, asym))
    return refs


@pytest.fixture(scope="module")
def attn_refs(nso):
    refs = {}
    for name in ("64", "128"):
        q, k, v = worker.attn_inputs(name)
        refs[name] = nso.attn_ref(q, k, v, float(1.0 / np.sqrt(int(name))), 1)
    return refs


@pytest.mark.parametrize("order", [("sym", "asym"), ("asym", "sym")])
def test_gemm3_256_row_tile_symmetric_and_asymmetric_in_either_order(nso, gemm_refs, order):
    outs = run_child("gemm3", order)
    for name in order:
        e = nso.rel_l2(outs[name], gemm_refs[name])
        print("gemm3 order %s: %s rel l2 %.3g" % (order, name, e))
        assert e < TOL, (order, name, e)


@pytest.mark.parametrize("order", [("64", "128"), ("128", "64")])
def test_causal_prefill_attention_head_sizes_64_and_128_in_either_order(nso, attn_refs, order):
    outs = run_child("attn", order)
    for name in order:
        e = nso.rel_l2(outs[name], attn_refs[name])
        print("attention order %s: head size %s rel l2 %.3g" % (order, name, e))
        assert e < TOL, (order, name, e)

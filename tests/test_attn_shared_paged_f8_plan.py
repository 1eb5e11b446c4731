"""attn_shared_paged_f8_plan (ns_attn_plan.cpp: what ns_hip_attn_decode_paged_shared_f8 launches).  tests/tools/attn_shared_paged_f8_plan_main.cpp, a
host program, prints the FP8 plan beside attn_shared_paged_plan of the same call: ten accepted calls, then every refusal."""
import importlib.util
import subprocess

import pytest

from test_attn_paged_plan import fields
from test_attn_plan import CSRC, ROOT, compiler

MAIN = ROOT + "/tests/tools/attn_shared_paged_f8_plan_main.cpp"
POOL = {"head_size_72": "head_size must be a multiple of 16", "step_sl": "row and head strides must be multiples of 16",
        "block_step": "block_step must be a multiple of 16", "base": "pool bases must be 16-byte aligned", "k_scale_nan": "must be positive and finite",
        "v_scale_inf": "must be positive and finite", "scale_in_front_of_sl_q": "must be positive and finite"}
FP16 = {"head_size_80": "head_size must be 64 or 128", "alibi_tanh": "ALiBi and the tanh cap are not served", "sl_q_2": "sl_q must be 1",
        "groups_0": "groups must be 1 .. 65535", "grid_limit_members": "groups * max_group above the grid limit"}


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    hipcc = compiler()
    if not hipcc:
        pytest.skip("the library's compiler is not installed")
    exe = str(tmp_path_factory.mktemp("attn_shared_paged_f8_plan") / "attn_shared_paged_f8_plan")
    subprocess.run([hipcc, "-std=c++20", "-x", "hip", "--offload-arch=gfx950", "--cuda-host-only", "-Wall", "-Werror", "-I", CSRC, MAIN, "-o", exe],
                   check=True, capture_output=True, text=True, timeout=300)
    return exe


def run(exe, *args):
    out = subprocess.run([exe] + [str(x) for x in args], check=True, capture_output=True, text=True, timeout=120).stdout.splitlines()
    return [(what, fields(o), fields(r)) for what, o, r in (line.split(" | ") for line in out)]


@pytest.fixture(scope="module")
def lines(exe):
    return run(exe)


def test_the_pool_of_the_far_address_test_takes_the_kernel_it_asserts(exe):
    """tests/test_gpu_attn_shared_paged_f8.py asserts attn_shared8_kernel<128> through ns_hip_attn_decode_paged_shared_f8_stats on a pool of 2^20 + 64
    blocks of 4096 bytes: accepted as the FP8 family with the caller's pool (no 32-bit rule: 64-bit addresses).  Numbers: tests/tools/attn_far_layout.py."""
    spec = importlib.util.spec_from_file_location("attn_far_layout", ROOT + "/tests/tools/attn_far_layout.py")
    FL = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(FL)
    step = FL.block_step(128, FL.SHARED_BK)
    assert step == 4096 and FL.F8_BLOCKS * step > 1 << 32
    (what, o, r), = run(exe, "far", 128, FL.SHARED_BK, FL.SHARED_CAP, len(FL.SHARED_LENS), len(FL.SHARED_PREFIX), FL.SHARED_MAX_GROUP, FL.F8_BLOCKS, step,
                        *FL.strides("pm", 128, FL.SHARED_BK))
    assert what == "far" and (o["ok"], o["f8"], o["why"], o["hspad"]) == (1, 1, "", 128), o
    assert (o["blocks"], o["bstep"], o["ksl"], o["khead"], o["vsl"], o["vhead"]) == (FL.F8_BLOCKS, step, 256, 128, 256, 128), o
    assert {k: (o[k], r[k]) for k in o if k != "f8" and o[k] != r[k]} == {}


def test_the_f8_plan_is_the_fp16_shared_plan_but_for_the_family(lines):
    """every field: both grids, the merge grid, ranges, records, partials, the page, the device arrays, pointers, strides, the folded scales"""
    plans = [(o, r) for what, o, r in lines if what == "plan"]
    assert len(plans) == 10
    for o, r in plans:
        assert (o["ok"], o["f8"], r["ok"], r["f8"], o["why"], r["why"]) == (1, 1, 1, 0, "", ""), (o, r)
        assert {k: (o[k], r[k]) for k in o if k != "f8" and o[k] != r[k]} == {}
        assert o["arrays"] == 4 and (float.fromhex(o["qk"]), float.fromhex(o["out"])) == (0.125 * 0.5 * 0.25, 2.0 / 4.0)
    assert len({(o["nsp"], o["kpsp"], o["nss"], o["kpss"]) for o, _ in plans}) > 3  # (the shapes reach several range layouts)


def test_pool_refusals_come_first_and_the_fp16_refusals_stay(lines):
    """the pool's refusals in the pool's words, in front of the fp16 plan's (head size 72; a bad scale beside sl_q = 2); the fp16 plan's own in its words"""
    got = {what: (o, r) for what, o, r in lines if what != "plan"}
    assert set(got) == set(POOL) | set(FP16)
    for what, (o, r) in got.items():
        assert (o["ok"], o["f8"]) == (0, 0) and (POOL.get(what) or FP16[what]) in o["why"], (what, o)
        assert r["why"] == o["why"] if what in FP16 else r["why"] != o["why"], (what, o, r)

"""attn_block_paged_f8_plan (neural-speed_amd/csrc/ns_attn_plan.cpp: what ns_hip_attn_block_paged_f8 launches).  A host program
(tests/tools/attn_block_paged_f8_plan_main.cpp, built with the library's compiler, nothing launched) prints the FP8 plan beside attn_block_paged_plan of
the same shape over 486 shapes, and the FP8 plan of each refused call."""
import importlib.util
import os
import subprocess

import pytest

from test_attn_paged_plan import fields
from test_attn_plan import CSRC, ROOT, compiler, num

MAIN = os.path.join(ROOT, "tests", "tools", "attn_block_paged_f8_plan_main.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    hipcc = compiler()
    if not hipcc:
        pytest.skip("the library's compiler is not installed")
    exe = str(tmp_path_factory.mktemp("attn_block_paged_f8_plan") / "attn_block_paged_f8_plan")
    subprocess.run([hipcc, "-std=c++20", "-x", "hip", "--offload-arch=gfx950", "--cuda-host-only", "-Wall", "-Werror", "-I", CSRC, MAIN, "-o", exe],
                   check=True, capture_output=True, text=True, timeout=300)
    return exe


def run(exe, *args):
    res = {"plan": [], "refuse": []}
    for line in subprocess.run([exe] + [str(x) for x in args], check=True, capture_output=True, text=True, timeout=120).stdout.splitlines():
        kind, rest = line.split(" ", 1)
        parts = rest.split(" | ")
        res[kind].append(({k: num(v) for k, v in (kv.split("=") for kv in parts[0].split())},) + tuple(fields(p) for p in parts[1:]))
    return res


@pytest.fixture(scope="module")
def lines(exe):
    return run(exe)


def test_the_pool_of_the_far_address_test_takes_the_kernel_it_asserts(exe):
    """tests/test_gpu_attn_block_paged_f8.py asserts attn_block_split8_kernel<128> through ns_hip_attn_block_paged_f8_stats on a pool of 2^20 + 64 blocks
    of 4096 bytes: accepted as the FP8 family with the caller's pool (no 32-bit rule: 64-bit addresses).  Numbers: tests/tools/attn_far_layout.py."""
    spec = importlib.util.spec_from_file_location("attn_far_layout", os.path.join(ROOT, "tests", "tools", "attn_far_layout.py"))
    FL = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(FL)
    step = FL.block_step(128, 16)
    assert step == 4096 and FL.F8_BLOCKS * step > 1 << 32
    (i, o, r), = run(exe, "far", 128, 16, FL.PAGED_CAP[16], len(FL.BLOCK_Q), max(FL.BLOCK_Q), FL.F8_BLOCKS, step, *FL.strides("pm", 128, 16))["plan"]
    assert i["what"] == "far" and (o["ok"], o["f8"], o["why"], o["hs_pad"]) == (1, 1, "", 128), o
    assert (o["blocks"], o["bstep"], o["ksl"], o["khead"], o["vsl"], o["vhead"]) == (FL.F8_BLOCKS, step, 256, 128, 256, 128), o
    assert {k: (o[k], r[k]) for k in o if k != "f8" and o[k] != r[k]} == {}


def test_the_f8_plan_is_the_fp16_block_plan_but_for_the_family(lines):
    """every field: grid, merge grid, ranges, dyn constant, partials, the page, pointers, strides, the folded scales"""
    assert len(lines["plan"]) == 486
    for i, o, r in lines["plan"]:
        assert o["why"] == "" and r["why"] == "" and (o["ok"], o["f8"], r["ok"], r["f8"]) == (1, 1, 1, 0), (i, o, r)
        diff = {k: (o[k], r[k]) for k in o if k != "f8" and o[k] != r[k]}
        assert not diff, (i, diff)
        assert o["hs_pad"] == i["hs"] and o["kmove"] == o["qstart"] == o["table"] == 1 and (float.fromhex(o["qk"]), float.fromhex(o["out"])) == (0.125 * 0.5 * 0.25, 2.0 / 4.0)
    assert len({(o["nsplit"], o["kps"]) for _, o, _ in lines["plan"]}) > 10  # (the grid of shapes reaches many range layouts)


def test_each_refusal_names_its_reason(lines):
    got = {i["what"]: o for i, o in lines["refuse"]}
    none = got.pop("none")
    assert (none["ok"], none["f8"], none["why"]) == (1, 1, "")
    want = {"head_size": "head_size must be a multiple of 16", "step_sl": "row and head strides must be multiples of 16",
            "step_head": "row and head strides must be multiples of 16", "block_step": "block_step must be a multiple of 16",
            "base": "pool bases must be 16-byte aligned", "k_scale_zero": "must be positive and finite", "v_scale_negative": "must be positive and finite",
            "v_scale_inf": "must be positive and finite", "k_scale_nan": "must be positive and finite", "head_size_80": "head_size must be 64 or 128",
            "null_table": "block table is null"}
    assert set(got) == set(want)
    for what, text in want.items():
        assert (got[what]["ok"], got[what]["f8"]) == (0, 0) and text in got[what]["why"], (what, got[what])

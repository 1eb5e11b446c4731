"""with_format (neural-speed_amd/csrc/ns_launch.h) is the one place that walks from a weight's run-time format to the template
arguments (KIND, SPS, SK, ASYM) the matrix kernels are instantiated for.  A host program (tests/tools/format_ladder_main.cpp, built
with the library's compiler) prints what it hands over for every combination of inputs; the rule it must follow is written out here."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "neural-speed_amd", "csrc")
MAIN = os.path.join(ROOT, "tests", "tools", "format_ladder_main.cpp")


def compiler():
    """HIPCC of the library's Makefile (the environment's HIPCC wins there too)"""
    with open(os.path.join(CSRC, "Makefile")) as f:
        default = re.search(r"^HIPCC\s*\?=\s*(\S+)", f.read(), re.M).group(1)
    path = os.environ.get("HIPCC", default)
    return path if os.path.exists(path) else shutil.which(path)


def expected(kind, sps, dt, asym):
    four_bit = kind in ("INT4", "F4")
    sps_out = sps if sps in ((4, 2, 1) if four_bit else (2, 1)) else 1   # any other count means 1
    sk = "F32" if kind == "F8" else dt if dt in ("F32", "F16") else "BF16"  # F8 scales are always fp32; any other type means bf16
    asym_out = asym if kind in ("INT4", "INT8") else 0                    # F4 and F8 have no zero points
    return (kind, sps_out, sk, asym_out)


@pytest.fixture(scope="module")
def ladder(tmp_path_factory):
    hipcc = compiler()
    if not hipcc:
        pytest.skip("the library's compiler is not installed")
    exe = str(tmp_path_factory.mktemp("format_ladder") / "format_ladder")
    subprocess.run([hipcc, "-std=c++20", "-x", "hip", "--offload-arch=gfx950", "--cuda-host-only", "-Wall", "-Werror", "-I", CSRC, MAIN,
                    "-o", exe], check=True, capture_output=True, text=True, timeout=300)
    out = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=60).stdout
    rows = {}
    for line in out.splitlines():
        m = re.fullmatch(r"(\w+) (\d+) (\w+) ([01]) -> (\w+) (\d+) (\w+) ([01])", line)
        assert m, line
        key = (m.group(1), int(m.group(2)), m.group(3), int(m.group(4)))
        assert key not in rows, line
        rows[key] = (m.group(5), int(m.group(6)), m.group(7), int(m.group(8)))
    return rows


def test_every_combination_follows_the_rule(ladder):
    keys = [(kind, sps, dt, asym) for kind in ("INT4", "INT8", "F4", "F8") for sps in (1, 2, 3, 4, 8)
            for dt in ("F32", "F16", "BF16", "OTHER") for asym in (0, 1)]
    assert sorted(ladder) == sorted(keys)
    wrong = {k: ladder[k] for k in keys if ladder[k] != expected(*k)}
    assert not wrong, wrong


def test_the_ladder_reaches_41_formats(ladder):
    tuples = set(ladder.values())
    count = lambda kind: sum(1 for t in tuples if t[0] == kind)
    assert (count("INT4"), count("INT8"), count("F4"), count("F8")) == (18, 12, 9, 2)
    assert len(tuples) == 41


def test_kind_and_sps_are_the_decode_slices(ladder):
    with open(os.path.join(CSRC, "ns_gemv.h")) as f:
        line = re.search(r"^#define NS_GEMV_SLICES\(X\)(.*)$", f.read(), re.M).group(1)
    slices = [(k, int(s)) for k, s in re.findall(r"X\((\w+), (\d+)\)", line)]
    assert len(slices) == 10 and len(set(slices)) == 10
    assert {(t[0], t[1]) for t in ladder.values()} == set(slices)

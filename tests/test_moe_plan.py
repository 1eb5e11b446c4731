"""moe_pair_plan (neural-speed_amd/csrc/ns_moe_plan.cpp) lays out the (token row, selection) pairs of a MoE block call for the grouped pass of
ns_hip_moe_ffn_silu / _gelu: which gathered row every pair gets, where every expert's group starts, how many rows its GEMMs are launched
with.  A host program (tests/tools/moe_plan_main.cpp, nothing launched) prints the plan for a list of id tables; the rule it must follow -
ns_moe_plan.h - is restated here independently, as properties of the printed layout.  The program is plain C++: it is built once with the
library's compiler and once with g++ under the address and undefined-behaviour sanitizers."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "neural-speed_amd", "csrc")
SOURCES = [os.path.join(ROOT, "tests", "tools", "moe_plan_main.cpp"), os.path.join(CSRC, "ns_moe_plan.cpp")]
PAD = 1 << 20          # what the padding columns of an id table hold: never an id


def compiler():
    """HIPCC of the library's Makefile (the environment's HIPCC wins there too)"""
    with open(os.path.join(CSRC, "Makefile")) as f:
        default = re.search(r"^HIPCC\s*\?=\s*(\S+)", f.read(), re.M).group(1)
    path = os.environ.get("HIPCC", default)
    return path if os.path.exists(path) else shutil.which(path)


def tables():
    """(name, ids [m][n_used], n_as, ids_stride)"""
    rng = np.random.default_rng(7)
    t = []
    t.append(("all_on_one_expert", np.full((6, 2), 2), 4, 2))
    t.append(("an_expert_with_none", np.array([[0, 1], [3, 0], [1, 3], [0, 3]]), 4, 3))
    t.append(("lone_pair_first_group", np.array([[1, 2], [0, 3], [2, 1], [3, 2]]), 4, 2))
    t.append(("lone_pair_last_group", np.array([[1, 2], [0, 1], [2, 3], [0, 2]]), 4, 4))
    t.append(("lone_pairs_in_a_row", np.array([[0, 1], [2, 3]]), 4, 2))            # every group has one row: each borrows its successor's
    t.append(("row_e_e", np.array([[1, 1], [0, 1], [1, 1]]), 3, 2))
    t.append(("bad_ids", np.array([[-1, 2], [4, 4], [0, -1], [4, 1], [-1, -1], [2, 0]]), 4, 3))   # -1 and n_as
    t.append(("all_bad", np.array([[-1, 9], [9, -1]]), 4, 2))
    t.append(("n_used_1", rng.integers(0, 5, (9, 1)), 5, 1))
    t.append(("n_used_8", np.stack([rng.permutation(12)[:8] for _ in range(5)]), 12, 11))
    t.append(("n_as_1", np.array([[0], [0], [1], [0], [-1]]), 1, 2))
    t.append(("n_as_64", rng.integers(-2, 66, (40, 4)), 64, 4))
    t.append(("m_1", np.array([[3, 0]]), 4, 2))
    t.append(("m_1_lone_last", np.array([[7]]), 8, 1))
    t.append(("prompt", np.stack([rng.permutation(8)[:2] for _ in range(300)]), 8, 2))
    return [(n, np.asarray(i, np.int64), a, s) for n, i, a, s in t]


REFUSED = [(0, 2, 4, 2), (2, 0, 4, 2), (2, 2, 0, 2), (2, 3, 4, 2)]     # m, n_used, n_as, ids_stride: no rows, no selections, no experts, a short stride


def program_input():
    lines = []
    for _, ids, n_as, stride in tables():
        m, n_used = ids.shape
        full = np.full((m, stride), PAD, np.int64)
        full[:, :n_used] = ids
        lines.append("%d %d %d %d %s" % (m, n_used, n_as, stride, " ".join(str(int(v)) for v in full.reshape(-1))))
    for m, n_used, n_as, stride in REFUSED:
        lines.append("%d %d %d %d %s" % (m, n_used, n_as, stride, " ".join(["0"] * (m * stride))))
    return "\n".join(lines) + "\n"


def run_program(exe):
    out = subprocess.run([exe], input=program_input(), check=True, capture_output=True, text=True, timeout=120)
    assert out.stderr == "", out.stderr
    plans = []
    for line in out.stdout.splitlines():
        if line == "refused":
            plans.append(None)
            continue
        d = {}
        for kv in line.split():
            k, v = kv.split("=")
            d[k] = [int(x) for x in v.split(",")] if v else []
        d["pairs"] = d["pairs"][0]
        plans.append(d)
    return plans


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    hipcc = compiler()
    if not hipcc:
        pytest.skip("the library's compiler is not installed")
    exe = str(tmp_path_factory.mktemp("moe_plan") / "moe_plan")
    subprocess.run([hipcc, "-std=c++20", "-x", "hip", "--offload-arch=gfx950", "--cuda-host-only", "-Wall", "-Werror", "-I", CSRC] + SOURCES + ["-o", exe],
                   check=True, capture_output=True, text=True, timeout=300)
    return run_program(exe)


def check_plan(name, ids, n_as, p):
    m, n_used = ids.shape
    good = [(t, i) for t in range(m) for i in range(n_used) if 0 <= ids[t, i] < n_as]       # (row, selection) ascending
    assert p["pairs"] == len(good), name
    assert len(p["offset"]) == len(p["count"]) == len(p["launch_rows"]) == n_as, name
    assert len(p["src_row"]) == p["pairs"] + 1 and len(p["pos"]) == m * n_used, name
    # groups are consecutive, in expert order, and hold exactly their expert's pairs in (row, selection) order
    at = 0
    for e in range(n_as):
        mine = [(t, i) for t, i in good if ids[t, i] == e]
        assert p["offset"][e] == at and p["count"][e] == len(mine), (name, e)
        for r, (t, i) in enumerate(mine):
            assert p["pos"][t * n_used + i] == at + r, (name, e, t, i)
            assert p["src_row"][at + r] == t, (name, e, t, i)
        # launch rows: the group's, except that one row is launched as two - the borrowed one is the next position, which exists
        assert p["launch_rows"][e] == (2 if len(mine) == 1 else len(mine)), (name, e)
        assert at + p["launch_rows"][e] <= p["pairs"] + 1, (name, e)
        at += len(mine)
    assert at == p["pairs"], name
    # every in-range pair exactly once, bad ids nowhere
    placed = [v for v in p["pos"] if v >= 0]
    assert sorted(placed) == list(range(p["pairs"])), name
    for t in range(m):
        for i in range(n_used):
            if not 0 <= ids[t, i] < n_as:
                assert p["pos"][t * n_used + i] == -1, (name, t, i)
    assert p["src_row"][p["pairs"]] == -1, name       # the padding row
    assert all(0 <= t < m for t in p["src_row"][:-1]), name


def test_the_plan_follows_the_rule(plans):
    tabs = tables()
    assert len(plans) == len(tabs) + len(REFUSED)
    for (name, ids, n_as, _), p in zip(tabs, plans):
        assert p is not None, name
        check_plan(name, ids, n_as, p)
    assert all(p is None for p in plans[len(tabs):])


def test_the_cases_cover_what_they_are_named_for(plans):
    """the edge cases are really in the tables (a table edited into something tamer must not pass silently)"""
    by_name = {t[0]: (t, p) for t, p in zip(tables(), plans)}
    count = lambda n: by_name[n][1]["count"]
    assert count("all_on_one_expert") == [0, 0, 12, 0]
    assert count("an_expert_with_none")[2] == 0 and min(count("an_expert_with_none")[i] for i in (0, 1, 3)) > 0
    assert count("lone_pair_first_group")[0] == 1 and by_name["lone_pair_first_group"][1]["launch_rows"][0] == 2
    p = by_name["lone_pair_last_group"][1]
    assert p["count"][3] == 1 and p["offset"][3] + 2 == p["pairs"] + 1        # its second launch row is the padding row
    assert count("lone_pairs_in_a_row") == [1, 1, 1, 1]
    p = by_name["row_e_e"][1]
    assert p["pos"][0] + 1 == p["pos"][1] and p["src_row"][p["pos"][0]] == p["src_row"][p["pos"][1]] == 0    # the row is gathered twice
    assert by_name["bad_ids"][1]["pos"][8:10] == [-1, -1] and by_name["bad_ids"][1]["pairs"] == 5
    assert by_name["all_bad"][1]["pairs"] == 0 and by_name["all_bad"][1]["src_row"] == [-1]
    assert by_name["n_as_1"][1]["count"] == [3]
    assert by_name["m_1_lone_last"][1]["launch_rows"][7] == 2 and by_name["m_1_lone_last"][1]["src_row"] == [0, -1]
    assert len(count("n_as_64")) == 64 and by_name["n_used_8"][0][1].shape[1] == 8


def test_the_program_is_clean_under_the_sanitizers(tmp_path, plans):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path / "moe_plan_san")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC] + SOURCES + ["-o", exe], check=True, capture_output=True, text=True, timeout=300)
    assert run_program(exe) == plans

"""The host decisions of the mixture-of-experts family (neural-speed_amd/csrc/ns_moe_plan.cpp), checked without a GPU.

moe_mm_plan / moe_ffn_plan say which server takes a call of ns_hip_mul_mat_id / of the block entries: the program's `plans` mode prints them
for a table of (knobs, facts), and the rule of ns_moe_plan.h is restated here independently (want_mm, want_ffn).

moe_pair_plan lays out the (token row, selection) pairs of a MoE block call for the grouped pass of
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


def run_program(exe, args=(), text=None):
    out = subprocess.run([exe] + list(args), input=program_input() if text is None else text, check=True, capture_output=True, text=True, timeout=120)
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
def program(tmp_path_factory):
    hipcc = compiler()
    if not hipcc:
        pytest.skip("the library's compiler is not installed")
    exe = str(tmp_path_factory.mktemp("moe_plan") / "moe_plan")
    subprocess.run([hipcc, "-std=c++20", "-x", "hip", "--offload-arch=gfx950", "--cuda-host-only", "-Wall", "-Werror", "-I", CSRC] + SOURCES + ["-o", exe],
                   check=True, capture_output=True, text=True, timeout=300)
    return exe


@pytest.fixture(scope="module")
def plans(program):
    return run_program(program)


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


def test_the_program_is_clean_under_the_sanitizers(tmp_path, program, plans):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path / "moe_plan_san")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC] + SOURCES + ["-o", exe], check=True, capture_output=True, text=True, timeout=300)
    assert run_program(exe) == plans
    assert run_program(exe, MIN17[0], MIN17[1]) == run_program(program, MIN17[0], MIN17[1])
    assert run_decisions(exe) == run_decisions(program)


# ---- the layout under ns_hip_mul_mat_id's grouped path: one id column (n_used = 1), a floor on the rows of a populated group -------------------
def column_tables():
    """(name, id column, n_as): lone last groups with out-of-range rows behind them in the old order, as ns_hip_mul_mat_id meets them"""
    t = []
    t.append(("lone_last_then_bad", [0, 0, 1, -1, 3, 4, 1, 0], 4))            # expert 3: one row, the last group; ids -1 and n_as present
    t.append(("lone_last_is_expert_1_then_bad", [0, 9, 0, 1, -1], 4))         # the last POPULATED group is not the last expert
    t.append(("lone_groups_to_the_end_then_bad", [-1, 1, 2, 3, 4, 0, 0], 4))
    t.append(("only_a_lone_group_and_bad", [-1, 2, 7], 4))
    return [(n, np.asarray(c, np.int64).reshape(-1, 1), a, 1) for n, c, a in t]


def test_one_column_tables_with_a_lone_last_group_followed_by_out_of_range_rows(program):
    tabs = column_tables()
    text = "".join("%d 1 %d 1 %s\n" % (len(ids), n_as, " ".join(str(int(v)) for v in ids.reshape(-1))) for _, ids, n_as, _ in tabs)
    got = run_program(program, text=text)
    assert len(got) == len(tabs)
    for (name, ids, n_as, _), p in zip(tabs, got):
        assert p is not None, name
        check_plan(name, ids, n_as, p)
        last = max(e for e in range(n_as) if p["count"][e])
        assert p["count"][last] == 1 and p["offset"][last] + 1 == p["pairs"], name      # the lone last group borrows ...
        assert p["src_row"][p["pairs"]] == -1, name                                      # ... the zero padding row, never an out-of-range row
        assert [t for t in range(len(ids)) if p["pos"][t] < 0] == [t for t in range(len(ids)) if not 0 <= ids[t, 0] < n_as], name


def _column(counts):
    return [e for e, c in enumerate(counts) for _ in range(c)]


MIN17_TABLES = [("group_of_16", _column([20, 16, 0, 17]), 4, False), ("group_of_17", _column([17, 0, 40, 17]), 4, True),
                ("group_of_1", _column([30, 1]) + [-1], 2, False), ("empty_groups_do_not_count", _column([0, 0, 17]) + [5], 3, True)]
MIN17 = (["min_group_rows", "17"], "".join("%d 1 %d 1 %s\n" % (len(c), n_as, " ".join(map(str, c))) for _, c, n_as, _ in MIN17_TABLES))


def test_min_group_rows_refuses_a_populated_group_below_it(program):
    got = run_program(program, MIN17[0], MIN17[1])
    assert [p is not None for p in got] == [ok for _, _, _, ok in MIN17_TABLES]
    for (name, col, n_as, ok), p in zip(MIN17_TABLES, got):
        if ok:
            check_plan(name, np.asarray(col, np.int64).reshape(-1, 1), n_as, p)
    assert all(p is not None for p in run_program(program, text=MIN17[1]))      # without the floor every one of them is laid out


# ---- which server takes a call ---------------------------------------------------------------------------------------------------------------
ROWS = [1, 8, 9, 31, 32, 33, 64, 65]
KNOBS = dict(gemv_rows=8, grouped_rows=32, ffn_grouped_rows=32, ffn_fused=-1)          # the defaults, resolved
FACTS = dict(gate_f8=0, up_f8=0, down_f8=0, k=128, ff=128, dn=128, n_as=8, n_used=2, m=1, single_span=1, shuf=0, all_tiled_f8=1,
             gate_up_one_format=1, capturing=0)
ORDER = ["gemv_rows", "grouped_rows", "ffn_grouped_rows", "ffn_fused", "gate_f8", "up_f8", "down_f8", "k", "ff", "dn", "n_as", "n_used", "m",
         "single_span", "shuf", "all_tiled_f8", "gate_up_one_format", "capturing"]


def decisions():
    """(entry, knobs + facts) of every case"""
    cases = []

    def add(entry, **kw):
        d = dict(KNOBS, **FACTS)
        assert set(kw) <= set(d)
        d.update(kw)
        cases.append((entry, d))

    for entry in ("mm", "ffn"):
        for m in ROWS:
            for cap in (0, 1):
                add(entry, m=m, capturing=cap)
            # every threshold at 0 (a resolved 0 - the environment variable set to 0 - means never, like -1), at positive values and at -1;
            # a tuning KEY of 0 never reaches the plan: moe_knobs() resolves it to the environment's value or the default above
            for key in ("gemv_rows", "grouped_rows", "ffn_grouped_rows"):
                for v in (0, 4, 16, 40, -1):
                    add(entry, m=m, **{key: v})
            for v in (0, 1, -1):
                add(entry, m=m, ffn_fused=v)
            add(entry, m=m, grouped_rows=-1, ffn_grouped_rows=16)       # the block's threshold is its own ...
            add(entry, m=m, grouped_rows=16, ffn_grouped_rows=-1)       # ... in both directions
            add(entry, m=m, shuf=1)
            add(entry, m=m, k=96)
            add(entry, m=m, single_span=0)
            add(entry, m=m, ff=96)
            add(entry, m=m, ff=130)
            add(entry, m=m, gate_up_one_format=0)
            for which in ("gate_f8", "up_f8", "down_f8"):
                add(entry, m=m, **{which: 1})
        for m in (64, 65):
            for tiled in (0, 1):
                add(entry, m=m, gate_f8=1, all_tiled_f8=tiled, capturing=0)
    for n_used in (1, 2, 8):                                            # the fused launches' pair bound: m * n_used < 65536 / n_used
        edge = (65536 // n_used + n_used - 1) // n_used                 # the first m that is too many
        for m in (edge - 1, edge):
            add("ffn", m=m, n_used=n_used, gemv_rows=1 << 20)
    return cases


def want_mm(d):
    tried_g = d["grouped_rows"] > 0 and d["m"] >= d["grouped_rows"] and not d["capturing"]
    refused_g = bool(d["shuf"] or d["k"] % 64 or (d["gate_f8"] and (d["m"] <= 64 or not d["all_tiled_f8"])))
    tried_d = d["m"] <= d["gemv_rows"]
    refused_d = bool(not d["single_span"] or d["gate_f8"])
    return "grouped=%d,%d decode=%d,%d min_group_rows=%d" % (tried_g, refused_g, tried_d, refused_d, 17 if d["gate_f8"] else 0)


def want_ffn(d):
    tried_f = d["ffn_fused"] != 0 and d["m"] <= d["gemv_rows"]
    refused_f = bool(d["gate_f8"] or d["down_f8"] or not d["single_span"] or d["ff"] % 4 or d["m"] * d["n_used"] >= 65536 // d["n_used"])
    tried_g = d["ffn_grouped_rows"] > 0 and d["m"] >= d["ffn_grouped_rows"] and not d["capturing"]
    refused_g = bool(d["gate_f8"] or d["up_f8"] or d["down_f8"] or d["k"] % 64 or d["ff"] % 64 or not d["gate_up_one_format"])
    return "fused=%d,%d grouped=%d,%d" % (tried_f, refused_f, tried_g, refused_g)


PREDICATES = [("fit 32767 1", 1), ("fit 65535 1", 1), ("fit 65536 1", 0), ("fit 16383 2", 1), ("fit 16384 2", 0), ("fit 1023 8", 1), ("fit 1024 8", 0),
              ("addressable 131072 16383 64 64", 1), ("addressable 131072 16384 64 64", 0), ("addressable 131072 64 16384 64", 0),
              ("addressable 131072 64 64 16384", 0), ("addressable 131071 64 64 16384", 1), ("addressable 1 128 128 128", 1)]


def run_decisions(exe):
    text = "".join("%s %s\n" % (entry, " ".join(str(int(d[k])) for k in ORDER)) for entry, d in decisions())
    text += "".join(q + "\n" for q, _ in PREDICATES)
    out = subprocess.run([exe, "plans"], input=text, check=True, capture_output=True, text=True, timeout=120)
    assert out.stderr == "", out.stderr
    return out.stdout.splitlines()


def test_the_server_of_every_call_follows_the_rule(program):
    cases, got = decisions(), run_decisions(program)
    assert len(got) == len(cases) + len(PREDICATES)
    for (entry, d), line in zip(cases, got):
        assert line == (want_mm(d) if entry == "mm" else want_ffn(d)), (entry, d, line)
    assert [int(x) for x in got[len(cases):]] == [w for _, w in PREDICATES]


def test_the_default_thresholds_send_the_rows_where_the_documents_say(program):
    """rows -> server at the default knobs, outside a capture, on weights every server takes: docs/kernels/other.md's path table"""
    cases, got = decisions(), run_decisions(program)
    served = {}
    for (entry, d), line in zip(cases, got):
        if d == dict(KNOBS, **dict(FACTS, m=d["m"])):
            first, second = (kv.split("=")[1] == "1,0" for kv in line.split()[:2])
            served[(entry, d["m"])] = ("grouped" if first else "decode" if second else "loop") if entry == "mm" else \
                ("fused" if first else "grouped" if second else "composition")
    assert [served[("mm", m)] for m in ROWS] == ["decode", "decode", "loop", "loop", "grouped", "grouped", "grouped", "grouped"]
    assert [served[("ffn", m)] for m in ROWS] == ["fused", "fused", "composition", "composition", "grouped", "grouped", "grouped", "grouped"]


def test_a_threshold_of_zero_or_below_turns_its_server_off(program):
    """MoeKnobs: gemv_rows / grouped_rows / ffn_grouped_rows <= 0 = never, whatever the row count"""
    cases, got = decisions(), run_decisions(program)
    seen = 0
    for (entry, d), line in zip(cases, got):
        first, second = (kv.split("=")[1].split(",")[0] for kv in line.split()[:2])      # tried?
        if entry == "mm":
            grouped, small = first, second
            off_g = d["grouped_rows"] <= 0
        else:
            small, grouped = first, second
            off_g = d["ffn_grouped_rows"] <= 0
        if off_g:
            assert grouped == "0", (entry, d)
            seen += 1
        if d["gemv_rows"] <= 0:
            assert small == "0", (entry, d)
            seen += 1
    assert seen >= 6 * len(ROWS)

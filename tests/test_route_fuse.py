"""The planner of the device route (neural-speed_amd/csrc/ns_route_fuse.cpp) decides what a token's launches are: the diff of two consecutive
tokens' traces, the fused launches of a plan or a window, the cut into segments.  A fusion that leaves out a tensor somebody still reads gives wrong
values, not a fault — so the file is compiled alone on the host (tests/tools/route_fuse_main.cpp, the library's compiler, nothing launched) and run on
traces of a 2-layer llama stack made of fake addresses.  The launch lists it must produce are written out here independently, from the rules in the
comment on ExecKind (ns_route_int.h); every list is also checked to be a partition of its trace.

Two of the rules are what the code does, not what one might expect: a rotation of kind ROPE_YARN keeps the K / V / Q group from being matched at all
(so no XK_ROPE2 is ever made for it), and a context length that stands still between the two tokens is accepted with delta 0 (it is verified every
token; a model with a fixed attention span replays that way)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "neural-speed_amd", "csrc")
MAIN = os.path.join(ROOT, "tests", "tools", "route_fuse_main.cpp")
GEMM, ADD, MUL, SILU, RMSNORM, ROPE, ROPE_YARN, DUP, MHA = range(1, 10)  # RouteKind
LAYER = [RMSNORM, MUL, GEMM, ROPE, DUP, GEMM, DUP, GEMM, ROPE, MHA, GEMM, ADD, RMSNORM, MUL, GEMM, SILU, GEMM, MUL, GEMM, ADD]
N1, M1, K, RK, DK, V, DV, Q, RQ, A, WO, AD1, N2, M2, W1, SI, W3, MU, W2, AD2 = range(20)  # a layer's ops, in the order the graph hands them over
SLOT_NORM16, SLOT_ATTN16, SLOT_FFN16 = 30, 31, 32
N_CASES = 47
TOKEN_SHIFT = 0x20000


def compiler():
    """HIPCC of the library's Makefile (the environment's HIPCC wins there too)"""
    with open(os.path.join(CSRC, "Makefile")) as f:
        default = re.search(r"^HIPCC\s*\?=\s*(\S+)", f.read(), re.M).group(1)
    path = os.environ.get("HIPCC", default)
    return path if os.path.exists(path) else shutil.which(path)


class X:
    """one launch"""

    def __init__(self, kind, idx, in_link=-1, out_link=-1, a16=-1, o16=-1, a16p=0, o16p=0, aux=-1):
        self.kind, self.idx = kind, list(idx) + [-1] * (10 - len(idx))
        self.in_link, self.out_link, self.a16, self.o16, self.a16p, self.o16p, self.aux = in_link, out_link, a16, o16, a16p, o16p, aux

    def key(self):
        return (self.kind, tuple(self.idx), self.in_link, self.out_link, self.a16, self.o16, self.a16p, self.o16p, self.aux)

    def __repr__(self):
        return repr(self.key())

    def owned(self):
        """the plan ops the launch stands for (a QKV_ROPE_M launch also NAMES the two cache writes, for the mirror's geometry: they stay a launch of their own)"""
        return [j for q, j in enumerate(self.idx) if j >= 0 and not (self.kind == "QKV_ROPE_M" and q in (7, 8))]


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    hipcc = compiler()
    if not hipcc:
        pytest.skip("the library's compiler is not installed")
    exe = str(tmp_path_factory.mktemp("route_fuse") / "route_fuse")
    subprocess.run([hipcc, "-std=c++20", "-x", "hip", "--offload-arch=gfx950", "--cuda-host-only", "-Wall", "-Werror", "-I", CSRC, MAIN, "-o", exe],
                   check=True, capture_output=True, text=True, timeout=300)
    run = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=120)
    out = {}
    for line in run.stdout.splitlines():
        tag, _, rest = line.partition(" ")
        if tag == "case":
            cur = out[rest] = dict(kinds=[], diff=None, plan=[], x=[], links=None, segs=[])
        elif tag == "k":
            cur["kinds"] = [int(v) for v in rest.split()]
        elif tag == "diff":
            f = rest.split(" ", 2)
            cur["diff"] = ("ok", int(f[1]), int(f[2])) if f[0] == "ok" else ("no", int(f[1]), f[2])
        elif tag == "p":
            cur["plan"].append(tuple(int(v) for v in rest.split()))
        elif tag == "x":
            f = rest.split()
            cur["x"].append(X(f[0], [int(v) for v in f[1].split(",")], *[int(v) for v in f[2:]]))
        elif tag == "links":
            cur["links"] = tuple(int(v) for v in rest.split())
        elif tag == "seg":
            cur["segs"].append(tuple(int(v) for v in rest.split()))
        else:
            raise AssertionError(line)
    out["stderr"] = run.stderr
    return out


def expected(layers=2, m=1, *, fuse=True, links=True, qkv_rope=True, append=True, mirror=True, k_first=False, group=True, k_f16=False, full_rotation=True,
             raw_wo_read=False, raw_w1_read=False, refused_w1=False, tail=(), prefill=True, scratch=(SLOT_NORM16, SLOT_ATTN16, SLOT_FFN16), qkv_rope_m=True,
             kv16=True):
    """the launches of the llama stack's trace, from the rules of the ExecKind comment.  m == 1: a plan (carried norms when `links`); m > 1: a window."""
    x, state = [], dict(links=0, shadows=0, first_rope=None)
    plan = m == 1 and links and fuse
    big = m > 16 and prefill and fuse

    def carry(norm, consumer, producer, consumer_ok=True):
        """rms_norm + mul in front of `consumer`: carried by `producer` (the mul_mat + add launch that wrote the normed tensor), or two launches"""
        src = producer and producer.src
        if plan and consumer_ok and producer and src and not (src.kind == "GATEUP" and src.in_link < 0):
            if src.o16 < 0:
                src.o16, state["shadows"] = state["shadows"], state["shadows"] + 1
            producer.out_link = consumer.in_link = state["links"]
            producer.a16 = src.o16
            consumer.idx[4], consumer.idx[5] = norm, norm + 1
            state["links"] += 1
        elif big and SLOT_NORM16 in scratch:
            x.append(X("NORM16", [norm, norm + 1], o16p=SLOT_NORM16))
            consumer.a16p = SLOT_NORM16
        else:
            x.extend([X("OP", [norm]), X("OP", [norm + 1])])

    def handover(producer_launch, consumer, slot):
        """a prompt-sized window: the attention's rows / the gate-up product as fp16 for the projection behind it"""
        if big and slot in scratch and (slot != SLOT_ATTN16 or kv16):
            producer_launch.o16p = consumer.a16p = slot

    residual = None  # the mul_mat + add launch that wrote the tensor the next norm reads
    for l in range(layers):
        b = 20 * l
        dup = lambda j, f16=False: X("OP" if f16 else "DUP2", [j])
        # ---- norm, K rope cpy, V cpy, Q rope ----
        if fuse and group:
            qkv = X("QKV", [b + K, b + Q, b + V] if k_first else [b + Q, b + K, b + V])
            carry(b + N1, qkv, residual)
            ropes = [b + RK, b + RQ] if k_first else [b + RQ, b + RK]
            if m == 1 and append and not k_f16:
                if qkv.in_link >= 0 and qkv_rope and kv16 and mirror and full_rotation:
                    qkv.kind, qkv.idx = "QKV_ROPE", [b + Q, b + K, b + V, b + RQ, qkv.idx[4], qkv.idx[5], b + RK, b + DK, b + DV, -1]
                    state["first_rope"] = b + RK if state["first_rope"] is None else state["first_rope"]
                    x.append(qkv)
                else:
                    x.extend([qkv, X("ROPE_APPEND", ropes + [b + DK, b + DV])])
            elif m == 1:
                x.extend([qkv, X("ROPE2", ropes), X("DUP2", [b + DK, b + DV])])
            elif big and kv16 and qkv_rope_m:
                qkv.kind, qkv.idx = "QKV_ROPE_M", [b + Q, b + K, b + V, b + RQ, -1, -1, b + RK, b + DK, b + DV, -1]
                x.extend([qkv, X("DUP2", [b + DK, b + DV])])
            else:
                x.extend([qkv, X("OP", [b + RK]), X("OP", [b + RQ]), X("DUP2", [b + DK, b + DV])])
        else:
            first = X("OP", [b + K])
            carry(b + N1, first, residual, consumer_ok=False)  # (the normed row has three readers: no single launch consumes it)
            x.extend([first, X("OP", [b + RK]), dup(b + DK, k_f16), X("OP", [b + V]), dup(b + DV), X("OP", [b + Q]), X("OP", [b + RQ])])
        # ---- attention, output projection + residual ----
        attn = X("OP", [b + A])
        x.append(attn)
        if fuse and not (raw_wo_read and l == 0):
            wo = X("GEMM_ADD", [b + WO, b + AD1])
            wo.src = attn
            handover(attn, wo, SLOT_ATTN16)
            x.append(wo)
        else:
            wo = None
            x.extend([X("OP", [b + WO]), X("OP", [b + AD1])])
        # ---- norm, gate / up ----
        if fuse and not (raw_w1_read and l == 0):
            gu = X("GATEUP", [b + W1, b + SI, b + W3, b + MU])
            carry(b + N2, gu, wo, consumer_ok=not (refused_w1 and l == 0))
            x.append(gu)
        else:
            gu = None
            first = X("OP", [b + W1])
            carry(b + N2, first, wo, consumer_ok=False)
            x.extend([first] + [X("OP", [b + j]) for j in (SI, W3, MU)])
        # ---- down projection + residual ----
        if fuse:
            residual = X("GEMM_ADD", [b + W2, b + AD2])
            residual.src = gu
            if gu:
                handover(gu, residual, SLOT_FFN16)
            x.append(residual)
        else:
            residual = None
            x.extend([X("OP", [b + W2]), X("OP", [b + AD2])])
    out = X("OP", [20 * layers + 2])
    carry(20 * layers, out, residual)
    x.append(out)
    x.extend(X("OP", [j]) for j in tail)
    if state["first_rope"] is not None:
        x.insert(0, X("ROPE_TABLE", [], aux=state["first_rope"]))
    return x, state


def check(case, want, n_links=None):
    got = case["x"]
    assert [g.key() for g in got] == [w.key() for w in want], "\n".join("%r\n%r" % (g, w) for g, w in zip(got, want) if g.key() != w.key())
    covered = sorted(j for g in got for j in g.owned())
    assert covered == list(range(len(case["kinds"]))), "the launches' plan ops are not a partition of the trace"
    if n_links is not None:
        assert case["links"][:2] == n_links


def test_every_case_ran_and_every_launch_list_is_a_partition_of_its_trace(cases):
    names = [n for n in cases if n != "stderr"]
    assert len(names) == N_CASES
    assert cases["decode_all"]["kinds"] == LAYER * 2 + [RMSNORM, MUL, GEMM]
    lists = 0
    for n in names:
        c = cases[n]
        if c["x"]:
            assert sorted(j for g in c["x"] for j in g.owned()) == list(range(len(c["kinds"]))), n
            lists += 1
    assert lists == N_CASES - 7  # (the seven cases that are about the token diff alone print no launches)


def test_decode_step_with_every_fusion_and_one_step_down_per_switch(cases):
    want, st = expected()
    kinds = [w.kind for w in want]
    assert kinds == ["ROPE_TABLE", "OP", "OP", "QKV", "ROPE_APPEND", "OP", "GEMM_ADD", "GATEUP", "GEMM_ADD", "QKV_ROPE", "OP", "GEMM_ADD", "GATEUP", "GEMM_ADD", "OP"]
    assert (want[5].o16, want[6].out_link, want[6].a16, want[7].in_link, want[7].o16, want[8].out_link, want[-1].in_link) == (0, 0, 0, 0, 1, 1, 3)
    check(cases["decode_all"], want, (4, 4))
    assert cases["decode_all"]["links"][3] % 256 == 0 and cases["decode_all"]["links"][2] >= cases["decode_all"]["links"][3] + 128 // 2 * 8
    check(cases["decode_links_off"], expected(links=False)[0], (0, 0))
    check(cases["decode_no_qkv_rope"], expected(qkv_rope=False)[0], (4, 4))
    check(cases["decode_no_rope_append"], expected(append=False)[0], (4, 4))
    check(cases["decode_no_fuse"], expected(fuse=False)[0], (0, 0))
    check(cases["decode_no_mirror"], expected(mirror=False)[0], (4, 4))
    check(cases["decode_kv16_off"], expected(kv16=False)[0], (4, 4))
    # each switch takes exactly its own step back
    count = lambda name, kind: sum(g.kind == kind for g in cases[name]["x"])
    assert count("decode_all", "QKV_ROPE") == 1 and count("decode_no_qkv_rope", "QKV_ROPE") == 0 and count("decode_no_qkv_rope", "ROPE_APPEND") == 2
    assert count("decode_no_rope_append", "ROPE2") == 2 and count("decode_no_rope_append", "DUP2") == 2 and count("decode_no_rope_append", "ROPE_APPEND") == 0
    assert count("decode_links_off", "GEMM_ADD") == 4 and count("decode_links_off", "GATEUP") == 2 and len(cases["decode_links_off"]["x"]) == 23
    assert {g.kind for g in cases["decode_no_fuse"]["x"]} == {"OP", "DUP2"} and len(cases["decode_no_fuse"]["x"]) == 43
    assert count("decode_no_mirror", "ROPE_TABLE") == 0 and count("decode_no_mirror", "ROPE_APPEND") == 2


def test_address_order_of_the_q_k_v_rows(cases):
    check(cases["order_k_first"], expected(k_first=True)[0], (4, 4))
    assert cases["order_k_first"]["x"][3].idx[:3] == [K, Q, V] and cases["order_k_first"]["x"][4].idx[:4] == [RK, RQ, DK, DV]
    for name in ("order_unequal", "order_ldc_small"):
        check(cases[name], expected(group=False)[0])
        assert not {"QKV", "QKV_ROPE", "ROPE2", "ROPE_APPEND"} & {g.kind for g in cases[name]["x"]}


def test_a_tensor_with_one_more_reader_is_not_left_out(cases):
    check(cases["reader_wo"], expected(raw_wo_read=True, tail=[43])[0])
    assert [g.kind for g in cases["reader_wo"]["x"] if g.idx[0] in (WO, AD1)] == ["OP", "OP"]
    check(cases["reader_gate"], expected(raw_w1_read=True, tail=[43])[0])
    assert [g.kind for g in cases["reader_gate"]["x"] if g.idx[0] in (W1, SI, W3, MU)] == ["OP"] * 4
    check(cases["reader_rewritten"], expected(tail=[43, 44])[0], (4, 4))  # rewritten before it is read again: the raw result may be left out
    check(cases["window_decode"], expected(links=False)[0])
    check(cases["window_copy_overlaps_1"], expected(links=False, raw_w1_read=True)[0])  # the copy that ends the window reads the raw result's last byte
    check(cases["window_copy_overlaps_0"], expected(links=False)[0])


def test_shapes_that_take_another_form(cases):
    check(cases["shape_gqa"], expected()[0], (4, 4))
    check(cases["shape_yarn"], expected(group=False)[0])  # (see the module's docstring)
    check(cases["shape_k_f16"], expected(k_f16=True)[0], (4, 4))
    assert [g.kind for g in cases["shape_k_f16"]["x"] if DK in g.idx[:2]] == ["DUP2"]
    check(cases["shape_k_f16_no_fuse"], expected(fuse=False, k_f16=True)[0])
    assert [g.kind for g in cases["shape_k_f16_no_fuse"]["x"] if g.idx[0] in (DK, DV)] == ["OP", "DUP2"]
    check(cases["shape_n_dims"], expected(full_rotation=False)[0], (4, 4))
    check(cases["shape_weight_refused"], expected(refused_w1=True)[0], (2, 2))
    assert [g.kind for g in cases["shape_weight_refused"]["x"] if g.idx[0] in (N2, M2)] == ["OP", "OP"]
    assert "route: the norm at launch 12 stays a launch: the consumer's mul_mat do not all read the normed row" in cases["stderr"]


def test_prompt_sized_windows(cases):
    check(cases["prompt_16"], expected(m=16)[0])
    assert not {"NORM16", "QKV_ROPE_M"} & {g.kind for g in cases["prompt_16"]["x"]} and all(g.a16p == g.o16p == 0 for g in cases["prompt_16"]["x"])
    want = expected(m=17)[0]
    assert [w.kind for w in want[:9]] == ["NORM16", "QKV_ROPE_M", "DUP2", "OP", "GEMM_ADD", "NORM16", "GATEUP", "GEMM_ADD", "NORM16"]
    assert [(w.a16p, w.o16p) for w in want[:8]] == [(0, 30), (30, 0), (0, 0), (0, 31), (31, 0), (0, 30), (30, 32), (32, 0)]
    check(cases["prompt_17"], want)
    check(cases["prompt_17_no_norm16_scratch"], expected(m=17, scratch=(SLOT_ATTN16, SLOT_FFN16))[0])
    check(cases["prompt_17_no_attn16_scratch"], expected(m=17, scratch=(SLOT_NORM16, SLOT_FFN16))[0])
    check(cases["prompt_17_no_ffn16_scratch"], expected(m=17, scratch=(SLOT_NORM16, SLOT_ATTN16))[0])
    for name in ("prompt_17_no_table_scratch", "prompt_17_no_mirror", "prompt_17_past_the_cache"):
        check(cases[name], expected(m=17, qkv_rope_m=False)[0])
    check(cases["prompt_17_no_prefill_fuse"], expected(m=17, prefill=False)[0])


def test_token_diff(cases):
    c = cases["decode_all"]
    assert c["diff"] == ("ok", TOKEN_SHIFT, 36)
    # per op: what moves (1 an integer, 2 the cache cell), by how much per token, which pointers are activations
    act = {GEMM: 0b101, ADD: 0b111, MUL: 0b101, SILU: 0b11, RMSNORM: 0b11, ROPE: 0b11, DUP: 0b01, MHA: 0b1001}
    for (j, moving, delta, pshift), kind in zip(c["plan"], c["kinds"]):
        want_shift = 0b111 if kind == MUL and j % 20 == MU and j < 40 else act[kind]  # (gamma is a weight; the gate * up multiply has two activations)
        want = {ROPE: (1, 1), MHA: (1, 1), DUP: (2, 128 * 4 if j % 20 == DK else 4)}.get(kind, (0, 0))
        assert (moving, delta, pshift) == want + (want_shift,), j
    assert len(c["plan"]) == 43
    assert cases["diff_two_shifts"]["diff"] == ("no", 25, "pointers shifted by different amounts")
    assert cases["diff_field"]["diff"] == ("no", 22, "a field other than the moving one differs")
    assert cases["diff_mha_rows"]["diff"] == ("no", A, "an attention over more than one row")
    assert cases["diff_foreign_write"]["diff"] == ("no", 20 + AD2, "an operator other than a cache write stores into a mirrored kv cache")
    assert cases["diff_length"]["diff"] == ("no", -1, "the two tokens have different numbers of ops (or none)")
    assert cases["diff_kind"]["diff"] == ("no", AD1, "another operator")
    # a context length that stands still: still the moving field, delta 0 (see the module's docstring)
    still = cases["diff_seq_all_still"]
    assert still["diff"][0] == "ok" and [p[1:3] for p in still["plan"] if still["kinds"][p[0]] == MHA] == [(1, 0), (1, 0)]
    assert [p[1:3] for p in still["plan"] if still["kinds"][p[0]] == ROPE] == [(1, 1)] * 4


@pytest.mark.parametrize("seg,seg0", [(64, 16), (12, 6), (1, 1)])
def test_segments(cases, seg, seg0):
    for name, n_min in (("seg_small", 15), ("seg_long", 190), ("seg_long_links", 190)):
        c = cases["%s_%d_%d" % (name, seg, seg0)] if name != "seg_long_links" else cases["seg_long_%d_%d_links" % (seg, seg0)]
        x, segs, n = c["x"], c["segs"], len(c["kinds"])
        assert len(x) >= n_min and segs
        # consecutive, covering every launch and every op
        assert segs[0][0] == 0 and segs[0][2] == 0 and segs[-1][1] == n and segs[-1][3] == len(x)
        assert all(a[1] == b[0] and a[3] == b[2] for a, b in zip(segs, segs[1:]))
        for beg, end, xbeg, xend in segs:
            assert beg < end and xbeg < xend
            # the launches up to the segment's end stand for exactly the reference's first `end` ops
            assert sorted(j for g in x[:xend] for j in g.owned()) == list(range(end))
            last = x[xend - 1]
            assert xend == len(x) or not (last.kind == "OP" and c["kinds"][last.idx[0]] in (RMSNORM, SILU))
        lens = [s[3] - s[2] for s in segs]
        if len(x) >= seg0 + seg // 3:
            assert lens[0] >= seg0 and all(v >= seg for v in lens[1:-1])
            assert len(segs) == 1 or lens[-1] >= seg // 3
        else:
            assert len(segs) == 1
    if seg == 1:
        assert len(cases["seg_long_1_1"]["segs"]) > 100

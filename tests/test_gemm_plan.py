"""gemm_plan (neural-speed_amd/csrc/ns_gemm_plan.cpp) is the one place that decides how a prefill GEMM is launched: kernel generation, tile
form, epilogue form, K split, grid, LDS, the fp16 conversion pass.  A host program (tests/tools/gemm_plan_main.cpp, built with the library's
compiler, nothing launched) prints the plan for a grid of calls; the rule it must follow — docs/kernels/gemm3.md, gemm2.md and the comments
of ns_gemm.h — is written out here independently, as a table of envelopes first and the arithmetic after it."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "neural-speed_amd", "csrc")
MAIN = os.path.join(ROOT, "tests", "tools", "gemm_plan_main.cpp")
INT4, INT8, F4, F8 = 0, 1, 2, 3
# the program's formats: kind, scales per k-step record, bytes per scale, zero points, usable on the tiled kernel (fp8: the load's range rule,
# fp32 scales)
FORMATS = [dict(kind=INT4, sps=4, sb=2, asym=0, f8_ok=1), dict(kind=INT4, sps=1, sb=4, asym=1, f8_ok=1), dict(kind=INT8, sps=2, sb=2, asym=0, f8_ok=1),
           dict(kind=F4, sps=2, sb=2, asym=0, f8_ok=1), dict(kind=F8, sps=2, sb=4, asym=0, f8_ok=1), dict(kind=F8, sps=2, sb=4, asym=0, f8_ok=0),
           dict(kind=F8, sps=2, sb=2, asym=0, f8_ok=0)]
DEFAULTS = dict(v1=0, gemm3=1, g3_min_m=2, g3_bm=0, g3_wide=0, g3_f8=1, no_splitk=0, no_partials=0, diag=0)
LDS_LIMIT = 160 * 1024


def compiler():
    """HIPCC of the library's Makefile (the environment's HIPCC wins there too)"""
    with open(os.path.join(CSRC, "Makefile")) as f:
        default = re.search(r"^HIPCC\s*\?=\s*(\S+)", f.read(), re.M).group(1)
    path = os.environ.get("HIPCC", default)
    return path if os.path.exists(path) else shutil.which(path)


def num(v):
    try:
        return int(v)
    except ValueError:
        try:
            return float(v)
        except ValueError:
            return v


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    hipcc = compiler()
    if not hipcc:
        pytest.skip("the library's compiler is not installed")
    exe = str(tmp_path_factory.mktemp("gemm_plan") / "gemm_plan")
    subprocess.run([hipcc, "-std=c++20", "-x", "hip", "--offload-arch=gfx950", "--cuda-host-only", "-Wall", "-Werror", "-I", CSRC, MAIN, "-o", exe],
                   check=True, capture_output=True, text=True, timeout=300)
    out = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=120).stdout
    rows = []
    for line in out.splitlines():
        call, plan = line.split(" | ")
        plan, why = plan.split(" why=")
        i = {k: num(v) for k, v in (kv.split("=") for kv in call.split())}
        o = {k: num(v) for k, v in (kv.split("=") for kv in plan.split())}
        o["why"] = why
        rows.append((i, o))
    return rows


def ceil_div(a, b):
    return -(-a // b)


def knobs_of(i):
    kn = dict(DEFAULTS)
    if i["knob"] != "none":
        kn[i["knob"]] = i["kval"]
    return kn


def matrices(i):
    """(columns of every matrix, head size, kv heads' columns) of the call as the program builds it"""
    rope = i["form"] in (5, 8)
    nq, nk, hs = i["n"], i["nkv"] or i["n"], i["hs"]
    nv = nk
    nseg = {0: 1, 8: 1, 2: 2, 7: 2}.get(i["form"], 3)
    b = i["brk"] if rope else 0
    if b == 1:
        nseg = 2
    hs = {3: 16, 4: 256, 6: 2, 7: 6}.get(b, hs)
    if b == 7:
        nq, nk, nv = 768, 384, 384
    if b == 12:
        nk *= 2
    if b == 29:
        nv *= 2
    if b == 13:
        nq += 64
    if b == 14:
        nk, nv = nk + 64, nv + 64
    if i["form"] == 7:
        nk = nq
        if i["brk"] == 1:
            nseg = 3
    if i["mis"] == 12:  # (the second matrix 16 columns wider: no mismatch for a fused QKV)
        nk += 16
    return [nq, nk, nv][:nseg], hs, (nv if b == 12 else nk)


def rope_ok(i, ns, hs, kv_cols):
    """the QKV + RoPE + kv-append epilogue's envelope (docs/kernels/gemm3.md, round 5): three matrices; whole-head RoPE in the mode the flag
    names; NeoX heads inside one 128-column block; heads of a multiple of 4 columns; cache, table and position present; widths = heads x head
    size and q / k whole 128-column blocks; 16-byte fp32 rows and stores, 8-byte cache stores; an fp32 q output; no fp16 shadow; no operator"""
    b, neox = i["brk"], i["neox"]
    if len(ns) != 3 or b in (2, 5, 8, 9, 10, 11, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 30):
        return False
    if i["out"] != 0:  # the program's out = 1 / 2 set fp16 shadows, 3 takes q's fp32 output away
        return False
    if neox and not (hs >= 32 and 128 % hs == 0):
        return False
    if hs < 4 or hs % 4:
        return False
    heads, heads_kv = ns[0] // hs, kv_cols // hs
    return ns[0] == heads * hs and ns[1] == heads_kv * hs and ns[2] == heads_kv * hs and ns[0] % 128 == 0 and ns[1] % 128 == 0


def expected(i):
    """None, "NOTSUP" / "INVAL", or the plan's fields"""
    kn, f = knobs_of(i), FORMATS[i["fmt"]]
    m, k, form, out = i["m"], i["k"], i["form"], i["out"]
    ns, hs, kv_cols = matrices(i)
    eight = f["kind"] in (INT8, F8)
    has_c, has_c16 = out in (0, 1), out in (1, 2)
    if form == 5 and i["brk"] == 21:
        has_c = False
    if kn["v1"]:
        return "NOTSUP"
    # ---- fp8: only weights the range rule passed, with "g3_f8" on; from 17 rows, a plain call (fp32 in, fp32 out, one matrix) from 65
    if f["kind"] == F8:
        plain = form == 0 and i["act"] != 4 and has_c
        if not (f["f8_ok"] and kn["g3_f8"] and kn["gemm3"] == 1 and m >= 17 and not (plain and m <= 64)):
            return "NOTSUP"
    # ---- activations: the caller's fp16 copy if it can be read by 16-byte DMA in whole 64-deep chunks, else one conversion pass
    nchunks = ceil_div(k, 64)
    kpad = nchunks * 64
    shadow = i["act"] in (1, 4) and k % 64 == 0  # (2: misaligned, 3: lda % 8 != 0)
    if not shadow and i["act"] == 4:
        return "NOTSUP"
    lda16 = k if shadow else kpad
    if m * lda16 * 2 >= 1 << 32:
        return "NOTSUP"
    e = dict(convert=int(not shadow), cvt_bytes=0 if shadow else m * kpad * 2, kpad=kpad, lda16=lda16, a16=int(shadow), nchunks=nchunks, pm=m, pk=k,
             pn=ns[0], part=0, diag=kn["diag"], smul=1, sshift=0, dual=0, tall=0, nseg=0, rope=0, ksplit=1, cps=nchunks, part_bytes=0,
             c=int(has_c), c16=int(has_c16), pkind=f["kind"], psps=f["sps"], pasym=f["asym"], codes2=0, c2=0)
    fused_ok = kn["gemm3"] == 1 and m >= kn["g3_min_m"]
    # ---- gate/up pairs: two matrices of one shape and format, no operand; a column block is 4 tile pairs; always the cross-wave epilogue
    if form == 7:
        if i["brk"] or not fused_ok or i["mis"]:
            return "NOTSUP"
        if not has_c and not has_c16:
            return "INVAL"
        nbn = ceil_div(ceil_div(ns[0], 16), 4)
        bm = 64 if m <= 64 else 128
        e.update(dual=1, wide=1, bm=bm, nbn=nbn, codes2=1, c2=1)
    else:
        nbn = sum(ceil_div(ceil_div(n, 16), 8) for n in ns)
        if len(ns) > 1 or form in (2, 3, 5):
            # ---- fused QKV: two or three matrices of one K and format (widths may differ), whole column blocks each
            if not fused_ok or (i["mis"] and i["mis"] <= 11):
                return "NOTSUP"
            if form == 5 and not rope_ok(i, ns, hs, kv_cols):
                return "NOTSUP"
            bn0, acc = [0, 0, 0], 0
            for s, n in enumerate(ns):
                bn0[s], acc = acc, acc + ceil_div(ceil_div(n, 16), 8)
            e.update(nseg=len(ns), bn0=",".join(map(str, bn0)), rope=(2 if i["neox"] else 1) if form == 5 else 0)
        elif form == 8:
            return "NOTSUP"
        e.update(nbn=nbn)
        if kn["gemm3"] != 0 and m >= kn["g3_min_m"]:
            # ---- gemm3_kernel.  Tile: on request; else 64 rows up to 64 rows, 256 when the output has >= 1024 tiles of 256 rows (not for 8-bit codes), else 128
            req = kn["g3_bm"]
            tall = int(req == 257 and f["kind"] == INT4)
            bm = 256 if tall else req if req in (64, 128, 256) else 64 if m <= 64 else 256 if nbn * ceil_div(m, 256) >= 1024 and not eight else 128
            f16_only = not has_c and e["nseg"] <= 1
            if f16_only:
                if not has_c16:
                    return "INVAL"
                if bm == 256 and not tall:
                    bm = 128
            wide = int((bm != 256 or tall) and not e["rope"] and (kn["g3_wide"] != 0 or f16_only))
            e.update(bm=bm, tall=tall, wide=wide)
            ks = 1
            while ks < 8 and nbn * ceil_div(m, bm) * ks * 2 <= 512 and nchunks // (ks * 2) >= 8:
                ks *= 2
            if ks > 1 and not kn["no_splitk"] and not kn["no_partials"] and e["nseg"] <= 1 and has_c:
                cps = ceil_div(nchunks, ks)
                e.update(ksplit=ks, cps=cps + (cps & 1), part_bytes=ks * m * ns[0] * 4)
        else:
            # ---- gemm2_kernel: single matrices of the integer / f4 formats with an fp32 output; 128-row tiles; fills 256 workgroups
            if e["rope"] or f["kind"] == F8:
                return "NOTSUP"
            if not has_c:
                return "NOTSUP" if has_c16 else "INVAL"
            nbm = ceil_div(m, 128)
            ks = 1
            while ks < 8 and nbn * nbm * ks * 2 <= 256 and nchunks // (ks * 2) >= 8:
                ks *= 2
            if ks > 1 and not kn["no_splitk"] and not kn["no_partials"]:
                e.update(ksplit=ks, cps=ceil_div(nchunks, ks), part_bytes=ks * m * ns[0] * 4)
            cpx = ceil_div(nbn, 8)
            e.update(kernel="GEMM2", cpx=cpx, grid="%d,%d,1" % (8 * cpx * nbm, e["ksplit"]), lds=2 * (128 * 72 * 2 + 8 * 2 * 64 * 16))
            return e
    cpx = ceil_div(e["nbn"], 8)
    e.update(kernel="GEMM3", cpx=cpx, grid="%d,%d,1" % (8 * cpx * ceil_div(m, e["bm"]), e["ksplit"]), lds=gemm3_lds(f, e["bm"], e["tall"], e["wide"]))
    return e


def gemm3_lds(f, bm, tall, wide):
    """two A stages of [bm][64] halves + one B stage (records, scale rows, zero-point rows of 8 column tiles for a 128-deep superstep); the
    epilogue parks over it: per wave 64 rows of (wave columns + 4) floats, the cross-wave form 64 rows of 128 + 4"""
    rps = 2 if f["kind"] in (INT8, F8) else 1
    stages = 2 * bm * 64 * 2 + 8 * rps * (1024 + 16 * f["sps"] * f["sb"] + (16 * f["sps"] if f["asym"] else 0))
    square = bm == 256 and not tall
    park = 4 * 64 * ((64 if square else 32) + 4) * 4
    if wide:
        assert not square
        park = max(park, 64 * (128 + 4) * 4)
    return max(stages, park)


def test_plan_follows_the_rule(plans):
    assert len(plans) > 5000
    bad = []
    for i, o in plans:
        e = expected(i)
        if isinstance(e, str):
            if o["kernel"] != "REFUSED" or o["err"] != e:
                bad.append((i, o, e))
            continue
        if o["kernel"] == "REFUSED":
            bad.append((i, o, e))
            continue
        diff = {k: (o.get(k), v) for k, v in e.items() if o.get(k) != v}
        if diff:
            bad.append((i, diff))
    assert not bad, "%d of %d plans differ, first: %r" % (len(bad), len(plans), bad[:3])


def test_every_envelope_is_exercised(plans):
    """the grid reaches both kernels, both refusal codes, every tile form, split K on both kernels, the conversion pass and every fused form"""
    acc = [o for _, o in plans if o["kernel"] != "REFUSED"]
    assert {o["kernel"] for o in acc} == {"GEMM2", "GEMM3"}
    assert {o["err"] for _, o in plans if o["kernel"] == "REFUSED"} == {"NOTSUP", "INVAL"}
    assert {(o["bm"], o["tall"], o["dual"]) for o in acc if o["kernel"] == "GEMM3"} == {(64, 0, 0), (128, 0, 0), (256, 0, 0), (256, 1, 0), (64, 0, 1), (128, 0, 1)}
    assert {o["ksplit"] for o in acc if o["kernel"] == "GEMM3"} == {1, 2, 4, 8} and {o["ksplit"] for o in acc if o["kernel"] == "GEMM2"} >= {1, 2}
    assert {o["convert"] for o in acc} == {0, 1} and {o["rope"] for o in acc} == {0, 1, 2} and {o["nseg"] for o in acc} == {0, 2, 3}
    assert any(i["m"] == 524288 and o["kernel"] == "REFUSED" for i, o in plans) and any(i["m"] == 524287 and o["kernel"] == "GEMM3" for i, o in plans)


def test_invariants_of_accepted_plans(plans):
    for i, o in plans:
        if o["kernel"] == "REFUSED":
            continue
        assert o["err"] == "OK" and o["part"] == 0, (i, o)
        assert 8 * o["cpx"] >= o["nbn"], (i, o)
        assert o["cps"] * o["ksplit"] >= o["nchunks"], (i, o)
        if o["kernel"] == "GEMM3":
            assert o["ksplit"] == 1 or o["cps"] % 2 == 0, (i, o)
            assert o["lds"] == o["ldsf"], (i, o)
        assert o["lds"] <= LDS_LIMIT, (i, o)
        assert o["part_bytes"] == (o["ksplit"] * o["pm"] * o["pn"] * 4 if o["ksplit"] > 1 else 0), (i, o)
        if not o["c"] or o["nseg"] > 1:
            assert o["ksplit"] == 1, (i, o)
        assert o["convert"] != o["a16"] and (o["lda16"] % 8 == 0), (i, o)  # what the kernels' 16-byte DMA of A relies on
        assert o["pm"] * o["lda16"] * 2 < 1 << 32, (i, o)

"""gemvs_plan (neural-speed_amd/csrc/ns_gemvs_plan.cpp) and gemv_plan (ns_gemv_plan.cpp) decide every launch of a generated token: which of the
two weight-streaming kernels serves a call, in which decomposition, with which LDS layout, or with which of three refusals.  A host program
(tests/tools/stream_plan_main.cpp, built with the library's compiler, nothing launched) prints both plans for a grid of calls; the rule they
must follow — docs/kernels/gemvs.md, gemv.md and the comments of ns_gemvs.h / ns_gemv.h — is written out here independently and compared
with EVERY line.  The last part of the grid is the group-size ladder of tests/test_gpu_group_sizes.py at that module's own shapes."""
import os
import re
import shutil
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "neural-speed_amd", "csrc")
MAIN = os.path.join(ROOT, "tests", "tools", "stream_plan_main.cpp")
INT4, INT8, F4, F8 = 0, 1, 2, 3
F32, F16, BF16 = 32, 16, 16 | (1 << 16)
# the program's formats: kind, scales per k-step record, scale type, zero points; 5 .. 7 are format 0 with a native bit-plane clone
FORMATS = [dict(kind=INT4, sps=4, sdt=BF16, asym=0), dict(kind=INT4, sps=1, sdt=F32, asym=1), dict(kind=INT8, sps=2, sdt=BF16, asym=0),
           dict(kind=F4, sps=2, sdt=F16, asym=0), dict(kind=F8, sps=2, sdt=F32, asym=0)]
LDS_LIMIT = 160 * 1024
ABSENT = 0xFFFFFFFF
GS_PF, GV_PF, GS_R, GS_CTL, GS_TABLE = 2, 4, 2, 32, 32 * 1024


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


def parse(out):
    rows = []
    for line in out.splitlines():
        call, plan = line.split(" | ")
        plan, why = plan.split(" why=")
        i = {k: num(v) for k, v in (kv.split("=") for kv in call.split())}
        o = {k: num(v) for k, v in (kv.split("=") for kv in plan.split())}
        o["why"] = why
        rows.append((i, o))
    return rows


def build(hipcc, exe, extra=()):
    subprocess.run([hipcc, "-std=c++20", "-x", "hip", "--offload-arch=gfx950", "--cuda-host-only", "-Wall", "-Werror", *extra, "-I", CSRC, MAIN, "-o", exe],
                   check=True, capture_output=True, text=True, timeout=600)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    hipcc = compiler()
    if not hipcc:
        pytest.skip("the library's compiler is not installed")
    d = tmp_path_factory.mktemp("stream_plan")
    exe = str(d / "stream_plan")
    build(hipcc, exe)
    return hipcc, str(d), subprocess.run([exe], check=True, capture_output=True, text=True, timeout=120).stdout


@pytest.fixture(scope="module")
def plans(program):
    return parse(program[2])


def ceil_div(a, b):
    return -(-a // b)


def up(a, b):
    return ceil_div(a, b) * b


# ---- the call as the program builds it -------------------------------------------------------------------------------------------------------
class Matrix:
    """one weight of the program: an allocation of codes | scales | zero points, [tile][k-step] records of 1024 bytes"""

    def __init__(self, fmt, n, k, grp=0):
        f = FORMATS[0 if fmt >= 5 else fmt]
        self.kind, self.sps, self.sdt, self.asym = f["kind"], f["sps"], f["sdt"], f["asym"]
        if grp:  # a group of whole k-steps, or one over K (-1): one scale per record, a scale row per group
            self.sps = 1
        self.n, self.k = n, k
        self.kstep = 64 if self.kind in (INT8, F8) else 128
        self.ks, self.tiles = ceil_div(k, self.kstep), ceil_div(n, 16)
        self.blocksize, self.srows = self.kstep // self.sps, self.ks
        if grp:
            self.blocksize, self.srows = (self.ks * self.kstep, 1) if grp < 0 else (grp, ceil_div(k, grp))
        sbytes = self.sps * (4 if self.sdt == F32 else 2)
        self.qstride, self.sstride, self.zstride = 1024, 16 * sbytes, 16 * self.sps if self.asym else 0
        self.soff = self.tiles * self.ks * 1024
        self.zoff = self.soff + self.tiles * self.srows * self.sstride if self.asym else 0
        self.slot = 1024 + 16 * sbytes + (16 * self.sps if self.asym else 0)  # a ring slot: the record, its scales, its zero points
        self.pl_bits, self.pl_lanes, self.qtype_differs = 0, 64, False

    def clone(self, bits, f16):
        """the native bit-plane layout: records of 256 x bits bytes with the scales behind them in the same stream"""
        self.pl_bits, self.rec, self.clone_f16 = bits, 256 * bits, f16

    def stream_clone(self):
        self.pl_lanes = self.rec // 16
        self.qstride = self.sstride = self.rec + self.sstride
        self.soff = self.rec


def matrices(i):
    form, nkv = i["form"], i["nkv"]
    nseg = {0: 1, 1: 2}.get(form, form)
    nq = i["n"] + 16 if i["rope"] and i["rbrk"] == 4 else i["n"]
    nk = nkv if form >= 2 and nkv else i["n"]
    ms = [Matrix(i["fmt"], 0 if i["spec"] == 4 else nq, i["k"], i["grp"]), Matrix(i["fmt"], nk, i["k"], i["grp"]), Matrix(i["fmt"], nk, i["k"], i["grp"])]
    if i["fmt"] >= 5:
        for j, w in enumerate(ms):
            w.clone(2 if i["fmt"] == 7 and j == 1 else 3, i["fmt"] == 6)
    if i["mis"] == 12:  # (after the arrays were laid out: the offsets stay)
        ms[1].n, ms[1].tiles = ms[1].n + 16, ms[1].tiles + 1
    if i["mis"] == 14:
        ms[1].n += 1
    if i["spec"] == 1:
        for w in ms:
            w.blocksize, w.srows = 1000 * w.kstep, ceil_div(w.ks, 1000)
    if i["spec"] == 5:
        nseg = 3
    return ms[:nseg], nq, nk


def second_matrix_differs(i, nseg, dual, expert_pair=False):
    """the program's `mis`: one field of the second matrix changed.  1 .. 11 are format and record-layout fields; 12 a tile more (gate/up pairs
    need equal widths); 13 the code type and 14 a column more, which only expert pairs compare"""
    mis = i["mis"]
    if nseg < 2 or not mis:
        return False
    return mis <= 11 or (mis == 12 and (dual or expert_pair)) or (mis in (13, 14) and expert_pair)


def scale_row(w):
    """scale row of k-step s as (s * mul) >> shift: one row (0, 0), a row per k-step (1, 0), a block of 2^j k-steps (1, j); any other
    ratio by a 20-bit reciprocal that must be exact for every k-step, else None"""
    if w.blocksize >= w.k:
        return 0, 0
    if w.sps > 1 or w.blocksize == w.kstep:
        return 1, 0
    ratio = w.blocksize // w.kstep
    if ratio & (ratio - 1) == 0:
        return 1, ratio.bit_length() - 1
    mul = ceil_div(1 << 20, ratio)
    return (mul, 20) if all((s * mul) >> 20 == s // ratio for s in range(w.ks)) else None


def activation_lda(i):
    return {3: i["k"] + 4, 5: i["k"] + 2, 6: 1 << 24}.get(i["act"], i["k"])


def mat_fields(e, ms, tbeg):
    for j in range(3):
        on = j < len(ms)
        e.update({"mn%d" % j: ms[j].n if on else 0, "mtb%d" % j: tbeg[j] if on else 0, "mc%d" % j: int(on), "mc16_%d" % j: int(on and j == 0)})


# ---- gemvs_kernel ----------------------------------------------------------------------------------------------------------------------------
def gemvs_candidate(S, tiles, ks, kstep, rows, nq, f4, slot, max_wg, kn):
    """S slices of ksl k-steps, tile groups = workgroups / S, the most streaming waves (<= 15, <= the workgroup's records) whose rings fit
    LDS beside [f4 pair table | A | control | 2 reduction slots]; cost in bytes a workgroup moves"""
    if S > ks or S > max_wg:
        return None
    ksl = ceil_div(ks, S)
    if ksl * (S - 1) >= ks:
        return None
    row_stride = ksl * kstep + 8
    a_bytes = up(rows * row_stride * 2, 16)
    tg = min(tiles, max_wg // S)
    if tg < 1:
        return None
    tiles_max = ceil_div(tiles, tg)
    table = bool(f4 and kn["tb"] != 0 and (kn["tb"] > 0 or tiles_max * ksl * nq >= 96))
    red_wave = nq * ceil_div(rows, 4) * 256
    for ns in range(15, 0, -1):
        if kn["wv"] > 0:
            if ns != min(kn["wv"], 15):
                continue
        elif ns > max(1, ksl * tiles_max):
            continue
        ring = up(min(ceil_div(ksl * tiles_max, ns) * nq, GS_PF) * slot, 16)
        a_off = GS_TABLE if table else 0
        ctl = a_off + a_bytes
        red = ctl + GS_CTL
        rings = red + GS_R * ns * red_wave
        lds = rings + ns * ring
        if lds <= LDS_LIMIT:
            break
    else:
        return None
    t = float(ksl) * (1.0 + 0.5 * max(0, 12 - ns) / 12.0)
    cost = float(tiles_max) * (t * nq * slot + 8e3) + 0.5 * float(a_bytes) + (75e3 if S > 1 else 0.0)
    return dict(S=S, ksl=ksl, rstride=row_stride, abytes=a_bytes, tg=tg, table=table, redw=red_wave, ns=ns, rings=ring, aoff=a_off, ctl=ctl, red=red,
                ring=rings, lds=lds, cost=cost)


def shape_clauses(i, ms):
    """the four reasons for which a call goes to gemvs_kernel by shape (docs/kernels/gemvs.md): activations beyond gemv_kernel's 64 KiB; f4
    codes on a wide launch (gate/up, or >= 512 tiles); five rows on a wide launch; nine rows"""
    w, dual = ms[0], i["form"] == 1
    tiles = w.tiles if dual else sum(x.tiles for x in ms)
    wide = dual or tiles >= 512
    return (i["m"] * (w.ks * w.kstep + 8) * 2 > 64 * 1024, w.kind == F4 and wide, i["m"] >= 5 and wide, i["m"] >= 9)


def gemvs_expected(i):
    ms, nq_cols, _ = matrices(i)
    nseg, dual, m, k, w = len(ms), i["form"] == 1, i["m"], i["k"], ms[0]
    if i["gvs"] == 0 or m < (1 if i["gvs"] == 2 else 2) or m > 16:
        return "NOTSUP"
    if i["feat"] or i["spec"] == 5:  # the other kernel's features; a gate/up pair is two matrices
        return "NOTSUP"
    shadow = i["act"] in (1, 2, 3)
    if (shadow and i["act"] != 1) or i["act"] == 4:  # a shadow must have 16-byte rows; no activations at all
        return "NOTSUP"
    if k % 8 or (m > 1 and k % w.kstep):
        return "NOTSUP"
    lda = activation_lda(i) if shadow else k
    if m * lda * 2 >= 1 << 30:
        return "NOTSUP"
    if i["spec"] in (2, 3) or second_matrix_differs(i, nseg, dual):
        return "NOTSUP"
    tiles = w.tiles if dual else sum(x.tiles for x in ms)
    if tiles == 0:
        return "NOTSUP"
    srow = scale_row(w)
    if srow is None:
        return "NOTSUP"
    if i["gvs"] == 1 and not any(shape_clauses(i, ms)):
        return "NOTSUP"
    nq = 2 if dual else 1
    max_wg = i["gr"] if i["gr"] > 0 else i["cus"]
    best = None
    for S in (1, 2, 4, 8, 16, 32):
        if i["sl"] > 0 and S != i["sl"]:
            continue
        c = gemvs_candidate(S, tiles, w.ks, w.kstep, m, nq, w.kind == F4, w.slot, max_wg, i)
        if c and (best is None or c["cost"] < best["cost"]):  # ties: the fewer slices
            best = c
    if best is None:
        return "NOTSUP"
    S = best["S"]
    slab = S * tiles * nq * 1024
    if S > 1 and slab >= 1 << 31:
        return "NOTSUP"
    mseg = not dual and nseg > 1
    tbeg = [0, 0, 0] if dual else [0, ms[0].tiles, ms[0].tiles + (ms[1].tiles if nseg > 1 else 0)]
    on = lambda j: j < nseg
    e = dict(kind=w.kind, sps=w.sps, sdt=w.sdt, asym=w.asym, mode=1 if dual else 2 if mseg else 0, grid=best["tg"] * S, nwaves=best["ns"] + 1, lds=best["lds"],
             convert=int(not shadow), cvt_bytes=0 if shadow else m * k * 2, slab_bytes=slab if S > 1 else 0,
             tickets=int(S > 1 and not i["fin"] and tiles <= 65536), tblimg=int(best["table"] and i["dma"] != 0), cost=best["cost"],
             so=",".join(str(ms[j].soff if on(j) else 0) for j in range(3)), zo=",".join(str(ms[j].zoff if on(j) else 0) for j in range(3)),
             wb=",".join(str(int(on(j))) for j in range(3)), a=int(shadow), ks=w.ks, ksl=best["ksl"], slog=S.bit_length() - 1, qstride=1024, sstride=w.sstride,
             zstride=w.zstride, srows=w.srows, smul=srow[0], sshift=srow[1], tb1=tbeg[1] if mseg else ABSENT, tb2=tbeg[2] if mseg and nseg > 2 else ABSENT,
             ntiles=tiles, tg=best["tg"], tbase=tiles // best["tg"], trem=tiles % best["tg"], ns=best["ns"], pm=m, pk=k, lda=lda, rstride=best["rstride"],
             ctl=best["ctl"], red=best["red"], ring=best["ring"], rings=best["rings"], redw=best["redw"], reds=best["ns"] * best["redw"], aoff=best["aoff"],
             abytes=best["abytes"], lut0=0xC700C800 if w.kind == F4 else 0, lut7=0x47004600 if w.kind == F4 else 0, owned=0, c2=int(dual), d=int(not dual),
             ldc=nq_cols, ldd=0 if dual else nq_cols + 32, epi=5 if dual else 1, pslab=slab & 0xFFFFFFFF, f8=0x20002000, fs=S, fnt=tiles, fnq=nq,
             fm=m, fn=",".join(str(ms[j].n if on(j) else 0) for j in range(3)), why="-")
    e.update(ftb1=e["tb1"], ftb2=e["tb2"], fc2=e["c2"], fd=e["d"], fldc=e["ldc"], fldd=e["ldd"], fepi=e["epi"])
    mat_fields(e, ms, tbeg)
    return e


# ---- gemv_kernel -----------------------------------------------------------------------------------------------------------------------------
def decode_waves(tiles, ks, dual, forced):
    """docs/kernels/gemv.md: 8 waves; 16 for up to 320 tiles of 32 .. 48 k-steps; halved while half the waves still put 2560 on the chip (not
    below 2); gate/up pairs 4 from 325 tile pairs; a forced 2 / 4 / 8 (16: single matrices) overrides; never more waves than k-steps"""
    if dual:
        nw = 4 if tiles * 4 >= 1300 else 8
    else:
        nw = 16 if tiles <= 320 and 32 <= ks <= 48 else 8
        while nw > 2 and tiles * (nw // 2) >= 2560:
            nw //= 2
    if forced in (2, 4, 8) or (forced == 16 and not dual):
        nw = forced
    while nw > 1 and nw > ks:
        nw //= 2
    return nw


def gemv_expected(i):
    ms, nq_cols, nk_cols = matrices(i)
    nseg, dual, m, k = len(ms), i["form"] == 1, i["m"], i["k"]
    rope, neox, i8, moe, link = i["rope"] != 0, i["rope"] == 2, i["i8"] != 0, i["moe"] != 0, i["link"]
    if i["gemv2"] == 0 or m < 1 or m > 16:
        return "NOTSUP"
    # native bit-plane records: every matrix has a clone of one bit width whose scales are not fp16; not for int8 numerics, experts, NeoX pairs
    planes = bool(i["planes"] and not i8 and not moe and not neox and i["fmt"] >= 5 and i["fmt"] != 6 and len({x.pl_bits for x in ms}) == 1)
    if planes:
        for x in ms:
            x.stream_clone()
    w = ms[0]
    if i["spec"] in (2, 3) and not planes:
        return "NOTSUP"
    mseg = not dual and nseg > 1
    if neox:  # a workgroup per pair of tiles: three matrices of whole heads, heads of whole 32-column pairs
        if not mseg or nseg != 3 or i["rbrk"] == 1 or i["hs"] < 32 or i["hs"] % 32:
            return "INVAL"
        if any(x.n % i["hs"] or x.n != 16 * x.tiles for x in ms):
            return "INVAL"
    tiles = w.tiles if dual else sum(x.tiles for x in ms)
    if tiles == 0:
        return "NOTSUP"
    srow = scale_row(w)
    if srow is None:
        return "NOTSUP"
    cols = w.ks * w.kstep
    row_stride = (cols + 16) // 2 if i8 else cols + 8
    if m * row_stride * 2 > 64 * 1024:
        return "NOTSUP"
    e = dict(i8corr=0, i8span=0, i8nblk=0, i8shift=0, inssq=0, inparts=0, instride=0, ininv=0.0, ogamma=0, ossq=0, ostride=0, ron=0, rhs=0, rnp=0, rkd=0, rk32=0)
    sums, i8q = 0, False
    if i8:
        nblk = i["nblk"] or ceil_div(k, i["i8bs"])
        one = nblk == 1
        bs = i["i8bs"]
        if w.kind not in (INT4, INT8) or m > 4 or link or rope or k % 32 or (not one and (bs & (bs - 1) or bs < 32)):
            return "NOTSUP"
        shift = 31 if one else bs.bit_length() - 1
        # quantized inside the launch: fp32 rows at hand, k-blocks of 32 .. 256 columns dividing K
        i8q = bool(i["i8k"] and i["i8a"] and not one and 5 <= shift <= 8 and k % bs == 0 and k % 4 == 0)
        if not i8q and not i["i8q"]:
            return "NOTREADY"
        span = up(m * nblk * 5, 4)
        sums = up(span, 1024)
        e.update(i8corr=1, i8span=span, i8nblk=nblk, i8shift=shift)
    lda = activation_lda(i)
    has16, has32 = i["act"] in (1, 2, 3), i["act"] != 4
    a16 = (i8 and not i8q) or (not i8 and i["act"] == 1 and k % 8 == 0)
    if moe:
        if m != 1 or nseg != (2 if dual else 1) or link or rope or i8 or has16:
            return "NOTSUP"
        a_stride = k + 2 if i["mbrk"] == 2 else k
        if not 1 <= i["pairs"] <= 65535 or i["nsel"] < 1 or i["pairs"] * i["nsel"] >= 65536 or a_stride % 4:
            return "NOTSUP"
        if dual and (i["mbrk"] == 1 or second_matrix_differs(i, nseg, dual, expert_pair=True)):
            return "NOTSUP"
    a32 = i8q or (not i8 and not a16 and has32 and not link and not rope and lda % 4 == 0 and k % 4 == 0)
    if moe and not a32:
        return "NOTSUP"
    if (not a16 and not a32) or (m > 1 and k % w.kstep):
        return "NOTSUP"
    if link:
        if link in (1, 3, 4, 6, 7):  # consumer: in_parts partial sums per row behind A, whole KiB pieces, 32 at most
            parts = {6: 3000, 7: 1536}.get(link, 256)
            stride = 252 if link == 4 else parts + 4
            if stride < parts or stride % 4:
                return "INVAL"
            sums = m * up(parts * 4, 1024)
            if sums > 32 * 1024:
                return "NOTSUP"
            e.update(inssq=1, inparts=parts, instride=stride, ininv=float("%.9g" % struct.unpack("f", struct.pack("f", 1.0 / k))[0]))  # (fp32, as printed)
        if link in (2, 3, 5):  # producer: a single matrix, a slot per tile
            ostride = ceil_div(nq_cols, 16) - (link == 5)
            if dual or nseg != 1 or ostride < w.tiles:
                return "INVAL"
            e.update(ogamma=1, ossq=1, ostride=ostride)
    if rope:
        hs = i["hs"]
        mode_ok = i["rbrk"] != 3
        if not mseg or nseg != 3 or not mode_ok or hs < 2 or hs % 2 or i["rbrk"] == 2 or ms[0].n != (i["n"] // hs) * hs or any(x.n != (nk_cols // hs) * hs for x in ms[1:]):
            return "INVAL"
        if i["rbrk"] == 1 and m != 1:
            return "INVAL"
        e.update(ron=1, rhs=hs, rnp=7, rkd=3 if i["rbrk"] == 1 else 0, rk32=int(i["rbrk"] == 1))
    if m * lda * 4 >= 1 << 30:
        return "NOTSUP"
    # waves by shape, halved until [A | sums | one ring per wave] fits; a ring: up to 4 slots, at least the reduction's KiB per matrix
    nq = 2 if dual or neox else 1
    ring = lambda nw: max(up(min(ceil_div(w.ks, nw) * nq, GV_PF) * w.slot, 16), nq * 1024)
    a_end = up(m * row_stride * 2, 16)
    nw = decode_waves(tiles, w.ks, dual, i["fnw"])
    while nw > 1 and a_end + sums + nw * ring(nw) > LDS_LIMIT:
        nw //= 2
    if a32 and m * ceil_div(cols * 4, 1024) > nw * 8:  # fp32 rows are held in registers while staged: 8 one-KiB pieces per wave
        return "NOTREADY" if i8q and not i["i8q"] else "NOTSUP"
    lds = a_end + sums + nw * ring(nw)
    if lds > LDS_LIMIT:
        return "NOTSUP"
    tbeg = [0, 0, 0] if dual else [0, ms[0].tiles, ms[0].tiles + (ms[1].tiles if nseg > 1 else 0)]
    div = 2 if neox else 1
    mode = 1 if dual else (3 if neox else 2) if mseg else 0
    e.update(kind=w.kind, sps=w.sps, sdt=w.sdt, asym=w.asym, modex=mode | (0x100 if a32 and not moe else 0) | (0x200 if i8 else 0) | (0x400 if moe else 0) |
             (0x800 if planes else 0), grid=tiles // div, gridy=i["pairs"] if moe else 1, nw=nw, lds=lds, asrc=4 if i8q else 3 if i8 else 1 if a16 else 2, ks=w.ks,
             qstride=w.qstride, nwlog=nw.bit_length() - 1, so="%d,%d" % (w.soff, ms[1].soff if nseg > 1 else 0), zo="%d,%d" % (w.zoff, ms[1].zoff if nseg > 1 else 0),
             sstride=w.sstride, zstride=w.zstride, srows=w.srows, smul=srow[0], sshift=srow[1], tb1=tbeg[1] // div if mseg else ABSENT,
             tb2=tbeg[2] // div if mseg and nseg > 2 else ABSENT, pm=m, pk=k, lda=k if i8q else up(k, 16) if i8 else lda, rstride=row_stride, ssq=a_end,
             ring=a_end + sums, rings=ring(nw), moet=int(moe), moet1=int(moe and dual), moen=8 if moe else 0, moew=int(moe), msel=i["nsel"] if moe else 0,
             mmul=ceil_div(65536, i["nsel"]) if moe else 0, mids=i["nsel"] if moe else 0, mws=i["nsel"] if moe else 0, mas=k if moe else 0,
             mcs=i["n"] if moe else 0, mds=i["n"] + 32 if moe else 0, plbits=w.pl_bits if planes else 0, pllanes=w.pl_lanes if planes else 64,
             pairt=i["hs"] // 32 if neox else 0, c2=int(dual and not moe), d=int(not dual), ldc=nq_cols, ldd=0 if dual else nq_cols + 32, epi=5 if dual else 1,
             oovf=0, f8=0x20002000, lut0=0, why="-")
    mat_fields(e, ms, tbeg)
    return e


def expected(i):
    return gemvs_expected(i) if i["fn"] == "gemvs" else gemv_expected(i)


# ---- the tests -------------------------------------------------------------------------------------------------------------------------------
def test_every_plan_follows_the_rule(plans):
    assert len(plans) > 30000
    bad = []
    for i, o in plans:
        e = expected(i)
        if isinstance(e, str):
            if o["err"] != e:
                bad.append((i, o, e))
        elif o["err"] != "OK":
            bad.append((i, o, "accepted"))
        else:
            assert set(e) | {"err"} == set(o), sorted(set(e) ^ set(o))  # every printed field has its rule
            diff = {k: (o[k], v) for k, v in e.items() if o[k] != v}
            if diff:
                bad.append((i, diff))
    assert not bad, "%d of %d plans differ, first: %r" % (len(bad), len(plans), bad[:3])


def aligned_ascending(offsets):
    return all(x % 16 == 0 for x in offsets) and all(a <= b for a, b in zip(offsets, offsets[1:]))


def test_invariants_of_accepted_plans(plans):
    for i, o in plans:
        if o["err"] != "OK":
            continue
        assert o["lds"] <= LDS_LIMIT, (i, o)
        if i["fn"] == "gemvs":
            S, ks, ksl, tiles = 1 << o["slog"], o["ks"], o["ksl"], o["ntiles"]
            # table | A | control | reduction slots | rings: 16-byte aligned, ascending, one behind the other
            assert o["aoff"] in (0, GS_TABLE) and o["ctl"] == o["aoff"] + o["abytes"] and o["red"] == o["ctl"] + GS_CTL, (i, o)
            assert o["ring"] == o["red"] + GS_R * o["reds"] and o["lds"] == o["ring"] + o["ns"] * o["rings"], (i, o)
            assert aligned_ascending([o["aoff"], o["ctl"], o["red"], o["ring"], o["lds"]]) and o["rings"] % 16 == 0 and o["reds"] % 16 == 0, (i, o)
            assert o["abytes"] >= o["pm"] * o["rstride"] * 2 and o["reds"] == o["ns"] * o["redw"], (i, o)
            assert ksl * (S - 1) < ks <= ksl * S, (i, o)
            assert o["tg"] * S == o["grid"] <= (i["gr"] if i["gr"] > 0 else i["cus"]), (i, o)
            assert o["tbase"] * o["tg"] + o["trem"] == tiles and o["trem"] < o["tg"], (i, o)
            assert 1 <= o["ns"] <= 15 and o["nwaves"] == o["ns"] + 1, (i, o)
            assert o["slab_bytes"] < 1 << 31 and (o["slab_bytes"] != 0) == (S > 1), (i, o)
            assert not o["tickets"] or (tiles <= 65536 and S > 1), (i, o)
            assert o["convert"] != o["a"] and o["owned"] == 0, (i, o)
        else:
            nw = o["nw"]
            assert nw & (nw - 1) == 0 and 1 <= nw <= o["ks"] and nw == 1 << o["nwlog"], (i, o)
            assert aligned_ascending([0, o["ssq"], o["ring"], o["lds"]]) and o["rings"] % 16 == 0, (i, o)
            assert o["ring"] + nw * o["rings"] == o["lds"], (i, o)
            assert o["pm"] * o["rstride"] * 2 <= 64 * 1024 and o["pm"] * o["rstride"] * 2 <= o["ssq"], (i, o)
            assert o["oovf"] == 0, (i, o)


def test_the_grid_reaches_every_branch(plans, program):
    gvs = [(i, o) for i, o in plans if i["fn"] == "gemvs"]
    acc = [(i, o) for i, o in gvs if o["err"] == "OK"]
    # every (kind, mode, one slice / several) combination; for f4 both table settings
    assert {(o["kind"], o["mode"], o["slog"] > 0) for _, o in acc} == {(kd, md, s) for kd in range(4) for md in range(3) for s in (False, True)}
    assert {o["aoff"] for _, o in acc if o["kind"] == F4} == {0, GS_TABLE} and {o["aoff"] for _, o in acc if o["kind"] != F4} == {0}
    # the by-shape rule: each clause alone accepts a call, and a call none of them holds for is refused for just that
    alone, none = set(), 0
    for i, o in gvs:
        if i["gvs"] == 1 and (o["err"] == "OK" or o["why"].startswith("by shape")):
            cl = shape_clauses(i, matrices(i)[0])
            assert any(cl) == (o["err"] == "OK"), (i, o)
            none += not any(cl)
            if sum(cl) == 1:
                alone.add(cl.index(True))
    assert alone == {0, 1, 2, 3} and none > 0
    # every refusal the two plan files can give, and all of gemv_plan's return codes
    said = set()
    for name in ("ns_gemvs_plan.cpp", "ns_gemv_plan.cpp"):
        with open(os.path.join(CSRC, name)) as f:
            src = f.read()
        said |= set(re.findall(r'(?:return|refuse\(|not_supported\(|invalid\(|hipErrorNotReady,)\s*"([^"]+)"', src))
    assert len(said) >= 30 and {o["why"] for _, o in plans} == said | {"-"}
    assert {o["err"] for i, o in plans if i["fn"] == "gemv"} == {"OK", "NOTSUP", "NOTREADY", "INVAL"}
    # the wave-halving loop ran somewhere, and the in-launch quantizer, every activation source and every mode bit were planned
    gv = [(i, o) for i, o in plans if i["fn"] == "gemv" and o["err"] == "OK"]
    assert any(o["nw"] < decode_waves(o["grid"], o["ks"], i["form"] == 1, i["fnw"]) for i, o in gv if i["rope"] != 2)
    assert {o["asrc"] for _, o in gv} == {1, 2, 3, 4} and {o["modex"] & 3 for _, o in gv} == {0, 1, 2, 3}
    assert all(any(o["modex"] & bit for _, o in gv) for bit in (0x100, 0x200, 0x400, 0x800))


def test_the_group_size_ladder_is_planned_as_the_gpu_module_says(plans):
    """the calls of tests/test_gpu_group_sizes.py at its own shapes (263 columns, K = 1920 / 2048 / 1952, groups above one k-step): which of
    them the two streaming kernels take, and with which words they refuse the others — the refusals that module's docstring lists.  No
    refusal is about the group size but ONE: gemv_kernel's int8-reference variant takes power-of-two k-blocks only"""
    lad = [(i, o) for i, o in plans if i["grp"]]
    assert len(lad) > 5000 and {i["k"] for i, _ in lad} == {1920, 2048, 1952} and {i["grp"] for i, _ in lad} == {64, 128, 192, 256, 320, 384, 512, 640, -1}
    whole_steps = "activations: aligned fp16 or fp32 rows; several rows need whole k-steps"
    for i, o in lad:
        kstep = 64 if i["fmt"] in (2, 4) else 128
        g, k, m = i["grp"], i["k"], i["m"]
        ratio = g // kstep
        regime = "row 0" if g < 0 else "shift" if ratio & (ratio - 1) == 0 else "reciprocal"
        if o["err"] == "OK":  # the scale-row rule of the regime
            want = {"row 0": (0, 0), "shift": (1, ratio.bit_length() - 1), "reciprocal": (ceil_div(1 << 20, max(ratio, 1)), 20)}[regime]
            assert (o["smul"], o["sshift"]) == want and o["srows"] == (1 if g < 0 else ceil_div(k, g)), (i, o)
        if i["fn"] == "gemvs":  # pinned, 2 .. 16 rows: K in whole k-steps, then EVERY forced slices x waves combination as forced
            if k % kstep:
                assert o["err"] == "NOTSUP" and o["why"] == "K: a multiple of 8, and of the k-step for several rows", (i, o)
            else:
                assert o["err"] == "OK" and (not i["sl"] or (1 << o["slog"], o["ns"]) == (i["sl"], i["wv"])), (i, o)
                assert o["tickets"] == int(i["sl"] > 1 and not i["fin"]), (i, o)
        elif i["i8"]:  # int8-reference variant: power-of-two k-blocks (or one block); 3 rows need whole k-steps like every other call
            if regime == "reciprocal":
                assert o["err"] == "NOTSUP" and o["why"] == "int8-reference numerics: integer weights, up to 4 rows, power-of-two k-blocks, aligned codes", (i, o)
            elif m > 1 and k % kstep:
                assert o["err"] in ("NOTSUP", "NOTREADY") and (o["err"] == "NOTREADY" or o["why"] == whole_steps), (i, o)
            else:
                assert o["err"] in ("OK", "NOTREADY") and (o["err"] == "OK" or not i["i8q"]), (i, o)
        elif m == 1:
            assert o["err"] == "OK", (i, o)
        elif k % kstep:  # several rows over K = 1952 (16 rows: whichever check comes first)
            assert o["err"] == "NOTSUP" and o["why"] in (whole_steps, "the staged activations exceed 64 KiB") and (m == 16 or o["why"] == whole_steps), (i, o)
        elif m == 16 and k == 2048:  # 16 x (2048 + 8) x 2 = 65,792 bytes
            assert o["err"] == "NOTSUP" and o["why"] == "the staged activations exceed 64 KiB", (i, o)
        elif m == 16 and i["act"] == 0:  # 16 fp32 rows of 1920 columns: 128 one-KiB pieces, the waves hold 64
            assert o["err"] == "NOTSUP" and o["why"] == "more fp32 activation pieces than the waves hold in registers", (i, o)
        else:
            assert o["err"] == "OK", (i, o)


def test_the_program_is_clean_under_sanitizers(program):
    """the same program with AddressSanitizer and UndefinedBehaviorSanitizer on the host: no report, the same lines"""
    hipcc, d, out = program
    exe = os.path.join(d, "stream_plan_san")
    build(hipcc, exe, ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", "-g"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, r.stderr[-2000:]
    assert r.stdout == out

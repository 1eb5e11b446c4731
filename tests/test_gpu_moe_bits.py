"""The output BITS of the mixture-of-experts family (csrc/ns_moe*.{cpp,hip}): ns_hip_mul_mat_id on each of its three servers (decode
launches, loop kernel, grouped path) and ns_hip_moe_ffn_silu / _gelu on each of theirs (fused launches, grouped pass, composition), held to
SHA-256 digests of the output bytes recorded in tests/golden/moe_bits.json.  tests/golden/make_moe_bits.py wrote that file from the library
NS_LIB_PATH named: the build in which the family was still one translation unit and ns_hip_mul_mat_id's grouped path sorted its id column by
hand (perm / valid tables, out-of-range rows gathered last) — the pair layout of ns_moe_plan.cpp serves both grouped forms since.

Every case asserts, with the deltas of ns_hip_moe_stats / ns_hip_moe_ffn_stats, that the server it is named for took the call, and that the
columns beyond the row (ldc / ldo wider than n) keep their fill; the digest covers the whole buffer, fill included.  How close the values
are to an fp64 product is the business of the other tests/test_gpu_moe*.py files, not of this one.

Shapes, the smallest the paths accept: k = 128, n = ff = 64 and 128, 4 experts, ids in rows of 3 ints, lda = k + 4 (k + 3 in two
grouped cases: the gather without 16-byte loads), ldc = n + 3, ldd = n + 5.
Rows: 1 and 8 (decode / fused), 9 and 16 (loop / composition), 32 and 33 (grouped), 72 for fp8 on the grouped path (more than 64 rows, every
populated expert at least 17).  Inputs: numpy.random.default_rng seeded by the case's name."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "moe_bits.json")
RECORDER = os.path.join(os.path.dirname(GOLDEN), "make_moe_bits.py")
N_AS, K, DN, N_USED = 4, 128, 128, 2
SENTINEL = 7.0
FMT = {"int4": ("S4", "BF16", False, 32, "CORE_AVX512_VNNI_KB"), "int8": ("S8", "BF16", False, 32, "CORE_AVX512_VNNI_KB"),
       "f4": ("F4_NF4", "BF16", False, 64, "CORE_AVX512F"), "f8": ("F8_E4M3", "F32", False, 32, "CORE_AVX512F")}
MM_SERVED = {"grouped": (1, 0, 0, 0), "decode": (0, 1, 0, 0), "loop": (0, 0, 1, 0)}   # ns_hip_moe_stats deltas of one call
FFN_SLOT = {"fused": 0, "composition": 1, "grouped": 3}                                # ns_hip_moe_ffn_stats
EPIS = ["none", "add", "mul", "add_gelu", "gelu", "silu"]
KEYS = ((b"moe_gemv_rows", 0), (b"moe_grouped_rows", 0), (b"moe_ffn_grouped_rows", 0), (b"moe_ffn_fused", -1))


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _padded(x, stride, fill):
    import torch
    full = np.full((x.shape[0], stride), fill, x.dtype)
    full[:, :x.shape[1]] = x
    return torch.from_numpy(full).cuda()


def _digest(t):
    return hashlib.sha256(np.ascontiguousarray(t.cpu().numpy()).tobytes()).hexdigest()


class World:
    """the library, the expert groups (quantised and uploaded once) and the digests of the cases run so far"""

    def __init__(self, L, pkg, nso):
        self.L, self.pkg, self.nso = L, pkg, nso
        self.groups, self.keep, self.out, self.failed = {}, [], {}, []

    def group(self, fmt, n, k, tag=""):
        key = (fmt, n, k, tag)
        if key not in self.groups:
            nso, rng = self.nso, _rng("weights-%s-%d-%d-%s" % key)
            qt, st, asym, bs, core = FMT[fmt]
            blobs = [nso.quant_pack((rng.standard_normal((n, k)) * 0.05).astype(np.float32), bs, getattr(nso, qt), getattr(nso, st), asym,
                                    getattr(nso, core)) for _ in range(N_AS)]
            ws = [self.pkg.Weight.from_host_blob(nso.ptr(b)) for b in blobs]
            g = self.L.ns_hip_expert_group_create((C.c_void_p * N_AS)(*[w.h for w in ws]), N_AS)
            assert g, self.pkg.last_error()
            self.keep.append((blobs, ws))
            self.groups[key] = g
        return self.groups[key]

    def free(self):
        for g in self.groups.values():
            self.L.ns_hip_expert_group_free(g)
        for _, ws in self.keep:
            for w in ws:
                w.free()

    def tune(self, pairs):
        for key, v in pairs:
            assert self.L.ns_hip_set_tuning(key, v) == 0

    def counters(self, fn):
        out = (C.c_uint64 * 4)()
        fn(out)
        return [int(v) for v in out]

    # ---- ns_hip_mul_mat_id -------------------------------------------------------------------------------------------------------------
    def case(self, fn, name, *args, **kw):
        """run one case; a case that fails is reported with all the others that do, at the end (run_all)"""
        try:
            fn(name, *args, **kw)
        except (AssertionError, RuntimeError) as e:
            self.failed.append((name, repr(e)))

    def mm(self, name, *args, **kw):
        self.case(self._mm, name, *args, **kw)

    def ffn(self, name, *args, **kw):
        self.case(self._ffn, name, *args, **kw)

    def _mm(self, name, fmt, n, path, col, epi="none", with_d=True, pad_a=4):
        """one call on `path` with the id column `col` (column 2 of a 3-wide table whose other columns name other experts)"""
        import torch
        L, pkg = self.L, self.pkg
        m, rng = len(col), _rng(name)
        a = rng.standard_normal((m, K)).astype(np.float32)
        d = rng.standard_normal((m, n)).astype(np.float32)
        col = np.asarray(col, np.int32)
        ids = np.stack([(col + 1) % N_AS, (col + 2) % N_AS, col], axis=1).astype(np.int32)
        dA, dI, dD = _padded(a, K + pad_a, 1000.0), torch.from_numpy(ids).cuda(), _padded(d, n + 5, -3.0)
        dC = torch.full((m, n + 3), SENTINEL, device="cuda")
        code = {"none": pkg.EPI_NONE, "add": pkg.EPI_ADD, "mul": pkg.EPI_MUL, "add_gelu": pkg.EPI_ADD_GELU, "gelu": pkg.EPI_GELU,
                "silu": pkg.EPI_SILU}[epi]
        if path == "loop":
            self.tune(((b"moe_gemv_rows", -1), (b"moe_grouped_rows", -1)))
        try:
            s0 = self.counters(L.ns_hip_moe_stats)
            pkg.check(L.ns_hip_mul_mat_id(dA.data_ptr(), dI.data_ptr(), 3, 2, self.group(fmt, n, K), dC.data_ptr(), m, K + pad_a, n + 3, code,
                                          dD.data_ptr() if with_d else None, n + 5, _stream()))
            torch.cuda.synchronize()
            delta = tuple(x - y for x, y in zip(self.counters(L.ns_hip_moe_stats), s0))
        finally:
            self.tune(KEYS)
        assert delta == MM_SERVED[path], (name, "served by (grouped, decode, loop, refused) = %s" % (delta,))
        assert bool((dC[:, n:] == SENTINEL).all()), name
        assert name not in self.out
        self.out[name] = _digest(dC)

    def mm_cases(self):
        def mixed(name, m, bad=True):
            col = _rng("ids-" + name).integers(0, N_AS, m)
            if bad and m >= 4:
                col[1], col[3] = -1, N_AS
            return col

        for fmt in ("int4", "int8", "f4"):
            for n in (64, 128):
                tag = "mm/%s-n%d/" % (fmt, n)
                self.mm(tag + "decode-m1", fmt, n, "decode", [2])
                self.mm(tag + "decode-m1-bad-id", fmt, n, "decode", [N_AS], epi="add")
                self.mm(tag + "decode-m8", fmt, n, "decode", mixed(tag + "d8", 8))
                self.mm(tag + "loop-m9", fmt, n, "loop", mixed(tag + "l9", 9))
                self.mm(tag + "loop-m33", fmt, n, "loop", mixed(tag + "l33", 33), epi="add")
                self.mm(tag + "grouped-m32", fmt, n, "grouped", mixed(tag + "g32", 32))
                self.mm(tag + "grouped-m33", fmt, n, "grouped", mixed(tag + "g33", 33, bad=False))
        for n in (64, 128):
            tag = "mm/f8-n%d/" % n
            self.mm(tag + "loop-m9", "f8", n, "loop", mixed(tag + "l9", 9))
            self.mm(tag + "loop-m72", "f8", n, "loop", mixed(tag + "l72", 72))
            self.mm(tag + "grouped-m72", "f8", n, "grouped", np.arange(72) % 3)           # 24 rows each, expert 3 none
            col = np.arange(72) % 3
            col[1], col[3] = -1, N_AS
            self.mm(tag + "grouped-m72-bad-ids", "f8", n, "grouped", col, epi="add")       # 24 / 23 / 23
        # every epilogue on the grouped path, with and without dD; the decode launches and the loop with the ones that read dD
        for epi in EPIS:
            self.mm("mm/epi/grouped-%s" % epi, "int4", 64, "grouped", mixed("epi-g", 33), epi=epi)
            self.mm("mm/epi/grouped-%s-no-d" % epi, "int4", 64, "grouped", mixed("epi-g", 33), epi=epi, with_d=False)   # dD == NULL: epi(x, 0)
            self.mm("mm/epi/decode-%s" % epi, "int4", 64, "decode", mixed("epi-d", 8), epi=epi)
            self.mm("mm/epi/loop-%s" % epi, "int4", 64, "loop", mixed("epi-l", 9), epi=epi)
        # lda = k + 3: rows that rule out the gather's 16-byte loads (its scalar branch), on the grouped path and - refused by the decode
        # launches - on the loop
        self.mm("mm/lda-odd/grouped-m33", "int4", 64, "grouped", mixed("lda-g", 33), epi="add", pad_a=3)
        self.mm("mm/lda-odd/grouped-m32-lone-last", "int4", 128, "grouped", [0, 1] * 15 + [3, -1], pad_a=3)
        # the row layouts of the grouped path: groups of ONE row are launched with two
        base = np.arange(32) % 2                       # experts 0 and 1, 16 rows each
        lay = {}
        lay["lone-last-with-bad-ids"] = base.copy()
        lay["lone-last-with-bad-ids"][[10, 1, 3]] = [3, -1, N_AS]
        lay["lone-last-no-bad-ids"] = base.copy()
        lay["lone-last-no-bad-ids"][10] = 3
        lay["lone-last-is-expert-2-with-bad-ids"] = base.copy()
        lay["lone-last-is-expert-2-with-bad-ids"][[10, 30, 31]] = [2, N_AS, -1]
        lay["lone-first"] = base.copy() + 1
        lay["lone-first"][10] = 0
        lay["consecutive-lone"] = base.copy() * 3       # experts 0 and 3
        lay["consecutive-lone"][[10, 20]] = [1, 2]
        lay["consecutive-lone-to-the-end-with-bad-ids"] = np.zeros(32, np.int64)
        lay["consecutive-lone-to-the-end-with-bad-ids"][[5, 6, 7, 0, 9]] = [1, 2, 3, -1, N_AS]
        lay["consecutive-lone-to-the-end-no-bad-ids"] = np.zeros(32, np.int64)
        lay["consecutive-lone-to-the-end-no-bad-ids"][[7, 6, 5]] = [1, 2, 3]
        lay["one-expert"] = np.full(32, 2)
        lay["every-id-bad"] = np.where(np.arange(32) % 2 == 0, -1, N_AS)
        for name, col in lay.items():
            self.mm("mm/layout/" + name, "int4", 64, "grouped", col, epi="add")
            self.mm("mm/layout/" + name + "-n128-silu", "int4", 128, "grouped", col, epi="silu", with_d=False)

    # ---- ns_hip_moe_ffn_silu / _gelu -----------------------------------------------------------------------------------------------------
    def _ffn(self, name, fmt, ff, path, m, act, weights=True, ldo=DN + 4, captured=False):
        import torch
        L, pkg = self.L, self.pkg
        rng = _rng(name)
        a = rng.standard_normal((m, K)).astype(np.float32)
        ids = np.stack([rng.permutation(N_AS)[:N_USED] for _ in range(m)]).astype(np.int32)
        if m >= 8:
            ids[2], ids[4], ids[5] = [-1, N_AS], [1, -1], [N_AS + 3, 2]     # a row without a good selection, two with one
        wts = rng.uniform(0.2, 0.8, (m, N_USED)).astype(np.float32)
        dA, dI = _padded(a, K + 4, np.nan), _padded(ids, N_USED + 1, -77)
        dW = _padded(wts, N_USED + 3, np.nan) if weights else None
        out = torch.full((m, ldo), SENTINEL, device="cuda")
        gg, gu, gd = self.group(fmt, ff, K, "gate"), self.group(fmt, ff, K, "up"), self.group(fmt, DN, ff, "down")
        fn = L.ns_hip_moe_ffn_gelu if act == "gelu" else L.ns_hip_moe_ffn_silu

        def call():
            pkg.check(fn(dA.data_ptr(), K + 4, m, dI.data_ptr(), N_USED + 1, dW.data_ptr() if weights else None, N_USED + 3 if weights else 0,
                         N_USED, gg, gu, gd, out.data_ptr(), ldo, _stream()))
        torch.cuda.synchronize()
        s0 = self.counters(L.ns_hip_moe_ffn_stats)
        if captured:
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                call()
            gr.replay()
        else:
            call()
        torch.cuda.synchronize()
        s1 = self.counters(L.ns_hip_moe_ffn_stats)
        delta = {p: s1[i] - s0[i] for p, i in FFN_SLOT.items()}
        assert delta == {p: int(p == path) for p in FFN_SLOT}, (name, delta)
        assert bool((out[:, DN:] == SENTINEL).all()), name
        if m >= 8:
            assert bool((out[2, :DN] == 0.0).all()), name
        assert name not in self.out
        self.out[name] = _digest(out)

    def ffn_cases(self):
        for fmt, ff in (("int4", 64), ("int4", 128), ("int8", 64), ("f4", 128)):
            tag = "ffn/%s-ff%d/" % (fmt, ff)
            for act in ("silu", "gelu"):
                self.ffn(tag + "fused-m1-" + act, fmt, ff, "fused", 1, act)
                self.ffn(tag + "fused-m8-" + act, fmt, ff, "fused", 8, act)
                self.ffn(tag + "grouped-m32-" + act, fmt, ff, "grouped", 32, act)
                self.ffn(tag + "composition-m16-" + act, fmt, ff, "composition", 16, act)
                self.ffn(tag + "composition-m32-captured-" + act, fmt, ff, "composition", 32, act, captured=True)
            self.ffn(tag + "fused-m8-null-weights", fmt, ff, "fused", 8, "silu", weights=False)
            self.ffn(tag + "grouped-m32-null-weights", fmt, ff, "grouped", 32, "gelu", weights=False)
            self.ffn(tag + "composition-m16-null-weights", fmt, ff, "composition", 16, "silu", weights=False)
            self.ffn(tag + "grouped-m33-ldo-odd", fmt, ff, "grouped", 33, "silu", ldo=DN + 1)


def run_all(L, pkg, nso):
    """every case -> {name: SHA-256 of its output bytes}"""
    w = World(L, pkg, nso)
    w.tune(KEYS)
    try:
        w.mm_cases()
        w.ffn_cases()
        assert not w.failed, w.failed
        return w.out
    finally:
        w.tune(KEYS)
        w.free()


@pytest.fixture(scope="module")
def bits(L, nso, tmp_path_factory):
    """run_all in a child process (the recorder, one pass): the counters are process-wide sums, and tests/test_gpu_moe_ffn.py - which sorts
    behind this file - holds the grouped pass's slot of ns_hip_moe_ffn_stats at 0, so the block's grouped cases must not run in this one"""
    out = str(tmp_path_factory.mktemp("moe_bits") / "bits.json")
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [RECORDER, out, "1"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    with open(out) as f:
        return json.load(f)


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_every_case_has_recorded_bits_and_every_recorded_case_is_run(bits):
    want = _golden()
    assert sorted(bits) == sorted(want)
    assert len([c for c in bits if c.startswith("mm/")]) >= 90 and len([c for c in bits if c.startswith("ffn/")]) >= 50


@pytest.mark.parametrize("family", ["mm/int4", "mm/int8", "mm/f4", "mm/f8", "mm/epi", "mm/layout", "mm/lda-odd", "ffn/"])
def test_bits_are_the_recorded_ones(bits, family):
    want = _golden()
    mine = [c for c in bits if c.startswith(family)]
    assert mine
    differ = [c for c in mine if bits[c] != want.get(c)]
    assert not differ, ("bits differ from the recorded ones", differ)

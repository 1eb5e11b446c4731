"""The output BITS of the reference device backend's own kernels (csrc/ns_device_mha.hip, csrc/ns_device_ops.hip): ns_hip_mha_f32_device_layout
on each of its three servers (the fp16 mirror + this library's attention kernels, the context-split kernel, the single-workgroup kernel),
ns_hip_binary_nd_f32 on both of its kernels and the three sequences of the lazy peephole, held to SHA-256 digests of whole output buffers -
fill values included - recorded in tests/golden/device_bits.json.  tests/golden/make_device_bits.py wrote that file from the library
NS_LIB_PATH named: the build in which the backend was still one translation unit (csrc/ns_device.hip) and chose its kernels inline.  It
records every case in two separate processes; a case whose two recordings differ holds null there and is not held to a digest (none does:
no floating-point atomics, the merges run in range order).

Which server takes which shape is the business of tests/test_device_plan.py, how close the values are to an fp64 model that of
tests/test_gpu_device_mha.py and tests/test_gpu_device_lazy.py, not of this file.

Attention: the shapes of tests/test_gpu_device_mha.py with fewer than 1000 keys, with the mirror on and off, two calls each (the second
re-uses the mirror and the scratch); a Q that is only 4-byte aligned (neither mirror nor split); 520 causal rows of 32 heads x 256 with the
mirror off (the split kernel's partials go through in two row chunks).  Cache cells past seq_all hold NaN.
Inputs: numpy.random.default_rng seeded by the case's name."""
import ctypes as C
import hashlib
import json
import os
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "device_bits.json")
FILL = 7.0
MHA_SHAPES = [  # batch, seq, seq_all, heads, heads_kv, head_size, n_ctx, masked
    (1, 1, 777, 8, 2, 64, 1024, 1), (1, 5, 300, 4, 4, 128, 512, 1), (2, 1, 513, 4, 1, 256, 600, 0), (1, 2, 100, 4, 4, 128, 256, 1),
    (1, 1, 400, 6, 3, 80, 512, 1), (1, 700, 900, 32, 32, 128, 1024, 1), (1, 64, 64, 8, 8, 128, 128, 1), (1, 200, 333, 8, 2, 64, 512, 1),
    (2, 130, 130, 4, 4, 96, 256, 0), (1, 31, 400, 4, 4, 128, 512, 1), (1, 1, 1, 32, 32, 128, 2048, 1)]
MISALIGNED_Q = (1, 1, 300, 4, 4, 128, 512, 1)
CHUNKED = (1, 520, 520, 32, 32, 256, 520, 1)


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _digest(t):
    return hashlib.sha256(np.ascontiguousarray(t.cpu().numpy()).tobytes()).hexdigest()


def _ll(*v):
    return (C.c_longlong * 4)(*v)


def _packed(ne):
    nb, s = [], 4
    for e in ne:
        nb.append(s)
        s *= e
    return nb


class World:
    def __init__(self, L, pkg):
        import torch
        self.L, self.pkg, self.out = L, pkg, {}
        self.st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        vp, ll4 = C.c_void_p, C.POINTER(C.c_longlong)
        L.ns_hip_mha_f32_device_layout.restype = C.c_int
        L.ns_hip_mha_f32_device_layout.argtypes = [vp] * 4 + [C.c_int] * 7 + [C.c_float, C.c_int, vp]
        L.ns_hip_set_tuning.argtypes = [C.c_char_p, C.c_int]
        L.ns_hip_binary_nd_f32.restype = C.c_int
        L.ns_hip_binary_nd_f32.argtypes = [C.c_int, vp, vp, vp, ll4, ll4, ll4, ll4, ll4, vp]
        L.ns_hip_lazy_rms_norm.argtypes = [C.c_int, C.c_int, C.c_float, vp, vp, vp]
        L.ns_hip_lazy_silu.argtypes = [vp, vp, C.c_size_t, vp]
        L.ns_hip_lazy_mul.argtypes = [vp, vp, vp, ll4, ll4, ll4, ll4, ll4, vp]
        L.ns_hip_lazy_flush.restype = C.c_int

    def put(self, name, t):
        assert name not in self.out
        self.out[name] = _digest(t)

    # ---- ns_hip_mha_f32_device_layout ------------------------------------------------------------------------------------------------------
    def mha(self, name, shape, kv16, q_offset=0):
        import torch
        batch, seq, seq_all, heads, hkv, hs, n_ctx, masked = shape
        rng = _rng(name)
        q = rng.standard_normal(batch * seq * heads * hs + q_offset).astype(np.float32)
        k = np.full((batch, hkv, n_ctx, hs), np.nan, np.float32)
        v = np.full((batch, hkv, hs, n_ctx), np.nan, np.float32)
        k[:, :, :seq_all] = rng.standard_normal((batch, hkv, seq_all, hs)).astype(np.float32)
        v[:, :, :, :seq_all] = rng.standard_normal((batch, hkv, hs, seq_all)).astype(np.float32)
        dq, dk, dv = torch.from_numpy(q).cuda(), torch.from_numpy(k).cuda(), torch.from_numpy(v).cuda()
        out = torch.empty((batch, seq, heads, hs), device="cuda")
        assert self.L.ns_hip_set_tuning(b"device_kv_f16", kv16) == 0
        try:
            for call in range(2):
                out.fill_(FILL)
                self.pkg.check(self.L.ns_hip_mha_f32_device_layout(dq.data_ptr() + 4 * q_offset, dk.data_ptr(), dv.data_ptr(), out.data_ptr(), batch, seq, seq_all,
                                                                   heads, hkv, hs, n_ctx, float(hs ** -0.5), masked, self.st))
                torch.cuda.synchronize()
                assert bool(torch.isfinite(out).all()), name
                self.put("%s/call%d" % (name, call), out)
        finally:
            self.L.ns_hip_set_tuning(b"device_kv_f16", -1)

    def mha_cases(self):
        for shape in MHA_SHAPES:
            for kv16 in (1, 0):
                self.mha("mha/%s/kv16-%d" % ("x".join(map(str, shape)), kv16), shape, kv16)
        for kv16 in (1, 0):
            self.mha("mha/misaligned-q/kv16-%d" % kv16, MISALIGNED_Q, kv16, q_offset=1)
        self.mha("mha/chunked-520/kv16-0", CHUNKED, 0)

    # ---- ns_hip_binary_nd_f32 --------------------------------------------------------------------------------------------------------------
    def binary(self, name, ne0, ne1=None, row_stride0=None, d_offset=0):
        """add and mul of src0 [ne0] with src1 [ne1] (default: the same shape); row_stride0: floats between the rows of src0;
        d_offset: floats the destination starts behind a 16-byte boundary"""
        import torch
        ne1 = ne1 or ne0
        rng = _rng(name)
        rs0 = row_stride0 or ne0[0]
        a = rng.standard_normal(rs0 * ne0[1] * ne0[2] * ne0[3]).astype(np.float32)
        b = rng.standard_normal(int(np.prod(ne1))).astype(np.float32)
        nb0 = [4, 4 * rs0, 4 * rs0 * ne0[1], 4 * rs0 * ne0[1] * ne0[2]]
        nb1 = [0 if (i > 0 and ne1[i] == 1) else s for i, s in enumerate(_packed(ne1))]      # as ne hands a broadcast operand over
        dA, dB = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
        for op, word in ((0, "add"), (1, "mul")):
            d = torch.full((int(np.prod(ne0)) + 8,), FILL, device="cuda")
            self.pkg.check(self.L.ns_hip_binary_nd_f32(op, dA.data_ptr(), dB.data_ptr(), d.data_ptr() + 4 * d_offset, _ll(*ne0), _ll(*nb0), _ll(*ne1), _ll(*nb1),
                                                       _ll(*_packed(ne0)), self.st))
            torch.cuda.synchronize()
            assert bool((d[:d_offset] == FILL).all()) and bool((d[d_offset + int(np.prod(ne0)):] == FILL).all()), name
            self.put("%s/%s" % (name, word), d)

    def binary_cases(self):
        self.binary("binary/64x64", (64, 64, 1, 1))
        self.binary("binary/64x64-rowvec", (64, 64, 1, 1), ne1=(64, 1, 1, 1))
        self.binary("binary/60x68", (60, 68, 1, 1))
        self.binary("binary/broadcast-dim1", (64, 64, 2, 1), ne1=(64, 1, 2, 1))
        self.binary("binary/src-row-stride", (64, 64, 1, 1), row_stride0=68)
        self.binary("binary/misaligned-dst", (64, 64, 1, 1), d_offset=1)

    # ---- the lazy peephole -----------------------------------------------------------------------------------------------------------------
    def mul(self, a, b, d, vec=False):
        ne0 = (a.shape[1], a.shape[0], 1, 1)
        ne1 = (ne0[0], 1, 1, 1) if vec else ne0
        nb1 = [4, 0, 0, 0] if vec else _packed(ne1)
        self.pkg.check(self.L.ns_hip_lazy_mul(a.data_ptr(), b.data_ptr(), d.data_ptr(), _ll(*ne0), _ll(*_packed(ne0)), _ll(*ne1), _ll(*nb1), _ll(*_packed(ne0)), self.st))

    def lazy_cases(self):
        import torch
        L, pkg, st = self.L, self.pkg, self.st
        for rows, cols in ((2, 100), (3, 4096)):
            name = "lazy/norm-weight-%dx%d" % (rows, cols)
            rng = _rng(name)
            x = torch.from_numpy((rng.standard_normal((rows, cols)) * 3).astype(np.float32)).cuda()
            gam = torch.from_numpy(rng.standard_normal(cols).astype(np.float32)).cuda()
            a, b = torch.full_like(x, FILL), torch.full_like(x, FILL)
            pkg.check(L.ns_hip_lazy_rms_norm(rows, cols, 1e-5, x.data_ptr(), a.data_ptr(), st))
            self.mul(a, gam, b, vec=True)
            torch.cuda.synchronize()
            self.put(name + "/norm", a)
            self.put(name + "/product", b)
            a.fill_(FILL)                                       # in place: the norm is launched as it stands, the plain multiply runs over it
            pkg.check(L.ns_hip_lazy_rms_norm(rows, cols, 1e-5, x.data_ptr(), a.data_ptr(), st))
            self.mul(a, gam, a, vec=True)
            torch.cuda.synchronize()
            self.put(name + "/in-place", a)
        name = "lazy/silu-up-3x11008"
        rng = _rng(name)
        gate = torch.from_numpy((rng.standard_normal((3, 11008)) * 4).astype(np.float32)).cuda()
        up = torch.from_numpy(rng.standard_normal((3, 11008)).astype(np.float32)).cuda()
        for order in ("silu-first", "silu-second"):
            s, p = torch.full_like(gate, FILL), torch.full_like(gate, FILL)
            pkg.check(L.ns_hip_lazy_silu(gate.data_ptr(), s.data_ptr(), gate.numel(), st))
            self.mul(s, up, p) if order == "silu-first" else self.mul(up, s, p)
            torch.cuda.synchronize()
            self.put("%s/%s/silu" % (name, order), s)
            self.put("%s/%s/product" % (name, order), p)
        s = torch.full_like(gate, FILL)
        pkg.check(L.ns_hip_lazy_silu(gate.data_ptr(), s.data_ptr(), gate.numel(), st))
        self.mul(s, up, s)
        torch.cuda.synchronize()
        self.put(name + "/in-place", s)
        assert L.ns_hip_lazy_flush() == 0


def run_all(L, pkg):
    """every case -> {name: SHA-256 of its output bytes}"""
    w = World(L, pkg)
    w.mha_cases()
    w.binary_cases()
    w.lazy_cases()
    return w.out


@pytest.fixture(scope="module")
def bits(L, pkg):
    return run_all(L, pkg)


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_every_case_has_a_record_and_every_recorded_case_is_run(bits):
    want = _golden()
    assert sorted(bits) == sorted(want)
    held = [c for c in want if want[c] is not None]
    for prefix, least in (("mha/", 40), ("binary/", 12), ("lazy/", 11)):
        assert len([c for c in held if c.startswith(prefix)]) >= least, prefix
    # each of the three attention servers and both binary kernels keeps a digest: a mirror case, the chunked split, the misaligned Q on the
    # whole kernel; a dense and a strided binary node
    for c in ("mha/1x1x777x8x2x64x1024x1/kv16-1/call1", "mha/chunked-520/kv16-0/call1", "mha/misaligned-q/kv16-0/call0", "binary/64x64/add", "binary/60x68/mul"):
        assert want[c] is not None, c


@pytest.mark.parametrize("family", ["mha/", "binary/", "lazy/"])
def test_bits_are_the_recorded_ones(bits, family):
    want = _golden()
    mine = [c for c in bits if c.startswith(family) and want.get(c) is not None]
    assert mine
    differ = [c for c in mine if bits[c] != want[c]]
    assert not differ, ("bits differ from the recorded ones", differ)

"""gemv_kernel's launch tail (csrc/ns_gemv.hip): the stretch between a workgroup's last record and its last store — epilogue arguments,
cross-wave reduction, epilogue.  Every form of the launch, at every wave count 1 / 2 / 4 / 8 / 16, returns

  * the bits of code that does not share that tail — `ns_hip_set_tuning("gemv2", 0)`: smallm_kernel, which adds the waves' partial sums
    in the same order — in everything the launch writes (np.array_equal, outputs prefilled so that what must NOT be written is compared too);
  * a float64 numpy model of the form within the suites' 1e-3 (rel. L2);
  * the bits recorded in tests/golden/gemv_tail_bits.json (SHA-256 of every case's output bytes; tests/golden/make_gemv_tail_bits.py
    writes the file from the library NS_LIB_PATH names — it was run on the build before the tail was rearranged).

Where no other code serves a call the first check has another yardstick, and the recorded bits pin the rest:
  * RoPE + kv-append (mode 0 and the NeoX pair mode): the two-launch composition, fused QKV under "gemv2" 0 + ns_hip_rope_qkv_append, as
    tests/test_gpu_qkv_rope_neox.py does (q and both caches);
  * carried norm: smallm_kernel refuses a norm link, so the fp32 output of the norm-OUT launch is held to the plain launch under "gemv2" 0
    (the producer side changes the shadow only) and the norm-IN launches to the model and the recorded bits;
  * expert-indexed launch: with "gemv2" 0 ns_hip_mul_mat_id takes its fp32-FMA loop kernel (other numerics): model + recorded bits; the
    out-of-range id gives exactly epi(0, d);
  * int8-reference forms (XV 3 / 5): with "gemv2" 0 the general int8 kernel serves (same integer dots, other order of the float sums):
    the oracle's gemm_u8s8 + recorded bits.

Shapes, the smallest that reach every path: n = 40 (three 16-column tiles, the last partial) and 64; K = 128 (one k-step: one wave), 512,
2048 (16 k-steps, so that 16 waves exist); 2 / 4 / 8 / 16 waves forced through "gv_nw" at K = 2048; "gvs" 0 keeps launches of several
rows on gemv_kernel (its general form) instead of the shared-activation kernel.  Inputs: seeded numpy on the host."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = 1e-3        # tests/test_gpu_parity.py: decode GEMV against the fp64 product on the dequantized weights
SENTINEL = 7.0
EPS = 1e-5
BASE = 10000.0
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemv_tail_bits.json")

# name, K, forced waves ("gv_nw"; 0: by shape).  K = 128 is one k-step of a nibble record: one wave whatever is forced
WCFG = [("k128-nw1", 128, 0), ("k2048-nw2", 2048, 2), ("k2048-nw4", 2048, 4), ("k2048-nw8", 2048, 8), ("k2048-nw16", 2048, 16),
        ("k512-rule", 512, 0)]
SYM, ASYM, INT8 = ("S4", "BF16", False, 32), ("S4", "BF16", True, 32), ("S8", "BF16", False, 32)
QKV_N = (64, 32, 32)
HEADS, HKV, HS, N_PAST, CTX = 2, 1, 32, 3, 8


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _full(shape, dtype=None):
    import torch
    return torch.full(shape, SENTINEL, device="cuda", dtype=dtype or torch.float32)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.detach().cpu().numpy()


def _bits(t):
    a = _np(t)
    return np.ascontiguousarray(a).view(np.uint16 if a.dtype == np.float16 else np.uint32)


def _ptr(t):
    return t.data_ptr() if t is not None else None


class _Mode:
    """the launches inside run on gemv_kernel (gemv2 = 1) or on the first-generation kernels (0), with `nw` waves forced"""
    def __init__(self, L, gemv2, nw):
        self.L, self.gemv2, self.nw = L, gemv2, nw

    def __enter__(self):
        assert self.L.ns_hip_set_tuning(b"gvs", 0) == 0
        assert self.L.ns_hip_set_tuning(b"gemv2", self.gemv2) == 0
        assert self.L.ns_hip_set_tuning(b"gv_nw", self.nw) == 0

    def __exit__(self, *exc):
        self.L.ns_hip_set_tuning(b"gv_nw", 0)
        self.L.ns_hip_set_tuning(b"gemv2", 1)
        self.L.ns_hip_set_tuning(b"gvs", -1)


def _silu(v):
    return v / (1.0 + np.exp(-v))


def _gelu(v):
    return 0.5 * v * (1.0 + np.tanh(0.7978845834732056 * (v + 0.044714998453855515 * v ** 3)))


def _rope64(x, n_past, hs, neox):
    """x: [m][heads * hs] float64 -> rotated, position n_past + row"""
    m = x.shape[0]
    y = x.reshape(m, -1, hs).copy()
    half = hs // 2
    ang = (n_past + np.arange(m))[:, None] * BASE ** (-2.0 * np.arange(half) / hs)[None, :]
    c, s = np.cos(ang)[:, None, :], np.sin(ang)[:, None, :]
    x0, x1 = (y[:, :, :half], y[:, :, half:]) if neox else (y[:, :, 0::2], y[:, :, 1::2])
    y0, y1 = x0 * c - x1 * s, x0 * s + x1 * c
    if neox:
        y[:, :, :half], y[:, :, half:] = y0, y1
    else:
        y[:, :, 0::2], y[:, :, 1::2] = y0, y1
    return y.reshape(m, -1)


class _Cfg:
    """one wave configuration: its weights and inputs (made once), and the cases"""

    def __init__(self, L, pkg, nso, name, k, nw):
        self.L, self.pkg, self.nso, self.name, self.k, self.nw = L, pkg, nso, name, k, nw
        self.rng = np.random.default_rng(1000 + k + nw)
        self.out = {}      # case -> digest
        self.keep = []
        st = _stream()

        def weight(n, fmt):
            qt, sd, asym, bs = fmt
            w = (self.rng.standard_normal((n, k)) * (1.0 / np.sqrt(k))).astype(np.float32)
            if asym:
                w += 0.05
            blob = nso.quant_pack(w, bs, getattr(nso, qt), getattr(nso, sd), asym, nso.CORE_AVX512_VNNI_KB)
            self.keep.append(blob)
            return pkg.Weight.from_host_blob(nso.ptr(blob), st), blob

        self.w = {(f, n): weight(n, f) for f, n in ((SYM, 40), (SYM, 64), (ASYM, 40), (INT8, 40))}
        self.w3 = weight(40, SYM)
        self.qkv = [weight(n, SYM) for n in QKV_N]
        self.experts = [weight(40, SYM) for _ in range(2)]
        arr = (C.c_void_p * 2)(*[w.h for w, _ in self.experts])
        self.group = L.ns_hip_expert_group_create(arr, 2)
        assert self.group, pkg.last_error()
        self.x = {m: self.rng.standard_normal((m, k)).astype(np.float32) for m in (1, 2, 5, 16)}
        self.d = {(m, n): self.rng.standard_normal((m, n + 3)).astype(np.float32) for m in (1, 2, 5, 16) for n in (40, 64)}
        self.gam = (1.0 + 0.2 * self.rng.standard_normal(k)).astype(np.float32)
        import torch
        torch.cuda.synchronize()

    def free(self):
        self.L.ns_hip_expert_group_free(self.group)

    # ---- plumbing -------------------------------------------------------------------------------------------------------------
    def both(self, run):
        """run() once on gemv_kernel and once with "gemv2" 0 -> (bits, bits of the reference), equal"""
        import torch
        got, outs = [], []
        for g2 in (1, 0):
            with _Mode(self.L, g2, self.nw):
                outs.append(run())
                torch.cuda.synchronize()
                got.append([_bits(t) for t in outs[-1]])
        for i, (a, b) in enumerate(zip(got[0], got[1])):
            assert np.array_equal(a, b), (self.name, "output %d differs from the gemv2 = 0 launch in %d words" % (i, int((a != b).sum())))
        return outs[0]

    def new(self, run):
        import torch
        with _Mode(self.L, 1, self.nw):
            outs = run()
            torch.cuda.synchronize()
        return outs

    def old(self, run):
        import torch
        with _Mode(self.L, 0, self.nw):
            outs = run()
            torch.cuda.synchronize()
        return outs

    def close(self, got, ref, what):
        err = self.nso.rel_l2(np.asarray(got, np.float64), np.asarray(ref, np.float64))
        assert err < TOL, (self.name, what, err)

    def record(self, case, tensors):
        h = hashlib.sha256()
        for t in tensors:
            h.update(_bits(t).tobytes())
        assert case not in self.out
        self.out[case] = h.hexdigest()

    def norm_inputs(self, m):
        """gamma-scaled fp16 shadow + partial sums of squares of x (ns_hip_norm_prep), the link, and the normalised rows (float64)"""
        import torch
        k, x = self.k, self.x[m]
        parts = (k + 15) // 16
        stride = (parts + 3) & ~3
        dx, dg = _dev(x), _dev(self.gam)
        xg16, ssq = torch.zeros(m, k, device="cuda", dtype=torch.float16), torch.zeros(m, stride, device="cuda")
        self.pkg.check(self.L.ns_hip_norm_prep(m, k, dx.data_ptr(), k, dg.data_ptr(), xg16.data_ptr(), ssq.data_ptr(), stride, _stream()))
        torch.cuda.synchronize()
        x64 = x.astype(np.float64)
        h = x64 * self.gam.astype(np.float64) / np.sqrt((x64 ** 2).mean(axis=1, keepdims=True) + EPS)
        self.keep += [dx, dg, xg16, ssq]
        return dx, xg16, ssq, parts, stride, h

    # ---- the cases ----------------------------------------------------------------------------------------------------------------
    def plain(self, fmt, tag, rows, ns):
        L, pkg, nso, k = self.L, self.pkg, self.nso, self.k
        import torch
        for m in rows:
            for n in ns:
                w, blob = self.w[(fmt, n)]
                x, d = _dev(self.x[m]), _dev(self.d[(m, n)])
                x16, ldc = x.half(), n + 4
                outs = []
                for epi, shadow in ((pkg.EPI_NONE, True), (pkg.EPI_NONE, False), (pkg.EPI_ADD, True), (pkg.EPI_ADD, False)):
                    def run():
                        c, c16 = _full((m, ldc)), _full((m, ldc), torch.float16)
                        pkg.check(L.ns_hip_f32f32_forward_h(x.data_ptr(), x16.data_ptr(), w.h, c.data_ptr(), c16.data_ptr() if shadow else None,
                                                            m, k, ldc, epi, d.data_ptr() if epi == pkg.EPI_ADD else None, n + 3, _stream()))
                        return [c, c16]
                    c, c16 = self.both(run)
                    ref = nso.gemm_f64(self.x[m], blob) + (self.d[(m, n)][:, :n] if epi == pkg.EPI_ADD else 0.0)
                    self.close(_np(c)[:, :n], ref, (tag, m, n, epi, shadow))
                    assert bool((c[:, n:] == SENTINEL).all()) and bool((c16[:, n:] == SENTINEL).all())
                    if shadow:
                        assert torch.equal(c16[:, :n], c[:, :n].half())
                    else:
                        assert bool((c16 == SENTINEL).all())
                    outs += [c, c16]
                self.record("plain-%s-m%d-n%d" % (tag, m, n), outs)

    def dual(self):
        L, pkg, nso, k, n = self.L, self.pkg, self.nso, self.k, 40
        import torch
        (w1, b1), (w3, b3) = self.w[(SYM, 40)], self.w3
        for m in (1, 5):
            x = _dev(self.x[m])
            x16 = x.half()
            outs = []
            for act, fn in ((pkg.EPI_SILU, _silu), (pkg.EPI_GELU, _gelu)):
                for with_t1 in (True, False):
                    def run():
                        t1, t2, t2h = _full((m, n)), _full((m, n)), _full((m, n), torch.float16)
                        pkg.check(L.ns_hip_fusion_ffn3_gateup_h(x.data_ptr(), x16.data_ptr(), w1.h, w3.h, t1.data_ptr() if with_t1 else None,
                                                                t2.data_ptr(), t2h.data_ptr(), m, act, _stream()))
                        return [t2, t2h, t1]
                    t2, t2h, t1 = self.both(run)
                    g, u = nso.gemm_f64(self.x[m], b1), nso.gemm_f64(self.x[m], b3)
                    self.close(_np(t2), fn(g) * u, ("dual", m, act, with_t1))
                    if with_t1:
                        self.close(_np(t1), fn(g), ("dual tmp1", m, act))
                    else:
                        assert bool((t1 == SENTINEL).all())
                    assert torch.equal(t2h, t2.half())
                    outs += [t2, t2h, t1]
            self.record("dual-m%d" % m, outs)

    def qkv_run(self, x, x16, m, link=None, c16=True):
        L, pkg, k = self.L, self.pkg, self.k
        import torch

        def run():
            c, ch = _full((3, m, 64)), _full((3, m, 64), torch.float16)
            pkg.check(L.ns_hip_fusion_qkv_forward_x(x.data_ptr(), _ptr(x16), self.qkv[0][0].h, self.qkv[1][0].h, self.qkv[2][0].h, c.data_ptr(),
                                                    ch.data_ptr() if c16 else None, m, k, 64, C.byref(link) if link is not None else None, _stream()))
            return [c, ch]
        return run

    def qkv_check(self, c, rows64, what):
        for i, n in enumerate(QKV_N):
            self.close(_np(c)[i][:, :n], self.nso.gemm_f64(rows64.astype(np.float32), self.qkv[i][1]), (what, i))
            assert bool((c[i][:, n:] == SENTINEL).all())

    def fused_qkv(self):
        for m in (1, 2):
            x = _dev(self.x[m])
            c, ch = self.both(self.qkv_run(x, x.half(), m))
            self.qkv_check(c, self.x[m], ("qkv", m))
            self.record("qkv-m%d" % m, [c, ch])

    def norm(self):
        L, pkg, nso, k, n = self.L, self.pkg, self.nso, self.k, 40
        import torch
        w, blob = self.w[(SYM, 40)]
        (w1, b1), (w3, b3) = self.w[(SYM, 40)], self.w3
        for m in (1, 2):
            dx, xg16, ssq, parts, stride, h = self.norm_inputs(m)
            x16, d = dx.half(), _dev(self.d[(m, n)])
            tiles = (n + 15) // 16
            ostride = (tiles + 3) & ~3
            g2 = torch.linspace(0.5, 1.5, n, device="cuda")
            outs = []
            for link_in, link_out in ((True, False), (False, True), (True, True)):
                def run():
                    c, c16, ossq = _full((m, n)), _full((m, n), torch.float16), _full((m, ostride))
                    lk = pkg.NormLink(ssq.data_ptr() if link_in else None, parts if link_in else 0, stride if link_in else 0, EPS if link_in else 0.0,
                                      k if link_in else 0, g2.data_ptr() if link_out else None, ossq.data_ptr() if link_out else None,
                                      ostride if link_out else 0)
                    pkg.check(L.ns_hip_f32f32_forward_x(dx.data_ptr(), (xg16 if link_in else x16).data_ptr(), w.h, c.data_ptr(), c16.data_ptr(), m, k, n,
                                                        pkg.EPI_ADD, d.data_ptr(), n + 3, C.byref(lk), _stream()))
                    return [c, c16, ossq]
                c, c16, ossq = self.new(run)
                rows = h if link_in else self.x[m].astype(np.float64)
                ref = nso.gemm_f64(rows.astype(np.float32), blob) + self.d[(m, n)][:, :n]
                self.close(_np(c), ref, ("forward_x", m, link_in, link_out))
                if link_out:
                    assert torch.equal(c16, (c * g2).half())
                    self.close(_np(ossq)[:, :tiles], np.add.reduceat(ref ** 2, np.arange(0, n, 16), axis=1), ("out_ssq", m, link_in))
                    assert bool((ossq[:, tiles:] == SENTINEL).all())
                else:
                    assert torch.equal(c16, c.half()) and bool((ossq == SENTINEL).all())
                if not link_in:  # the producer side leaves the fp32 output what the plain launch writes
                    def plain():
                        cp = _full((m, n))
                        pkg.check(L.ns_hip_f32f32_forward_h(dx.data_ptr(), x16.data_ptr(), w.h, cp.data_ptr(), None, m, k, n, pkg.EPI_ADD, d.data_ptr(),
                                                            n + 3, _stream()))
                        return [cp]
                    assert np.array_equal(_bits(self.old(plain)[0]), _bits(c))
                outs += [c, c16, ossq]
            lk_in = pkg.NormLink(ssq.data_ptr(), parts, stride, EPS, k, None, None, 0)
            c, ch = self.new(self.qkv_run(dx, xg16, m, lk_in))
            self.qkv_check(c, h, ("qkv norm in", m))
            outs += [c, ch]

            def gateup():
                t1, t2, t2h = _full((m, n)), _full((m, n)), _full((m, n), torch.float16)
                pkg.check(L.ns_hip_fusion_ffn3_gateup_x(dx.data_ptr(), xg16.data_ptr(), w1.h, w3.h, t1.data_ptr(), t2.data_ptr(), t2h.data_ptr(), m,
                                                        pkg.EPI_SILU, C.byref(lk_in), _stream()))
                return [t2, t2h, t1]
            t2, t2h, t1 = self.new(gateup)
            g, u = nso.gemm_f64(h.astype(np.float32), b1), nso.gemm_f64(h.astype(np.float32), b3)
            self.close(_np(t2), _silu(g) * u, ("gate/up norm in", m))
            outs += [t2, t2h, t1]
            self.record("norm-m%d" % m, outs)

    def rope(self):
        L, pkg, nso, k = self.L, self.pkg, self.nso, self.k
        import torch
        wq, wk, wv = (w for w, _ in self.qkv)
        for neox in (False, True):
            mode, flags = (2, pkg.QKV_ROPE_NEOX) if neox else (0, 0)
            for m in (1, 2):
                x = _dev(self.x[m])
                x16 = x.half()
                tab = torch.zeros(m, HS // 2, 2, device="cuda")
                if neox:
                    pkg.check(L.ns_hip_rope_cos_sin_mode(m, N_PAST, HS, 2, BASE, 1.0, 1.0, tab.data_ptr(), _stream()))
                else:
                    pkg.check(L.ns_hip_rope_cos_sin(m, N_PAST, HS, BASE, 1.0, 1.0, tab.data_ptr(), _stream()))

                def fused(a16, link):
                    def run():
                        c = _full((3, m, 64))
                        kc, vc = _full((1, CTX, HKV, HS), torch.float16), _full((1, CTX, HKV, HS), torch.float16)
                        rp = pkg.QkvRope(kc.data_ptr(), vc.data_ptr(), tab.data_ptr(), HEADS, HKV, HS, N_PAST, HS, mode, HKV * HS, HS, flags)
                        pkg.check(L.ns_hip_fusion_qkv_rope_forward_x(x.data_ptr(), a16.data_ptr(), wq.h, wk.h, wv.h, c.data_ptr(), m, k, 64,
                                                                     C.byref(link) if link is not None else None, C.byref(rp), _stream()))
                        return [c, kc, vc]
                    return run
                c, kc, vc = self.new(fused(x16, None))

                def two_launches():
                    qkv = _full((3, m, 64))
                    kc_a, vc_a = _full((1, CTX, HKV, HS), torch.float16), _full((1, CTX, HKV, HS), torch.float16)
                    pkg.check(L.ns_hip_fusion_qkv_forward_x(x.data_ptr(), x16.data_ptr(), wq.h, wk.h, wv.h, qkv.data_ptr(), None, m, k, 64, None, _stream()))
                    q_a, k_a, v_a = qkv[0].contiguous(), qkv[1][:, :HKV * HS].contiguous(), qkv[2][:, :HKV * HS].contiguous()
                    pkg.check(L.ns_hip_rope_qkv_append(q_a.data_ptr(), k_a.data_ptr(), v_a.data_ptr(), kc_a.data_ptr(), vc_a.data_ptr(), m, HEADS, HKV, HS,
                                                       N_PAST, HS, mode, BASE, 1.0, 0.0, 1.0, HKV * HS, HS, _stream()))
                    return [q_a, kc_a, vc_a]
                q_a, kc_a, vc_a = self.old(two_launches)
                assert torch.equal(c[0], q_a), (self.name, "rope q", neox, m)
                assert torch.equal(kc, kc_a) and torch.equal(vc, vc_a), (self.name, "rope caches", neox, m)
                assert bool((kc[0, :N_PAST] == SENTINEL).all()) and bool((kc[0, N_PAST + m:] == SENTINEL).all())
                xh = _np(x16.float())
                q64, k64, v64 = (nso.gemm_f64(xh, b) for _, b in self.qkv)
                self.close(_np(c)[0], _rope64(q64, N_PAST, HS, neox), ("rope q", neox, m))
                self.close(_np(c)[1][:, :32], _rope64(k64, N_PAST, HS, neox), ("rope k", neox, m))
                self.close(_np(c)[2][:, :32], v64, ("rope v", neox, m))
                self.close(_np(kc.float())[0, N_PAST:N_PAST + m].reshape(m, -1), _rope64(k64, N_PAST, HS, neox), ("rope k cache", neox, m))
                outs = [c, kc, vc]
                # ... and behind a carried norm
                dx, xg16, ssq, parts, stride, h = self.norm_inputs(m)
                lk_in = pkg.NormLink(ssq.data_ptr(), parts, stride, EPS, k, None, None, 0)
                c2, kc2, vc2 = self.new(fused(xg16, lk_in))
                self.close(_np(c2)[0], _rope64(nso.gemm_f64(h.astype(np.float32), self.qkv[0][1]), N_PAST, HS, neox), ("rope q, norm in", neox, m))
                outs += [c2, kc2, vc2]
                self.record("rope-%s-m%d" % ("neox" if neox else "mode0", m), outs)

    def fp32_rows(self):
        """no fp16 shadow: the kernel converts the fp32 rows while staging (XV 2)"""
        L, pkg, nso, k, n = self.L, self.pkg, self.nso, self.k, 40
        w, blob = self.w[(SYM, 40)]
        for m in (1, 2):
            x, d = _dev(self.x[m]), _dev(self.d[(m, n)])

            def run():
                c = _full((m, n))
                pkg.check(L.ns_hip_f32f32_forward(x.data_ptr(), w.h, c.data_ptr(), m, k, n, pkg.EPI_ADD, d.data_ptr(), n + 3, _stream()))
                return [c]
            c, = self.both(run)
            self.close(_np(c), nso.gemm_f64(self.x[m], blob) + self.d[(m, n)][:, :n], ("fp32 rows", m))
            cq, _ = self.both(self.qkv_run(x, None, m, c16=False))
            self.qkv_check(cq, self.x[m], ("fp32 rows qkv", m))
            self.record("fp32rows-m%d" % m, [c, cq])

    def int8_reference(self):
        """ns_hip_set_compute_mode(1): fp32 rows quantized inside the launch (XV 5); a row 4 bytes past a 16-byte boundary takes its codes
        from the quantizer launch in front (XV 3)"""
        L, pkg, nso, k, n = self.L, self.pkg, self.nso, self.k, 40
        import torch
        w, blob = self.w[(SYM, 40)]
        (w1, b1), (w3, b3) = self.w[(SYM, 40)], self.w3
        prev = L.ns_hip_set_compute_mode(1)
        try:
            for m in (1, 2):
                d = _dev(self.d[(m, n)])
                outs = []
                for off in (0, 1):
                    if off and m > 1:
                        continue
                    buf = torch.zeros(m * k + 4, device="cuda")
                    x = buf[off:off + m * k].view(m, k)
                    x.copy_(_dev(self.x[m]))

                    def run():
                        c = _full((m, n))
                        pkg.check(L.ns_hip_f32f32_forward(x.data_ptr(), w.h, c.data_ptr(), m, k, n, pkg.EPI_ADD, d.data_ptr(), n + 3, _stream()))
                        return [c]
                    c, = self.new(run)
                    self.close(_np(c), nso.gemm_u8s8(self.x[m], blob) + self.d[(m, n)][:, :n], ("int8 plain", m, off))
                    outs.append(c)
                x = _dev(self.x[m])
                cq, _ = self.new(self.qkv_run(x, None, m, c16=False))
                for i, nq in enumerate(QKV_N):
                    self.close(_np(cq)[i][:, :nq], nso.gemm_u8s8(self.x[m], self.qkv[i][1]), ("int8 qkv", m, i))

                def gateup():
                    t1, t2 = _full((m, n)), _full((m, n))
                    pkg.check(L.ns_hip_fusion_ffn3_gateup(x.data_ptr(), w1.h, w3.h, t1.data_ptr(), t2.data_ptr(), m, pkg.EPI_SILU, _stream()))
                    return [t2, t1]
                t2, t1 = self.new(gateup)
                self.close(_np(t2), _silu(nso.gemm_u8s8(self.x[m], b1)) * nso.gemm_u8s8(self.x[m], b3), ("int8 gate/up", m))
                self.record("int8ref-m%d" % m, outs + [cq, t2, t1])
        finally:
            L.ns_hip_set_compute_mode(prev)

    def expert(self):
        """ns_hip_mul_mat_id at one row: the expert picked on the device (XV 4); id 1 of two experts, and an id outside the group"""
        L, pkg, nso, k, n = self.L, self.pkg, self.nso, self.k, 40
        x, d = _dev(self.x[1]), _dev(self.d[(1, n)])
        ids = _dev(np.array([[1, 99]], np.int32))
        outs = []
        for sel in (0, 1):
            def run():
                c = _full((1, n + 4))
                stats = (C.c_uint64 * 4)()
                L.ns_hip_moe_stats(stats)
                before = stats[1]
                pkg.check(L.ns_hip_mul_mat_id(x.data_ptr(), ids.data_ptr(), 2, sel, self.group, c.data_ptr(), 1, k, n + 4, pkg.EPI_ADD, d.data_ptr(),
                                              n + 3, _stream()))
                L.ns_hip_moe_stats(stats)
                assert stats[1] == before + 1, "not served by the decode kernel"
                return [c]
            c, = self.new(run)
            dv = self.d[(1, n)][:, :n]
            if sel == 0:
                self.close(_np(c)[:, :n], nso.gemm_f64(self.x[1], self.experts[1][1]) + dv, ("expert", sel))
            else:
                assert np.array_equal(_np(c)[:, :n], dv)  # epi(0, d)
            assert bool((c[:, n:] == SENTINEL).all())
            outs.append(c)
        self.record("expert-m1", outs)

    def graph(self):
        """plain, gate / up and fused QKV captured in one graph and replayed: the eager launches' bits"""
        L, pkg, k, n = self.L, self.pkg, self.k, 40
        import torch
        w, _ = self.w[(SYM, 40)]
        w3, _ = self.w3
        x, d = _dev(self.x[1]), _dev(self.d[(1, n)])
        x16 = x.half()
        bufs = [_full((1, n)), _full((1, n), torch.float16), _full((1, n)), _full((1, n)), _full((3, 1, 64))]

        def launches(c, c16, t1, t2, cq):
            pkg.check(L.ns_hip_f32f32_forward_h(x.data_ptr(), x16.data_ptr(), w.h, c.data_ptr(), c16.data_ptr(), 1, k, n, pkg.EPI_ADD, d.data_ptr(), n + 3, _stream()))
            pkg.check(L.ns_hip_fusion_ffn3_gateup_h(x.data_ptr(), x16.data_ptr(), w.h, w3.h, t1.data_ptr(), t2.data_ptr(), None, 1, pkg.EPI_SILU, _stream()))
            pkg.check(L.ns_hip_fusion_qkv_forward_h(x.data_ptr(), x16.data_ptr(), self.qkv[0][0].h, self.qkv[1][0].h, self.qkv[2][0].h, cq.data_ptr(), None, 1, k, 64,
                                                    _stream()))

        def eager():
            e = [torch.full_like(b, SENTINEL) for b in bufs]
            launches(*e)
            return e
        ref = self.old(eager)
        with _Mode(L, 1, self.nw):
            launches(*bufs)  # (first launches outside the capture)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                launches(*bufs)
            for _ in range(2):
                for b in bufs:
                    b.fill_(SENTINEL)
                g.replay()
                torch.cuda.synchronize()
                for b, r in zip(bufs, ref):
                    assert np.array_equal(_bits(b), _bits(r)), (self.name, "replayed graph")
        self.record("graph-m1", bufs)

    def run(self):
        self.plain(SYM, "sym", (1, 2, 5, 16), (40, 64))
        self.plain(ASYM, "asym", (1, 5), (40,))
        self.plain(INT8, "int8", (1, 5), (40,))
        self.dual()
        self.fused_qkv()
        self.norm()
        self.rope()
        self.fp32_rows()
        self.int8_reference()
        self.expert()
        self.graph()
        return self.out


def run_config(L, pkg, nso, cfg):
    """every case of one wave configuration, checked against the other kernels and the float64 models -> {case: SHA-256 of its output bytes}"""
    name, k, nw = cfg
    c = _Cfg(L, pkg, nso, name, k, nw)
    try:
        return {"%s/%s" % (name, case): dig for case, dig in c.run().items()}
    finally:
        c.free()


@pytest.mark.parametrize("cfg", WCFG, ids=[c[0] for c in WCFG])
def test_launch_tail_bits(L, pkg, nso, cfg):
    got = run_config(L, pkg, nso, cfg)
    with open(GOLDEN) as f:
        want = json.load(f)
    assert len(got) >= 28
    missing = [c for c in got if c not in want]
    assert not missing, ("cases without recorded bits", missing)
    differ = [c for c in got if got[c] != want[c]]
    assert not differ, ("bits differ from the recorded ones", differ)


def test_every_recorded_case_is_run():
    with open(GOLDEN) as f:
        want = json.load(f)
    assert {c.split("/")[0] for c in want} == {c[0] for c in WCFG} and len(want) == 28 * len(WCFG)

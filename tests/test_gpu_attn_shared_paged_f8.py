"""ns_hip_attn_decode_paged_shared_f8 (docs/kernels/attention.md, "Shared-prefix decode over an FP8 paged cache").  The fp16 module's steps with K / V
rounded to E4M3 of x / scale, scale a power of two: the fp16 arrays hold code * scale exactly.  The uint8 pools hold 0x7f (NaN) behind every live length,
in spare blocks and in every member's own, unnamed prefix blocks; guards on either side; dst starts as 7.0.  Bounds: (1) check() / rounding_model() per
request against nso.attn_ref over the decoded values, (2) rel_l2 < 2e-4 against the fp16 entry over fp16 pools of them (tests/test_gpu_attn_block_paged_f8.py's)."""
import ctypes as C
import functools

import numpy as np
import pytest

from test_gpu_attention_paths import rounding_model
from test_gpu_attn_block_paged_f8 import all_codes
from test_gpu_attn_paged import NAN16, Pools, delta
from test_gpu_attn_paged_f8 import NAN8, Pools8, decoded, to_codes
from test_gpu_attn_shared_paged import CASES, Step, check_step, run_shared, shared_stats

pytestmark = pytest.mark.gpu
CASES8 = {name: dict(CASES[name]) for name in CASES if name != "b_three_groups_pages_of_64"}
CASES8["f_every_code"] = dict(hn=4, hkv=2, hs=64, cap=256, bk=16, start=[0, 2], prefix=[128], lens=[256, 200], max_group=2, scales=(2.0 ** -6, 0.25, 2.0, 4.0),
                              codes=all_codes)


def shared8_stats(L):
    out = (C.c_ulonglong * 4)()
    L.ns_hip_attn_decode_paged_shared_f8_stats(out)
    return list(out)


class Entry:
    """shared_call's library handle: the FP8 entry (or the fp16 one) in the fp16 entry's place, the argument block given the step's scales"""
    def __init__(self, L, c, f8=True):
        self.fn, self.scales = (L.ns_hip_attn_decode_paged_shared_f8, c.f8_scales) if f8 else (L.ns_hip_attn_decode_paged_shared, c.scales)

    def ns_hip_attn_decode_paged_shared(self, a, *rest):
        a._obj.Q_sc, a._obj.K_sc, a._obj.V_sc, a._obj.dst_sc = self.scales
        return self.fn(a, *rest)


class Step8(Step):
    """Step over E4M3 K / V: kc / vc the codes (codes: given, not drawn), k / v = code * scale in fp16; scales: the fp16 entry's, f8_scales: the FP8 entry's"""
    def __init__(self, nso, scales=(1.0, 0.125, 0.125, 1.0), codes=None, **kw):
        Step.__init__(self, nso, **kw)
        qs, ks, vs, ds = scales
        self.kc, self.vc = codes(self.k.shape) if codes else (to_codes(self.k.astype(np.float32), ks), to_codes(self.v.astype(np.float32), vs))
        for b, (leader, P) in self.members.items():
            self.kc[b, :P], self.vc[b, :P] = self.kc[leader, :P], self.vc[leader, :P]
        self.k, self.v, self.f8_scales, self.scales = decoded(self.kc, ks), decoded(self.vc, vs), scales, (qs, 1.0, 1.0, ds)
        assert np.array_equal(to_codes(self.k, ks), self.kc) and np.array_equal(to_codes(self.v, vs), self.vc)  # the fp16 copy is exact
        for b in self.ref:
            qb, kb, vb = self.q[b:b + 1], self.k[b:b + 1, :self.lens[b]], self.v[b:b + 1, :self.lens[b]]
            self.ref[b] = nso.attn_ref(qb, kb, vb, self.scale, self.flags, scales=self.scales)
            self.model[b] = rounding_model(qb, kb, vb, self.scale, self.flags, self.scales)

    def pools(self, f8=True, table_edit=None, nan_own=True):
        make, k, v, nan = (Pools8, self.kc, self.vc, NAN8) if f8 else (Pools, self.k, self.v, NAN16)
        p = make(self.bs, self.hkv, self.hs, self.cap, self.bk, self.layout, seed=5).fill(k, v, self.lens)
        for b, (leader, P) in self.members.items():
            if b != leader and P:
                own = p.table[b, :P // self.bk].copy()
                p.table[b, :P // self.bk] = p.table[leader, :P // self.bk]
                if nan_own:
                    p.k[own + 1], p.v[own + 1] = nan, nan
        if table_edit:
            table_edit(p)
        return p.upload()


@functools.lru_cache(None)
def step8(nso, name):
    return Step8(nso, **CASES8[name])


@pytest.mark.parametrize("name", list(CASES8))
def test_f8_shared_prefix_decode_against_the_reference_and_the_fp16_entry(L, pkg, nso, name):
    c = step8(nso, name)
    p8, p16 = c.pools(), c.pools(f8=False)
    assert np.array_equal(p8.table, p16.table) and sum(int(np.all(p8.k[j + 1] == NAN8)) for j in range(p8.pool_blocks)) >= 3  # (the spare blocks at least)
    s0, f0 = shared8_stats(L), shared_stats(L)
    out = run_shared(Entry(L, c), pkg, c, p8)[0]
    assert delta(s0, shared8_stats(L)) == ([2, 0, 1, 0] if c.hs == 64 else [0, 2, 1, 0]) and shared_stats(L) == f0
    assert np.all(np.isfinite(out)) and p8.guards_intact() and p8.unchanged(), name  # no code behind a limit, no unnamed or spare block was consumed
    check_step(nso, "f8 " + name, c, out)
    half = run_shared(Entry(L, c, f8=False), pkg, c, p16)[0]
    e = nso.rel_l2(out[sorted(c.members)], half[sorted(c.members)])
    print("ATTN_SHARED_PAGED_F8 %s: rel_l2 against ns_hip_attn_decode_paged_shared %.3g" % (name, e))
    assert e < 2e-4, (name, e)


@pytest.mark.parametrize("edit", ["junk_member_entries", "leader_minus_one", "leader_pool_blocks"])
def test_table_entries(L, pkg, nso, edit):
    """junk in the members' own entries below the prefix: every bit stays.  A bad entry inside the first leader's prefix: the other groups keep their bits"""
    c = step8(nso, "b_three_groups_pages_of_32")
    good = run_shared(Entry(L, c), pkg, c, c.pools())[0]

    def change(p):
        if edit != "junk_member_entries":
            p.table[1, 3] = -1 if edit == "leader_minus_one" else p.pool_blocks
            return
        spare = sorted(set(range(p.pool_blocks)) - set(p.table.ravel()))[0]  # (a block of NaN codes)
        for b, (leader, P) in c.members.items():
            if b != leader:
                p.table[b, :P // c.bk] = [(-1, p.pool_blocks, spare)[j % 3] for j in range(P // c.bk)]

    p = c.pools(table_edit=change)
    out = run_shared(Entry(L, c), pkg, c, p)[0]
    same = list(range(c.bs)) if edit == "junk_member_entries" else [0, 6, 7, 8, 9, 10]
    assert np.all(np.isfinite(out)) and np.array_equal(out[same].view(np.uint32), good[same].view(np.uint32)) and p.guards_intact()


def test_far_pool_is_bit_equal_to_the_compact_twin(L, pkg, nso):
    """The far step of tests/test_gpu_attn_far_addresses.py (one group of three over a prefix of 64 keys, lens 70 / 200 / 64, a request of no group;
    4 / 2 heads of 128, blocks of 16 = 4096 bytes) on FarPools8 of tests/test_gpu_attn_paged_f8.py: an untouched pool of 2^20 + 64 blocks, every live
    block but block 2 — the leader's prefix blocks the members' entries name among them — above 2^32 bytes; 0x7f in the first and the last 64 blocks,
    the members' own prefix blocks included.  The compact twin meets the reference and the fp16 entry; the far run holds its bits, consumes no 0x7f
    byte and changes none."""
    import torch
    from test_gpu_attn_far_addresses import FL, need, release, same_bits
    from test_gpu_attn_paged_f8 import FarPools8
    bk = FL.SHARED_BK
    c = Step8(nso, hn=FL.HN, hkv=FL.HKV, hs=128, cap=FL.SHARED_CAP, bk=bk, start=FL.SHARED_START, prefix=FL.SHARED_PREFIX, lens=FL.SHARED_LENS,
              max_group=FL.SHARED_MAX_GROUP)
    live = [-(-n // bk) for n in c.lens]
    need(2 * FL.F8_BLOCKS * FL.block_step(128, bk))
    got, p = [], None
    try:
        for blocks in (FL.pool_blocks("near", FL.block_step(128, bk), sum(live)) + 128, FL.F8_BLOCKS):
            p = FarPools8(blocks, c, bk, live)
            assert blocks < 1 << 20 or all(i == 2 or i * p.block_step >= 1 << 32 for i in p.ids.values())
            for b, n in enumerate(c.lens):
                kc, vc = c.kc[b, :n].copy(), c.vc[b, :n].copy()
                if b in c.members and c.members[b][0] != b:
                    P = c.members[b][1]
                    kc[:P], vc[:P] = NAN8, NAN8  # (the member's own prefix blocks, which no entry names)
                    p.table[b, :P // bk] = p.table[c.members[b][0], :P // bk]
                p.put(b, kc, vc)
            p.dt = torch.from_numpy(p.table).cuda()
            s0 = shared8_stats(L)
            out = run_shared(Entry(L, c), pkg, c, p)[0]
            assert delta(s0, shared8_stats(L)) == [0, 2, 1, 0], blocks
            cells, clean = p.live()
            assert clean and np.all(np.isfinite(out)), blocks
            got.append((out, cells))
            p = None
            release()
        (on, cn), (of, cf) = got
        check_step(nso, "far addresses, near twin: decode_paged_shared_f8", c, on)
        half = run_shared(Entry(L, c, f8=False), pkg, c, c.pools(f8=False))[0]
        e = nso.rel_l2(on[sorted(c.members)], half[sorted(c.members)])
        assert e < 2e-4, e
        assert same_bits(on, of) and all(same_bits(cn[key][x], cf[key][x]) for key in cn for x in (0, 1))
    finally:
        p = None
        release()

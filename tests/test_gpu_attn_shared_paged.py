"""ns_hip_attn_decode_paged_shared (docs/kernels/attention.md, "Shared-prefix decode over a paged cache").  Reference and bounds are the project's: every
request on its own against nso.attn_ref through check() / rounding_model() of tests/test_gpu_attention_paths.py (rel_l2 < 1e-3 and, per row,
max(2^-11, 4 d)); no case and no row is left out.  K / V per request are random with k[b, :P_g] = k[leader, :P_g].  The pools (Pools of
tests/test_gpu_attn_paged.py: NaN fill, guards) are filled through a table of distinct blocks; then every member's entries below P_g / block_keys are
aliased to the leader's and the member's own, now unnamed, prefix blocks are overwritten with NaN, as is everything behind a live length.  dst starts as 7.0."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_attention_paths import check, rounding_model
from test_gpu_attn_paged import NAN16, Pools, delta, run_paged
from test_gpu_attn_rows import CAUSAL, HM, PM, stream_ptr

pytestmark = pytest.mark.gpu


def shared_stats(L):
    out = (C.c_ulonglong * 4)()
    L.ns_hip_attn_decode_paged_shared_stats(out)
    return list(out)


class Step:
    """inputs of one step, made once; members[b] = (leader, P_g) of every request a group names; reference and rounding model of each with a key"""

    def __init__(self, nso, hn, hkv, hs, cap, bk, start, prefix, lens, max_group, flags=CAUSAL, bias=0, layout=PM):
        self.bs, self.hn, self.hkv, self.hs, self.cap, self.bk, self.flags, self.bias, self.layout = len(lens), hn, hkv, hs, cap, bk, flags, bias, layout
        self.start, self.prefix, self.lens, self.max_group, self.scales = list(start), list(prefix), list(lens), max_group, (1.0, 1.0, 1.0, 1.0)
        rng = np.random.default_rng(hs * 7 + cap + self.bs + bk)
        self.q = rng.standard_normal((self.bs, 1, hn, hs)).astype(np.float32)
        self.k = rng.standard_normal((self.bs, cap, hkv, hs)).astype(np.float16)
        self.v = rng.standard_normal((self.bs, cap, hkv, hs)).astype(np.float16)
        self.scale, self.members, self.ref, self.model = float(1.0 / np.sqrt(hs)), {}, {}, {}
        for g, given in enumerate(prefix):
            P = min(max(given, 0), cap) // bk * bk
            for b in range(start[g], start[g] + min(max(start[g + 1] - start[g], 0), max_group)):
                self.members[b] = (start[g], P)
                self.k[b, :P], self.v[b, :P] = self.k[start[g], :P], self.v[start[g], :P]
        for b, n in enumerate(lens):
            if b in self.members and n > 0:
                qb, kb, vb = self.q[b:b + 1], self.k[b:b + 1, :n], self.v[b:b + 1, :n]
                self.ref[b], self.model[b] = nso.attn_ref(qb, kb, vb, self.scale, flags), rounding_model(qb, kb, vb, self.scale, flags)
        for x in (self.q, self.k, self.v):
            x.setflags(write=False)

    def pools(self, table_edit=None, nan_own=True):
        p = Pools(self.bs, self.hkv, self.hs, self.cap, self.bk, self.layout, seed=5).fill(self.k, self.v, self.lens)
        for b, (leader, P) in self.members.items():
            if b != leader and P:
                own = p.table[b, :P // self.bk].copy()
                p.table[b, :P // self.bk] = p.table[leader, :P // self.bk]
                if nan_own:
                    p.k[own + 1], p.v[own + 1] = NAN16, NAN16
        if table_edit:
            table_edit(p)
        return p.upload()


def shared_call(L, pkg, c, p, q_ptr, dst_ptr, dev, row=None, tmp=None, dst16=None):
    """dev: the device tensors (dGroupStart, dPrefixKeys, dKvLens); row: floats per (request, head) of dst"""
    row = row or c.hs
    a = pkg.attn_args(q_ptr, p.kp, p.vp, dst_ptr, c.bs, c.hn, c.hkv, c.hs, 1, c.cap, c.scale, c.flags)
    a.step_k_bs = a.step_v_bs = 12345  # (not used: must not matter)
    a.step_k_sl = a.step_v_sl = p.step_sl
    a.step_k_head_num = a.step_v_head_num = p.step_head
    a.step_dst_bs, a.step_dst_head_num, a.step_dst_sl = c.hn * row, row, c.hn * row
    a.tmp = tmp.data_ptr() if tmp is not None else None
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    pkg.check(L.ns_hip_attn_decode_paged_shared(C.byref(a), ptr(dev[0]), len(c.prefix), c.max_group, ptr(dev[1]), ptr(dev[2]), c.bias, *p.table_args(), ptr(dst16),
                                                stream_ptr()))


def run_shared(L, pkg, c, p, dst16=False, dst_pad=0, tmp=None):
    """-> (dst [bs][1][hn][hs], the fp16 shadow, the whole dst buffer); dst_pad > 0: rows of hs + dst_pad floats, dst one float behind a 16-byte boundary"""
    import torch
    dq = torch.from_numpy(c.q.copy()).cuda()
    row, skew = c.hs + dst_pad, 1 if dst_pad else 0
    buf = torch.full((c.bs * c.hn * row + skew,), 7.0, device="cuda")
    b16 = torch.full((c.bs * c.hn * row,), 7.0, device="cuda", dtype=torch.float16) if dst16 else None
    dev = [torch.tensor(x, dtype=torch.int32, device="cuda") for x in (c.start, c.prefix, [n - c.bias for n in c.lens])]
    shared_call(L, pkg, c, p, dq.data_ptr(), buf.data_ptr() + 4 * skew, dev, row, tmp, b16)
    torch.cuda.synchronize()
    whole = buf[skew:].cpu().numpy().reshape(c.bs, 1, c.hn, row)
    return np.ascontiguousarray(whole[..., :c.hs]), (b16.cpu().numpy().reshape(c.bs, 1, c.hn, row) if dst16 else None), whole


def check_step(nso, tag, c, out):
    """every request on its own; an idle member's row is zeros, a request no group names keeps its 7.0"""
    for b, n in enumerate(c.lens):
        if b not in c.members or n == 0:
            assert np.all(out[b] == (0.0 if b in c.members else 7.0)), (tag, b)
        else:
            check(nso, "%s request %d (%d keys, prefix %d)" % (tag, b, n, c.members[b][1]), out[b:b + 1], c.ref[b], c.model[b])


# (b): requests 0 and 10 in no group; group 0 = requests 1 .. 5 (one shorter than the prefix, one idle), group 1 empty, group 2 the singleton 6 with
# prefix 0, group 3 = requests 7 .. 9 whose leader ends at the prefix
B = dict(hn=8, hkv=2, hs=64, cap=1024, start=[1, 6, 6, 7, 10], lens=[50, 1024, 500, 100, 0, 417, 333, 64, 65, 200, 60], max_group=5)
CASES = {
    "a_suffix_of_one_key_across_a_range_and_empty": dict(hn=4, hkv=4, hs=128, cap=512, bk=16, start=[0, 3], prefix=[256], lens=[257, 326, 256], max_group=3),
    "b_three_groups_pages_of_32": dict(bk=32, prefix=[352, 5, 0, 64], **B),
    "b_three_groups_pages_of_64": dict(bk=64, prefix=[384, 5, 0, 64], **B),
    "c_72_slots_second_slot_block": dict(hn=8, hkv=1, hs=128, cap=512, bk=256, start=[0, 9], prefix=[256], lens=[300, 257, 512, 256, 400, 258, 511, 320, 384],
                                         max_group=9),
    "d_many_ranges_beside_a_short_group": dict(hn=4, hkv=4, hs=128, cap=4096, bk=64, start=[0, 2, 4], prefix=[2048, 64], lens=[2178, 4096, 70, 130], max_group=2),
    "e_head_major_not_causal_prefix_rounded_down_bias": dict(hn=4, hkv=2, hs=128, cap=1024, bk=128, start=[0, 3], prefix=[600], lens=[700, 513, 1024], max_group=3,
                                                             flags=0, bias=1, layout=HM),
}
_steps = {}


def step(nso, name):
    if name not in _steps:
        _steps[name] = Step(nso, **CASES[name])
    return _steps[name]


@pytest.mark.parametrize("name", list(CASES))
def test_shared_prefix_decode_against_the_reference(L, pkg, nso, name):
    c = step(nso, name)
    p = c.pools()
    s0 = shared_stats(L)
    out = run_shared(L, pkg, c, p)[0]
    assert delta(s0, shared_stats(L)) == ([2, 0, 1, 0] if c.hs == 64 else [0, 2, 1, 0])
    assert np.all(np.isfinite(out)), name  # nothing behind a live length, no unnamed prefix block and no spare block was consumed
    check_step(nso, name, c, out)
    pk, pv = p.download()
    assert p.guards_intact() and np.array_equal(pk, p.k) and np.array_equal(pv, p.v)  # the attention writes no cache byte


@pytest.mark.parametrize("edit", ["junk_member_entries", "leader_minus_one", "leader_pool_blocks"])
def test_table_entries(L, pkg, nso, edit):
    """junk (-1, pool_blocks, a NaN block) in the members' own entries below the prefix: never read, every bit stays.  A bad entry inside the first
    leader's prefix: the requests of the other groups keep their bits, nothing is NaN, the guards are intact."""
    c = step(nso, "b_three_groups_pages_of_32")
    good = run_shared(L, pkg, c, c.pools())[0]

    def change(p):
        if edit != "junk_member_entries":
            p.table[1, 3] = -1 if edit == "leader_minus_one" else p.pool_blocks
            return
        spare = sorted(set(range(p.pool_blocks)) - set(p.table.ravel()))[0]
        assert np.all(p.k[spare + 1] == NAN16)
        for b, (leader, P) in c.members.items():
            if b != leader:
                p.table[b, :P // c.bk] = [(-1, p.pool_blocks, spare)[j % 3] for j in range(P // c.bk)]

    p = c.pools(table_edit=change)
    out = run_shared(L, pkg, c, p)[0]
    same = list(range(c.bs)) if edit == "junk_member_entries" else [0, 6, 7, 8, 9, 10]
    assert np.all(np.isfinite(out)) and np.array_equal(out[same].view(np.uint32), good[same].view(np.uint32)) and p.guards_intact()


def test_against_the_paged_decode_entry_on_the_aliased_table(L, pkg, nso):
    """two kernel families, different operand rounding: both pass check(); the rel_l2 between them is printed (the docs record it) and is no bound"""
    c = step(nso, "b_three_groups_pages_of_64")
    p = c.pools()
    out, parent = run_shared(L, pkg, c, p)[0], run_paged(L, pkg, c, p, bias=0)
    named = sorted(c.members)
    parent[[b for b in range(c.bs) if b not in c.members]] = 7.0  # (the parent form serves every request)
    check_step(nso, "shared entry", c, out)
    check_step(nso, "paged decode entry", c, parent)
    print("ATTN_SHARED_PAGED against ns_hip_attn_decode_paged on the aliased table: rel_l2 %.3g" % nso.rel_l2(out[named], parent[named]))


def test_strided_unaligned_dst_with_the_fp16_shadow_and_the_callers_workspace(L, pkg, nso):
    """tmp of exactly the size function's bytes, with 256 bytes behind it that must stay as they were — and the tmp is what the partials went to"""
    import torch
    c = step(nso, "d_many_ranges_beside_a_short_group")
    p = c.pools()
    plain = run_shared(L, pkg, c, p)[0]
    size = L.ns_hip_attn_decode_paged_shared_workspace_size(c.bs, c.hn, c.hkv, c.hs, c.max_group, c.cap)
    assert size > 0 and size % 4 == 0
    tmp = torch.full((size + 256,), 0x5A, dtype=torch.uint8, device="cuda")
    out, o16, whole = run_shared(L, pkg, c, p, dst16=True, dst_pad=3, tmp=tmp)
    assert np.array_equal(out.view(np.uint32), plain.view(np.uint32)) and np.array_equal(o16[..., :c.hs], out.astype(np.float16))
    assert np.all(whole[..., c.hs:] == 7.0) and np.all(o16[..., c.hs:] == 7.0)  # the padding of every row
    t = tmp.cpu().numpy()
    assert np.all(t[size:] == 0x5A) and not np.all(t[:size] == 0x5A)


def test_captured_call_replayed_on_new_contents(L, pkg, nso):
    """One call captured ONCE (tmp given, after one eager call), replayed after the CONTENTS of all four device arrays changed: step 1 names other groups
    (6 alone, 7 .. 9, an empty one, 10 alone), moves three lengths and points the leader 7's first entry at request 1's first block.  Every replay, step
    0's again at the end, equals the eager call on the same contents bit for bit."""
    import torch
    c = step(nso, "b_three_groups_pages_of_32")
    steps = [(c.start, c.prefix, c.lens, 7), ([6, 7, 10, 10, 11], [0, 64, 999, 32], c.lens[:8] + [64, 130, 33], 1)]
    size = L.ns_hip_attn_decode_paged_shared_workspace_size(c.bs, c.hn, c.hkv, c.hs, c.max_group, c.cap)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        p = c.pools(nan_own=False)
        dq = torch.from_numpy(c.q.copy()).cuda()
        dev = [torch.zeros(n, dtype=torch.int32, device="cuda") for n in (len(c.start), len(c.prefix), c.bs)]
        outs = [torch.full((c.bs, 1, c.hn, c.hs), 7.0, device="cuda") for _ in range(2)]  # the captured call's and the eager call's, each with its tmp
        tmps = [torch.empty(size, dtype=torch.uint8, device="cuda") for _ in range(2)]
        call = lambda n: shared_call(L, pkg, c, p, dq.data_ptr(), outs[n].data_ptr(), dev, tmp=tmps[n])

        def move_to(s):
            for t, x in zip(dev, s[:3]):
                t.copy_(torch.tensor(x, dtype=torch.int32))
            p.dt[7, 0] = int(p.table[s[3], 0])

        move_to(steps[0])
        call(1)  # (one eager call in front of the capture: the kernels' code objects are in place)
        side.synchronize()
        s0 = shared_stats(L)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            call(0)
        assert delta(s0, shared_stats(L)) == [2, 0, 1, 0]  # (captured: two range launches and the merge; nothing has run)
        seen = []
        for n in (0, 1, 0):
            move_to(steps[n])
            for dst in outs:
                dst.fill_(7.0)
            g.replay()
            call(1)
            side.synchronize()
            assert torch.equal(outs[0], outs[1]) and bool(torch.all(torch.isfinite(outs[0]))), n
            seen.append(outs[0].cpu().numpy())
        assert np.array_equal(seen[0], seen[2]) and not np.array_equal(seen[0][7:10], seen[1][7:10])
        assert np.all(seen[1][:6] == 7.0) and not np.any(seen[1][6:] == 7.0)  # step 1 names requests 6 .. 10 only
        check_step(nso, "replayed step 0", c, seen[2])
    torch.cuda.synchronize()


def test_refusals_are_counted_and_write_nothing(L, pkg, nso):
    import torch
    c = step(nso, "a_suffix_of_one_key_across_a_range_and_empty")
    p = c.pools()
    dq = torch.from_numpy(c.q.copy()).cuda()
    dd = torch.full((c.bs, 1, c.hn, c.hs), 7.0, device="cuda")
    dev = [torch.tensor(x, dtype=torch.int32, device="cuda") for x in (c.start, c.prefix, c.lens)]

    def call(null=-1, groups=1, max_group=3, table=True, ts=p.ts, bk=c.bk, sl_q=1, hs=c.hs, flags=CAUSAL):
        a = pkg.attn_args(dq.data_ptr(), p.kp, p.vp, dd.data_ptr(), c.bs, c.hn, c.hkv, hs, sl_q, c.cap, c.scale, flags)
        a.step_k_sl = a.step_v_sl = p.step_sl
        ptrs = [None if n == null else C.c_void_p(t.data_ptr()) for n, t in enumerate(dev)]
        return L.ns_hip_attn_decode_paged_shared(C.byref(a), ptrs[0], groups, max_group, ptrs[1], ptrs[2], 0, C.c_void_p(p.dt.data_ptr()) if table else None, ts,
                                                 bk, p.pool_blocks, p.block_step, None, stream_ptr())

    calls = [("dGroupStart is null", dict(null=0)), ("dPrefixKeys is null", dict(null=1)), ("dKvLens is null", dict(null=2)),
             ("groups must be 1 .. 65535", dict(groups=0)), ("max_group, the most requests of one group", dict(max_group=0)), ("sl_q must be 1", dict(sl_q=2)),
             ("head_size must be 64 or 128", dict(hs=80)), ("ALiBi and the tanh cap are not served", dict(flags=CAUSAL | 2)),
             ("ALiBi and the tanh cap are not served", dict(flags=CAUSAL | 8)), ("groups * max_group above the grid limit", dict(groups=256, max_group=256)),
             ("block table is null", dict(table=False)), ("power of two from 16 to 256", dict(bk=48)), ("must equal table_stride * block_keys", dict(ts=p.ts - 1))]
    s0 = shared_stats(L)
    for n, (text, kw) in enumerate(calls):
        L.ns_hip_reset_error()
        assert call(**kw) == -1 and text in pkg.last_error(), (text, pkg.last_error())
        assert delta(s0, shared_stats(L)) == [0, 0, 0, n + 1]
    torch.cuda.synchronize()
    assert bool(torch.all(dd == 7.0)) and L.ns_hip_attn_decode_paged_shared_workspace_size(c.bs, c.hn, c.hkv, 80, 3, c.cap) == 0
    L.ns_hip_reset_error()

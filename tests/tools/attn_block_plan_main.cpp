// Program of tests/test_attn_block_plan.py: prints the plan attn_plan (neural-speed_amd/csrc/ns_attn_plan.cpp) makes for a grid of calls with the
// opt-in context-split block path (AttnKnobs::block_split) at a value and, for the same call, at 0 — one line each:
//   <the call, key=value> | <every field of the plan, key=value>
// Host code only: no HIP call is made, no tensor exists — the pointers are made-up addresses.
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "ns_attn.h"
#include "ns_attn_plan.cpp"

using namespace ns;

struct Case {
  int hs = 128, slq = 16, slkv = 2048, hn = 8, hkv = 8, bs = 1, flags = 0;
  int klay = 0;     // K / V: 0 head-major rows, 2 row stride hs + 4 (no multiple of 8), 3 position-major rows
  int cap = 0;      // > 0: a moving context length up to cap
  int bsplit = 1;   // AttnKnobs::block_split
  int target = AttnKnobs().block_target, minkeys = AttnKnobs().block_min_keys;  // the range rule's constants (the defaults: what ships)
  const char* knob = "none";  // a bool knob set beside it: no_mfma, v1, no_partials
};

static void run(const Case& c) {
  attn_fp32_fp16_fp16_fp32_fwd_args_t a;
  memset(&a, 0, sizeof(a));
  a.Q = reinterpret_cast<float*>(uintptr_t(0x10000));
  a.K = reinterpret_cast<decltype(a.K)>(uintptr_t(0x100000));
  a.V = reinterpret_cast<decltype(a.V)>(uintptr_t(0x200000));
  a.dst = reinterpret_cast<float*>(uintptr_t(0x300000));
  a.Q_sc = a.K_sc = a.V_sc = a.dst_sc = 1.f;
  a.QK_scale = 0.125f;
  a.attn_flags = c.flags;
  a.batch_size = c.bs, a.head_num = c.hn, a.heads_kv = c.hkv, a.head_size = c.hs, a.sl_q = c.slq, a.sl_kv = c.slkv;
  a.Q_layout = a.K_layout = a.V_layout = a.dst_layout = ATTN_FWD_LAYOUT_PLAIN;
  a.step_q_sl = a.step_dst_sl = c.hs;
  a.step_q_head_num = a.step_dst_head_num = c.slq * c.hs;
  a.step_q_bs = a.step_dst_bs = c.hn * c.slq * c.hs;
  const int rows = c.cap > 0 ? c.cap : c.slkv;  // the cache's rows
  const int row = c.klay == 2 ? c.hs + 4 : c.hs;
  a.step_k_head_size = a.step_v_head_size = 1;
  a.step_k_sl = a.step_v_sl = row;
  a.step_k_head_num = a.step_v_head_num = (long long)rows * row;
  a.step_k_bs = a.step_v_bs = (long long)c.hkv * rows * row;
  if (c.klay == 3) {  // position-major: the heads of a position side by side
    a.step_k_sl = a.step_v_sl = c.hkv * c.hs;
    a.step_k_head_num = a.step_v_head_num = c.hs;
  }
  static const int moving = 0;  // (only its address is used)
  Affine aff;
  if (c.cap > 0) aff.k = &moving, aff.delta = 1, aff.cap = c.cap, aff.inlaunch = 1;
  for (int on = 1; on >= 0; on--) {
    AttnKnobs kn;
    kn.block_split = on ? c.bsplit : 0;
    kn.block_target = c.target, kn.block_min_keys = c.minkeys;
    kn.no_mfma = !strcmp(c.knob, "no_mfma"), kn.v1 = !strcmp(c.knob, "v1"), kn.no_partials = !strcmp(c.knob, "no_partials");
    std::string why;
    const AttnPlan pl = attn_plan(a, nullptr, kn, aff, &why);
    const AttnSplitParams& sp = pl.sp;
    const size_t ws = attn_ws_bytes(kn, c.bs, c.hn, c.hkv, c.hs, c.slq, c.cap > 0 ? c.cap : c.slkv);
    const char* path[] = {"REFUSED", "GENERIC", "SPLIT_REGS", "RING", "ROWS64", "ROWS128", "PIPELINED", "BLOCK_SPLIT"};
    printf("hs=%d slq=%d slkv=%d hn=%d hkv=%d bs=%d flags=%d klay=%d cap=%d knob=%s target=%d minkeys=%d want=%d bsplit=%d | ", c.hs, c.slq, c.slkv, c.hn,
           c.hkv, c.bs, c.flags, c.klay, c.cap, c.knob, c.target, c.minkeys, c.bsplit, kn.block_split);
    printf("path=%s G=%d lpk=%d dpl=%d hsp=%d sb=%d pad=%d grid=%u,%u,%u block=%u lds=%zu nsplit=%d kps=%d chunks=%d gfull=%d hf=%d dyn=%d,%d,%d tick=%d merge=%d "
           "pbytes=%zu nqb=%d al=%d xcd=%d kmove=%d kdelta=%d phs=%d qk=%g ws=%zu why=%s\n",
           path[pl.path], pl.G, pl.lpk, pl.dpl, pl.hs_pad, pl.sb, pl.pad, pl.grid.x, pl.grid.y, pl.grid.z, pl.block.x, pl.lds, sp.nsplit, sp.keys_per_split,
           sp.chunks, sp.g_full, sp.heads_first, sp.dyn_min_keys, sp.dyn_batch_keys, sp.dyn_single_below, int(pl.want_tickets), int(pl.merge),
           pl.partial_bytes, pl.nqb, pl.aligned, pl.xcd_map, sp.kmove != nullptr, sp.kdelta, sp.a.hs_pad, double(sp.a.qk_scale), ws, why.c_str());
  }
}

int main() {
  const int rows[] = {1, 2, 5, 15, 16, 64, 127, 128}, keys[] = {255, 256, 257, 300, 1000, 2048, 8192};
  const int groups[][2] = {{8, 8}, {8, 2}, {8, 1}, {71, 1}};  // (heads, kv heads)
  const int flags[] = {0, NS_ATTN_FLAG_IS_CAUSAL, NS_ATTN_FLAG_IS_ALIBI8, NS_ATTN_FLAG_IS_TANH30};
  // 1. every shape, flag and batch, contiguous aligned tensors, the key at 1 (on from 256 keys)
  for (int slq : rows)
    for (int slkv : keys)
      for (const auto& g : groups)
        for (int hs : {64, 80, 128, 256})
          for (int f : flags)
            for (int bs : {1, 2, 8}) {
              Case c;
              c.hs = hs, c.slq = slq, c.slkv = slkv, c.hn = g[0], c.hkv = g[1], c.flags = f, c.bs = bs;
              run(c);
            }
  // 2. over a smaller set of shapes: the threshold, a position-major cache, rows that are not 16-byte aligned, a moving length, the knobs that
  // keep the matrix cores / the partials away, other constants of the range rule
  for (int slq : {1, 2, 16, 100})
    for (int slkv : {256, 1000, 1023, 1024, 2048})
      for (const auto& g : {groups[0], groups[1], groups[3]}) {
        Case b;
        b.slq = slq, b.slkv = slkv, b.hn = g[0], b.hkv = g[1], b.flags = NS_ATTN_FLAG_IS_CAUSAL;
        for (int bsplit : {-5, 1024, 2048, 100000}) {
          Case c = b;
          c.bsplit = bsplit;
          run(c);
        }
        for (int klay : {2, 3}) {
          Case c = b;
          c.klay = klay;
          run(c);
        }
        Case m = b;
        m.cap = 4096;
        run(m);
        for (const char* knob : {"no_mfma", "v1", "no_partials"}) {
          Case c = b;
          c.knob = knob;
          run(c);
        }
        for (int target : {128, 1024})
          for (int minkeys : {64, 256}) {
            Case c = b;
            c.target = target, c.minkeys = minkeys;
            run(c);
          }
      }
  // 3. single cases: more (kv head, slot block) pairs than the grid's x takes; one range only (so many workgroups that the rule asks for no split)
  Case c;
  c.hn = c.hkv = 40000, c.slq = 127, c.slkv = 512, c.target = 1 << 20;  // (a target that asks for ranges at any number of workgroups)
  run(c);
  c.slq = 64;
  run(c);
  c = Case(), c.hn = c.hkv = 64, c.bs = 8, c.slq = 16, c.slkv = 4096;  // 512 workgroups per range: the target
  run(c);
  return 0;
}

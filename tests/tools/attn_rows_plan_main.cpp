// Program of tests/test_attn_rows_plan.py: prints, for a grid of decode calls, the plan attn_plan (neural-speed_amd/csrc/ns_attn_plan.cpp) makes for
// the per-request form (ns_hip_attn_decode_rows: Affine::rows, one live length per batch entry, sl_kv = the capacity of a request's slab) and the plan
// of the existing moving-length form of the same shape (one length per launch, Affine::cap = the capacity) — two lines per call:
//   <the call, key=value> | <every field of the plan, key=value>
// For the per-request plan it walks every live length 0 .. capacity of a request through attn_live_kv<true> / attn_live_kps / attn_live_splits
// (ns_attn.h: the functions the kernels run) and prints what must hold of the live ranges: viol counts the lengths at which they do not tile
// [0, len) exactly once, or are more than the launch has workgroups for; laid counts the lengths at which the ranges are NOT those laid out.
// Host code only: no HIP call is made, no tensor exists — the pointers are made-up addresses.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <vector>

#include "ns_attn.h"
#include "ns_attn_plan.cpp"

using namespace ns;

struct Case {
  int hs = 128, slq = 1, cap = 2048, hn = 8, hkv = 8, bs = 1, flags = 0;
  int klay = 0;     // K / V: 0 head-major rows, 1 transposed K, 2 row stride hs + 4 halves, 3 position-major rows
  int dyn = 1;      // AttnKnobs::dyn_ranges
  int stream = 1;   // AttnKnobs::attn_stream
  int inl = 0;      // AttnKnobs::attn_inlaunch
  int bias = 1;
};

static void print_plan(const Case& c, const char* form, const AttnPlan& pl, size_t ws, long long viol, long long laid, unsigned long long sum,
                       const std::string& why) {
  const AttnSplitParams& sp = pl.sp;
  const char* path[] = {"REFUSED", "GENERIC", "SPLIT_REGS", "RING", "ROWS64", "ROWS128", "PIPELINED", "BLOCK_SPLIT"};
  printf("form=%s hs=%d slq=%d cap=%d hn=%d hkv=%d bs=%d flags=%d klay=%d dynr=%d stream=%d inl=%d bias=%d | ", form, c.hs, c.slq, c.cap, c.hn, c.hkv, c.bs,
         c.flags, c.klay, c.dyn, c.stream, c.inl, c.bias);
  printf("path=%s G=%d lpk=%d dpl=%d grid=%u,%u,%u block=%u lds=%zu nsplit=%d kps=%d chunks=%d gfull=%d hf=%d dyn=%d,%d,%d tick=%d merge=%d pbytes=%zu "
         "kmove=%d kdelta=%d rows=%d slkv=%d ws=%zu viol=%lld laid=%lld sum=%llu why=%s\n",
         path[pl.path], pl.G, pl.lpk, pl.dpl, pl.grid.x, pl.grid.y, pl.grid.z, pl.block.x, pl.lds, sp.nsplit, sp.keys_per_split, sp.chunks, sp.g_full,
         sp.heads_first, sp.dyn_min_keys, sp.dyn_batch_keys, sp.dyn_single_below, int(pl.want_tickets), int(pl.merge), pl.partial_bytes,
         sp.kmove != nullptr, sp.kdelta, int(pl.rows), sp.a.sl_kv, ws, viol, laid, sum, why.c_str());
}

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
  a.batch_size = c.bs, a.head_num = c.hn, a.heads_kv = c.hkv, a.head_size = c.hs, a.sl_q = c.slq, a.sl_kv = c.cap;
  a.Q_layout = a.K_layout = a.V_layout = a.dst_layout = ATTN_FWD_LAYOUT_PLAIN;
  a.step_q_sl = a.step_dst_sl = c.hs;
  a.step_q_head_num = a.step_dst_head_num = c.slq * c.hs;
  a.step_q_bs = a.step_dst_bs = c.hn * c.slq * c.hs;
  const int rows = std::max(c.cap, 1);
  const int row = c.klay == 2 ? c.hs + 4 : c.hs;
  a.step_k_head_size = a.step_v_head_size = 1;
  a.step_k_sl = a.step_v_sl = row;
  a.step_k_head_num = a.step_v_head_num = rows * row;
  a.step_k_bs = a.step_v_bs = c.hkv * rows * row;
  if (c.klay == 1) a.step_k_head_size = rows, a.step_k_sl = 1;
  if (c.klay == 3) {  // position-major: the heads of a position side by side
    a.step_k_sl = a.step_v_sl = c.hkv * c.hs;
    a.step_k_head_num = a.step_v_head_num = c.hs;
  }
  AttnKnobs kn;
  kn.dyn_ranges = c.dyn != 0, kn.attn_stream = c.stream, kn.attn_inlaunch = c.inl;
  std::vector<int> lens(size_t(std::max(c.bs, 1)), 0);  // the device array, here on the host: attn_live_kv<true> reads it
  const size_t ws = attn_ws_bytes(kn, c.bs, c.hn, c.hkv, c.hs, c.slq, c.cap);

  Affine rows_aff;  // what ns_hip_attn_decode_rows builds
  rows_aff.k = lens.data(), rows_aff.delta = 1, rows_aff.cap = c.cap, rows_aff.inlaunch = 0, rows_aff.rows = 1, rows_aff.bias = c.bias;
  std::string why;
  const AttnPlan pl = attn_plan(a, nullptr, kn, rows_aff, &why);
  long long viol = 0, laid = 0;
  unsigned long long sum = 0;
  if (pl.path != AP_REFUSED) {
    const AttnSplitParams& sp = pl.sp;
    const int b = c.bs - 1;  // the last request's slot; every other slot holds another length meanwhile
    for (int len = 0; len <= c.cap; len++) {
      for (int x = 0; x < c.bs; x++) lens[size_t(x)] = (len * 7 + x * 13) % (c.cap + 1) - c.bias;
      lens[size_t(b)] = len - c.bias;
      const int live_kv = attn_live_kv<true>(sp, b);
      viol += live_kv != len;
      const int kps = attn_live_kps(sp, live_kv), n = attn_live_splits(sp, live_kv);
      // the ranges the workgroups take: [s * kps, min(len, (s + 1) * kps)) for s < n — they tile [0, len) exactly once when none is empty but a
      // lone range over no key, and the last one reaches len
      long long covered = 0;
      for (int s = 0; s < n; s++) {
        const int j0 = s * kps, j1 = std::min(len, j0 + kps);
        viol += (j1 <= j0 && len > 0);
        covered += std::max(0, j1 - j0);
      }
      viol += (covered != len) + (n > sp.nsplit) + (n < 1) + (kps < 1);
      laid += (kps != sp.keys_per_split) || (n != std::max(1, (len + sp.keys_per_split - 1) / sp.keys_per_split));
      sum += ((unsigned long long)n * 65537ull + (unsigned long long)kps) * (unsigned long long)(len + 1);
    }
    // beyond both ends of the clamp
    lens[size_t(b)] = c.cap + 100 - c.bias;
    viol += attn_live_kv<true>(sp, b) != c.cap;
    lens[size_t(b)] = -3 - c.bias;
    viol += attn_live_kv<true>(sp, b) != 0;
    lens[size_t(b)] = 0x7fffffff;
    viol += attn_live_kv<true>(sp, b) != c.cap;
  }
  print_plan(c, "rows", pl, ws, viol, laid, sum, why);

  static const int moving = 0;  // (only its address is used)
  Affine aff;                   // the replayed route's form of the same shape, merge by the knob
  aff.k = &moving, aff.delta = 1, aff.cap = c.cap, aff.inlaunch = 0;
  std::string why2;
  const AttnPlan pm = attn_plan(a, nullptr, kn, aff, &why2);
  print_plan(c, "moving", pm, ws, 0, 0, 0, why2);
}

int main() {
  const int groups[][2] = {{8, 8}, {8, 2}, {8, 1}, {71, 1}};  // (heads, kv heads)
  // 1. the grid of calls
  for (int bs : {1, 2, 8, 33})
    for (const auto& g : groups)
      for (int hs : {32, 64, 80, 128, 256})
        for (int cap : {1, 255, 256, 300, 2048, 8192}) {
          Case c;
          c.bs = bs, c.hn = g[0], c.hkv = g[1], c.hs = hs, c.cap = cap;
          run(c);
        }
  // 2. over a smaller set: ranges as laid out (dyn_ranges off), the register kernel where the ring would serve, the merge inside the launch, a
  // position-major cache, flags, another bias
  for (int bs : {1, 8})
    for (const auto& g : {groups[0], groups[1], groups[3]})
      for (int hs : {64, 128, 256})
        for (int cap : {300, 2048, 8192}) {
          Case b;
          b.bs = bs, b.hn = g[0], b.hkv = g[1], b.hs = hs, b.cap = cap;
          Case c = b;
          c.dyn = 0;
          run(c);
          c = b, c.stream = 0;
          run(c);
          c = b, c.inl = 1;
          run(c);
          c = b, c.klay = 3;
          run(c);
          c = b, c.flags = NS_ATTN_FLAG_IS_CAUSAL | NS_ATTN_FLAG_IS_ALIBI8;
          run(c);
          c = b, c.bias = 0;
          run(c);
        }
  // 3. the refusals
  Case c;
  c.slq = 2;
  run(c);
  c = Case(), c.klay = 2;
  run(c);
  c = Case(), c.klay = 1;
  run(c);
  c = Case(), c.cap = 0;
  run(c);
  return 0;
}

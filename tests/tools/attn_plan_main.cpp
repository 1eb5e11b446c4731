// Program of tests/test_attn_plan.py: prints the plan attn_plan (neural-speed_amd/csrc/ns_attn_plan.cpp) makes for a fixed grid of calls, one line
// each:  <the call, key=value> | <every field of the plan, key=value>.  For a plan with a moving context length it walks every live length through
// attn_live_kps / attn_live_splits (ns_attn.h, the functions the kernels run) and prints the violations and a checksum of what they returned.
// Host code only: no HIP call is made, no tensor exists — the pointers are made-up addresses.
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "ns_attn.h"
#include "ns_attn_plan.cpp"

using namespace ns;

struct Case {
  int hs = 128, slq = 1, slkv = 2048, hn = 8, hkv = 8, bs = 1, flags = 0;
  int klay = 0;  // K / V: 0 head-major rows, 1 transposed K, 2 row stride hs + 4 (no multiple of 8), 3 position-major rows, 4 rows 2^24 halves apart,
                 // 5 position-major rows ksl halves apart (0: dense) and batch entries kbs halves apart (0: dense) — tests/tools/attn_far_layout.py
  long long ksl = 0, kbs = 0;
  int qal = 1, dal = 1, d16 = 0;  // Q / dst 16-byte aligned; fp16 shadow: 0 none, 1 aligned, 2 not
  float scale = 0.125f;
  const char* knob = "none";
  int kval = 0;
  int cap = 0;       // > 0: a moving context length up to cap
  int affil = 1;     // Affine::inlaunch
};

static void run(const Case& c) {
  attn_fp32_fp16_fp16_fp32_fwd_args_t a;
  memset(&a, 0, sizeof(a));
  a.Q = reinterpret_cast<float*>(uintptr_t(0x10000) + (c.qal ? 0 : 4));
  a.K = reinterpret_cast<decltype(a.K)>(uintptr_t(0x100000));
  a.V = reinterpret_cast<decltype(a.V)>(uintptr_t(0x200000));
  a.dst = reinterpret_cast<float*>(uintptr_t(0x300000) + (c.dal ? 0 : 4));
  const void* dst16 = c.d16 ? reinterpret_cast<const void*>(uintptr_t(0x400000) + (c.d16 == 2 ? 2 : 0)) : nullptr;
  a.Q_sc = a.K_sc = a.V_sc = a.dst_sc = 1.f;
  a.QK_scale = c.scale;
  a.attn_flags = c.flags;
  a.batch_size = c.bs, a.head_num = c.hn, a.heads_kv = c.hkv, a.head_size = c.hs, a.sl_q = c.slq, a.sl_kv = c.slkv;
  a.Q_layout = a.K_layout = a.V_layout = a.dst_layout = ATTN_FWD_LAYOUT_PLAIN;
  a.step_q_sl = a.step_dst_sl = c.hs;
  a.step_q_head_num = a.step_dst_head_num = c.slq * c.hs;
  a.step_q_bs = a.step_dst_bs = c.hn * c.slq * c.hs;
  const int rows = c.cap > 0 ? c.cap : c.slkv;  // the cache's rows
  const int row = c.klay == 2 ? c.hs + 4 : c.klay == 4 ? 1 << 24 : c.hs;
  a.step_k_head_size = a.step_v_head_size = 1;
  a.step_k_sl = a.step_v_sl = row;
  a.step_k_head_num = a.step_v_head_num = (long long)rows * row;
  a.step_k_bs = a.step_v_bs = (long long)c.hkv * rows * row;
  if (c.klay == 1) a.step_k_head_size = rows, a.step_k_sl = 1;
  if (c.klay == 3 || c.klay == 4) {  // position-major: the heads of a position side by side
    if (c.klay == 3) a.step_k_sl = a.step_v_sl = c.hkv * c.hs;
    a.step_k_head_num = a.step_v_head_num = c.hs;
    if (c.klay == 4) a.step_k_bs = a.step_v_bs = c.hkv * c.hs;  // (strides that fit the arguments' ints; nothing is read)
  }
  if (c.klay == 5) {
    a.step_k_head_num = a.step_v_head_num = c.hs;
    a.step_k_sl = a.step_v_sl = int(c.ksl ? c.ksl : (long long)c.hkv * c.hs);
    a.step_k_bs = a.step_v_bs = int(c.kbs ? c.kbs : (long long)c.hkv * rows * c.hs);
  }
  AttnKnobs kn;
  const struct {
    const char* name;
    int* field;
  } ints[] = {{"attn_stream", &kn.attn_stream}, {"attn_mfma2_rows", &kn.attn_mfma2_rows}, {"attn_inlaunch", &kn.attn_inlaunch},
              {"attn_heads_first", &kn.attn_heads_first}, {"wg_target", &kn.wg_target}, {"min_keys", &kn.min_keys}, {"wg_target_s", &kn.wg_target_s},
              {"min_keys_s", &kn.min_keys_s}, {"pipe", &kn.pipe}, {"pvar", &kn.pvar}, {"alibi_heads", &kn.alibi_heads}};
  for (const auto& e : ints)
    if (!strcmp(c.knob, e.name)) *e.field = c.kval;
  if (!strcmp(c.knob, "alibi_heads")) kn.alibi_off = c.kval - c.hn;  // this rank's heads are the last of the model's (kval < hn: refused)
  const struct {
    const char* name;
    bool* field;
  } bools[] = {{"no_mfma", &kn.no_mfma}, {"no_xcd_map", &kn.no_xcd_map}, {"v1", &kn.v1}, {"dyn_ranges", &kn.dyn_ranges}, {"no_partials", &kn.no_partials}};
  for (const auto& e : bools)
    if (!strcmp(c.knob, e.name)) *e.field = c.kval != 0;
  static const int moving = 0;  // (only its address is used)
  Affine aff;
  if (c.cap > 0) aff.k = &moving, aff.delta = 1, aff.cap = c.cap, aff.inlaunch = c.affil;
  std::string why;
  const AttnPlan pl = attn_plan(a, dst16, kn, aff, &why);
  const AttnSplitParams& sp = pl.sp;
  // every live length of a moving plan through the functions the kernels run
  long long viol = 0;
  unsigned long long sum = 0;
  if (c.cap > 0 && pl.path != AP_REFUSED && sp.nsplit > 1)
    for (int len = 1; len <= c.cap; len++) {
      const int kps = attn_live_kps(sp, len), n = attn_live_splits(sp, len);
      viol += (n > sp.nsplit) + ((long long)n * kps < len);
      sum += ((unsigned long long)n * 65537ull + (unsigned long long)kps) * (unsigned long long)len;
    }
  const size_t ws = attn_ws_bytes(kn, c.bs, c.hn, c.hkv, c.hs, c.slq, c.cap > 0 ? c.cap : c.slkv);
  const char* path[] = {"REFUSED", "GENERIC", "SPLIT_REGS", "RING", "ROWS64", "ROWS128", "PIPELINED"};
  printf("hs=%d slq=%d slkv=%d hn=%d hkv=%d bs=%d flags=%d klay=%d qal=%d dal=%d d16=%d scale=%g knob=%s kval=%d cap=%d affil=%d ksl=%lld kbs=%lld | ", c.hs,
         c.slq, c.slkv, c.hn, c.hkv, c.bs, c.flags, c.klay, c.qal, c.dal, c.d16, double(c.scale), c.knob, c.kval, c.cap, c.affil, c.ksl, c.kbs);
  printf("path=%s G=%d lpk=%d dpl=%d hsp=%d sb=%d pad=%d grid=%u,%u,%u block=%u lds=%zu nsplit=%d kps=%d chunks=%d gfull=%d hf=%d dyn=%d,%d,%d tick=%d merge=%d "
         "pbytes=%zu nqb=%d al=%d xcd=%d kmove=%d kdelta=%d phs=%d off=%d lf=%d qk=%g ws=%zu viol=%lld sum=%llu why=%s\n",
         path[pl.path], pl.G, pl.lpk, pl.dpl, pl.hs_pad, pl.sb, pl.pad, pl.grid.x, pl.grid.y, pl.grid.z, pl.block.x, pl.lds, sp.nsplit, sp.keys_per_split,
         sp.chunks, sp.g_full, sp.heads_first, sp.dyn_min_keys, sp.dyn_batch_keys, sp.dyn_single_below, int(pl.want_tickets), int(pl.merge),
         pl.partial_bytes, pl.nqb, pl.aligned, pl.xcd_map, sp.kmove != nullptr, sp.kdelta, sp.a.hs_pad, sp.a.alibi_head_off, sp.a.alibi_log2_floor,
         double(sp.a.qk_scale), ws, viol, sum, why.c_str());
}

int main() {
  const int head_sizes[] = {24, 32, 40, 64, 80, 128, 160, 256}, rows[] = {1, 4, 15, 16, 64, 127, 128, 257};
  const int keys[] = {1, 128, 129, 600, 2048, 3071, 3072, 5000};
  const int groups[][2] = {{8, 8}, {8, 4}, {8, 2}, {8, 1}, {71, 1}};  // (heads, kv heads)
  const int flags[] = {0, NS_ATTN_FLAG_IS_CAUSAL, NS_ATTN_FLAG_IS_ALIBI8, NS_ATTN_FLAG_IS_TANH30};
  const struct {
    const char* name;
    int value;
  } knobs[] = {{"none", 0}, {"attn_stream", 0}, {"attn_mfma2_rows", 64}, {"attn_inlaunch", 1}, {"attn_heads_first", 0}, {"attn_heads_first", 1},
               {"wg_target", 512}, {"min_keys", 64}, {"wg_target_s", 128}, {"min_keys_s", 64}, {"pipe", 0}, {"pvar", 1}, {"no_mfma", 1},
               {"no_xcd_map", 1}, {"v1", 1}, {"dyn_ranges", 0}, {"no_partials", 1}, {"alibi_heads", 142}, {"alibi_heads", 4}};
  // 1. every shape and flag, batch 1, contiguous aligned tensors, default knobs
  for (int hs : head_sizes)
    for (int slq : rows)
      for (int slkv : keys)
        for (const auto& g : groups)
          for (int f : flags) {
            Case c;
            c.hs = hs, c.slq = slq, c.slkv = slkv, c.hn = g[0], c.hkv = g[1], c.flags = f;
            run(c);
          }
  // 2. batch, layouts, alignment, the fp16 shadow and every knob over a smaller set of shapes
  for (int hs : {32, 64, 80, 128, 256})
    for (int slq : {1, 16, 64, 128, 257})
      for (int slkv : {129, 600, 3072})
        for (const auto& g : {groups[0], groups[2], groups[4]}) {
          Case b;
          b.hs = hs, b.slq = slq, b.slkv = slkv, b.hn = g[0], b.hkv = g[1];
          for (int bs : {2, 8}) {
            Case c = b;
            c.bs = bs;
            run(c);
          }
          for (int klay : {1, 2, 3}) {
            Case c = b;
            c.klay = klay;
            run(c);
          }
          for (int al = 0; al < 4; al++) {
            Case c = b;
            c.qal = al & 1, c.dal = al >> 1, c.d16 = al == 3 ? 1 : 2;
            run(c);
          }
          for (const auto& k : knobs)
            for (int klay : {0, 3})
              for (int f : {0, int(NS_ATTN_FLAG_IS_ALIBI8)}) {
                Case c = b;
                c.knob = k.name, c.kval = k.value, c.klay = klay, c.flags = f;
                run(c);
              }
          for (float scale : {-1.f, 0.f}) {
            Case c = b;
            c.scale = scale;
            run(c);
          }
        }
  // 3. a moving context length (decode steps of a replayed route), with and without the merge inside the launch
  for (int hs : {32, 64, 128, 256})
    for (int cap : {128, 600, 2048, 5000})
      for (const auto& g : groups)
        for (int bs : {1, 8})
          for (const auto& k : {knobs[0], knobs[1], knobs[8], knobs[9], knobs[15]})
            for (int affil : {1, 0}) {
              Case c;
              c.hs = hs, c.slkv = cap < 600 ? cap : 600, c.cap = cap, c.hn = g[0], c.hkv = g[1], c.bs = bs, c.knob = k.name, c.kval = k.value, c.affil = affil;
              run(c);
            }
  // 4. single cases: refusals, rows beyond a 32-bit descriptor, the grid limit of the split kernels
  Case c;
  c.slq = 2, c.cap = 4096;  // a moving length with two query rows
  run(c);
  c = Case(), c.slkv = 2048, c.cap = 1024;  // ... beyond the cache
  run(c);
  c = Case(), c.hs = 257;
  run(c);
  c = Case(), c.hn = 6, c.hkv = 4;
  run(c);
  c = Case(), c.slq = 4, c.slkv = 2, c.flags = NS_ATTN_FLAG_IS_CAUSAL;
  run(c);
  c = Case(), c.slkv = 0;
  run(c);
  c = Case(), c.hn = c.hkv = 65536;
  run(c);
  c = Case(), c.bs = 65536;
  run(c);
  for (int slq : {1, 128, 257}) {
    c = Case(), c.klay = 4, c.slq = slq, c.slkv = 128;  // in32 false
    run(c);
    c.slkv = 127;                                       // ... and just inside for its keys, not for the 128 rows of its two tiles
    run(c);
    c.slkv = 64;                                        // ... inside for both
    run(c);
  }
  // the addresses of tests/test_gpu_attn_far_addresses.py (tests/tools/attn_far_layout.py states the same numbers; 4 / 2 heads, causal): 300 keys at the
  // largest row step inside a descriptor and one step of 8 more, for the keys (the ring kernel's rule) and for the 320 rows of their five tiles
  // (attn_mfma3_kernel's); batch entries 2^30 + 2^21 halves apart, which no rule looks at
  const long long edge300 = ((1ll << 31) - 257) / 300 / 8 * 8, edge320 = ((1ll << 31) - 257) / 320 / 8 * 8;
  for (int hs : {64, 128}) {
    Case f;
    f.hs = hs, f.hn = 4, f.hkv = 2, f.flags = NS_ATTN_FLAG_IS_CAUSAL, f.klay = 5, f.slkv = 300;
    for (long long ksl : {edge300, edge300 + 8}) {
      c = f, c.slq = 1, c.ksl = ksl;
      run(c);
    }
    for (long long ksl : {edge320, edge320 + 8, edge300}) {
      c = f, c.slq = 130, c.ksl = ksl;
      run(c);
    }
    for (int slq : {1, 5, 40, 130}) {
      c = f, c.slq = slq, c.slkv = 200, c.bs = 3, c.kbs = (1ll << 30) + (1ll << 21);
      run(c);
    }
  }
  c = Case(), c.hn = c.hkv = 8192, c.slq = 15;  // 122880 workgroups per range: past the grid's y
  run(c);
  c.slq = 7;
  run(c);
  return 0;
}

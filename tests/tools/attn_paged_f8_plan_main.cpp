// Program of tests/test_attn_paged_f8_plan.py: attn_decode_paged_f8_plan (neural-speed_amd/csrc/ns_attn_plan.cpp) beside the paged fp16 plan of the same
// shape and capacity, and the writers' conversion (e4m3_cell, ns_attn.h).  Host code only.  Lines:
//   plan   <the call> | <the fields of the FP8 plan> | <the fields of the fp16 paged plan>
//   rule   pool_blocks=.. block_step=.. hs=.. | path=.. f8=.. why=..
//   refuse what=.. | path=.. why=..
// With the argument "codes <scale>": one line of 65536 hex bytes, e4m3_cell of every fp16 bit pattern under 1.0f / scale.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

#include "ns_attn.h"
#include "ns_attn_plan.cpp"

using namespace ns;

struct Case {
  int hs = 128, cap = 2048, hn = 8, hkv = 8, bs = 1, bk = 16, head_major = 0;
  int pool_blocks = 0;       // 0: one block per table entry and four spare
  long long block_step = 0;  // 0: a block's own size
  long long step_sl = 0;     // 0: by the layout
  uintptr_t kbase = 0x100000;
  float k_sc = 1.f;
  bool null_table = false;
};
static const int g_lens[64] = {0};
static const int g_table[1] = {0};  // (only its address is used by a plan)

static AttnPlan plan(const Case& c, bool f8, std::string* why) {
  attn_fp32_fp16_fp16_fp32_fwd_args_t a;
  memset(&a, 0, sizeof(a));
  a.Q = reinterpret_cast<float*>(uintptr_t(0x10000));
  a.K = reinterpret_cast<decltype(a.K)>(c.kbase);
  a.V = reinterpret_cast<decltype(a.V)>(uintptr_t(0x200000));
  a.dst = reinterpret_cast<float*>(uintptr_t(0x300000));
  a.Q_sc = a.V_sc = a.dst_sc = 1.f, a.K_sc = c.k_sc;
  a.QK_scale = 0.125f;
  a.attn_flags = NS_ATTN_FLAG_IS_CAUSAL;
  a.batch_size = c.bs, a.head_num = c.hn, a.heads_kv = c.hkv, a.head_size = c.hs, a.sl_q = 1, a.sl_kv = c.cap;
  a.Q_layout = a.K_layout = a.V_layout = a.dst_layout = ATTN_FWD_LAYOUT_PLAIN;
  a.step_q_sl = a.step_dst_sl = a.step_q_head_num = a.step_dst_head_num = c.hs;
  a.step_q_bs = a.step_dst_bs = c.hn * c.hs;
  a.step_k_head_size = a.step_v_head_size = 1;
  a.step_k_sl = a.step_v_sl = c.step_sl ? c.step_sl : (c.head_major ? c.hs : c.hkv * c.hs);
  a.step_k_head_num = a.step_v_head_num = c.head_major ? (long long)c.bk * c.hs : c.hs;
  AttnPage pg;
  pg.table = c.null_table ? nullptr : g_table;
  pg.block_shift = attn_block_shift(c.bk);
  pg.table_stride = c.cap / c.bk;
  pg.pool_blocks = c.pool_blocks ? c.pool_blocks : pg.table_stride * c.bs + 4;
  pg.block_step = c.block_step ? c.block_step : (long long)c.bk * c.hkv * c.hs;
  if (f8) return attn_decode_paged_f8_plan(a, nullptr, AttnKnobs(), g_lens, 1, pg, why);
  Affine aff;  // what ns_hip_attn_decode_paged builds
  aff.k = g_lens, aff.delta = 1, aff.cap = c.cap, aff.inlaunch = 0, aff.rows = 1, aff.bias = 1;
  return attn_plan(a, nullptr, AttnKnobs(), aff, why, &pg);
}

static void print_fields(const AttnPlan& pl, const std::string& why) {
  const AttnSplitParams& sp = pl.sp;
  const char* path[] = {"REFUSED", "GENERIC", "SPLIT_REGS", "RING", "ROWS64", "ROWS128", "PIPELINED", "BLOCK_SPLIT"};
  printf("path=%s f8=%d G=%d lpk=%d dpl=%d grid=%u,%u,%u block=%u lds=%zu nsplit=%d kps=%d chunks=%d gfull=%d hf=%d dyn=%d,%d,%d tick=%d merge=%d "
         "pbytes=%zu kmove=%d kdelta=%d rows=%d paged=%d slkv=%d kbs=%lld blocks=%d bstep=%lld qk=%a out=%a why=%s",
         path[pl.path], int(pl.f8), pl.G, pl.lpk, pl.dpl, pl.grid.x, pl.grid.y, pl.grid.z, pl.block.x, pl.lds, sp.nsplit, sp.keys_per_split, sp.chunks,
         sp.g_full, sp.heads_first, sp.dyn_min_keys, sp.dyn_batch_keys, sp.dyn_single_below, int(pl.want_tickets), int(pl.merge), pl.partial_bytes,
         sp.kmove != nullptr, sp.kdelta, int(pl.rows), int(pl.paged), sp.a.sl_kv, (long long)sp.a.step_k_bs, pl.page.pool_blocks, pl.page.block_step,
         sp.a.qk_scale, sp.a.out_scale, why.c_str());
}
static void run_pair(const char* kind, const char* what, const Case& c, bool both) {
  std::string why8, why16;
  const AttnPlan p8 = plan(c, true, &why8);
  printf("%s what=%s hs=%d cap=%d hn=%d hkv=%d bs=%d bk=%d hm=%d | ", kind, what, c.hs, c.cap, c.hn, c.hkv, c.bs, c.bk, c.head_major);
  print_fields(p8, why8);
  if (both) {
    printf(" | ");
    print_fields(plan(c, false, &why16), why16);
  }
  printf("\n");
}

int main(int argc, char** argv) {
  if (argc == 3 && !strcmp(argv[1], "codes")) {
    const float inv = 1.0f / float(atof(argv[2]));
    for (unsigned b = 0; b < 65536; b++) {
      const unsigned short bits = (unsigned short)b;
      _Float16 h;
      memcpy(&h, &bits, 2);
      printf("%02x", e4m3_cell(h, inv));
    }
    printf("\n");
    return 0;
  }
  const int groups[][2] = {{8, 8}, {8, 2}, {8, 1}, {71, 1}};  // the grid of tests/tools/attn_paged_plan_main.cpp
  int n = 0;
  for (int bk : {16, 32, 128, 256})
    for (int bs : {1, 2, 8, 33})
      for (const auto& g : groups)
        for (int hs : {32, 64, 80, 128, 256})
          for (int cap : {1, 255, 256, 300, 2048, 8192}) {
            Case c;
            c.bs = bs, c.hn = g[0], c.hkv = g[1], c.hs = hs, c.bk = bk, c.cap = (cap + bk - 1) / bk * bk, c.head_major = n++ & 1;
            run_pair("plan", "grid", c, true);
          }
  // the byte rule, pool_blocks * block_step + 256 < 2^32: one pool either side (and the fp16 rule's own boundary, which must not matter)
  const long long step = 128ll * 8 * 128, limit = (1ll << 32) - 256;
  for (int hs : {128, 256})
    for (long long blocks : {((1ll << 31) - 256) / step, ((1ll << 31) - 256) / step + 1, (limit - 1) / step, (limit - 1) / step + 1}) {
      Case c;
      c.hs = hs, c.bk = 128, c.pool_blocks = int(blocks), c.block_step = hs == 128 ? step : 2 * step;
      run_pair("rule", "pool", c, false);
    }
  Case c;
  run_pair("refuse", "none", c, false);
  c = Case(), c.hs = 72, c.hn = c.hkv = 8;
  run_pair("refuse", "head_size", c, false);
  c = Case(), c.step_sl = 8 * 128 + 8, c.block_step = 16 * (8 * 128 + 8);
  run_pair("refuse", "step_sl", c, false);
  c = Case(), c.block_step = 16 * 8 * 128 + 8;
  run_pair("refuse", "block_step", c, false);
  c = Case(), c.kbase = 0x100008;
  run_pair("refuse", "base", c, false);
  c = Case(), c.k_sc = 0.f;
  run_pair("refuse", "scale", c, false);
  c = Case(), c.null_table = true;
  run_pair("refuse", "null_table", c, false);
  c = Case(), c.pool_blocks = -1;
  run_pair("refuse", "pool_blocks", c, false);
  c = Case(), c.block_step = 16 * 8 * 128 - 16;
  run_pair("refuse", "block_step_small", c, false);
  c = Case(), c.bk = 8, c.cap = 2048;
  run_pair("refuse", "block_keys_8", c, false);
  return 0;
}

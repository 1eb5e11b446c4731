// Program of tests/test_attn_prefill_paged_wide_f8_plan.py: the plan of ns_hip_attn_prefill_paged_wide_f8 (attn_prefill_paged_wide_f8_plan,
// neural-speed_amd/csrc/ns_attn_plan.cpp) beside the fp16 wide plan of the same numbers, its refusals, and a host walk of the request rule its kernel
// moves tiles of codes by (attn_wide_table_slot, attn_wide8_desc, attn_wide8_k_offset / attn_wide8_v_offset, attn_wide8_k_lds / attn_wide8_v_lds,
// ns_attn.h).  The lines are those of tests/tools/attn_prefill_paged_wide_plan_main.cpp:
//   plan   <the call> | ok=.. f8=.. lds=.. got=<ok:pad:grid:block:nqb:aligned:xcd of the FP8 plan> half=<the same of the fp16 plan> why=..
//   refuse what=.. | ok=.. why=..
//   walk   case=.. hs=.. .. table=<ids> | pos0:w:kv:u:l:slot:id:base:bytes:offset:lds0:lds1 per (tile, wave, K / V, request, lane) — base in bytes,
//          lds0 / lds1: where the lane's two decoded 16-byte pieces go
// Host code only: no HIP call is made, no tensor exists — the pointers are made-up addresses.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "ns_attn.h"
#include "ns_attn_plan.cpp"

using namespace ns;

struct Case {
  int hs = 256, cap = 2048, hn = 8, hkv = 8, bs = 2, bk = 16, max_q = 256, head_major = 0, dst_off = 0, d16 = 0, k_off = 0;
  long long sl_add = 0, head_add = 0, step_add = 0;
  unsigned flags = NS_ATTN_FLAG_IS_CAUSAL;
  float scale = 0.0625f, k_sc = 0.5f, v_sc = 2.f;
};
static const int g_ints[64] = {0};  // (only its address is used by a plan)

static std::string fields(const AttnPrefillWidePlan& pl) {
  char s[128];
  snprintf(s, sizeof(s), "%d:%d:%u:%u:%d:%d:%d", int(pl.ok), pl.pad, pl.grid.x, pl.block.x, pl.nqb, pl.aligned, pl.xcd_map);
  return s;
}

static AttnPrefillWidePlan plan_of(const Case& c, bool f8, std::string* why) {
  attn_fp32_fp16_fp16_fp32_fwd_args_t a;
  memset(&a, 0, sizeof(a));
  a.Q = reinterpret_cast<float*>(uintptr_t(0x10000));
  a.K = reinterpret_cast<decltype(a.K)>(uintptr_t(0x100000 + c.k_off));
  a.V = reinterpret_cast<decltype(a.V)>(uintptr_t(0x200000));
  a.dst = reinterpret_cast<float*>(uintptr_t(0x300000 + c.dst_off));
  a.Q_sc = a.dst_sc = 1.f, a.K_sc = c.k_sc, a.V_sc = c.v_sc;
  a.QK_scale = c.scale;
  a.attn_flags = ns_attn_flags_t(c.flags);
  a.batch_size = c.bs, a.head_num = c.hn, a.heads_kv = c.hkv, a.head_size = c.hs, a.sl_q = c.max_q, a.sl_kv = c.cap;
  a.Q_layout = a.K_layout = a.V_layout = a.dst_layout = ATTN_FWD_LAYOUT_PLAIN;
  a.step_q_sl = a.step_dst_sl = c.hn * c.hs;
  a.step_q_head_num = a.step_dst_head_num = c.hs;
  a.step_k_head_size = a.step_v_head_size = 1;
  a.step_k_sl = a.step_v_sl = c.head_major ? c.hs : (long long)c.hkv * c.hs;
  a.step_k_head_num = a.step_v_head_num = c.head_major ? (long long)c.bk * c.hs : c.hs;
  a.step_k_sl += c.sl_add, a.step_v_head_num += c.head_add;
  const AttnPage pg = {g_ints, c.cap / c.bk, attn_block_shift(c.bk), c.cap / c.bk * c.bs + 4, (long long)c.bk * c.hkv * c.hs + 16384 + c.step_add};
  const void* d16 = c.d16 ? reinterpret_cast<const void*>(uintptr_t(0x400000 + (c.d16 == 2 ? 2 : 0))) : nullptr;
  return (f8 ? attn_prefill_paged_wide_f8_plan : attn_prefill_paged_wide_plan)(a, d16, AttnKnobs(), pg, g_ints, g_ints + 8, 1, why);
}

static void run_refusal(const char* what, const Case& c) {
  std::string why;
  const AttnPrefillWidePlan pl = plan_of(c, true, &why);
  printf("refuse what=%s | ok=%d why=%s\n", what, int(pl.ok), why.c_str());
}

// every request of every wave of every tile, as attn_wide_paged8_kernel's issue() and commit() make it; two kv heads, the walk is kv head ihkv's
static void run_walk(int index, int hs, int bk, int kv_len, int pool_blocks, int head_major, int ihkv, const std::vector<int>& table) {
  const AttnPage pg = {table.data(), int(table.size()), attn_block_shift(bk), pool_blocks, (long long)bk * 2 * hs + 64};
  const long long step_sl = head_major ? hs : 2 * hs, step_head = head_major ? (long long)bk * hs : hs;
  printf("walk case=%d hs=%d bk=%d kvlen=%d blocks=%d step=%lld stepsl=%lld stephead=%lld ihkv=%d table=", index, hs, bk, kv_len, pool_blocks, pg.block_step,
         step_sl, step_head, ihkv);
  for (size_t i = 0; i < table.size(); i++) printf("%s%d", i ? "," : "", table[i]);
  printf(" |");
  for (int pos0 = 0; pos0 < kv_len; pos0 += kA2KB)
    for (int w = 0; w < 4; w++) {
      const int slot = attn_wide_table_slot(pg, pos0, w, kv_len);
      const AttnWideDesc d = attn_wide8_desc(pg, table[slot], pos0, w, kv_len, ihkv, step_sl, step_head, hs);
      for (int kv = 0; kv < 2; kv++)
        for (int u = 0; u < kAw8Req; u++)
          for (int l = 0; l < 64; l++)
            printf(" %d:%d:%d:%d:%d:%d:%d:%lld:%u:%u:%d:%d", pos0, w, kv, u, l, slot, table[slot], d.base, d.bytes,
                   kv ? attn_wide8_v_offset(u, l, step_sl, hs) : attn_wide8_k_offset(u, l, step_sl, hs),
                   kv ? attn_wide8_v_lds(w, u, l) : attn_wide8_k_lds(w, u, l, 0), kv ? attn_wide8_v_lds(w, u, l) + 16 : attn_wide8_k_lds(w, u, l, 1));
    }
  printf("\n");
}

int main() {
  const int groups[][2] = {{8, 8}, {8, 1}, {16, 4}}, rows[] = {1, 128, 129, 700};
  int n = 0;
  for (int hs = 144; hs <= 256; hs += 16)
    for (int hm = 0; hm < 2; hm++)
      for (int bk : {16, 32, 64, 128, 256})
        for (const auto& g : groups) {
          Case c;
          c.hs = hs, c.head_major = hm, c.bk = bk, c.hn = g[0], c.hkv = g[1], c.bs = 1 + n % 4, c.max_q = rows[n % 4];
          c.dst_off = n % 5 == 4 ? 4 : 0, c.d16 = n % 3, c.sl_add = 16 * (n % 3), c.head_add = n % 7 == 6 ? 16 : 0, c.step_add = 16 * (n % 2);
          n++;
          std::string why, why16;
          const AttnPrefillWidePlan pl = plan_of(c, true, &why), half = plan_of(c, false, &why16);
          printf("plan hs=%d hm=%d bk=%d hn=%d hkv=%d maxq=%d | ok=%d f8=%d lds=%zu got=%s half=%s why=%s\n", hs, hm, bk, c.hn, c.hkv, c.max_q, int(pl.ok), int(pl.f8),
                 pl.lds, fields(pl).c_str(), fields(half).c_str(), why.c_str());
        }
  Case c;
  run_refusal("none", c);
  c = Case(), c.k_sc = 0.f; run_refusal("k_sc_0", c);
  c = Case(), c.v_sc = -1.f; run_refusal("v_sc_negative", c);
  c = Case(), c.k_sc = 1.f / 0.f; run_refusal("k_sc_inf", c);
  c = Case(), c.v_sc = 0.f / 0.f; run_refusal("v_sc_nan", c);
  for (int hs : {136, 152, 128, 272}) {
    c = Case(), c.hs = hs;
    run_refusal(("head_size_" + std::to_string(hs)).c_str(), c);
  }
  c = Case(), c.sl_add = 8; run_refusal("row_stride", c);
  c = Case(), c.head_add = 8; run_refusal("head_stride", c);
  c = Case(), c.step_add = 8; run_refusal("block_step", c);
  c = Case(), c.k_off = 8; run_refusal("base", c);
  c = Case(), c.flags |= NS_ATTN_FLAG_IS_ALIBI8; run_refusal("alibi", c);
  c = Case(), c.flags |= NS_ATTN_FLAG_IS_TANH30; run_refusal("tanh", c);
  c = Case(), c.scale = -0.0625f; run_refusal("score_scale", c);
  // 255 rows of hkv * 256 BYTES: 16512 kv heads span 1.004 GiB (2.008 GiB of fp16, which the fp16 plan refuses), 33024 span 2.008 GiB
  c = Case(), c.bk = 256, c.hn = c.hkv = 16512; run_refusal("span_1gib", c);
  c = Case(), c.bk = 256, c.hn = c.hkv = 33024; run_refusal("span_2gib", c);

  // the walk: live blocks in a permutation, junk behind them, bad ids inside the live length
  run_walk(0, 256, 16, 130, 40, 0, 1, {7, 3, 39, 0, 12, 5, 9, 1, 2, -1, 40, 1 << 30, -5, 17, 4, 4});  // three tiles, the last of two keys
  run_walk(1, 240, 64, 65, 6, 1, 0, {4, 2, 6, -1});                                                   // padded, head-major, a tile of one key
  run_walk(2, 160, 256, 300, 3, 0, 0, {1, 0, 99, -1});                                                // padded, a page holds four tiles
  run_walk(3, 144, 16, 100, 8, 1, 1, {3, 8, -1, 2, 0, 5, 6, 44, 45});                                 // padded, head-major, bad ids INSIDE the live length
  run_walk(4, 256, 64, 128, 9, 1, 1, {8, 0, -1, 9, 123456});                                          // ends on a tile
  return 0;
}

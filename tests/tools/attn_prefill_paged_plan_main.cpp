// Program of tests/test_attn_prefill_paged_plan.py: the plan of ns_hip_attn_prefill_paged (attn_prefill_paged_plan, neural-speed_amd/csrc/ns_attn_plan.cpp)
// and a host walk of the row -> cell rule its kernel stages K / V rows by (attn_prefill_tile_key and attn_page_at, ns_attn.h).  Three kinds of line:
//   plan   <the call, key=value> | <the fields of the plan>
//   refuse what=<what is wrong> | ok=.. why=..
//   walk   case=<index> hs=.. bk=.. kvlen=.. blocks=.. step=.. stepsl=.. table=<ids, comma-separated> | <one cell per (tile, thread, staging step, K / V)>
//          cell = pos0:tid:u:kv:row:group:key:slot:id:offset — row: the tile row the thread stages at step u (the kernel's krow / vrow), group: the first
//          row of its wave's group of that step, key: the key the row is clamped to, slot: the table slot read (that of the key the GROUP's first row
//          clamps to), id: what the table holds there, offset: attn_page_at's answer
// Host code only: no HIP call is made, no tensor exists — the pointers are made-up addresses.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>

#include "ns_attn.h"
#include "ns_attn_plan.cpp"

using namespace ns;

struct Case {
  int hs = 128, cap = 2048, hn = 8, hkv = 8, bs = 2, bk = 16, max_q = 256;
  int head_major = 0;
  int pool_blocks = 0;       // 0: one block per table entry and four spare
  long long block_step = 0;  // 0: a block's own size
  int table_stride = 0;      // 0: cap / bk
  bool null_table = false, null_qstart = false, null_lens = false;
  unsigned flags = NS_ATTN_FLAG_IS_CAUSAL;
  int k_sl_add = 0;  // added to K's row stride
  float scale = 0.125f;
  int dst_off = 0;   // bytes added to dst
  int d16 = 0;       // 0: no dst16, 1: 8-byte aligned, 2: 2 bytes off
  int dst_sl_add = 0;
  bool no_xcd = false;
  int alibi_heads = 0, alibi_off = 0;
  int layout = ATTN_FWD_LAYOUT_PLAIN;
};

static const int g_ints[64] = {0};  // (only its address is used by a plan)

static AttnPrefillPagedPlan plan_of(const Case& c, std::string* why) {
  attn_fp32_fp16_fp16_fp32_fwd_args_t a;
  memset(&a, 0, sizeof(a));
  a.Q = reinterpret_cast<float*>(uintptr_t(0x10000));
  a.K = reinterpret_cast<decltype(a.K)>(uintptr_t(0x100000));
  a.V = reinterpret_cast<decltype(a.V)>(uintptr_t(0x200000));
  a.dst = reinterpret_cast<float*>(uintptr_t(0x300000 + c.dst_off));
  a.Q_sc = a.K_sc = a.V_sc = a.dst_sc = 1.f;
  a.QK_scale = c.scale;
  a.attn_flags = ns_attn_flags_t(c.flags);
  a.batch_size = c.bs, a.head_num = c.hn, a.heads_kv = c.hkv, a.head_size = c.hs, a.sl_q = c.max_q, a.sl_kv = c.cap;
  a.Q_layout = a.K_layout = a.V_layout = ATTN_FWD_LAYOUT_PLAIN;
  a.dst_layout = ATTN_FWD_LAYOUT(c.layout);
  a.step_q_sl = c.hn * c.hs;
  a.step_dst_sl = c.hn * c.hs + c.dst_sl_add;
  a.step_q_head_num = a.step_dst_head_num = c.hs;
  a.step_q_bs = a.step_dst_bs = a.step_k_bs = a.step_v_bs = 12345;  // (not used)
  a.step_k_head_size = a.step_v_head_size = 1;
  if (c.head_major) {
    a.step_k_sl = a.step_v_sl = c.hs;
    a.step_k_head_num = a.step_v_head_num = (long long)c.bk * c.hs;
  } else {
    a.step_k_sl = a.step_v_sl = c.hkv * c.hs;
    a.step_k_head_num = a.step_v_head_num = c.hs;
  }
  a.step_k_sl += c.k_sl_add;
  AttnPage pg;
  pg.table = c.null_table ? nullptr : g_ints;
  pg.block_shift = attn_block_shift(c.bk);
  pg.table_stride = c.table_stride ? c.table_stride : c.cap / std::max(c.bk, 1);
  pg.pool_blocks = c.pool_blocks ? c.pool_blocks : pg.table_stride * c.bs + 4;
  pg.block_step = c.block_step ? c.block_step : (long long)c.bk * c.hkv * c.hs;
  AttnKnobs kn;
  kn.no_xcd_map = c.no_xcd;
  kn.alibi_heads = c.alibi_heads, kn.alibi_off = c.alibi_off;
  const void* d16 = c.d16 == 0 ? nullptr : reinterpret_cast<const void*>(uintptr_t(0x400000 + (c.d16 == 2 ? 2 : 0)));
  return attn_prefill_paged_plan(a, d16, kn, pg, c.null_qstart ? nullptr : g_ints, c.null_lens ? nullptr : g_ints + 8, 1, why);
}

static void run_plan(const Case& c) {
  std::string why;
  const AttnPrefillPagedPlan pl = plan_of(c, &why);
  const AttnParams& p = pl.pp.a;
  printf("plan bs=%d hn=%d hkv=%d hs=%d maxq=%d cap=%d bk=%d hm=%d flags=%u scale=%g dsto=%d d16=%d dstadd=%d noxcd=%d | ok=%d hspad=%d sb=%d pad=%d grid=%u,%u,%u "
         "block=%u lds=%zu nqb=%d aligned=%d xcd=%d slq=%d slkv=%d kdelta=%d shift=%d bsteps=%lld qstart=%d lens=%d why=%s\n",
         c.bs, c.hn, c.hkv, c.hs, c.max_q, c.cap, c.bk, c.head_major, c.flags, double(c.scale), c.dst_off, c.d16, c.dst_sl_add, int(c.no_xcd), int(pl.ok), pl.hs_pad,
         pl.sb, pl.pad, pl.grid.x, pl.grid.y, pl.grid.z, pl.block.x, pl.lds, pl.nqb, pl.aligned, pl.xcd_map, p.sl_q, p.sl_kv, pl.pp.kdelta, pl.pp.pg.block_shift,
         p.step_q_bs + p.step_k_bs + p.step_v_bs + p.step_dst_bs, int(pl.pp.q_start == g_ints), int(pl.pp.kv_lens == g_ints + 8), why.c_str());
}

static void run_refusal(const char* what, const Case& c) {
  std::string why;
  const AttnPrefillPagedPlan pl = plan_of(c, &why);
  printf("refuse what=%s | ok=%d why=%s\n", what, int(pl.ok), why.c_str());
}

// The kernel's staging geometry (attn_mfma2_body, ns_attn_prefill.hip): thread tid stages tile rows krow / vrow at step u; its wave reads ONE table
// entry per step, that of the key the group's first row clamps to.
template <int HS>
static void run_walk(int index, int bk, int kv_len, int pool_blocks, const std::vector<int>& table) {
  constexpr int NCH = HS / 8, NSUB = HS / 16, KU = NCH / 4;
  constexpr int VRG = NSUB <= 8 ? 4 : 2, VRGL = NSUB <= 8 ? 2 : 1, VRW = VRG * (32 / VRG / NSUB), VU = kA2KB / (4 * VRW);
  static_assert(KU == VU && 256 / NCH == 4 * VRW, "K and V rows of a staging step: the same group of a wave");
  AttnPage pg;
  pg.table = table.data(), pg.table_stride = int(table.size()), pg.block_shift = attn_block_shift(bk), pg.pool_blocks = pool_blocks;
  const long long step_sl = 2 * HS;  // two kv heads, position-major
  pg.block_step = (long long)bk * step_sl;
  printf("walk case=%d hs=%d bk=%d kvlen=%d blocks=%d step=%lld stepsl=%lld table=", index, HS, bk, kv_len, pool_blocks, pg.block_step, step_sl);
  for (size_t i = 0; i < table.size(); i++) printf("%s%d", i ? "," : "", table[i]);
  printf(" |");
  const int nb = (kv_len + kA2KB - 1) / kA2KB;
  for (int b = 0; b < nb; b++) {
    const int pos0 = b * kA2KB;
    for (int tid = 0; tid < 256; tid++) {
      const int w = tid >> 6, l = tid & 63;
      const int vrq = (l >> (1 + VRGL)) / NSUB, vr = (l >> 1) & (VRG - 1);
      for (int u = 0; u < KU; u++) {
        const int rows[2] = {(tid + 256 * u) / NCH, u * (4 * VRW) + w * VRW + vrq * VRG + vr};
        const int group = u * (64 / KU) + w * (16 / KU);
        const int slot = attn_prefill_tile_key(pos0, group, kv_len) >> pg.block_shift;
        for (int kv = 0; kv < 2; kv++) {
          const int key = attn_prefill_tile_key(pos0, rows[kv], kv_len);
          printf(" %d:%d:%d:%d:%d:%d:%d:%d:%d:%lld", pos0, tid, u, kv, rows[kv], group, key, slot, table[slot], attn_page_at(pg, table[slot], key, step_sl));
        }
      }
    }
  }
  printf("\n");
}

int main() {
  const int groups[][2] = {{8, 8}, {8, 2}, {71, 1}};
  const unsigned flag_sets[] = {0, NS_ATTN_FLAG_IS_CAUSAL, NS_ATTN_FLAG_IS_CAUSAL | NS_ATTN_FLAG_IS_ALIBI8, NS_ATTN_FLAG_IS_CAUSAL | NS_ATTN_FLAG_IS_TANH30};
  const float scales[] = {0.125f, -0.125f, 0.f};
  int n = 0;
  for (int bk : {16, 64, 256})
    for (int bs : {1, 3, 8})
      for (const auto& g : groups)
        for (int hs : {40, 64, 80, 96, 128, 160, 256})
          for (int max_q : {1, 16, 127, 128, 129, 2048})
            for (int cap : {200, 2048})
              for (unsigned flags : flag_sets) {
                Case c;
                c.bs = bs, c.hn = g[0], c.hkv = g[1], c.hs = hs, c.bk = bk, c.max_q = max_q, c.cap = (cap + bk - 1) / bk * bk, c.flags = flags;
                c.head_major = n & 1, c.scale = scales[n % 3], c.dst_off = (n / 3) % 4 == 3 ? 4 : 0, c.d16 = (n / 5) % 3, c.dst_sl_add = (n / 7) % 5 == 4 ? 2 : 0;
                c.no_xcd = (n / 11) % 4 == 3;
                n++;
                run_plan(c);
              }
  Case c;
  run_refusal("none", c);
  c = Case(), c.null_qstart = true;
  run_refusal("null_qstart", c);
  c = Case(), c.null_lens = true;
  run_refusal("null_lens", c);
  c = Case(), c.layout = ATTN_FWD_LAYOUT_NTILE48_ROWPACK4;
  run_refusal("layout", c);
  c = Case(), c.bs = 0;
  run_refusal("no_requests", c);
  c = Case(), c.hs = 84;
  run_refusal("head_size_84", c);
  c = Case(), c.hs = 264;
  run_refusal("head_size_264", c);
  c = Case(), c.hs = 136;
  run_refusal("head_size_136", c);
  c = Case(), c.hs = 256;
  run_refusal("head_size_256", c);
  c = Case(), c.hn = 8, c.hkv = 3;
  run_refusal("head_group", c);
  c = Case(), c.max_q = 0;
  run_refusal("max_q_0", c);
  c = Case(), c.cap = 0, c.table_stride = 1;
  run_refusal("capacity_0", c);
  c = Case(), c.bk = 48, c.table_stride = 2048 / 48;
  run_refusal("block_keys_48", c);
  c = Case(), c.bk = 8, c.table_stride = 256;
  run_refusal("block_keys_8", c);
  c = Case(), c.bk = 512, c.table_stride = 4;
  run_refusal("block_keys_512", c);
  c = Case(), c.table_stride = 2048 / 16 - 1;
  run_refusal("capacity", c);
  c = Case(), c.null_table = true;
  run_refusal("null_table", c);
  c = Case(), c.pool_blocks = -1;
  run_refusal("pool_blocks", c);
  c = Case(), c.block_step = 16 * 8 * 128 - 8;
  run_refusal("block_step_small", c);
  c = Case(), c.block_step = 16 * 8 * 128 + 4;
  run_refusal("block_step_unaligned", c);
  c = Case(), c.k_sl_add = 4, c.block_step = 2 * 16 * 8 * 128;
  run_refusal("kv_rows_unaligned", c);
  c = Case(), c.hn = 65536, c.hkv = 65536, c.bs = 2048, c.max_q = 2048, c.block_step = 16ll * 65536 * 128;  // 16 * 65536 * 2048 = 2^31 workgroups
  run_refusal("grid_limit", c);
  c = Case(), c.hn = 65536, c.hkv = 65536, c.bs = 2047, c.max_q = 2048, c.block_step = 16ll * 65536 * 128;
  run_refusal("grid_limit_below", c);
  c = Case(), c.flags |= NS_ATTN_FLAG_IS_ALIBI8, c.alibi_heads = 12, c.alibi_off = 8;  // heads 8 .. 15 of 12
  run_refusal("alibi_partition", c);
  c = Case(), c.flags |= NS_ATTN_FLAG_IS_ALIBI8, c.alibi_heads = 16, c.alibi_off = 8;
  run_refusal("alibi_partition_fits", c);
  c = Case(), c.alibi_heads = 12, c.alibi_off = 8;  // (no ALiBi: the partition is not read)
  run_refusal("partition_without_alibi", c);

  // the walk: live blocks in a permutation, junk (ids that are no block of the pool, and ids of blocks other requests own) behind them
  run_walk<64>(0, 16, 130, 40, {7, 3, 39, 0, 12, 5, 9, 1, 2, -1, 40, 1 << 30, -5, 17, 4, 4});   // 9 live blocks of 16; three tiles, the last of two keys
  run_walk<128>(1, 16, 64, 9, {8, 0, 3, 5, -1, 9, 123456, -2});                                 // ends on a tile
  run_walk<128>(2, 64, 65, 6, {4, 2, 6, -1});                                                   // one page per tile, a tile of one key
  run_walk<64>(3, 256, 300, 3, {1, 0, 99, -1});                                                 // a page holds four tiles
  run_walk<128>(4, 32, 1, 2, {1, -1, 2, 77});                                                   // one key
  run_walk<64>(5, 16, 100, 8, {3, 8, -1, 2, 0, 5, 6, 44, 45});                                  // bad ids INSIDE the live length: no address
  return 0;
}

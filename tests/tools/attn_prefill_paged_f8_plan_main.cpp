// Program of tests/test_attn_prefill_paged_f8_plan.py: attn_prefill_paged_f8_plan (neural-speed_amd/csrc/ns_attn_plan.cpp) beside attn_prefill_paged_plan of
// the same call, and a host walk of the staging map of the kernel's F8 instantiations (attn_prefill8_*, ns_attn.h).  Host code only.  Lines:
//   plan   <the call> | <the fields of the FP8 plan> | <the fields of the fp16 plan>
//   refuse what=.. | <the fields of the FP8 plan>
//   walk   hs=.. bk=.. kvlen=.. blocks=.. | <one cell per (tile, wave, step, lane, K / V)>
//          cell = pos0:w:u:l:kv:row:col:key:whole:got:want — row / col: the tile row and 16-dim column the lane stages, key: the row clamped to the last
//          live key, got: the offset the kernel forms (whole tile: the group's base + the lane's part; else attn_page_at through the GROUP's entry),
//          want: attn_page_at of the lane's own key through that key's OWN table entry, + 16 col
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <limits>
#include <vector>

#include "ns_attn.h"
#include "ns_attn_plan.cpp"

using namespace ns;

struct Case {
  int hs = 128, cap = 2048, hn = 8, hkv = 8, bs = 2, bk = 16, max_q = 256, head_major = 0;
  long long block_step = 0, step_sl = 0;  // 0: by the layout
  uintptr_t kbase = 0x100000;
  float k_sc = 0.25f, v_sc = 2.f, scale = 0.125f;
  unsigned flags = NS_ATTN_FLAG_IS_CAUSAL;
  int d16 = 0, dst_off = 0;
  bool null_qstart = false;
};
static const int g_ints[64] = {0};  // (only its address is used by a plan)

static AttnPrefillPagedPlan plan(const Case& c, bool f8, std::string* why) {
  attn_fp32_fp16_fp16_fp32_fwd_args_t a;
  memset(&a, 0, sizeof(a));
  a.Q = reinterpret_cast<float*>(uintptr_t(0x10000));
  a.K = reinterpret_cast<decltype(a.K)>(c.kbase);
  a.V = reinterpret_cast<decltype(a.V)>(uintptr_t(0x200000));
  a.dst = reinterpret_cast<float*>(uintptr_t(0x300000 + c.dst_off));
  a.Q_sc = 0.5f, a.dst_sc = 4.f, a.K_sc = c.k_sc, a.V_sc = c.v_sc, a.QK_scale = c.scale;
  a.attn_flags = ns_attn_flags_t(c.flags);
  a.batch_size = c.bs, a.head_num = c.hn, a.heads_kv = c.hkv, a.head_size = c.hs, a.sl_q = c.max_q, a.sl_kv = c.cap;
  a.Q_layout = a.K_layout = a.V_layout = a.dst_layout = ATTN_FWD_LAYOUT_PLAIN;
  a.step_q_head_num = a.step_dst_head_num = c.hs;
  a.step_q_sl = a.step_dst_sl = c.hn * c.hs;
  a.step_k_head_size = a.step_v_head_size = 1;
  a.step_k_sl = a.step_v_sl = c.step_sl ? c.step_sl : (c.head_major ? c.hs : c.hkv * c.hs);
  a.step_k_head_num = a.step_v_head_num = c.head_major ? (long long)c.bk * c.hs : c.hs;
  AttnPage pg;
  pg.table = g_ints, pg.block_shift = attn_block_shift(c.bk), pg.table_stride = c.cap / c.bk, pg.pool_blocks = pg.table_stride * c.bs + 4;
  pg.block_step = c.block_step ? c.block_step : (long long)c.bk * c.hkv * c.hs;
  const void* d16 = c.d16 ? reinterpret_cast<const void*>(uintptr_t(0x400000 + (c.d16 == 2 ? 2 : 0))) : nullptr;
  const int* qs = c.null_qstart ? nullptr : g_ints;
  return f8 ? attn_prefill_paged_f8_plan(a, d16, AttnKnobs(), pg, qs, g_ints + 8, 1, why) : attn_prefill_paged_plan(a, d16, AttnKnobs(), pg, qs, g_ints + 8, 1, why);
}

static void print_fields(const AttnPrefillPagedPlan& pl, const std::string& why) {
  const AttnParams& p = pl.pp.a;
  printf("ok=%d f8=%d hspad=%d sb=%d pad=%d grid=%u,%u,%u block=%u lds=%zu nqb=%d aligned=%d xcd=%d qstart=%d lens=%d kdelta=%d table=%d ts=%d shift=%d blocks=%d "
         "bstep=%lld k=%llx v=%llx q=%llx dst=%llx d16=%llx slq=%d slkv=%d hn=%d hkv=%d hs=%d flags=%u ksl=%lld khead=%lld vsl=%lld vhead=%lld qsl=%lld qhead=%lld "
         "dsl=%lld dhead=%lld qk=%a out=%a m0=%a m1=%a lf=%d aoff=%d why=%s",
         int(pl.ok), int(pl.f8), pl.hs_pad, pl.sb, pl.pad, pl.grid.x, pl.grid.y, pl.grid.z, pl.block.x, pl.lds, pl.nqb, pl.aligned, pl.xcd_map,
         int(pl.pp.q_start == g_ints), int(pl.pp.kv_lens == g_ints + 8), pl.pp.kdelta, int(pl.pp.pg.table == g_ints), pl.pp.pg.table_stride, pl.pp.pg.block_shift,
         pl.pp.pg.pool_blocks, pl.pp.pg.block_step, (unsigned long long)uintptr_t(p.k), (unsigned long long)uintptr_t(p.v), (unsigned long long)uintptr_t(p.q),
         (unsigned long long)uintptr_t(p.dst), (unsigned long long)uintptr_t(p.dst16), p.sl_q, p.sl_kv, p.head_num, p.heads_kv, p.head_size, p.flags, p.step_k_sl,
         p.step_k_head_num, p.step_v_sl, p.step_v_head_num, p.step_q_sl, p.step_q_head_num, p.step_dst_sl, p.step_dst_head_num, p.qk_scale, p.out_scale,
         p.alibi_m0, p.alibi_m1, p.alibi_log2_floor, p.alibi_head_off, why.c_str());
}
static void run(const char* kind, const char* what, const Case& c, bool both) {
  std::string why8, why16;
  printf("%s what=%s hs=%d | ", kind, what, c.hs);
  print_fields(plan(c, true, &why8), why8);
  if (both) {
    printf(" | ");
    print_fields(plan(c, false, &why16), why16);
  }
  printf("\n");
}

// every (tile, wave, step, lane) of the F8 staging map (attn_mfma2_body's fetch8, ns_attn_prefill.hip), two kv heads, position-major
template <int HS>
static void walk(int bk, int kv_len, int pool_blocks, const std::vector<int>& table) {
  constexpr int KU8 = HS / 64;
  AttnPage pg;
  pg.table = table.data(), pg.table_stride = int(table.size()), pg.block_shift = attn_block_shift(bk), pg.pool_blocks = pool_blocks;
  const long long step_sl = 2 * HS;
  pg.block_step = (long long)bk * step_sl;
  printf("walk hs=%d bk=%d kvlen=%d blocks=%d |", HS, bk, kv_len, pool_blocks);
  for (int pos0 = 0; pos0 < kv_len; pos0 += kA2KB) {
    const bool whole = pos0 + kA2KB <= kv_len;
    for (int w = 0; w < 4; w++)
      for (int u = 0; u < KU8; u++) {
        const int first = attn_prefill8_group<HS>(w, u);
        const int id = table[attn_prefill_tile_key(pos0, first, kv_len) >> pg.block_shift];  // the ONE entry of the wave's step
        for (int l = 0; l < 64; l++)
          for (int kv = 0; kv < 2; kv++) {
            const int lr = kv ? attn_prefill8_vrow<HS>(l) : attn_prefill8_krow<HS>(l), col = kv ? attn_prefill8_vcol<HS>(l) : attn_prefill8_kcol<HS>(l);
            const int key = attn_prefill_tile_key(pos0, first + lr, kv_len);
            long long got;
            if (whole) {
              const long long base = attn_prefill8_group_base(pg, id, pos0 + first, step_sl);
              got = base < 0 ? -1 : base + lr * step_sl + 16 * col;
            } else {
              const long long cell = attn_page_at(pg, id, key, step_sl);
              got = cell < 0 ? -1 : cell + 16 * col;
            }
            const long long own = attn_page_cell(pg, 0, key, step_sl);
            printf(" %d:%d:%d:%d:%d:%d:%d:%d:%d:%lld:%lld", pos0, w, u, l, kv, first + lr, col, key, int(whole), got, own < 0 ? -1 : own + 16 * col);
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
        for (int hs : {48, 64, 80, 96, 128})
          for (int max_q : {1, 127, 129, 2048})
            for (unsigned flags : flag_sets) {
              Case c;
              c.bs = bs, c.hn = g[0], c.hkv = g[1], c.hs = hs, c.bk = bk, c.max_q = max_q, c.flags = flags, c.cap = n & 2 ? 2048 : 256;
              c.head_major = n & 1, c.scale = scales[n % 3], c.dst_off = (n / 3) % 4 == 3 ? 4 : 0, c.d16 = (n / 5) % 3;
              n++;
              run("plan", "grid", c, true);
            }
  Case c;
  run("refuse", "none", c, false);
  c = Case(), c.hs = 40;  // (a multiple of 8: the fp16 plan would take it — the pool's refusal comes first)
  run("refuse", "head_size_40", c, false);
  c = Case(), c.hs = 144;
  run("refuse", "head_size_144", c, false);
  c = Case(), c.step_sl = 8 * 128 + 8, c.block_step = 16 * (8 * 128 + 8);
  run("refuse", "step_sl", c, false);
  c = Case(), c.block_step = 16 * 8 * 128 + 8;
  run("refuse", "block_step", c, false);
  c = Case(), c.kbase = 0x100008;
  run("refuse", "base", c, false);
  c = Case(), c.k_sc = 0.f;
  run("refuse", "k_scale_zero", c, false);
  c = Case(), c.v_sc = std::numeric_limits<float>::infinity();
  run("refuse", "v_scale_inf", c, false);
  c = Case(), c.null_qstart = true;
  run("refuse", "null_qstart", c, false);

  walk<64>(16, 130, 40, {7, 3, 39, 0, 12, 5, 9, 1, 2, -1, 40, 1 << 30, -5, 17, 4, 4});  // four pages per tile; two whole tiles, a last one of two keys
  walk<128>(16, 128, 9, {8, 0, 3, 5, 1, 7, 2, 6, -1});                                   // ends on a tile: whole tiles only
  walk<128>(64, 65, 6, {4, 2, 6, -1});                                                   // one page per tile, a tile of one key
  walk<64>(256, 300, 3, {1, 0, 99, -1});                                                 // a page holds four tiles
  walk<128>(32, 200, 8, {3, 8, -1, 2, 0, 5, 6, 44});                                     // bad ids INSIDE the live length: no address
  return 0;
}

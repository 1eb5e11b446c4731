// Program of tests/test_attn_shared_paged_plan.py: the plan of ns_hip_attn_decode_paged_shared (attn_shared_paged_plan, ns_attn_plan.cpp), the workspace
// size function's value and the live rule its range workgroups and its merge run (attn_block_live, ns_attn.h).  Lines: `plan <call> | <fields>`,
// `refuse what=.. | ok=.. why=..`, `live dyn=.. bk=.. P=.. len=.. | <the plan's ranges> prefix=<kps:live> suffix=<kps:live>`.
// Host code only: no HIP call is made, no tensor exists — the pointers are made-up addresses.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "ns_attn.h"
#include "ns_attn_plan.cpp"

using namespace ns;

struct Case {
  int hs = 128, cap = 2048, hn = 8, hkv = 8, bs = 8, bk = 16, groups = 2, max_group = 4, sl_q = 1, table_stride = 0, null_arg = -1;
  unsigned flags = NS_ATTN_FLAG_IS_CAUSAL;
  bool dyn = true;
  long long step_sl = 0, step_head = 0, block_step = 0;  // 0: position-major blocks of their own size
  int pool_blocks = 0;
};
static const int g_ints[64] = {0};  // (only its address is used by a plan)

static AttnSharedPagedPlan plan_of(const Case& c, std::string* why) {
  attn_fp32_fp16_fp16_fp32_fwd_args_t a;
  memset(&a, 0, sizeof(a));
  a.Q = reinterpret_cast<float*>(uintptr_t(0x10000)), a.dst = reinterpret_cast<float*>(uintptr_t(0x300000));
  a.K = reinterpret_cast<decltype(a.K)>(uintptr_t(0x100000)), a.V = reinterpret_cast<decltype(a.V)>(uintptr_t(0x200000));
  a.Q_sc = a.K_sc = a.V_sc = a.dst_sc = 1.f, a.QK_scale = 0.125f, a.attn_flags = ns_attn_flags_t(c.flags);
  a.batch_size = c.bs, a.head_num = c.hn, a.heads_kv = c.hkv, a.head_size = c.hs, a.sl_q = c.sl_q, a.sl_kv = c.cap;
  a.Q_layout = a.K_layout = a.V_layout = a.dst_layout = ATTN_FWD_LAYOUT_PLAIN;
  a.step_q_bs = a.step_dst_bs = a.step_q_sl = a.step_dst_sl = c.hn * c.hs, a.step_q_head_num = a.step_dst_head_num = c.hs;
  a.step_k_head_size = a.step_v_head_size = 1, a.step_k_sl = a.step_v_sl = c.hkv * c.hs, a.step_k_head_num = a.step_v_head_num = c.hs;
  if (c.step_sl) a.step_k_sl = a.step_v_sl = c.step_sl, a.step_k_head_num = a.step_v_head_num = c.step_head;
  const int ts = c.table_stride ? c.table_stride : c.cap / c.bk;
  const AttnPage pg = {g_ints, ts, attn_block_shift(c.bk), c.pool_blocks ? c.pool_blocks : ts * c.bs + 4,
                       c.block_step ? c.block_step : (long long)c.bk * c.hkv * c.hs};
  AttnKnobs kn;
  kn.dyn_ranges = c.dyn;
  why->clear();
  return attn_shared_paged_plan(a, nullptr, kn, pg, c.null_arg == 0 ? nullptr : g_ints, c.groups, c.max_group, c.null_arg == 1 ? nullptr : g_ints,
                                c.null_arg == 2 ? nullptr : g_ints, 1, why);
}

// far hs bk cap requests groups max_group pool_blocks block_step step_sl step_head: a pool of the far-address tests, whose numbers
// (tests/tools/attn_far_layout.py) the caller passes; 4 / 2 heads -> far hs=.. blocks=.. step=.. | ok=.. hspad=.. pgrid=.. sgrid=.. why=..
static int far_call(char** argv) {
  const auto at = [&](int i) { return atoll(argv[i]); };
  Case c;
  c.hn = 4, c.hkv = 2, c.hs = int(at(2)), c.bk = int(at(3)), c.cap = int(at(4)), c.bs = int(at(5)), c.groups = int(at(6)), c.max_group = int(at(7));
  c.pool_blocks = int(at(8)), c.block_step = at(9), c.step_sl = at(10), c.step_head = at(11);
  std::string why;
  const AttnSharedPagedPlan pl = plan_of(c, &why);
  printf("far hs=%d blocks=%d step=%lld | ok=%d hspad=%d pgrid=%u,%u,%u sgrid=%u,%u,%u bstep=%lld ksl=%lld khead=%lld why=%s\n", c.hs, pl.sp.pg.pool_blocks, c.block_step,
         int(pl.ok), pl.hs_pad, pl.grid_prefix.x, pl.grid_prefix.y, pl.grid_prefix.z, pl.grid_suffix.x, pl.grid_suffix.y, pl.grid_suffix.z, pl.sp.pg.block_step,
         (long long)pl.sp.a.step_k_sl, (long long)pl.sp.a.step_k_head_num, why.c_str());
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 12 && std::string(argv[1]) == "far") return far_call(argv);
  std::string why;
  const int heads[][2] = {{8, 8}, {32, 32}, {32, 8}, {8, 1}, {71, 1}};
  const int shapes[][3] = {{1, 1, 1}, {32, 1, 32}, {32, 4, 8}, {32, 32, 1}, {9, 3, 5}};  // (requests, groups, max_group)
  int n = 0;
  for (const auto& gs : shapes)
    for (const auto& h : heads)
      for (int cap : {256, 2048, 4096}) {
        Case c;
        c.bs = gs[0], c.groups = gs[1], c.max_group = gs[2], c.hn = h[0], c.hkv = h[1], c.hs = n & 1 ? 64 : 128, c.bk = n & 2 ? 16 : 64, c.cap = cap, c.dyn = n++ % 5 != 0;
        const AttnSharedPagedPlan pl = plan_of(c, &why);
        const AttnSharedParams& sp = pl.sp;
        printf("plan bs=%d hn=%d hkv=%d hs=%d groups=%d maxg=%d cap=%d dynon=%d | ok=%d hspad=%d pgrid=%u,%u,%u sgrid=%u,%u,%u mgrid=%u,%u,%u block=%u nsp=%d kpsp=%d "
               "nss=%d kpss=%d stride=%d sufoff=%d gfull=%d dyn=%d pbytes=%zu ws=%zu why=%s\n",
               c.bs, c.hn, c.hkv, c.hs, c.groups, c.max_group, c.cap, int(c.dyn), int(pl.ok), pl.hs_pad, pl.grid_prefix.x, pl.grid_prefix.y, pl.grid_prefix.z,
               pl.grid_suffix.x, pl.grid_suffix.y, pl.grid_suffix.z, pl.merge_grid.x, pl.merge_grid.y, pl.merge_grid.z, pl.block.x, sp.nsp, sp.kps_p, sp.nss,
               sp.kps_s, sp.rec_stride, sp.suf_off, sp.g_full, sp.min_keys, pl.partial_bytes,
               attn_shared_paged_ws_bytes(AttnKnobs(), c.bs, c.hn, c.hkv, c.hs, c.max_group, c.cap), why.c_str());
        if (n % 13 != 1) continue;  // six plans: the live rule on a coarse grid of (P, len)
        for (int P = 0; P <= c.cap; P += c.cap / 4)
          for (int len : {0, 1, P - 1, P, P + 1, P + 63, P + 65, (P + c.cap) / 2, c.cap}) {
            if (len < 0 || len > c.cap) continue;
            const AttnBlockLive lp = attn_block_live(P, sp.nsp, sp.kps_p, sp.min_keys), ls = attn_block_live(len - P, sp.nss, sp.kps_s, sp.min_keys);
            printf("live dyn=%d bk=%d P=%d len=%d | nsp=%d kpsp=%d nss=%d kpss=%d prefix=%d:%d suffix=%d:%d\n", int(c.dyn), c.bk, P, len, sp.nsp, sp.kps_p, sp.nss,
                   sp.kps_s, lp.kps, lp.live, ls.kps, ls.live);
          }
      }
  auto refusal = [&](const char* what, auto edit) {
    Case c;
    edit(c);
    const bool ok = plan_of(c, &why).ok;
    printf("refuse what=%s | ok=%d why=%s\n", what, int(ok), why.c_str());
  };
  refusal("none", [](Case&) {});
  refusal("null_start", [](Case& c) { c.null_arg = 0; });
  refusal("null_prefix", [](Case& c) { c.null_arg = 1; });
  refusal("null_lens", [](Case& c) { c.null_arg = 2; });
  refusal("groups_0", [](Case& c) { c.groups = 0; });
  refusal("max_group_0", [](Case& c) { c.max_group = 0; });
  refusal("sl_q_2", [](Case& c) { c.sl_q = 2; });
  refusal("head_size_80", [](Case& c) { c.hs = 80; });
  refusal("alibi", [](Case& c) { c.flags |= NS_ATTN_FLAG_IS_ALIBI8; });
  refusal("grid_limit_members", [](Case& c) { c.groups = 256, c.max_group = 256; });
  refusal("capacity", [](Case& c) { c.table_stride = 2048 / 16 - 1; });
  return 0;
}

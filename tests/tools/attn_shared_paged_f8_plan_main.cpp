// Program of tests/test_attn_shared_paged_f8_plan.py (host code only, made-up addresses).  Lines: `<what> | <the FP8 plan's fields> | <the fp16 plan's>`.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>

#include "ns_attn.h"
#include "ns_attn_plan.cpp"

using namespace ns;
struct Case {
  int hs = 128, cap = 2048, hn = 8, hkv = 8, bs = 8, bk = 16, groups = 2, max_group = 4, sl_q = 1;
  long long step_sl = 8 * 128, step_head = 128, block_step = 16 * 8 * 128;
  uintptr_t vbase = 0x200000;
  float k_sc = 0.25f, v_sc = 2.f;
  unsigned flags = NS_ATTN_FLAG_IS_CAUSAL;
  int pool_blocks = 0;  // 0: the table's blocks + 4
};
static const int g_ints[64] = {0};  // (only its address is used by a plan)

static void print_plan(const Case& c, bool f8) {
  attn_fp32_fp16_fp16_fp32_fwd_args_t a;
  memset(&a, 0, sizeof(a));
  a.Q = reinterpret_cast<float*>(uintptr_t(0x10000)), a.dst = reinterpret_cast<float*>(uintptr_t(0x300000));
  a.K = reinterpret_cast<decltype(a.K)>(uintptr_t(0x100000)), a.V = reinterpret_cast<decltype(a.V)>(c.vbase);
  a.Q_sc = 0.5f, a.dst_sc = 4.f, a.K_sc = c.k_sc, a.V_sc = c.v_sc, a.QK_scale = 0.125f, a.attn_flags = ns_attn_flags_t(c.flags);
  a.batch_size = c.bs, a.head_num = c.hn, a.heads_kv = c.hkv, a.head_size = c.hs, a.sl_q = c.sl_q, a.sl_kv = c.cap;
  a.Q_layout = a.K_layout = a.V_layout = a.dst_layout = ATTN_FWD_LAYOUT_PLAIN;
  a.step_q_bs = a.step_dst_bs = a.step_q_sl = a.step_dst_sl = c.hn * c.hs, a.step_q_head_num = a.step_dst_head_num = c.hs;
  a.step_k_head_size = a.step_v_head_size = 1, a.step_k_sl = a.step_v_sl = c.step_sl, a.step_k_head_num = a.step_v_head_num = c.step_head;
  const AttnPage pg = {g_ints, c.cap / c.bk, attn_block_shift(c.bk), c.pool_blocks ? c.pool_blocks : c.cap / c.bk * c.bs + 4, c.block_step};
  std::string why;
  const AttnSharedPagedPlan pl = f8 ? attn_shared_paged_f8_plan(a, nullptr, AttnKnobs(), pg, g_ints, c.groups, c.max_group, g_ints, g_ints, 1, &why)
                                    : attn_shared_paged_plan(a, nullptr, AttnKnobs(), pg, g_ints, c.groups, c.max_group, g_ints, g_ints, 1, &why);
  const AttnSharedParams& sp = pl.sp;
  printf(" | ok=%d f8=%d hspad=%d pgrid=%u,%u,%u sgrid=%u,%u,%u mgrid=%u,%u block=%u pbytes=%zu nsp=%d kpsp=%d nss=%d kpss=%d stride=%d sufoff=%d gfull=%d "
         "dyn=%d req=%d groups=%d maxg=%d kdelta=%d arrays=%d shift=%d ts=%d blocks=%d bstep=%lld k=%llx v=%llx ksl=%lld khead=%lld vsl=%lld vhead=%lld "
         "qbs=%lld dbs=%lld qk=%a out=%a why=%s",
         int(pl.ok), int(pl.f8), pl.hs_pad, pl.grid_prefix.x, pl.grid_prefix.y, pl.grid_prefix.z, pl.grid_suffix.x, pl.grid_suffix.y, pl.grid_suffix.z,
         pl.merge_grid.x, pl.merge_grid.y, pl.block.x, pl.partial_bytes, sp.nsp, sp.kps_p, sp.nss, sp.kps_s, sp.rec_stride, sp.suf_off, sp.g_full, sp.min_keys,
         sp.requests, sp.groups, sp.max_group, sp.kdelta, (sp.group_start == g_ints) + (sp.prefix_keys == g_ints) + (sp.kv_lens == g_ints) + (sp.pg.table == g_ints),
         sp.pg.block_shift, sp.pg.table_stride, sp.pg.pool_blocks, sp.pg.block_step, (unsigned long long)uintptr_t(sp.a.k), (unsigned long long)uintptr_t(sp.a.v),
         (long long)sp.a.step_k_sl, (long long)sp.a.step_k_head_num, (long long)sp.a.step_v_sl, (long long)sp.a.step_v_head_num, (long long)sp.a.step_q_bs,
         (long long)sp.a.step_dst_bs, sp.a.qk_scale, sp.a.out_scale, why.c_str());
}

int main(int argc, char** argv) {
  const auto run = [](const char* what, const Case& c) { printf("%s", what), print_plan(c, true), print_plan(c, false), printf("\n"); };
  // far hs bk cap requests groups max_group pool_blocks block_step step_sl step_head: the pool of the far-address test (4 / 2 heads), whose numbers
  // (tests/tools/attn_far_layout.py) the caller passes
  if (argc == 12 && std::string(argv[1]) == "far") {
    const auto at = [&](int i) { return atoll(argv[i]); };
    Case c;
    c.hn = 4, c.hkv = 2, c.hs = int(at(2)), c.bk = int(at(3)), c.cap = int(at(4)), c.bs = int(at(5)), c.groups = int(at(6)), c.max_group = int(at(7));
    c.pool_blocks = int(at(8)), c.block_step = at(9), c.step_sl = at(10), c.step_head = at(11);
    run("far", c);
    return 0;
  }
  const int shapes[][6] = {{8, 8, 8, 2, 4, 2048}, {32, 8, 32, 1, 32, 4096}, {32, 32, 32, 4, 8, 4096}, {8, 1, 9, 3, 5, 256}, {71, 1, 1, 1, 1, 1024}};
  for (const auto& s : shapes)  // (hn, hkv, requests, groups, max_group, capacity): head size 128 position-major, then 64 head-major
    for (int hs : {128, 64}) {
      Case c;
      c.hn = s[0], c.hkv = s[1], c.bs = s[2], c.groups = s[3], c.max_group = s[4], c.cap = s[5], c.hs = hs, c.bk = hs == 64 ? 64 : 16;
      c.step_sl = hs == 64 ? hs : c.hkv * hs, c.step_head = hs == 64 ? c.bk * hs : hs, c.block_step = (long long)c.bk * c.hkv * hs;
      run("plan", c);
    }
  const auto refusal = [&](const char* what, auto edit) {
    Case c;
    edit(c);
    run(what, c);
  };
  refusal("head_size_72", [](Case& c) { c.hs = 72; });
  refusal("step_sl", [](Case& c) { c.step_sl += 8, c.block_step = 16 * c.step_sl; });
  refusal("block_step", [](Case& c) { c.block_step += 8; });
  refusal("base", [](Case& c) { c.vbase += 8; });
  refusal("k_scale_nan", [](Case& c) { c.k_sc = std::numeric_limits<float>::quiet_NaN(); });
  refusal("v_scale_inf", [](Case& c) { c.v_sc = std::numeric_limits<float>::infinity(); });
  refusal("scale_in_front_of_sl_q", [](Case& c) { c.v_sc = -1.f, c.sl_q = 2; });
  refusal("head_size_80", [](Case& c) { c.hs = 80; });  // (a legal FP8 pool: the shared entry's own refusals from here on)
  refusal("alibi_tanh", [](Case& c) { c.flags |= NS_ATTN_FLAG_IS_ALIBI8 | NS_ATTN_FLAG_IS_TANH30; });
  refusal("sl_q_2", [](Case& c) { c.sl_q = 2; });
  refusal("groups_0", [](Case& c) { c.groups = 0; });
  refusal("grid_limit_members", [](Case& c) { c.groups = 256, c.max_group = 256; });
  return 0;
}

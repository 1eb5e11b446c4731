// Program of tests/test_attn_paged_plan.py: the paged form of attn_plan (neural-speed_amd/csrc/ns_attn_plan.cpp: what ns_hip_attn_decode_paged builds —
// the per-request Affine plus an AttnPage) and the key -> cell translation the kernels run (attn_page_cell / attn_page_at, ns_attn.h).  Four kinds of line:
//   plan  <the call, key=value> | <the fields of the paged plan> | <the fields of the per-request (rows) plan of the same shape and capacity>
//   refuse <what is wrong, key=value> | path=.. why=..
//   rule32 pool_blocks=.. block_step=.. hs=.. | path=.. in32=..
//   far32 hs=.. bk=.. over=.. pool_blocks=.. block_step=.. | path=.. in32=..
//   walk  table=<name> | keys=.. cells=.. outside=.. collide=.. noaccess=.. wantno=.. shared=..
// Host code only: no HIP call is made, no tensor exists — the pointers are made-up addresses, the tables live on the host.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <map>
#include <numeric>
#include <random>
#include <set>
#include <vector>

#include "ns_attn.h"
#include "ns_attn_plan.cpp"

using namespace ns;

struct Case {
  int hs = 128, cap = 2048, hn = 8, hkv = 8, bs = 1, bk = 16;
  int head_major = 0;  // blocks: 0 [key][head][dim], 1 [head][key][dim]
  int pool_blocks = 0;  // 0: one block per table entry and four spare
  long long block_step = 0;  // 0: a block's own size
  int table_stride = 0;      // 0: cap / bk
  bool null_table = false;
};

static attn_fp32_fp16_fp16_fp32_fwd_args_t make_args(const Case& c, long long* block_elems) {
  attn_fp32_fp16_fp16_fp32_fwd_args_t a;
  memset(&a, 0, sizeof(a));
  a.Q = reinterpret_cast<float*>(uintptr_t(0x10000));
  a.K = reinterpret_cast<decltype(a.K)>(uintptr_t(0x100000));
  a.V = reinterpret_cast<decltype(a.V)>(uintptr_t(0x200000));
  a.dst = reinterpret_cast<float*>(uintptr_t(0x300000));
  a.Q_sc = a.K_sc = a.V_sc = a.dst_sc = 1.f;
  a.QK_scale = 0.125f;
  a.attn_flags = NS_ATTN_FLAG_IS_CAUSAL;
  a.batch_size = c.bs, a.head_num = c.hn, a.heads_kv = c.hkv, a.head_size = c.hs, a.sl_q = 1, a.sl_kv = c.cap;
  a.Q_layout = a.K_layout = a.V_layout = a.dst_layout = ATTN_FWD_LAYOUT_PLAIN;
  a.step_q_sl = a.step_dst_sl = c.hs;
  a.step_q_head_num = a.step_dst_head_num = c.hs;
  a.step_q_bs = a.step_dst_bs = c.hn * c.hs;
  a.step_k_head_size = a.step_v_head_size = 1;
  *block_elems = (long long)c.bk * c.hkv * c.hs;
  return a;
}
// strides of K / V: inside a block of bk keys (paged) or inside a slab of `rows` keys (rows form)
static void set_kv(attn_fp32_fp16_fp16_fp32_fwd_args_t& a, const Case& c, int rows, bool slab) {
  if (c.head_major) {
    a.step_k_sl = a.step_v_sl = c.hs;
    a.step_k_head_num = a.step_v_head_num = (long long)rows * c.hs;
  } else {
    a.step_k_sl = a.step_v_sl = c.hkv * c.hs;
    a.step_k_head_num = a.step_v_head_num = c.hs;
  }
  a.step_k_bs = a.step_v_bs = slab ? (long long)rows * c.hkv * c.hs : 0;
}

static void print_fields(const AttnPlan& pl, size_t ws, const std::string& why) {
  const AttnSplitParams& sp = pl.sp;
  const char* path[] = {"REFUSED", "GENERIC", "SPLIT_REGS", "RING", "ROWS64", "ROWS128", "PIPELINED", "BLOCK_SPLIT"};
  printf("path=%s G=%d lpk=%d dpl=%d grid=%u,%u,%u block=%u lds=%zu nsplit=%d kps=%d chunks=%d gfull=%d hf=%d dyn=%d,%d,%d tick=%d merge=%d pbytes=%zu "
         "kmove=%d kdelta=%d rows=%d paged=%d slkv=%d kbs=%lld ws=%zu why=%s",
         path[pl.path], pl.G, pl.lpk, pl.dpl, pl.grid.x, pl.grid.y, pl.grid.z, pl.block.x, pl.lds, sp.nsplit, sp.keys_per_split, sp.chunks, sp.g_full,
         sp.heads_first, sp.dyn_min_keys, sp.dyn_batch_keys, sp.dyn_single_below, int(pl.want_tickets), int(pl.merge), pl.partial_bytes,
         sp.kmove != nullptr, sp.kdelta, int(pl.rows), int(pl.paged), sp.a.sl_kv, (long long)sp.a.step_k_bs, ws, why.c_str());
}

static const int g_lens[64] = {0};
static const int g_table[1] = {0};  // (only its address is used by a plan)

static AttnPlan paged_plan(const Case& c, std::string* why, AttnPage* page_out = nullptr) {
  long long block_elems;
  attn_fp32_fp16_fp16_fp32_fwd_args_t a = make_args(c, &block_elems);
  set_kv(a, c, c.bk, false);
  AttnPage pg;
  pg.table = c.null_table ? nullptr : g_table;
  pg.block_shift = attn_block_shift(c.bk);
  pg.table_stride = c.table_stride ? c.table_stride : c.cap / std::max(c.bk, 1);
  pg.pool_blocks = c.pool_blocks ? c.pool_blocks : pg.table_stride * c.bs + 4;
  pg.block_step = c.block_step ? c.block_step : block_elems;
  if (page_out) *page_out = pg;
  Affine aff;  // what ns_hip_attn_decode_paged builds: the rows entry's
  aff.k = g_lens, aff.delta = 1, aff.cap = c.cap, aff.inlaunch = 0, aff.rows = 1, aff.bias = 1;
  return attn_plan(a, nullptr, AttnKnobs(), aff, why, &pg);
}

static void run_plan(const Case& c) {
  std::string why, why_rows;
  const AttnPlan pl = paged_plan(c, &why);
  long long block_elems;
  attn_fp32_fp16_fp16_fp32_fwd_args_t a = make_args(c, &block_elems);
  set_kv(a, c, c.cap, true);
  Affine aff;
  aff.k = g_lens, aff.delta = 1, aff.cap = c.cap, aff.inlaunch = 0, aff.rows = 1, aff.bias = 1;
  const AttnPlan pr = attn_plan(a, nullptr, AttnKnobs(), aff, &why_rows);
  const size_t ws = attn_ws_bytes(AttnKnobs(), c.bs, c.hn, c.hkv, c.hs, 1, c.cap);
  printf("plan hs=%d cap=%d hn=%d hkv=%d bs=%d bk=%d hm=%d | ", c.hs, c.cap, c.hn, c.hkv, c.bs, c.bk, c.head_major);
  print_fields(pl, ws, why);
  printf(" | ");
  print_fields(pr, ws, why_rows);
  printf("\n");
}

static void run_refusal(const char* what, const Case& c) {
  std::string why;
  const AttnPlan pl = paged_plan(c, &why);
  printf("refuse what=%s | path=%s why=%s\n", what, pl.path == AP_REFUSED ? "REFUSED" : "SERVED", why.c_str());
}

static void run_rule32(int pool_blocks, long long block_step, int hs) {
  Case c;
  c.hs = hs, c.cap = 2048, c.bk = 128, c.pool_blocks = pool_blocks, c.block_step = block_step;
  std::string why;
  AttnPage pg;
  const AttnPlan pl = paged_plan(c, &why, &pg);
  const char* path = pl.path == AP_RING ? "RING" : pl.path == AP_SPLIT_REGS ? "SPLIT_REGS" : "OTHER";
  printf("rule32 pool_blocks=%d block_step=%lld hs=%d | path=%s in32=%d why=%s\n", pool_blocks, block_step, hs, path, int(attn_page_in32(pg)), why.c_str());
}

// the pools of tests/test_gpu_attn_far_addresses.py (tests/tools/attn_far_layout.py states the same numbers): 2 requests, 4 / 2 heads, position-major
// blocks of bk keys, the largest pool the rule accepts ("under") and one of 1.4 * 2^31 elements ("over")
static void run_far32(int hs, int bk) {
  for (int over = 0; over < 2; over++) {
    Case c;
    c.hs = hs, c.bk = bk, c.hn = 4, c.hkv = 2, c.bs = 2, c.cap = bk == 16 ? 256 : 512;
    const long long step = (long long)bk * c.hkv * hs;
    c.pool_blocks = over ? int((long long)(1.4 * double(1ll << 31)) / step) : int(((1ll << 31) - 257) / step);
    std::string why;
    AttnPage pg;
    const AttnPlan pl = paged_plan(c, &why, &pg);
    const char* path = pl.path == AP_RING ? "RING" : pl.path == AP_SPLIT_REGS ? "SPLIT_REGS" : "OTHER";
    printf("far32 hs=%d bk=%d over=%d pool_blocks=%d block_step=%lld | path=%s in32=%d why=%s\n", hs, bk, over, pg.pool_blocks, pg.block_step, path,
           int(attn_page_in32(pg)), why.c_str());
  }
}

// every key of every request of a table through attn_page_cell, for K's and V's row strides of both block layouts
static void run_walk(const char* name, const std::vector<int>& table, int requests, int table_stride, int bk, int pool_blocks, int shared_blocks) {
  const int hkv = 2, hs = 64;
  long long outside = 0, collide = 0, noaccess = 0, wantno = 0, keys = 0, shared = 0;
  std::set<long long> all_cells;
  for (int hm = 0; hm < 2; hm++) {
    const long long step_sl = hm ? hs : hkv * hs, step_head = hm ? (long long)bk * hs : hs;
    AttnPage pg;
    pg.table = table.data(), pg.table_stride = table_stride, pg.block_shift = attn_block_shift(bk), pg.pool_blocks = pool_blocks;
    pg.block_step = (long long)bk * hkv * hs + 8;  // (a gap between blocks: the stride is the caller's)
    const long long pool_elems = (long long)pool_blocks * pg.block_step;
    std::map<long long, std::pair<int, int>> owner;  // first element of a key's row of head 0 -> (physical block, key in block)
    for (int b = 0; b < requests; b++)
      for (int n = -1; n <= table_stride * bk; n++) {  // one key in front of and one behind the capacity as well
        const long long cell = attn_page_cell(pg, b, n, step_sl);
        const bool in_cap = n >= 0 && n < table_stride * bk;
        const int id = in_cap ? table[size_t(b) * table_stride + n / bk] : -1;
        const bool valid = in_cap && id >= 0 && id < pool_blocks;
        keys++;
        if (!valid) {
          wantno++;
          noaccess += cell == -1;
          continue;
        }
        if (cell < 0) {
          outside++;
          continue;
        }
        // the whole row of every head lies inside the pool, and inside the key's own block
        for (int h = 0; h < hkv; h++) {
          const long long first = cell + h * step_head, last = first + hs - 1;
          outside += first < 0 || last >= pool_elems || first / pg.block_step != id || last / pg.block_step != id;
        }
        const std::pair<int, int> me(id, n % bk);
        auto it = owner.find(cell);
        if (it == owner.end()) {
          owner[cell] = me;
        } else if (it->second != me) {
          collide++;  // two different (block, key) pairs at one cell
        } else {
          shared++;  // the same physical cell again: two requests naming one block
        }
        if (hm == 0) all_cells.insert(cell);
      }
    // distinct (block, key) pairs never overlap: rows of step_sl elements starting at distinct cells of one head are at least hs apart
    long long prev = -(1ll << 60);
    for (const auto& kv : owner) {
      collide += kv.first - prev < hs;
      prev = kv.first;
    }
  }
  printf("walk table=%s | keys=%lld cells=%zu outside=%lld collide=%lld noaccess=%lld wantno=%lld shared=%lld sharedwant=%lld\n", name, keys, all_cells.size(),
         outside, collide, noaccess, wantno, shared, 2ll * shared_blocks * bk);
}

int main() {
  const int groups[][2] = {{8, 8}, {8, 2}, {8, 1}, {71, 1}};  // (heads, kv heads)
  // 1. the grid of tests/test_attn_rows_plan.py, each capacity rounded up to whole blocks (a paged capacity is table_stride * block_keys), times the
  // block sizes; block layouts alternate
  int n = 0;
  for (int bk : {16, 32, 128, 256})
    for (int bs : {1, 2, 8, 33})
      for (const auto& g : groups)
        for (int hs : {32, 64, 80, 128, 256})
          for (int cap : {1, 255, 256, 300, 2048, 8192}) {
            Case c;
            c.bs = bs, c.hn = g[0], c.hkv = g[1], c.hs = hs, c.bk = bk, c.cap = (cap + bk - 1) / bk * bk, c.head_major = n++ & 1;
            run_plan(c);
          }
  // 2. the refusals
  Case c;
  c.bk = 48;
  c.table_stride = 2048 / 48;
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
  c = Case();
  run_refusal("none", c);
  // 3. the 32-bit rule: (pool_blocks * block_step + 256) * 2 < 2^32 — the ring kernel's descriptor spans the pool; at the boundary and on both sides
  const long long step = 128ll * 8 * 128;            // 131072 elements: a block of 128 keys, 8 kv heads, 128 dims
  const long long limit = (1ll << 31) - 256;         // pool elements from which the rule says no
  run_rule32(int(limit / step), step, 128);          // 16383 blocks: below
  run_rule32(int(limit / step) + 1, step, 128);      // 16384 blocks: 2^31 elements, above
  run_rule32(1, limit - 8, 128);                     // one block just below the boundary (a multiple of 8 elements)
  run_rule32(1, limit, 128);                         // ... at it
  run_rule32(1, limit + 8, 128);
  run_rule32(int(limit / step) + 1, 2 * step, 256);  // the register kernel's own shapes do not care
  for (int hs : {64, 128})
    for (int bk : {16, 128}) run_far32(hs, bk);
  // 4. the translation over every key of a few tables
  {
    const int bk = 16, ts = 6, req = 3, pool = req * ts + 5;
    std::vector<int> ident(static_cast<size_t>(req * ts), 0);
    std::iota(ident.begin(), ident.end(), 0);
    run_walk("identity", ident, req, ts, bk, pool, 0);
    std::vector<int> perm(static_cast<size_t>(pool), 0);
    std::iota(perm.begin(), perm.end(), 0);
    std::mt19937 rng(7);
    std::shuffle(perm.begin(), perm.end(), rng);
    std::vector<int> rnd(perm.begin(), perm.begin() + req * ts);
    run_walk("permutation", rnd, req, ts, bk, pool, 0);
    std::vector<int> share(rnd.begin(), rnd.begin() + 2 * ts);
    share[size_t(ts)] = share[0], share[size_t(ts) + 1] = share[1];  // request 1's first two blocks are request 0's
    run_walk("shared_prefix", share, 2, ts, bk, pool, 2);
    std::vector<int> bad = rnd;
    bad[2] = -1, bad[size_t(ts) + 3] = pool, bad[size_t(2 * ts)] = 0x7fffffff, bad[size_t(2 * ts) + 1] = -0x7fffffff - 1;
    run_walk("out_of_range", bad, req, ts, bk, pool, 0);
    const std::vector<int> big = {3, 1, 0, 2};
    run_walk("block_256", big, 2, 2, 256, 4, 0);
  }
  return 0;
}

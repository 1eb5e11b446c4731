// Program of tests/test_device_plan.py over neural-speed_amd/csrc/ns_device_plan.cpp: one command per input line, one output line per command.
// Addresses are made up (the module never dereferences one); numbers are read with %lli, so 0x10000 is an address.
// One KvMirrorTable lives across the lines; the program plays its owner the way ns_device_kvm.cpp does (lookup; on a miss evict, erase, add)
// and hands out fp16 "allocations" 0x1000000, 0x2000000, ...  A record is named by the number of the add that made it (0, 1, ...).
//   reset                                          -> ok                       (a fresh table)
//   get K V slots heads_kv hs n_ctx                -> hit=1 rec=R slot0=S   |  hit=0 evicted=R,R rec=R slot0=0
//   lookup K V slots heads_kv hs n_ctx             -> rec=R slot0=S | none
//   erase R                                        -> ok
//   hull                                           -> lo=A hi=A                (0 0: no record)
//   cell A                                         -> base=A m16=A elems=N n_ctx=N hs=N transposed=T | none
//   write A bytes                                  -> hit=0|1
//   set_valid A valid                              -> ok
//   fresh R lo hi                                  -> ok                       (sets the mark directly)
//   state R                                        -> valid=v,v fresh=lo,hi
//   producer kv16 K V heads_kv hs n_ctx n_past m   -> refused | rec=R slot0=S k16=A v16=A
//   convert R slot0 batch seq seq_all executing    -> lo=N
//   partials batch rows heads head_size keys       -> N
//   mha batch seq seq_all heads heads_kv head_size n_ctx masked q16 k16 v16 moving attn_supported executing kv16 no_split inlaunch_off
//        -> mirror=T,R split=T,R whole=T,R o16=B inlaunch=N nsplit=N per_row=N chunk=N bytes=N lds=N chunks=r0:nr:sa:ns_c:t:m:o,..|split error or -|whole error or -
//   binary aligned16 dense_off ne0[4] nb0[4] ne1[4] nb1[4] nbd[4]                 -> dense=B bcols4=N
//   lazy kind src dst cols n same_stream a b d ne0[4] nb0[4] ne1[4] nb1[4] nbd[4]  -> plain | norm_mul | silu_first | silu_second
// Plain host C++ (linked with ns_device_plan.cpp): builds with the library's compiler and with g++, sanitizers included.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>

#include "ns_device_plan.h"

static bool rd(long long* v, int n) {
  for (int i = 0; i < n; i++)
    if (scanf("%lli", &v[i]) != 1) return false;
  return true;
}
static void* A(long long v) { return reinterpret_cast<void*>(static_cast<uintptr_t>(v)); }
static unsigned long long U(const void* p) { return static_cast<unsigned long long>(reinterpret_cast<uintptr_t>(p)); }

struct Owner {
  ns::KvMirrorTable table;
  std::map<ns::KvMirrorRec*, int> id;
  std::vector<ns::KvMirrorRec*> by_id;
  long long next16 = 0x1000000;
  // ns_device_kvm.cpp kvm_get, with the evicted records reported
  ns::KvMirrorRec* get(long long* v, int* slot0, bool* hit, std::vector<int>* evicted) {
    ns::KvMirrorRec* m = table.lookup(A(v[0]), A(v[1]), int(v[2]), int(v[3]), int(v[4]), int(v[5]), slot0);
    *hit = m != nullptr;
    if (m) return m;
    for (ns::KvMirrorRec* old : table.evicted_by(A(v[0]), A(v[1]), int(v[2]), int(v[3]), int(v[4]), int(v[5]))) {
      evicted->push_back(id[old]);
      by_id[size_t(id[old])] = nullptr;
      id.erase(old);
      table.erase(old);
    }
    void *k16 = A(next16), *v16 = A(next16 + 0x800000);
    next16 += 0x1000000;
    m = table.add(A(v[0]), A(v[1]), int(v[2]), int(v[3]), int(v[4]), int(v[5]), k16, v16);
    id[m] = int(by_id.size());
    by_id.push_back(m);
    *slot0 = 0;
    return m;
  }
  ns::KvMirrorRec* rec(long long r) { return r >= 0 && size_t(r) < by_id.size() ? by_id[size_t(r)] : nullptr; }
};

static void print_candidate(const char* name, const ns::MhaCandidate& c) { printf("%s=%d,%d ", name, c.tried ? 1 : 0, c.refused ? 1 : 0); }

int main() {
  Owner* o = new Owner();
  char what[16];
  long long v[64];
  while (scanf("%15s", what) == 1) {
    if (!strcmp(what, "reset")) {
      delete o;
      o = new Owner();
      printf("ok\n");
    } else if (!strcmp(what, "get")) {
      if (!rd(v, 6)) return 2;
      int slot0 = -1;
      bool hit = false;
      std::vector<int> ev;
      ns::KvMirrorRec* m = o->get(v, &slot0, &hit, &ev);
      printf("hit=%d", hit ? 1 : 0);
      if (!hit) {
        printf(" evicted=");
        for (size_t i = 0; i < ev.size(); i++) printf(i ? ",%d" : "%d", ev[i]);
      }
      printf(" rec=%d slot0=%d\n", o->id[m], slot0);
    } else if (!strcmp(what, "lookup")) {
      if (!rd(v, 6)) return 2;
      int slot0 = -1;
      ns::KvMirrorRec* m = o->table.lookup(A(v[0]), A(v[1]), int(v[2]), int(v[3]), int(v[4]), int(v[5]), &slot0);
      if (m) printf("rec=%d slot0=%d\n", o->id[m], slot0);
      else printf("none\n");
    } else if (!strcmp(what, "erase")) {
      if (!rd(v, 1) || !o->rec(v[0])) return 2;
      ns::KvMirrorRec* m = o->rec(v[0]);
      o->by_id[size_t(v[0])] = nullptr;
      o->id.erase(m);
      o->table.erase(m);
      printf("ok\n");
    } else if (!strcmp(what, "hull")) {
      printf("lo=%llu hi=%llu\n", U(o->table.hull_lo()), U(o->table.hull_hi()));
    } else if (!strcmp(what, "cell")) {
      if (!rd(v, 1)) return 2;
      ns::KvMirrorCell c;
      if (o->table.args_for_cell(A(v[0]), &c))
        printf("base=%llu m16=%llu elems=%lld n_ctx=%d hs=%d transposed=%d\n", U(c.base32), U(c.m16), c.elems, c.n_ctx, c.hs, c.transposed);
      else printf("none\n");
    } else if (!strcmp(what, "write")) {
      if (!rd(v, 2)) return 2;
      printf("hit=%d\n", o->table.note_foreign_write(A(v[0]), size_t(v[1])) ? 1 : 0);
    } else if (!strcmp(what, "set_valid")) {
      if (!rd(v, 2)) return 2;
      o->table.set_valid(A(v[0]), int(v[1]));
      printf("ok\n");
    } else if (!strcmp(what, "fresh")) {
      if (!rd(v, 3) || !o->rec(v[0])) return 2;
      o->rec(v[0])->fresh_lo = int(v[1]), o->rec(v[0])->fresh_hi = int(v[2]);
      printf("ok\n");
    } else if (!strcmp(what, "state")) {
      if (!rd(v, 1) || !o->rec(v[0])) return 2;
      const ns::KvMirrorRec* m = o->rec(v[0]);
      printf("valid=");
      for (size_t i = 0; i < m->valid.size(); i++) printf(i ? ",%d" : "%d", m->valid[i]);
      printf(" fresh=%d,%d\n", m->fresh_lo, m->fresh_hi);
    } else if (!strcmp(what, "producer")) {
      if (!rd(v, 8)) return 2;
      if (!ns::KvMirrorTable::producer_admits(v[0] != 0, int(v[5]), int(v[6]), int(v[7]))) {
        printf("refused\n");
        continue;
      }
      long long g[6] = {v[1], v[2], 1, v[3], v[4], v[5]};
      int slot0 = -1;
      bool hit = false;
      std::vector<int> ev;
      ns::KvMirrorRec* m = o->get(g, &slot0, &hit, &ev);
      ns::KvMirrorTable::producer_rows(m, slot0, int(v[6]), int(v[7]));
      printf("rec=%d slot0=%d k16=%llu v16=%llu\n", o->id[m], slot0, U(m->k16) + 2ull * slot0 * m->slot_elems(), U(m->v16) + 2ull * slot0 * m->slot_elems());
    } else if (!strcmp(what, "convert")) {
      if (!rd(v, 6) || !o->rec(v[0])) return 2;
      printf("lo=%d\n", ns::KvMirrorTable::convert_from(o->rec(v[0]), int(v[1]), int(v[2]), int(v[3]), int(v[4]), v[5] != 0));
    } else if (!strcmp(what, "partials")) {
      if (!rd(v, 5)) return 2;
      printf("%zu\n", ns::mha_f32_partials_bytes(int(v[0]), int(v[1]), int(v[2]), int(v[3]), int(v[4])));
    } else if (!strcmp(what, "mha")) {
      if (!rd(v, 17)) return 2;
      ns::MhaF32Facts f;
      f.batch = int(v[0]), f.seq = int(v[1]), f.seq_all = int(v[2]), f.heads = int(v[3]), f.heads_kv = int(v[4]), f.head_size = int(v[5]), f.n_ctx = int(v[6]);
      f.masked = v[7] != 0, f.q16 = v[8] != 0, f.k16 = v[9] != 0, f.v16 = v[10] != 0, f.moving = v[11] != 0, f.attn_supported = v[12] != 0, f.executing = v[13] != 0;
      ns::MhaF32Knobs kn;
      kn.kv16 = v[14] != 0, kn.no_split = v[15] != 0, kn.inlaunch_off = v[16] != 0;
      const ns::MhaF32Plan p = ns::mha_f32_plan(f, kn);
      print_candidate("mirror", p.mirror);
      print_candidate("split", p.split);
      print_candidate("whole", p.whole);
      printf("o16=%d inlaunch=%d nsplit=%d per_row=%zu chunk=%d bytes=%zu lds=%zu chunks=", p.mirror_o16 ? 1 : 0, p.mirror_inlaunch, p.nsplit, p.per_row, p.chunk,
             p.partials_bytes, p.lds);
      for (int r0 = 0; r0 < f.seq && p.chunk > 0; r0 += p.chunk) {
        const ns::MhaChunk c = p.chunk_at(r0);
        printf(r0 ? ",%d:%d:%d:%d:%d:%d:%d" : "%d:%d:%d:%d:%d:%d:%d", c.r0, c.nr, c.sa, c.ns_c, c.tickets ? 1 : 0, c.merge ? 1 : 0, c.o16 ? 1 : 0);
      }
      printf("|%s|%s\n", p.split.error ? p.split.error : "-", p.whole.error ? p.whole.error : "-");
    } else if (!strcmp(what, "binary")) {
      if (!rd(v, 22)) return 2;
      const ns::BinaryPlan p = ns::binary_plan(v + 2, v + 6, v + 10, v + 14, v + 18, v[0] != 0, v[1] != 0);
      printf("dense=%d bcols4=%d\n", p.dense ? 1 : 0, p.bcols4);
    } else if (!strcmp(what, "lazy")) {
      if (!rd(v, 29)) return 2;
      ns::LazyNodeFacts n;
      n.kind = int(v[0]), n.src = A(v[1]), n.dst = A(v[2]), n.cols = int(v[3]), n.n = size_t(v[4]), n.same_stream = v[5] != 0;
      static const char* names[] = {"plain", "norm_mul", "silu_first", "silu_second"};
      printf("%s\n", names[ns::lazy_mul_plan(n, A(v[6]), A(v[7]), A(v[8]), v + 9, v + 13, v + 17, v + 21, v + 25)]);
    } else {
      return 2;
    }
  }
  delete o;
  return 0;
}

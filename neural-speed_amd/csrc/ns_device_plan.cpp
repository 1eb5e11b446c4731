// ns_device_plan.cpp — the decisions of ns_device_plan.h as pure code (no HIP call, no environment; the only state is a KvMirrorTable's
// own records); tests/test_device_plan.py checks them on the CPU against the rules written out independently.
#include "ns_device_plan.h"

#include <algorithm>

namespace ns {
namespace {
inline bool overlaps(const char* a, size_t na, const char* b, size_t nb) { return a < b + nb && b < a + na; }
inline const char* bytes_of(const void* p) { return static_cast<const char*>(p); }
inline size_t range_bytes(int slots, int heads_kv, int hs, int n_ctx) { return size_t(heads_kv) * n_ctx * hs * 4 * slots; }
}  // namespace

// ---- KvMirrorTable ------------------------------------------------------------------------------------------------------------------------------
void KvMirrorTable::hull() {
  lo_ = hi_ = nullptr;
  for (const auto& m : recs_)
    for (const char* b : {m->k32, m->v32}) {
      if (!lo_ || b < lo_) lo_ = b;
      if (!hi_ || b + m->bytes32 > hi_) hi_ = b + m->bytes32;
    }
}
KvMirrorRec* KvMirrorTable::lookup(const void* dK, const void* dV, int slots, int heads_kv, int hs, int n_ctx, int* slot0) const {
  const char *k = bytes_of(dK), *v = bytes_of(dV);
  const size_t per_slot = range_bytes(1, heads_kv, hs, n_ctx), bytes = per_slot * slots;
  for (const auto& m : recs_) {
    if (m->heads_kv != heads_kv || m->hs != hs || m->n_ctx != n_ctx || k < m->k32 || k + bytes > m->k32 + m->bytes32) continue;
    const size_t off = size_t(k - m->k32);
    if (off % per_slot != 0 || v != m->v32 + off) continue;
    *slot0 = int(off / per_slot);
    return m.get();
  }
  return nullptr;
}
std::vector<KvMirrorRec*> KvMirrorTable::evicted_by(const void* dK, const void* dV, int slots, int heads_kv, int hs, int n_ctx) const {
  const char *k = bytes_of(dK), *v = bytes_of(dV);
  const size_t bytes = range_bytes(slots, heads_kv, hs, n_ctx);
  std::vector<KvMirrorRec*> out;
  for (size_t i = recs_.size(); i-- > 0;) {
    const KvMirrorRec& m = *recs_[i];
    if (overlaps(k, bytes, m.k32, m.bytes32) || overlaps(v, bytes, m.v32, m.bytes32) || overlaps(k, bytes, m.v32, m.bytes32) ||
        overlaps(v, bytes, m.k32, m.bytes32))
      out.push_back(recs_[i].get());
  }
  return out;
}
KvMirrorRec* KvMirrorTable::add(const void* dK, const void* dV, int slots, int heads_kv, int hs, int n_ctx, void* k16, void* v16) {
  recs_.push_back(std::make_unique<KvMirrorRec>());
  KvMirrorRec* m = recs_.back().get();
  m->k32 = bytes_of(dK), m->v32 = bytes_of(dV), m->bytes32 = range_bytes(slots, heads_kv, hs, n_ctx);
  m->slots = slots, m->heads_kv = heads_kv, m->hs = hs, m->n_ctx = n_ctx, m->k16 = k16, m->v16 = v16;
  m->valid.assign(size_t(slots), 0);
  hull();
  return m;
}
void KvMirrorTable::erase(KvMirrorRec* rec) {
  recs_.erase(std::remove_if(recs_.begin(), recs_.end(), [rec](const std::unique_ptr<KvMirrorRec>& m) { return m.get() == rec; }), recs_.end());
  hull();
}
bool KvMirrorTable::args_for_cell(const void* cell, KvMirrorCell* out) const {
  const char* c = bytes_of(cell);
  if (!lo_ || c < lo_ || c >= hi_) return false;
  for (const auto& m : recs_) {
    const bool in_k = c >= m->k32 && c < m->k32 + m->bytes32, in_v = c >= m->v32 && c < m->v32 + m->bytes32;
    if (!in_k && !in_v) continue;
    out->base32 = in_k ? m->k32 : m->v32, out->m16 = in_k ? m->k16 : m->v16, out->elems = (long long)(m->bytes32 / 4);
    out->n_ctx = m->n_ctx, out->hs = m->hs, out->transposed = in_k ? 0 : 1;
    return true;
  }
  return false;
}
bool KvMirrorTable::note_foreign_write(const void* dst, size_t bytes) {
  const char* c = bytes_of(dst);
  if (!lo_ || !c || c >= hi_ || c + bytes <= lo_) return false;
  bool hit = false;
  for (const auto& m : recs_)
    if (overlaps(c, bytes ? bytes : 1, m->k32, m->bytes32) || overlaps(c, bytes ? bytes : 1, m->v32, m->bytes32)) {
      std::fill(m->valid.begin(), m->valid.end(), 0);
      m->fresh_lo = m->fresh_hi = 0;
      hit = true;
    }
  return hit;
}
void KvMirrorTable::set_valid(const void* k32, int valid) {
  const char* c = bytes_of(k32);
  if (!lo_ || c < lo_ || c >= hi_) return;
  for (const auto& m : recs_)
    if (c >= m->k32 && c < m->k32 + m->bytes32) {
      const size_t per_slot = m->bytes32 / size_t(m->slots);
      m->valid[size_t(c - m->k32) / per_slot] = std::min(valid, m->n_ctx);
    }
}
void KvMirrorTable::producer_rows(KvMirrorRec* rec, int slot0, int n_past, int m) {
  if (slot0 == 0) rec->fresh_lo = n_past, rec->fresh_hi = n_past + m;
}
int KvMirrorTable::convert_from(KvMirrorRec* rec, int slot0, int batch, int seq, int seq_all, bool executing) {
  // (a caller outside the route — a test, a bench — may have filled the cache by any means: everything live is converted for it)
  int lo = executing ? seq_all - seq : 0;
  for (int b = 0; b < batch; b++) lo = std::min(lo, rec->valid[size_t(slot0 + b)]);
  lo = std::max(0, lo);
  // rows the fused QKV launch of this evaluation stored into the mirror itself (ns_route_exec.cpp XK_QKV_ROPE_M) are in place
  if (executing && batch == 1 && slot0 == 0 && rec->fresh_hi > rec->fresh_lo && lo >= rec->fresh_lo && seq_all <= rec->fresh_hi) lo = seq_all;
  rec->fresh_lo = rec->fresh_hi = 0;
  for (int b = 0; b < batch; b++) rec->valid[size_t(slot0 + b)] = seq_all;
  return lo;
}

// ---- mha_f32_plan -------------------------------------------------------------------------------------------------------------------------------
MhaF32Plan mha_f32_plan(const MhaF32Facts& f, const MhaF32Knobs& kn) {
  MhaF32Plan p;
  p.seq = f.seq, p.seq_all = f.seq_all, p.moving = f.moving;
  const auto refuse = [](MhaCandidate& c, bool cond, const char* why) {
    if (cond && !c.refused) c.refused = true, c.why = why;
  };
  // the fp16 mirror + this library's attention kernels: every call shape — a prompt's rows on the matrix-core prefill kernels, a decode
  // step on the LDS-ring kernel, a replayed decode step on the same kernel with its context length moving with the token counter
  p.mirror.tried = kn.kv16;
  refuse(p.mirror, f.head_size % 8 != 0 || f.head_size > 256, "head size not a multiple of 8 up to 256");
  refuse(p.mirror, !f.k16 || !f.v16 || !f.q16, "q / k / v not 16-byte aligned");
  refuse(p.mirror, size_t(f.batch) * f.heads_kv > 65535, "batch x kv heads beyond a grid dimension");
  refuse(p.mirror, size_t(f.seq) * f.heads * f.head_size >= (size_t(1) << 31) || size_t(f.n_ctx) * f.heads_kv * f.head_size >= (size_t(1) << 31),
         "32-bit element steps");
  refuse(p.mirror, f.moving && f.seq != 1, "a moving length is a decode step");
  refuse(p.mirror, !f.attn_supported, "the attention kernels do not take the shape");
  p.mirror_o16 = f.executing;
  p.mirror_inlaunch = kn.inlaunch_off ? 0 : 1;

  // the context split over workgroups: head sizes 64 / 128 / 256, from two 128-key ranges on; a moving length always
  const bool split_hs = f.head_size == 64 || f.head_size == 128 || f.head_size == 256;
  if (f.moving && !(f.seq == 1 && split_hs && f.n_ctx >= f.seq_all))
    p.split.error = "mha_f32: a moving context length needs the context-split kernel (decode step, head size 64 / 128 / 256)";
  const int keys = f.moving ? f.n_ctx : f.seq_all;
  p.nsplit = (keys + kMhaKS - 1) / kMhaKS;
  p.split.tried = (!kn.no_split || f.moving) && (p.nsplit >= 2 || f.moving);
  refuse(p.split, !split_hs, "head size not 64 / 128 / 256");
  refuse(p.split, size_t(f.batch) * f.seq > 65535 || f.heads > 65535, "rows or heads beyond a grid dimension");
  refuse(p.split, !f.q16 || !f.k16, "q / k not 16-byte aligned");
  // a prompt's rows (batch 1, causal) go through in chunks so that the partials stay within 64 MB of scratch whatever the prompt length
  // (2048 rows x 32 heads x 16 ranges would be 545 MB, kept for the life of the stream)
  p.per_row = mha_f32_partials_bytes(1, 1, f.heads, f.head_size, keys);
  p.chunk = f.seq;
  if (f.batch == 1 && f.masked && size_t(f.seq) * p.per_row > kMhaPartialsCap) p.chunk = int(std::max<size_t>(1, kMhaPartialsCap / p.per_row));
  p.partials_bytes = mha_f32_partials_bytes(f.batch, p.chunk, f.heads, f.head_size, keys);
  // replayed decode step: the last live range merges inside the launch (tickets zeroed when allocated, self-resetting)
  p.tickets = f.moving && f.seq == 1 && !kn.inlaunch_off && size_t(f.batch) * f.heads <= 65536;

  p.whole.tried = true;
  p.lds = (size_t((f.seq_all + 3) & ~3) + 256) * sizeof(float);
  if (f.moving) {
    p.whole.refused = true, p.whole.why = "no moving length";
    p.whole.error = "mha_f32: the moving-length form needs 16-byte aligned q / k and scratch for the partials";
  } else if (p.lds > kMhaWholeLds) {
    p.whole.refused = true, p.whole.why = "scores beyond the LDS";
    p.whole.error = "mha_f32: context too long for the device-layout attention kernel";
  }
  return p;
}
MhaChunk MhaF32Plan::chunk_at(int r0) const {
  MhaChunk c;
  c.r0 = r0, c.nr = std::min(chunk, seq - r0);
  c.sa = chunk == seq ? seq_all : seq_all - seq + r0 + c.nr;
  c.ns_c = moving ? nsplit : (c.sa + kMhaKS - 1) / kMhaKS;
  c.tickets = tickets;
  c.merge = !tickets && (c.ns_c > 1 || moving);
  c.o16 = moving && seq == 1;
  return c;
}

// ---- binary_plan, lazy_mul_plan -----------------------------------------------------------------------------------------------------------------
namespace {
bool dense(const long long* ne, const long long* nb) {
  long long st = 4;
  for (int i = 0; i < 4; i++) {
    if (ne[i] != 1 && nb[i] != st) return false;
    st *= ne[i];
  }
  return true;
}
bool packed(const long long ne[4], const long long nb[4]) {
  return nb[0] == 4 && nb[1] == 4 * ne[0] && nb[2] == nb[1] * ne[1] && nb[3] == nb[2] * ne[2];
}
}  // namespace
BinaryPlan binary_plan(const long long ne0[4], const long long nb0[4], const long long ne1_[4], const long long nb1[4], const long long nbd[4],
                       bool aligned16, bool dense_off) {
  long long ne1[4], total = 1;
  for (int i = 0; i < 4; i++) ne1[i] = ne1_[i] > 0 ? ne1_[i] : 1, total *= ne0[i];
  const bool same = ne1[0] == ne0[0] && ne1[1] == ne0[1] && ne1[2] == ne0[2] && ne1[3] == ne0[3];
  const bool rowvec = ne1[0] == ne0[0] && ne1[1] == 1 && ne1[2] == 1 && ne1[3] == 1 && nb1[0] == 4;
  BinaryPlan p;
  p.dense = !dense_off && total >= kDenseBinaryMin && (ne0[0] & 3) == 0 && dense(ne0, nb0) && dense(ne0, nbd) &&
            ((same && dense(ne1, nb1)) || rowvec) && aligned16;
  p.bcols4 = p.dense && !same ? int(ne0[0] / 4) : 0;
  return p;
}
LazyMul lazy_mul_plan(const LazyNodeFacts& n, const void* a, const void* b, const void* d, const long long ne0[4], const long long nb0[4],
                      const long long ne1[4], const long long nb1[4], const long long nbd[4]) {
  if (!n.kind || !a || !b || !d || !n.same_stream || !packed(ne0, nb0) || !packed(ne0, nbd)) return LAZY_PLAIN;
  // (in place — ne_mul_inplace: dst == the node's output — the two stores of a fused kernel would alias)
  if (d == n.src || d == n.dst || ne0[0] * ne0[1] * ne0[2] * ne0[3] != (long long)n.n) return LAZY_PLAIN;
  if (n.kind == 1 && a == n.dst && ne0[0] == n.cols && ne1[0] == n.cols && ne1[1] <= 1 && ne1[2] <= 1 && ne1[3] <= 1 && nb1[0] == 4) return LAZY_NORM_MUL;
  const bool same_shape = ne1[0] == ne0[0] && ne1[1] == ne0[1] && ne1[2] == ne0[2] && ne1[3] == ne0[3] && packed(ne1, nb1);
  if (n.kind == 2 && same_shape && (a == n.dst) != (b == n.dst)) return a == n.dst ? LAZY_SILU_FIRST : LAZY_SILU_SECOND;
  return LAZY_PLAIN;
}

}  // namespace ns

// ns_device_plan.h — what the device backend decides on the host, as values: the records of the fp16 kv mirrors (KvMirrorTable: which mirror
// holds a cache range, which ones a new range evicts, which positions are converted again), the server of a device-layout attention call
// (mha_f32_plan), the kernel of a binary node (binary_plan) and what the lazy peephole makes of a multiply (lazy_mul_plan).  Plain C++: no
// HIP type, no library header, and no pointer it is given is ever dereferenced — it builds with any host compiler and takes made-up
// addresses (tests/tools/device_plan_main.cpp, tests/test_device_plan.py).  ns_device_kvm.cpp, ns_device_mha.hip and ns_device_ops.hip fill
// knobs and facts and follow the plans.
#pragma once
#include <cstddef>
#include <cstdint>
#include <memory>
#include <vector>

namespace ns {

// ---- the fp16 mirrors of the reference's fp32 device kv cache (ns_route.h says why and how they stay coherent) --------------------------------
struct KvMirrorRec {
  const char* k32 = nullptr;   // the fp32 K cache the graph handed to the attention node ([slots][heads_kv][n_ctx][hs])
  const char* v32 = nullptr;   // ... and its V cache ([slots][heads_kv][hs][n_ctx])
  size_t bytes32 = 0;          // of each
  int slots = 0, heads_kv = 0, hs = 0, n_ctx = 0;
  void *k16 = nullptr, *v16 = nullptr;  // the owner's fp16 allocations, [slots][heads_kv][n_ctx][hs] both: opaque here
  std::vector<int> valid;      // per slot: positions [0, valid) of the mirror hold the cache
  int fresh_lo = 0, fresh_hi = 0;  // slot 0: positions a producer stored into the mirror itself since the last attention (producer_rows)
  size_t slot_elems() const { return size_t(heads_kv) * n_ctx * hs; }  // elements of one slot, fp32 and fp16 alike
};
// what a cache-writing launch is told about the mirror behind one fp32 cell (KvMirrorArgs of ns_route.h, without the overflow word)
struct KvMirrorCell {
  const char* base32 = nullptr;
  void* m16 = nullptr;
  long long elems = 0;
  int n_ctx = 0, hs = 0, transposed = 0;  // K is reported as transposed = 0, V as 1
};
class KvMirrorTable {
 public:
  // the record that holds the `slots` slots starting at (k, v): same geometry, the range inside the record, the offset a multiple of one
  // slot, V at the same offset; *slot0 = the first slot.  nullptr: none does
  KvMirrorRec* lookup(const void* k, const void* v, int slots, int heads_kv, int hs, int n_ctx, int* slot0) const;
  // the records a new mirror of that range evicts: any of its K / V ranges overlaps any of theirs (newest first).  The caller frees
  // their fp16 memory and erases them
  std::vector<KvMirrorRec*> evicted_by(const void* k, const void* v, int slots, int heads_kv, int hs, int n_ctx) const;
  KvMirrorRec* add(const void* k, const void* v, int slots, int heads_kv, int hs, int n_ctx, void* k16, void* v16);  // every slot valid = 0
  void erase(KvMirrorRec* rec);
  bool empty() const { return recs_.empty(); }
  KvMirrorRec* newest() const { return recs_.empty() ? nullptr : recs_.back().get(); }
  const char* hull_lo() const { return lo_; }  // hull of every mirrored fp32 range (one compare rules a pointer out); nullptr: no record
  const char* hull_hi() const { return hi_; }

  bool args_for_cell(const void* cell, KvMirrorCell* out) const;
  // mirrors that overlap [dst, dst + bytes) start over (every valid and fresh mark cleared); bytes == 0 counts as 1.  true: there was one
  bool note_foreign_write(const void* dst, size_t bytes);
  void set_valid(const void* k32, int valid);  // the slot that holds the K cell k32; clamped to n_ctx
  // may a producer store rows [n_past, n_past + m) into a mirror itself?
  static bool producer_admits(bool kv16, int n_ctx, int n_past, int m) { return kv16 && n_past >= 0 && m >= 1 && n_past + m <= n_ctx; }
  // ... it is about to: the rows are marked fresh when the mirror starts at slot 0 (a later slot's rows are converted like any others)
  static void producer_rows(KvMirrorRec* rec, int slot0, int n_past, int m);
  // an attention call outside a replay reads slots slot0 .. slot0 + batch: the first position of [0, seq_all) it has to convert (seq_all:
  // nothing).  The rows this evaluation wrote (the last `seq`, when the route is executing: its cache protocol is known) are converted
  // again, older ones once, each slot from its own mark; rows a producer stored into the mirror itself are in place.  Clears the fresh
  // mark and sets the batch's slots to valid = seq_all.
  static int convert_from(KvMirrorRec* rec, int slot0, int batch, int seq, int seq_all, bool executing);

 private:
  void hull();
  std::vector<std::unique_ptr<KvMirrorRec>> recs_;
  const char *lo_ = nullptr, *hi_ = nullptr;
};

// ---- ns_hip_mha_f32_device_layout: which server takes a call ------------------------------------------------------------------------------------
constexpr int kMhaKS = 128;                      // keys per workgroup of mha_f32_split_kernel: one range
constexpr size_t kMhaTicketBytes = 65536 * 4;    // its merge tickets: one word per (row, head) of a replayed decode step
constexpr size_t kMhaPartialsCap = size_t(64) << 20;  // a causal prompt goes through in row chunks so that the partials stay within this
constexpr size_t kMhaWholeLds = 160 * 1024;      // mha_f32_kernel: LDS of one workgroup
// partials of `rows` query rows per batch entry over `keys` keys: (max, sum, head_size outputs) per (row, head, range)
inline size_t mha_f32_partials_bytes(int batch, int rows, int heads, int head_size, int keys) {
  return size_t(batch) * rows * heads * size_t((keys + kMhaKS - 1) / kMhaKS) * (2 + head_size) * sizeof(float);
}

struct MhaF32Knobs {      // resolved by mha_f32_knobs() (ns_device_mha.hip, the only reader)
  bool kv16 = true;           // NS_DEVICE_KV / "device_kv_f16": attention reads the fp16 mirror
  bool no_split = false;      // NS_MHA_NO_SPLIT: diagnostics (A/B), ignored for a moving length
  bool inlaunch_off = false;  // NS_MHA_INLAUNCH=0: a replayed decode step merges its ranges in a launch of its own
};
struct MhaF32Facts {
  int batch = 0, seq = 0, seq_all = 0, heads = 0, heads_kv = 0, head_size = 0, n_ctx = 0;
  bool masked = false;
  bool q16 = true, k16 = true, v16 = true;  // the operand's address is a multiple of 16
  bool moving = false;          // the context length moves with the replayed graph's token counter (Affine::k is set)
  bool attn_supported = false;  // bestla_fusion_attn_fp32_fp16_fp16_fp32_support takes the shape
  bool executing = false;       // route_executing(): the call is a launch the route issues
};
// One server of a call.  tried: the knobs admit it; refused: its envelope excludes the call, `why` says which bound.  error != nullptr: a
// call that gets as far as this server ends there with that text (a moving length has no server behind the context split).
struct MhaCandidate {
  bool tried = false, refused = false;
  const char* why = "";
  const char* error = nullptr;
  bool offered() const { return tried && !refused; }
};
struct MhaChunk {
  int r0, nr;    // query rows r0 .. r0 + nr of every batch entry
  int sa;        // keys the chunk's last row sees: a causal call's rows r0 .. r0 + nr are the same call on nr rows over the first sa keys
  int ns_c;      // ranges of the launch (and of the partials' layout)
  bool tickets;  // the last live range merges inside the launch
  bool merge;    // mha_f32_merge_kernel follows
  bool o16;      // the fp16 copy of the output rows is written if the route asked for one
};
// mirror (this library's attention kernels on the fp16 mirror), split (mha_f32_split_kernel), whole (mha_f32_kernel) — in this order.
// At run time the mirror hands the call on when no mirror can be allocated, the split without scratch for the partials.
struct MhaF32Plan {
  MhaCandidate mirror, split, whole;
  bool mirror_o16 = false;   // mirror: the route's fp16 output copy is passed on
  int mirror_inlaunch = 1;   // mirror, moving: Affine::inlaunch
  int nsplit = 0;            // split: ranges of the partials' layout (of n_ctx for a moving length, else of seq_all)
  size_t per_row = 0;        // ... bytes of partials per query row
  int chunk = 0;             // ... query rows per launch
  size_t partials_bytes = 0; // ... scratch of the partials: mha_f32_partials_bytes(batch, chunk, ...) = batch * chunk * per_row
  size_t lds = 0;            // whole: dynamic LDS bytes
  MhaChunk chunk_at(int r0) const;  // r0 = 0, chunk, 2 chunk, ... < seq
  // (what chunk_at needs of the call)
  int seq = 0, seq_all = 0;
  bool moving = false, tickets = false;
};
MhaF32Plan mha_f32_plan(const MhaF32Facts& f, const MhaF32Knobs& kn);

// ---- ns_hip_binary_nd_f32: dense_binary_kernel or nd_binary_kernel ------------------------------------------------------------------------------
constexpr long long kDenseBinaryMin = 4096;  // elements from which the four-per-thread kernel is worth its conditions
struct BinaryPlan {
  bool dense = false;  // dense_binary_kernel: src0, dst dense, src1 dense of the same shape or a row vector, ne0[0] in fours, 16-byte aligned
  int bcols4 = 0;      // ... 0: same shape; else ne0[0] / 4, src1 is a row vector
};
// aligned16: all three addresses are multiples of 16; dense_off: NS_DENSE_BINARY=0.  An extent of src1 below 1 counts as 1
BinaryPlan binary_plan(const long long ne0[4], const long long nb0[4], const long long ne1[4], const long long nb1[4], const long long nbd[4],
                       bool aligned16, bool dense_off);

// ---- the lazy peephole: what ns_hip_lazy_mul makes of the recorded node -------------------------------------------------------------------------
struct LazyNodeFacts {
  int kind = 0;  // 0 none, 1 rms norm, 2 silu
  const void *src = nullptr, *dst = nullptr;
  int cols = 0;
  size_t n = 0;               // elements
  bool same_stream = false;   // the multiply is issued on the stream the node was recorded for
};
enum LazyMul : int {
  LAZY_PLAIN = 0,     // the recorded node is launched as it stands, then the plain multiply
  LAZY_NORM_MUL,      // norm . weight in one launch (a = the norm's output, b = a row vector)
  LAZY_SILU_FIRST,    // silu(x) . b: a is the silu's output
  LAZY_SILU_SECOND,   // a . silu(x): b is
};
// plain whenever the product is written over the node's input or output (the fused kernels' two stores would alias), the node is
// consumed as both operands, src0 / dst are not packed, or the shapes are not the recorded ones
LazyMul lazy_mul_plan(const LazyNodeFacts& n, const void* a, const void* b, const void* d, const long long ne0[4], const long long nb0[4],
                      const long long ne1[4], const long long nb1[4], const long long nbd[4]);

}  // namespace ns

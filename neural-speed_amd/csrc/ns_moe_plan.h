// ns_moe_plan.h — what the mixture-of-experts family decides on the host, as values: which server takes a call (moe_mm_plan, moe_ffn_plan)
// and the (row, selection) pair layout both grouped forms gather by (moe_pair_plan).  Plain C++: no HIP type, no library header — it builds
// with any host compiler (tests/tools/moe_plan_main.cpp, tests/test_moe_plan.py).  ns_moe.cpp fills knobs and facts and follows the plan.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace ns {

// Every tunable the family reads, resolved by moe_knobs() (ns_moe.cpp, the only reader): a non-zero tuning key wins, else the environment
// variable (read once per process), else the built-in value.
struct MoeKnobs {
  int gemv_rows = 8;          // "moe_gemv_rows" / NS_MOE_GEMV_ROWS: the decode launches and the block's fused launches serve m <= this; <= 0 = never
  int grouped_rows = 32;      // "moe_grouped_rows" / NS_MOE_GROUPED_ROWS: ns_hip_mul_mat_id's grouped path serves m >= this; <= 0 = never
  int ffn_grouped_rows = 32;  // "moe_ffn_grouped_rows", else NS_MOE_GROUPED_ROWS, else 32 (NOT "moe_grouped_rows"): the block's grouped pass; <= 0 = never
  int ffn_fused = -1;         // "moe_ffn_fused": 0 = the block never takes its fused launches; 1 / -1 (default) = inside their envelope
  int ffn_device_rows = 0;    // "moe_ffn_device_rows" / NS_MOE_FFN_DEVICE_ROWS: the block's device-grouped pass serves m <= this; 0 (default) = never
  int ffn_chunk_rows = 0;     // "moe_ffn_chunk_rows" (no environment variable): cap of 1 .. 16 on the rows of a chunk; 0 = by LDS fit (moe_chunk_rows)
};

// What a decision needs from the weights and the call.  ns_hip_mul_mat_id describes its one group as `gate` (k = its K, ff = its N).
struct MoeFacts {
  bool gate_f8 = false, up_f8 = false, down_f8 = false;  // the group's weight kind is fp8 (all a decision asks about a kind)
  int k = 0, ff = 0, dn = 0;                              // gate / up: [ff][k], down: [dn][ff]
  int n_as = 0, n_used = 1, m = 0;
  bool single_span = true;   // every group's records, scales and zero points lie in one allocation (the decode kernel's addressing)
  bool shuf = false;         // an activation shuffle (act-order weights)
  bool all_tiled_f8 = true;  // fp8 only: the tiled kernel takes EVERY expert of the group (gemm3_takes)
  bool gate_up_one_format = true;
  bool capturing = false;    // the stream is being captured: nothing may read the ids on the host
  // the device-grouped pass alone: columns of a k-step record of the gate / up and of the down format (0: unknown, the pass refuses), and
  // whether the int8-reference compute mode is on
  int gu_kstep = 0, dn_kstep = 0;
  bool i8_mode = false;
};

// One server of a call.  tried: the row thresholds and the capture state admit it; refused: its static envelope excludes the call (the
// reasons stand beside the conditions in ns_moe_plan.cpp).  A candidate that is offered() may still hand the call on at run time.
struct MoeCandidate {
  bool tried = false, refused = false;
  bool offered() const { return tried && !refused; }
};

// ns_hip_mul_mat_id: grouped path, decode launches, loop kernel — the last takes every call.  At run time the grouped path hands the call on
// when a populated expert has fewer than min_group_rows rows, without scratch, and when launch_gemm2 answers hipErrorNotSupported; the decode
// launches when launch_gemv does so for row 0.  ns_hip_moe_stats: [0] / [1] / [2] count the calls grouped / decode / loop served; [3] every
// grouped candidate that was TRIED and did not serve, refused here or at run time alike (never a call below the threshold or being captured).
struct MoeMmPlan {
  MoeCandidate grouped, decode;
  int min_group_rows = 0;  // of the grouped path: 17 for fp8 experts (the tiled kernel's fp8 range), else 0
};
MoeMmPlan moe_mm_plan(const MoeKnobs& kn, const MoeFacts& f);

// The block entries: fused decode launches, device-grouped pass, grouped pass, composition of ns_hip_mul_mat_id calls — in this order, the
// last takes every call.  At run time the fused launches hand the call on without scratch and when launch_gemv answers
// hipErrorNotSupported to the gate / up or the first down launch; the device-grouped pass without scratch and when gemv_plan refuses one of
// its two launches (both are planned before the first launch goes out); the grouped pass when moe_pair_plan refuses the table, when
// !moe_rows_addressable, without scratch and when launch_gemm2 answers hipErrorNotSupported.  dOut is untouched in each case.
// ns_hip_moe_ffn_stats: [0] / [1] / [3] count the calls fused / composition / grouped served; [2] counts fused LAUNCHES: 1 + n_used of a
// served call, and 1 when the gate / up launch went out and the first down launch refused.  ns_hip_moe_ffn_stats_ex adds [4]: the calls the
// device-grouped pass served, [5]: the launches it issued, [6]: the calls where it was TRIED and handed on (refused here or at run time).
struct MoeFfnPlan {
  MoeCandidate fused, grouped;
  MoeCandidate device;  // the device-grouped pass (opt-in: MoeKnobs::ffn_device_rows), asked between the two
};
MoeFfnPlan moe_ffn_plan(const MoeKnobs& kn, const MoeFacts& f);

// the fused launches put the pairs along grid.y and divide by n_used with a 16-bit reciprocal (GemvParams::moe_sel_mul)
bool moe_pairs_fit_grid(int m, int n_used);
// the tiled GEMM indexes the gathered buffers with 32-bit element offsets: rows x the widest of them stays below 2^31
bool moe_rows_addressable(size_t rows, int k, int ff, int dn);

// Pair (t, i) is selection i of token row t, its expert is ids[t * ids_stride + i].  The pairs whose id lies in [0, n_as) are laid out in
// GROUP ORDER: expert 0's pairs first, then expert 1's, ...; inside a group by (t, i) ascending (a stable counting sort).  A gathered
// position j in [0, pairs) is one row of the fp16 activations, of the fp16 intermediate and of the fp32 products.  ns_hip_mul_mat_id's
// grouped path is the n_used = 1 case over the id column it reads back.
struct MoePairPlan {
  int pairs = 0;                     // pairs with an id in range = gathered rows
  std::vector<int32_t> offset;       // [n_as] first gathered position of expert e's group (consecutive: offset[e + 1] = offset[e] + count[e])
  std::vector<int32_t> count;        // [n_as] pairs of expert e (0: no launch for it)
  // [n_as] rows expert e's GEMMs are launched with: count[e], except that a ONE-row group is launched with 2 rows, the tiled kernel's
  // minimum.  Its second row is position offset[e] + 1: the first row of the next populated group — rewritten when that group is launched,
  // which is why the groups go out in ascending expert order — or, for the last group, the padding row at position `pairs`.  Every
  // buffer indexed by position therefore has pairs + 1 rows.
  std::vector<int32_t> launch_rows;
  std::vector<int32_t> src_row;      // [pairs + 1] token row gathered at position j; src_row[pairs] = -1: the padding row (zeros)
  std::vector<int32_t> pos;          // [m * n_used] gathered position of pair t * n_used + i; -1: its id is outside [0, n_as), it is in no group
};

// false (plan untouched): m, n_used or n_as below 1, ids_stride below n_used, over 2^30 pairs, or a populated group below min_group_rows pairs
bool moe_pair_plan(const int32_t* ids, int ids_stride, int m, int n_used, int n_as, MoePairPlan* plan, int min_group_rows = 0);

// ---- the device-grouped pass: the same pair layout, made by moe_pair_sort_kernel (ns_moe_group.hip), and its CHUNKS ----------------------------
// A chunk is what one workgroup column of the expert-chunk streaming launch (gemv_kernel XV = 6) serves: up to R consecutive gathered positions
// of ONE expert, staged as R activation rows beside one stream of that expert's weights.
constexpr size_t kMoeChunkALds = 64 * 1024;  // = kGvMaxALds (ns_gemv.h; ns_moe.cpp asserts it): fp16 activation bytes a workgroup stages
constexpr int kMoeChunkMaxRows = 16;         // = kGvMaxRows: the rows of the MFMA's A operand
constexpr int kMoeDevMaxPairs = 1024;        // one workgroup sorts the pairs
// rows of k columns one workgroup can stage (a staged row: ks k-steps + 8 halves), at most 16, at most cap when cap > 0; at least 1
int moe_chunk_rows(int k, int kstep, int cap);
struct MoeChunk {
  int32_t expert, first, rows;  // gathered positions first .. first + rows - 1, all of `expert`
};
struct MoeChunkPlan {
  int pairs = 0;
  std::vector<int32_t> offset, count;  // [n_as], as in MoePairPlan
  std::vector<int32_t> src_row;        // [m * n_used]: token row of position j < pairs, -1 behind them
  std::vector<int32_t> pos;            // [m * n_used]: as in MoePairPlan
  std::vector<MoeChunk> chunks;        // e ascending, c = 0 .. ceil(count[e] / R) - 1: {e, offset[e] + c R, min(R, count[e] - c R)}
};
// false (out untouched): as moe_pair_plan, or R outside 1 .. 16
bool moe_chunk_plan(const int32_t* ids, int ids_stride, int m, int n_used, int n_as, int R, MoeChunkPlan* out);
// upper bound of the chunk count over ALL id tables: with P = m n_used pairs, floor((P + min(n_as, P) (R - 1)) / R).  The grid of the
// streaming launch is sized by it, without a look at the ids
int moe_chunk_slots(int m, int n_used, int n_as, int R);

}  // namespace ns

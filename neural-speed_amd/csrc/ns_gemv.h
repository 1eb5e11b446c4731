// ns_gemv.h — what the files of the decode kernel share.  ns_gemv.hip holds gemv_kernel, its device helpers and the launch ladder, compiled
// once per weight kind and scales-per-record count (NS_GEMV_SLICES below: the 1169 instantiations in one translation unit took thirteen
// minutes to compile).  Host: ns_gemv_plan.cpp decides a launch (gemv_plan: a pure function, checked on the CPU by tests/test_stream_plan.py),
// ns_gemv_host.cpp holds the tuning state and launches what the plan says.  The last part is what BOTH weight-streaming kernels' plans
// share (ns_gemvs.h: gemvs_kernel): the matrix table, the ring-slot size, the one-format rule.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>

#include "ns_common.h"
#include "ns_dev.h"
#include "ns_moe.h"  // MoeExpertRow: one row of an expert group's device table

namespace ns {

#ifndef NS_GV_PF
#define NS_GV_PF 4
#endif
// records each wave keeps in flight (fused gate/up: half of them per matrix).  A CU's memory pipeline holds about
// 50 KiB of requests; beyond that the ISSUE of further requests stalls (profiles/r02h_wave_trace: ring fills of a
// 24-wave CU complete 0.5 ... 6 us after entry), so a deeper ring only delays the other waves' first records:
// 8 deep measured 12 % slower on the whole chain than 4 deep (profiles/r02g_sweep.txt)
constexpr int kGvPF = NS_GV_PF;
constexpr int kGvMaxRows = 16;
constexpr size_t kGvMaxALds = 64 * 1024;    // staged activations (fp16) per workgroup
constexpr size_t kGvMaxLds = 160 * 1024;
constexpr int kGvA32Regs = 8;  // 16-byte loads of fp32 activations a wave holds in registers (XV = 2)

// one matrix of a launch as the kernel sees it; a fused QKV launch looks its matrix up BY INDEX in the kernel-argument
// segment (one scalar load) instead of carrying three of everything in SGPRs
struct GemvMat {
  const uint8_t* wbase;  // ONE allocation: records at 0, scales at s_off, zero points at z_off
  uint32_t s_off, z_off;
  uint32_t tile_begin;   // first global tile of this matrix in the launch
  int n;
  float* c;
  _Float16* c16;
};
static_assert(sizeof(GemvMat) == 40, "GemvMat is addressed by index in the kernel-argument segment");

// RoPE of q and k + kv-cache append as the epilogue of a fused QKV launch (ns_qkv_rope).  Adjacent pairs (mode 0) always lie
// inside one 16-column tile (GV_MSEG).  NeoX pairs (e, e + head_size / 2) lie head_size / 32 tiles apart: a workgroup of the
// pair mode (GV_MSEGP) streams both tiles, so no value is handed between workgroups
struct GemvRope {
  _Float16* kc;
  _Float16* vc;
  long long c_sl, c_head;  // cache element strides per position / per head
  const float2* cos_sin;   // [row][head_size / 2] (cos, sin) * attn_factor of position n_past + row (ns_hip_rope_cos_sin)
  int head_size, n_past;
  int on;
  // replayed device route (QkvRopeRoute, ns_common.h; one row): k (rotated) and v also go to the reference's fp32 cache cells, and the
  // position follows the captured graph's token counter
  int kd_pos;
  const int* kmove;
  float* k32;
  float* v32;
  long long k32_head, k32_dim, k32_tok, v32_head, v32_dim, v32_tok;
  uint32_t* ovf;
};

struct GemvParams {
  // ---- hot head: everything the prologue needs, fetched by one batch of scalar loads ----
  const uint8_t* wbase0;    // matrix 0 (and, for the fused gate/up launch, matrix 1)
  const uint8_t* wbase1;
  const void* a;            // activations, fp16 [m][lda]
  uint32_t ks;              // k-steps per tile
  uint32_t qstride;         // bytes per (tile, k-step) record
  uint32_t nw_log2;         // log2(waves per workgroup)
  uint32_t s_off0, s_off1;
  uint32_t sstride;
  uint32_t srows, srow_mul, srow_shift;
  uint32_t tb1, tb2;        // first global tile of matrices 1 and 2 of a fused QKV launch (2^32 - 1: absent)
  int m, k, lda;
  uint32_t row_stride;      // halves per staged row in LDS
  uint32_t ring_off;        // byte offset of the per-wave rings in LDS (the reduction scratch reuses them)
  uint32_t ring_stride;     // bytes of one wave's ring = slots x slot size
  uint32_t z_off0, z_off1, zstride;  // asymmetric formats only: last, so that the rest is one contiguous run of words
  // int8-reference numerics (XV = 3): a = u8 activation codes [m][lda]; i8_corr = [m][nblk] fp32 scales followed by
  // [m][nblk] u8 zero points (one span, staged at ssq_off); k-block of column kk = kk >> i8_bshift
  const uint8_t* i8_corr;
  uint32_t i8_span, i8_nblk, i8_bshift;
  // expert-indexed launch (XV = 4, ns_hip_mul_mat_id at decode size): the weight base is table[*moe_id].codes — every expert of a
  // group has the same shape and layout, so the offsets above hold for all of them; an id outside [0, moe_n) gives epi(0, d)
  const MoeExpertRow* moe_table;
  const int32_t* moe_id;
  int moe_n;
  // ... and its (row, selection) pairs along grid.y (ns_hip_moe_ffn_silu; a ns_hip_mul_mat_id launch is the single pair 0): pair y is
  // row = (y * moe_sel_mul) >> 16 (= y / moe_nsel, exact while y * moe_nsel < 65536), sel = y - row * moe_nsel; its id is
  // moe_id[row * moe_ids_stride + sel], its activations a + row * moe_a_stride, its output (and D operand) row y * moe_c_stride
  // (moe_d_stride) floats behind mat[0].c (d); moe_w (nullptr: 1) holds a factor per pair, [row * moe_w_stride + sel], multiplied into the
  // product in front of the epilogue.  GV_DUAL: the second matrix is moe_table1[id].codes (the up group; same shape and format)
  // Expert CHUNKS along grid.y (XV = 6, the block entries' device-grouped pass) reuse five of these fields: moe_id is the chunk list
  // (MoeRoute::chunks), moe_table / moe_table1 / moe_n as above, moe_nsel the gathered positions (no chunk reaches beyond them); m is the
  // most rows a chunk has (what LDS is sized for), a / mat[0].c / mat[0].c16 are indexed by gathered position with strides lda / ldc
  const MoeExpertRow* moe_table1;
  const float* moe_w;
  uint32_t moe_sel_mul, moe_nsel;
  int moe_ids_stride, moe_w_stride;
  uint32_t moe_a_stride, moe_c_stride, moe_d_stride;
  // native bit-plane records (PL = true: ns_weight::native): the format's bit width and the lanes of a record request
  // (record bytes / 16; the record's planes are contiguous, so a k-step is still ONE request)
  uint32_t pl_bits, pl_lanes;
  // segment pairs (GV_MSEGP): 16-column tiles per half head (head_size / 32) — workgroup u of a matrix owns tiles
  // t0 = head * 2 pair_tiles + j and t0 + pair_tiles (head = u / pair_tiles, j = u % pair_tiles); tb1 / tb2 count workgroups there
  uint32_t pair_tiles;
  // ---- epilogue: mat[].n / .c / .c16, c2, d, ldc, ldd, epilogue and the carried norm's words are requested behind the ring fill and held in
  //      SGPRs through the loop; the RoPE words and the overflow flags are read at the tail, through the kernel-argument pointer ----
  GemvMat mat[3];
  float* c2;
  const float* d;
  int ldc, ldd, epilogue;
  // carried RMS norm, consumer side (ns_norm_link): per row, in_parts partial sums of squares of the un-normalised
  // activations, staged into LDS at ssq_off beside A (nullptr: A is already normalised);
  // row scale = 1 / sqrt(sum * in_inv_size + in_eps)
  const float* in_ssq;
  uint32_t in_parts, in_stride;
  uint32_t ssq_off;
  float in_eps, in_inv_size;
  const float* out_gamma;     // carried norm, producer: fp16 shadow = v * gamma[col] ...
  float* out_ssq;             // ... and out_ssq[row * out_stride + tile] = sum of v^2 over the tile's columns
  uint32_t out_stride;
  uint32_t* out_ovf;          // pinned host word, set when gamma * v does not fit the fp16 shadow (ns_route.h: the route then evaluates the token again without carried norms)
  GemvRope rope;
  F4Lut lut;
  F8Consts f8;
#ifdef NS_TRACE
  unsigned long long* trace;
#endif
};

// MODE of gemv_kernel (described above the kernel)
enum GemvMode { GV_PLAIN = 0, GV_DUAL = 1, GV_MSEG = 2, GV_MSEGP = 3 };
constexpr int kGvModeA32 = 0x100;  // or-ed into the launch mode: fp32 activations (XV = 2)
constexpr int kGvModeI8 = 0x200;   // int8-reference numerics (XV = 3)
constexpr int kGvModeMoe = 0x400;  // expert picked on the device (XV = 4; fp32 activations)
constexpr int kGvModePlanes = 0x800;  // native bit-plane records (PL = true)
constexpr int kGvModeGrp = 0x1000;    // expert chunks along grid.y (XV = 6; fp16 activations in gathered order)

bool gemv_rows1();  // ns_gemv_host.cpp: the "gv_rows1" tuning value — launches of one row take the one-row form

// ---- the launch decision as a value (ns_gemv_plan.cpp) --------------------------------------------------------------------------------------
// Every switch the decision reads.  gemv_knobs() (ns_gemv_host.cpp) fills it from ns_hip_set_tuning's atomics and the environment.
struct GemvKnobs {
  int gemv2 = 1;            // "gemv2" / NS_GEMV2: 0 = every call is refused, the first-generation kernel serves
  bool planes = true;       // "planes" / NS_GEMV_PLANES: bit-plane formats stream their native records
  int forced_nw = 0;        // "gv_nw" / NS_GV_NW: 2 / 4 / 8 / 16 = that many waves per workgroup (diagnostics), else by shape
  bool i8_inkernel = true;  // NS_I8_INKERNEL: int8-reference numerics quantize inside the launch where they can
};
// What a launch needs; nothing is decided after it.  p.out_ovf (when p.out_gamma is set) and p.trace are null: the launcher's.
struct GemvPlan {
  // hipSuccess: launch.  hipErrorNotSupported: outside the kernel's envelope, smallm_kernel serves the call; hipErrorNotReady: the caller runs
  // the quantizer launch (i8_quantize_finish) and comes back; hipErrorInvalidValue: the call itself is wrong
  hipError_t refusal = hipErrorNotSupported;
  int kind = 0, sps = 0;  // the weight's slice (NS_GEMV_SLICES) ...
  uint32_t scale_dt = 0;  // ... and the instantiation inside it
  bool asym = false;
  int mode_x = 0;         // GemvMode | kGvMode* bits
  int grid = 0, grid_y = 1, nw = 0;
  size_t lds = 0;         // dynamic LDS bytes: [A | carried sums or int8 scales at p.ssq_off | nw rings at p.ring_off]
  GemvParams p;
};
// refused: *why says what the call lacks.  Pointers are only compared with null and looked at for their alignment.
GemvPlan gemv_plan(const SmallMArgs& a, const GemvKnobs& knobs, std::string* why);
// ns_gemv_host.cpp: launch_gemv (ns_common.h) in its two halves, for a caller that plans several launches before the first goes out
// (ns_moe.cpp: the device-grouped pass).  plan_gemv: gemv_plan with the live tunables; launch_gemv_planned: a plan that did not refuse
GemvPlan plan_gemv(const SmallMArgs& a);
hipError_t launch_gemv_planned(GemvPlan& pl, hipStream_t st);
// waves per workgroup of a decode launch by shape; forced: GemvKnobs::forced_nw.  decode_waves (ns_common.h) asks with the live value
int decode_waves_rule(int grid, int ks, bool dual, int forced);

// ---- shared by gemv_plan and gemvs_plan (ns_gemvs.h) ------------------------------------------------------------------------------------------
// the matrices of a launch as both kernels address them: one base per matrix, 32-bit offsets of its scales and zero points, its first tile
struct StreamTable {
  GemvMat mat[3];
  const uint8_t* wb[3] = {nullptr, nullptr, nullptr};
  uint32_t soff[3] = {0, 0, 0}, zoff[3] = {0, 0, 0};
  uint32_t tbeg[3] = {0, 0xffffffffu, 0xffffffffu};  // absent matrices begin beyond every tile
  uint32_t tiles = 0;                                // tile units of the launch (gate/up: tile pairs)
};
// pick: the layout of a weight that is streamed (launch_gemv: its native bit-plane clone).  false: a matrix is not one allocation below 2 GiB
template <class Pick>
inline bool stream_table(const SmallMArgs& a, Pick pick, StreamTable* t) {
  for (int i = 0; i < a.nseg; i++) {
    const ns_weight* w = pick(a.seg[i].w);
    if (!w->single_span || w->alloc_bytes >= (size_t(1) << 31)) return false;
    t->wb[i] = reinterpret_cast<const uint8_t*>(w->codes);
    t->soff[i] = uint32_t(reinterpret_cast<const uint8_t*>(w->scales) - t->wb[i]);
    t->zoff[i] = w->zps ? uint32_t(reinterpret_cast<const uint8_t*>(w->zps) - t->wb[i]) : 0u;
    t->tbeg[i] = a.dual ? 0u : t->tiles;
    if (!a.dual || i == 0) t->tiles += uint32_t(w->ntiles);
    t->mat[i] = GemvMat{t->wb[i], t->soff[i], t->zoff[i], t->tbeg[i], w->n, a.seg[i].c, static_cast<_Float16*>(a.seg[i].c16)};
  }
  return true;
}
// bytes of one ring slot: a k-step's code record with its scales and zero points behind it
inline uint32_t record_slot_bytes(const ns_weight* w) {
  const uint32_t sbytes = uint32_t(w->sps) * (w->scale_dt == DT_F32 ? 4u : 2u);
  return 1024u + 16u * sbytes + (w->asym ? 16u * uint32_t(w->sps) : 0u);
}
// the matrices of a fused launch share one format and one record layout, so that one set of strides serves all of them
inline bool same_stream_layout(const ns_weight* w, const ns_weight* w0) {
  return w->kind == w0->kind && w->sps == w0->sps && w->scale_dt == w0->scale_dt && w->asym == w0->asym && w->k == w0->k &&
         w->ksteps == w0->ksteps && w->qstride == w0->qstride && w->sstride == w0->sstride && w->zstride == w0->zstride &&
         w->srows == w0->srows && w->blocksize == w0->blocksize;
}

// One object per slice X(weight kind, scales per record), each with its own device code object.  Per slice:
//   launch_gemv_<KIND>_<SPS>: launches the instantiation for (scale type, sym / asym, mode bits) on a prepared GemvParams;
//     hipErrorNotSupported: no such instantiation (the caller falls back to smallm_kernel); grid_y: the (row, selection) pairs of an
//     expert-indexed launch
//   touch_gemv_<KIND>_<SPS>: makes the runtime load the slice's code object (touch_gemv_module, ns_common.h)
#define NS_GEMV_SLICES(X) X(INT4, 4) X(INT4, 2) X(INT4, 1) X(INT8, 2) X(INT8, 1) X(F4, 4) X(F4, 2) X(F4, 1) X(F8, 2) X(F8, 1)
#define NS_GEMV_DECLARE(KIND, SPS)                                                                                      \
  hipError_t launch_gemv_##KIND##_##SPS(const GemvParams& p, uint32_t scale_dt, bool asym, int mode, int grid, int nw, \
                                        size_t lds, hipStream_t st, int grid_y = 1);                                   \
  void touch_gemv_##KIND##_##SPS();
NS_GEMV_SLICES(NS_GEMV_DECLARE)
#undef NS_GEMV_DECLARE

}  // namespace ns

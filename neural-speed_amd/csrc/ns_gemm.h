// ns_gemm.h — what the prefill GEMM files share (internal).  Kernels by generation: ns_gemm3.hip (gemm3_kernel, the product), ns_gemm2.hip
// (gemm2_kernel, the split-K reduction, the fp16 conversion pass).  Host: ns_gemm_plan.cpp decides what serves a call (gemm_plan: a pure
// function, checked on the CPU by tests/test_gemm_plan.py), ns_gemm.cpp reads the tunables, takes scratch and launches what the plan says.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "../../include/ns_bestla.h"
#include "ns_common.h"
#include "ns_dev.h"

namespace ns {

#ifndef NS_G2_MI
#define NS_G2_MI 4
#endif
#ifndef NS_G2_STAGES
#define NS_G2_STAGES 2
#endif
#ifndef NS_G2_OCC
#define NS_G2_OCC 2
#endif
constexpr int kG2Stages = NS_G2_STAGES;  // LDS stages (2: one barrier per chunk; 1: two barriers, more workgroups per CU)
constexpr int kG2MI = NS_G2_MI;  // 16-row MFMA tiles per wave along M: wave tile = 16*MI x 64, workgroup = 32*MI x 128
constexpr int kG2BM = 32 * kG2MI, kG2Tiles = 8, kG2KC = 64;  // rows x 8 column tiles (128 columns) x 64-deep chunks
constexpr int kG2AStr = kG2KC + 8;                    // halves per A row in LDS (+16 B skews banks)
constexpr int kG2StageBytes = kG2BM * kG2AStr * 2 + kG2Tiles * 2 * 64 * 16;

constexpr int kG3BM = 256, kG3KC = 64, kG3Tiles = 8;
// MFMA shape of gemm3_kernel's main loop (round 4): v_mfma_f32_32x32x16_f16 — twice the multiply-adds per instruction and per operand
// register of v_mfma_f32_16x16x32_f16 (8 vs 5 cycles per CU for 32 K vs 16 K MACs, MI355X_MICROARCH.md: 2382 vs 2075 TFLOPS
// micro-benchmark ceilings).  A lane is then (row or column l & 31, k half l >> 5) of a 32 x 16 operand: the A image and its
// swizzle serve that read as they are (the sixteen lanes of a ds_read_b128 group still cover sixteen distinct 16-byte slots),
// a B operand is word t of record lane (2 e + k half, column & 15) of the column's tile, e = which 16 of the 32-deep slice.
// Measured (profiles/r04t_gemm3_mfma_shape_ab.txt, M = 2048, same box, alternating): 4096^2 888 vs 882 TFLOPS, 11008 x 4096 945 vs 983,
// 4096 x 11008 988 vs 974, 32000 x 4096 984 vs 1015 (32x32x16 vs 16x16x32) — no gain: the loop is not bound by the matrix pipe's issue rate.
// The 16x16x32 loop stays the default; NS_G3_M32=1 builds this one (parity-tested on both: tests/test_gpu_gemm3.py, test_gpu_fuzz.py).
#ifndef NS_G3_M32
#define NS_G3_M32 0
#endif
constexpr bool kG3M32 = NS_G3_M32 != 0;
typedef float floatx16 __attribute__((ext_vector_type(16)));
// rows from which the third-generation kernel is used (tuning: g3_min_m).  Round 3 (scripts/m_sweep.py, profiles/r03_m_sweep.txt):
// with its 128-row tile it beats gemm2_kernel everywhere below the old threshold of 192 — 4096 x 4096: 17.5 vs 24.2 us at 65
// rows, 21.7 vs 34.2 at 128, 25.0 vs 36.4 at 191; 11008 x 4096: 26.0 vs 44.6, 29.0 vs 49.6, 40.5 vs 71.0 — and the streaming
// kernel from 17 rows on wide outputs (11008 x 4096: 22.5 vs 33.0 us at 17 rows, 25.9 vs 44.8 at 64; ns_dispatch.cpp decides)
constexpr int kG3MinM = 2;  // (the caller decides from where on: ns_dispatch.cpp)
constexpr int kG3StageBytes = kG3BM * kG3KC * 2;  // 32 KiB
constexpr int kG3Stages = 2;
constexpr int kG3BStageMax = 8 * 2 * 1024 + 8 * 2 * 16 * 16 + 8 * 2 * 16 * 4;  // B stage upper bound: codes + scale rows + zero points

// gemm3_kernel's dynamic LDS, stated once for the kernel and for the launch: [kG3Stages A stages][B stage: codes | scale rows | zero points];
// the epilogue parks accumulators over the same memory.  sps / sk / asym: the kernel's template arguments (ns_launch.h with_format).
struct Gemm3Lds {
  uint32_t stage;               // bytes of one A stage: [bm rows][64 halves]
  uint32_t codes, scal, zp;     // B stage: [tile][record][64 lanes x 16 B] | [record][tile][16 columns x scale bytes] | [record][tile][16 x sps]
  uint32_t park, park_wide;     // per-wave epilogue: 64 rows x (wave columns + 4) floats per wave (the 64-row tile's stages alone are smaller
                                // than that); cross-wave epilogue (waves 1 x 4): 64 rows of the tile width, 128 columns (64 gate/up pairs) + 4
  constexpr uint32_t bytes(bool wide) const { return std::max(kG3Stages * stage + codes + scal + zp, std::max(park, wide ? park_wide : 0u)); }
};
constexpr Gemm3Lds gemm3_lds(int kind, int sps, int sk, bool asym, int bm, bool tall) {
  const uint32_t rps = kind_is_8bit(kind) ? 2 : 1;  // records per 128-deep superstep
  const uint32_t sbytes = uint32_t(sps) * (sk == SK_F32 ? 4 : 2);
  const bool sq = bm == 256 && !tall;  // waves 2 x 2
  return {uint32_t(bm) * kG3KC * 2, kG3Tiles * rps * 1024u, kG3Tiles * rps * 16u * sbytes, asym ? kG3Tiles * rps * 16u * uint32_t(sps) : 0u,
          4u * 64 * ((sq ? 64 : 32) + 4) * 4, sq ? 0u : 64u * (128 + 4) * 4};
}

struct Gemm2Params {
  const _Float16* a16;  // [m][lda16] fp16, zero padded to a multiple of 64 columns
  int lda16, m, k, n;
  int nchunks;          // ceil(k / 64)
  int ksteps, ntiles;
  const uint4* codes;
  const void* scales;
  const int8_t* zps;
  uint32_t codes_bytes, scales_bytes, zps_bytes;
  uint32_t qstride, sstride, zstride;
  float* c;
  _Float16* c16;  // optional fp16 shadow of C (same leading dimension) for the next GEMM's activations
  int ldc;
  int srows, srow_mul, srow_shift;
  int epilogue;
  const float* d;
  int ldd;
  int nbn, cpx;  // column blocks; column blocks per XCD
  // gemm3_kernel, fused QKV with RoPE(q, k) + kv-cache append as its epilogue (round 5; ns_qkv_rope at prefill size): segment 0 = q (rotated, fp32),
  // 1 = k (rotated -> fp16 cache [+ fp32]), 2 = v (-> fp16 cache [+ fp32]); cos / sin pairs per (row, pair) from the caller's table
  float seg_spre[3], seg_spost[3];  // fused QKV: each matrix's own factors (round 5: real models' q / k / v scales differ in range)
  int rope_on, rope_hs, rope_npast;  // rope_on: 1 = mode 0 (adjacent pairs), 2 = NeoX pairs (e, e + rope_hs / 2)
  const float2* rope_tab;
  _Float16 *rope_kc, *rope_vc;
  long long rope_csl, rope_chead;
  int ksplit;    // > 1: split-K (few output tiles): workgroup z = blockIdx.y takes chunks [z*cps, (z+1)*cps) and writes a
  int cps;       //      raw fp32 partial tile to `part` [ksplit][m][n]; gemm2_reduce_kernel sums them and applies the epilogue
  float* part;
  float spre, spost;  // power-of-two pair (spre * spost == 1): group scales are multiplied by spre before they are rounded
                      // to fp16 and the accumulators by spost on the way out, so that weights with very small or very
                      // large magnitudes stay inside fp16's normal range (1, 1 for ordinary LLM weights)
  F4Lut lut;
  F8Consts f8;  // gemm3_kernel, fp8 codes: the encoding's two conversion constants (cvt_f8x8, ns_dev.h) — E4M3 and E5M2 share one instantiation
  // gemm3_kernel, fused QKV (ip_fusion_qkv.cpp:84-86 at GEMM size): up to three matrices of one K and one format side by
  // side along the column blocks; nseg <= 1: the single matrix above
  int nseg;
  int seg_bn0[3];   // first column block of matrix s
  int seg_n[3];
  const void* seg_codes[3];
  const void* seg_scales[3];
  const int8_t* seg_zps[3];
  uint32_t seg_codes_bytes[3], seg_scales_bytes[3], seg_zps_bytes[3];
  float* seg_c[3];
  _Float16* seg_c16[3];
  int bm3;   // gemm3_kernel: rows of the workgroup tile (256 / 128)
  int tall3; // gemm3_kernel, bm3 = 256: waves 1 x 4 of 256 x 32 instead of 2 x 2 of 128 x 64
  int diag;  // NS_G3_DIAG (diagnostics): 1 = skip the output stores, 2 = skip the main loop, 3 = DMA and barriers only, 4 = no DMA
  // gemm3_kernel, fused gate/up (round 5; ip_fusion_ffn.cpp:364-406 at GEMM size): codes / scales / zps = W1 (gate), *2 = W3 (up), same
  // shape and format; a column block is 4 tile PAIRS = 64 output columns, wave w multiplies gate tile and up tile 4 bn + w, the MFMA
  // layout puts gate and up of one (row, column) into the same lane: out = act(gate) * up in registers.  c / c16 / c2 are each optional.
  int dual;
  const void* codes2;
  const void* scales2;
  const int8_t* zps2;
  float* c2;  // optional act(gate) (the reference's tmp1)
  int wide;   // 1: the cross-wave epilogue (waves 1 x 4 only): whole tile rows leave as 256 / 512-byte runs, the fp16 shadow as 16-byte stores
};

// ---- the launch decision as a value (ns_gemm_plan.cpp) --------------------------------------------------------------------------------------
// Every switch the decision reads.  gemm_knobs() (ns_gemm.cpp) fills it from ns_hip_set_tuning's atomics and the environment.
struct GemmKnobs {
  bool v1 = false;         // NS_GEMM_V1 set: every call is refused, the first-generation kernel serves (diagnostics)
  int gemm3 = 1;           // NS_GEMM3: 1 = gemm3_kernel; 0 = gemm2_kernel serves single matrices; any value but 1 refuses the fp8 and the fused forms
  int g3_min_m = kG3MinM;  // "g3_min_m": rows from which gemm3_kernel is used
  int g3_bm = 0;           // "g3_bm" / NS_G3_BM: 64 / 128 / 256 = that row tile, 257 = 256 rows with tall wave tiles (int4 only), else automatic
  int g3_wide = 0;         // "g3_wide" / NS_G3_WIDE: 1 = the cross-wave epilogue wherever the tile has one
  bool g3_f8 = true;       // "g3_f8" / NS_G3_F8: fp8 weights take gemm3_kernel
  bool no_splitk = false;  // NS_NO_SPLITK set (diagnostics)
  int diag = 0;            // NS_G3_DIAG (Gemm2Params::diag)
  bool no_partials = false;  // not a tunable: launch_gemm2's second plan when the split-K scratch cannot be had — one split, still correct
};
enum GemmKernel { GK_REFUSED = 0, GK_GEMM2, GK_GEMM3 };
// What a launch needs; nothing is decided after it.  p.a16 (when `convert`) and p.part are null: the launcher's scratch.
struct GemmPlan {
  GemmKernel kernel = GK_REFUSED;
  hipError_t refusal = hipSuccess;  // GK_REFUSED: hipErrorNotSupported (another kernel serves the call) or hipErrorInvalidValue (no output)
  int kind = 0, sps = 0;             // the format the kernel is instantiated for (with_format, ns_launch.h)
  uint32_t scale_dt = 0;
  bool asym = false;
  Gemm2Params p;                     // tile form of gemm3_kernel: p.bm3, p.tall3, p.dual; K split: p.ksplit, p.cps
  dim3 grid;
  size_t lds = 0;                    // dynamic LDS bytes
  bool convert = false;              // an fp32 -> fp16 pass over A comes first: cvt_bytes of scratch, rows of kpad halves
  size_t cvt_bytes = 0;
  int kpad = 0;
  size_t part_bytes = 0;             // of p.part when p.ksplit > 1
};
// may this weight's prompt-size GEMMs run on the tiled kernel?  (gemm3_takes(w), ns_common.h, asks with the live knobs)
bool gemm3_takes(const ns_weight* w, const GemmKnobs& knobs);
// GK_REFUSED: *why says what the call lacks.  Pointers are only compared with null and looked at for their alignment.
GemmPlan gemm_plan(const SmallMArgs& a, const GemmKnobs& knobs, std::string* why);

// ---- launches of a plan ----------------------------------------------------------------------------------------------------------------------
hipError_t launch_gemm3_plan(const GemmPlan& pl, hipStream_t st);  // ns_gemm3.hip: GK_GEMM3
hipError_t launch_gemm2_plan(const GemmPlan& pl, hipStream_t st);  // ns_gemm2.hip: GK_GEMM2
// ns_gemm2.hip: the reduction pass of a launch that split K (e: the result of the main launch)
hipError_t launch_gemm_reduce(hipError_t e, const Gemm2Params& p, hipStream_t st);

}  // namespace ns

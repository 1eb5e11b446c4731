// ns_gemv.hip — gemv_kernel: the decode (M <= 16 rows) weight-streaming kernel of libns_hip.so, second generation.
//
// Same arithmetic as smallm_kernel (ns_kernels.hip): per 1 KiB weight record NJ x v_mfma_f32_16x16x32_f16 on the raw
// codes, the group scale applied to the fp32 MFMA result — exactly w = (code - zp) * scale with fp32 accumulation
// (reference: bestla/bestla/kernel_ref.h:2489-2531 gemv_4bit_fp32_fp32, :1027-1127 decompress_kblock_s4_fp,
// :1456-1478 decompress_kblock_f4_fp), fp16 activations; one workgroup = one 16-column tile over the whole K, waves
// split the k-steps, deterministic cross-wave reduction.  What changed is everything AROUND the arithmetic, because a
// decode launch on MI355X is latency-, not bandwidth-bound:
//
//   * lean prologue.  Every launch starts with cold instruction and scalar caches, so the time to the first weight
//     request is the number of code lines and of dependent kernel-argument fetches in front of it.  smallm_kernel had
//     1.8 KB of code and two argument round trips there (first request 1.3-1.8 us after entry); here ONE batch of scalar
//     loads fetches the 30 words the prologue needs and the ring is filled ~0.6 KB into the code.  The epilogue's arguments
//     are a second batch BEHIND the ring fill, so they do not delay the first weight request either, and stay in SGPRs through
//     the loop (7-8 registers; the kernel has room).  Up to round 13 they were read at the tail instead: on argument lines no
//     earlier instruction had touched, a scalar-cache miss between the last record and the reduction barrier of every launch
//     (docs/kernels/gemv.md, "launch tail").
//   * weight records go HBM -> LDS directly (buffer_load ... lds into the wave's PRIVATE ring: codes, scales and zero
//     points; no VGPRs, no cross-wave synchronisation).  The ring depth is therefore set by LDS, not by the register
//     file: up to 8 records per wave, up to ~140 KiB per CU in flight from the first microsecond of a launch.
//   * waits by hand.  No request of the stream returns to a register, so hipcc inserts no vmcnt waits of its own (it
//     does not order an LDS read behind an LDS-DMA write at all); before a record is consumed the kernel waits for
//     exactly the requests older than the ones that may stay in flight (requests retire in order): s_waitcnt
//     vmcnt(OPS * min(PF - 1, records still to come)).  Nothing is ever requested that is not consumed (out-of-range
//     "dead" requests were measured to cost a full pass through the address pipeline each, profiles/r02d-r02e).
//
// Tried here and dropped (profiles/r02a-r02b): cutting the 688 gate/up tiles into equal K-ranges over the CUs
// ("stream-K") with partial sums handed between workgroups through write-through stores + flags.  The hand-off costs
// 3-5 us under load (the poll queues behind the consumer CU's own weight requests) — more than the 2 us of imbalance it
// removes in an 11 us launch; narrow tensor-parallel shards lost 3 us per launch to it.
//
// This file is compiled once per SLICE — weight kind x scales per record (NS_GEMV_KIND, NS_GEMV_SPS; csrc/Makefile: GEMV) —
// into objects built side by side: the kernel, the ladder that picks an instantiation from a launch's run-time format and mode,
// and the ONE exported launcher of the slice, named after the two macros.  ns_gemv.h has the parameter structs and the
// launchers' declarations, ns_gemv_host.cpp the host logic in front of them (launch_gemv, decode_waves, tuning state).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <type_traits>
#include <utility>

#include "../../include/ns_bestla.h"
#include "ns_common.h"
#include "ns_dev.h"
#include "ns_gemv.h"
#include "ns_launch.h"

// the slice this object holds (Makefile: GEMV_SLICES); a bare `hipcc -c ns_gemv.hip` builds the Q4_0 one
#ifndef NS_GEMV_KIND
#define NS_GEMV_KIND INT4
#define NS_GEMV_SPS 4
#endif

namespace ns {

// the kernel-argument segment as an opaque pointer: loads through it cannot be hoisted above the point it is made
using KArgs = const __attribute__((address_space(4))) GemvParams*;
__device__ __forceinline__ KArgs late_args() {
  uint64_t v = reinterpret_cast<uint64_t>(__builtin_amdgcn_kernarg_segment_ptr());
  asm volatile("" : "+s"(v));
  return reinterpret_cast<KArgs>(v);
}

#ifdef NS_TRACE
#define NS_GSTAMP(i)                                                                                     \
  do {                                                                                                   \
    __builtin_amdgcn_sched_barrier(0);                                                                   \
    if ((threadIdx.x & 63) == 0 && blockIdx.x < 4096)                                                     \
      p.trace[(size_t(blockIdx.x) * 16 + (threadIdx.x >> 6)) * 8 + (i)] = wall_clock64();                 \
    __builtin_amdgcn_sched_barrier(0);                                                                   \
  } while (0)
#else
#define NS_GSTAMP(i)
#endif

template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// one NeoX pair: y0 = x0 c - x1 s, y1 = x0 s + x1 c with separately rounded products (no contraction into FMAs: the separate
// operator's translation unit is built with -ffp-contract=off, this one is not)
__device__ __forceinline__ void neox_rotate(float x0, float x1, float c, float s, float* y0, float* y1) {
#pragma clang fp contract(off)
  const float a = x0 * c, b = x1 * s, d = x0 * s, e = x1 * c;
  *y0 = a - b;
  *y1 = d + e;
}

// MODE: one matrix / two matrices of one shape streamed in lockstep (gate/up, SiLU-mul epilogue) / several matrices
// side by side along N (QKV) / the same with "segment pairs" (GV_MSEGP, XV = 1 only): the NeoX form of the RoPE epilogue.  A
// workgroup streams the two tiles of a rotation pair (columns e and e + head_size / 2 of a head) with GV_DUAL's machinery — ring
// slots alternating between the two streams, two accumulator sets — through the segment's ONE descriptor; lane (nn, g) ends
// up with both elements of its pairs.  The grid is half the tile count; the wave count is the one the GV_MSEG launch of the
// same weights and rows gets (decode_waves on the full tile count), so every column's fp32 sum is built in the same order as in
// the two-launch form (fused QKV, then ns_hip_rope_qkv_append) and the results are the same bits.  Exception: the doubled
// rings may not fit LDS beside the staged rows (many rows of a large K); the wave count is then halved further and the result
// differs in fp32 summation order only.  Activations arrive as fp16 (the producer's shadow); fp32-only callers stay on
// smallm_kernel, which converts while staging.
// EXT: the launch carries an RMS norm (ns_norm_link) and / or the RoPE + kv-append epilogue (ns_qkv_rope).  A separate
// instantiation, because even untaken these paths cost every launch 0.1-0.3 us (later argument fetch, longer cold
// epilogue code: 1057 vs 1036 us on the 7B chain, profiles/r02o_ext_ab.txt).
// XV: 0 plain; 1 = EXT; 2 = A32: the activations arrive as fp32 only (a caller without a producer shadow: the reference's
// device graph hands bestla_device_f32f32_forward fp32 tensors).  The wave's share of A is loaded into registers in
// front of the ring requests, converted (round to nearest even, as the shadow's producers do) and written to LDS once
// only ring requests are left in flight — the weights are requested exactly as early as with a shadow.
// XV = 4 (MOE): A32 + the weight picked on the DEVICE: ne_compute_forward_mul_mat_id_q_f32_bestla (ne_layers.c:7783-7916) reads
// ids[token][id] on the host and calls bestla_f32f32_forward per (token, expert); here the id stays where the router's top-k left
// it — one scalar load of the id, one of the expert's base pointer, in front of the first weight request (two dependent round
// trips, ~1 us, instead of a host synchronisation) — and the token's row streams the expert at this kernel's rate.  These launches alone
// read blockIdx.y: a (token row, selection) pair with its own id, activation row, output row and factor (GemvParams::moe_*), each
// workgroup still staging ONE row; with GV_DUAL the gate and up matrices of the pair's expert come from two tables (ns_hip_moe_ffn_silu).
// XV = 6 (GRP): expert CHUNKS — the device-grouped pass of ns_hip_moe_ffn_silu / _gelu (ns_moe.cpp: ffn_device_grouped).  blockIdx.y is a chunk
// slot of the list moe_pair_sort_kernel (ns_moe_group.hip) left on the device: {expert, first gathered position, rows}; a slot beyond the
// list's count exits at once (the host sizes grid.y for the worst id table).  The workgroup stages the chunk's `rows` (<= p.m, what LDS is
// sized for) contiguous fp16 rows through the fp16 staging path below, streams the expert's matrix (GV_DUAL: the gate and up matrices) out of
// the tables exactly like XV = 4 and writes output rows first + r: one stream of an expert serves every pair routed to it in the chunk.
// Either output, fp32 or fp16, may be absent.
// XV = 3 (I8S): the REFERENCE'S int8-compute numerics (its default for Q4_0: gemv_4bit_u8s8_fp32, kernel_ref.h:2371-2429) on the
// same streaming skeleton: A arrives as the u8 codes / scales / zero points of quantize_fp_u8_colblock (aquant_u8_kernel,
// bit-exact), a lane (column nn, k-slot g) takes exact integer dots of its eight codes per 32-deep slice with v_dot4 on the
// stored codes,  sum (a - za)(q - zb) = sum a u - (zb + bias) sum a - za sum u + 8 za (zb + bias)  (u = q + bias), and adds
// float(sum) * (scale_a * scale_b) per slice; up to four rows.  Reduction, epilogues, fused QKV / gate-up modes are shared.
// XV = 5 (I8Q, round 5): I8S with the activation quantizer INSIDE the launch — the rows arrive as fp32 (staged through registers like
// XV = 2), every workgroup quantizes them itself (quantize_fp_u8_colblock's arithmetic operation by operation: the lanes of a k-block
// combine max / min by xor-shuffles, order-independent like in aquant_u8_coop_kernel, so codes / scales / zero points are the same bits)
// and leaves codes, scales and zero points in LDS where XV = 3 finds the ones it fetched.  Saves the aquant launch in front of every
// GEMV of an int8-reference decode step (129 per Llama-2-7B token, ~3 us each); k-blocks of 32 .. 256 that divide K.
// PL (round 4): the codes arrive as the NATIVE bit planes of a 1-3 / 5-7 bit format (ns_weight::native, repack_planes_kernel) —
// 256 .. 896 bytes per k-step instead of the 1 KiB nibble / byte container — and each lane rebuilds its container words from its
// plane words with shifts and masks (stored codes, bias 2^(bits-1) folded into the conversion constants: the same fp16 values,
// hence the same bits out, as from the widened records).  KIND says which container: WK_INT4 for 1-3 bits, WK_INT8 for 5-7.
// R1 (round 7): the launch has ONE activation row (m == 1, what a batch-1 decode chain runs) and the arithmetic beside the stream is
// sized for it: element 0 of each MFMA result is the only live output (every A row of the fragment is row 0), so the post-scale is
// one FMA per slice instead of four, the accumulators one register per stream, the reduction one float per lane; the int8-reference
// path has no row loop, no per-slice guard on full k-steps and 24-bit integer algebra.  Which bytes are requested, and when, is the
// same as without it, and so are the bits out: the live row goes through the same operations in the same order.
// Instantiated for integer weights, XV 0 / 1 / 3 / 5, modes PLAIN / DUAL / MSEG (gemv_has_rows1); ns_hip_set_tuning("gv_rows1", 0)
// or NS_GV_ROWS1=0 keep every launch on the general form.
template <int KIND, int SPS, int SK, bool ASYM, int MODE, int XV, bool PL = false, bool R1 = false>
__global__ __launch_bounds__(1024) void gemv_kernel(const GemvParams p) {
  constexpr bool EXT = XV == 1, MOE = XV == 4, I8Q = XV == 5, GRP = XV == 6, A32 = XV == 2 || MOE || I8Q, I8S = XV == 3 || I8Q;
  static_assert(!GRP || (!PL && !R1 && (MODE == GV_PLAIN || MODE == GV_DUAL)), "expert chunks: one matrix or gate / up, widened records");
  static_assert(!R1 || ((KIND == WK_INT4 || KIND == WK_INT8) && !PL && (XV == 0 || XV == 1 || XV == 3 || XV == 5) && MODE != GV_MSEGP),
                "one-row form: integer weights, fp16 / carried-norm / int8-reference launches");
  constexpr int RR = R1 ? 1 : 4;  // result rows a lane finishes in the epilogue
  static_assert(!PL || ((KIND == WK_INT4 || KIND == WK_INT8) && !I8S && !MOE), "native planes: integer formats, fp16 numerics");
  static_assert(!I8S || KIND == WK_INT4 || KIND == WK_INT8, "integer weights only");
  constexpr uint32_t AEL = I8S ? 1u : 2u;  // bytes per staged activation element
  constexpr bool DUAL = MODE == GV_DUAL, MSEG = MODE == GV_MSEG, MSEGP = MODE == GV_MSEGP;
  constexpr bool MSEGX = MSEG || MSEGP;  // the tile's matrix is selected among up to three
  static_assert(!MSEGP || (EXT && !PL), "segment pairs exist for the RoPE epilogue only");
  constexpr int NJ = kind_is_8bit(KIND) ? 2 : 4;
  constexpr int KSTEP = NJ * 32;
  constexpr int NQ = (DUAL || MSEGP) ? 2 : 1;
  constexpr int PF = kGvPF;
  static_assert(PF % NQ == 0, "ring slots alternate between the two matrices");
  constexpr int SBYTES = SPS * (SK == SK_F32 ? 4 : 2);
  using Corr = CorrRaw<SPS, SK, ASYM>;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  _Float16* a_lds = reinterpret_cast<_Float16*>(smem);
  NS_GSTAMP(0);

  // every kernel argument the prologue needs is fetched by ONE batch of scalar loads: without this hipcc sinks each
  // load to its first use and the first weight request waits for several dependent argument round trips
  {
    asm volatile("" ::"s"(p.wbase0), "s"(p.a), "s"(p.ks), "s"(p.qstride), "s"(p.nw_log2), "s"(p.s_off0), "s"(p.sstride),
                 "s"(p.srows), "s"(p.srow_mul), "s"(p.srow_shift), "s"(p.m), "s"(p.k), "s"(p.lda), "s"(p.row_stride),
                 "s"(p.ring_off), "s"(p.ring_stride));
    if constexpr (DUAL) asm volatile("" ::"s"(p.wbase1), "s"(p.s_off1));
    if constexpr (MSEGX)
      asm volatile("" ::"s"(p.tb1), "s"(p.tb2), "s"(p.mat[0].wbase), "s"(p.mat[1].wbase), "s"(p.mat[2].wbase), "s"(p.mat[0].s_off),
                   "s"(p.mat[1].s_off), "s"(p.mat[2].s_off));
    if constexpr (MSEGP) asm volatile("" ::"s"(p.pair_tiles));
    if constexpr (ASYM) asm volatile("" ::"s"(p.z_off0), "s"(p.z_off1), "s"(p.zstride));
    if constexpr (PL) asm volatile("" ::"s"(p.pl_bits), "s"(p.pl_lanes));
  }
  const int tid = threadIdx.x;
  const uint32_t w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l = tid & 63;
  const int nn = l & 15, g = l >> 4;
  const uint32_t NW = 1u << p.nw_log2;
  const uint32_t ks = p.ks;
  const uint32_t T = blockIdx.x;  // global tile (across the matrices of a fused QKV launch; GV_MSEGP: global tile pair)

  typedef __attribute__((address_space(3))) unsigned char* LdsPtr;
  // ---- descriptors: one per matrix over its whole allocation (codes, scales and zero points share the base) ----
  Rsrc rw[NQ];
  uint32_t so[NQ], zo[NQ];
  int sg = 0;       // matrix of the fused launch the tile belongs to (QKV)
  uint32_t tl = T;  // tile inside that matrix
  uint32_t moe_y = 0, moe_row = 0;  // MOE: this workgroup's (row, selection) pair and its token row
  float moe_wsc = 1.f;              // MOE: the pair's factor (routing weight)
  uint32_t grp_first = 0;           // GRP: this workgroup's chunk — its first gathered position ...
  int grp_rows = 0;                 // ... and its rows (wave-uniform: scalar loads)
  if constexpr (GRP) {
    const int32_t* ch = p.moe_id;  // the chunk list moe_pair_sort_kernel wrote: count, then {expert, first position, rows} per chunk
    const uint32_t slot = blockIdx.y;
    if (slot >= uint32_t(ch[0])) return;  // the grid is sized for the worst id table (moe_chunk_slots)
    const int e = ch[1 + 3 * slot];
    grp_first = uint32_t(ch[2 + 3 * slot]);
    grp_rows = ch[3 + 3 * slot];
    // (what the sort never writes: a chunk outside the table, the staged rows or the gathered positions is not touched)
    if (e < 0 || e >= p.moe_n || grp_rows < 1 || grp_rows > p.m || grp_first + uint32_t(grp_rows) > p.moe_nsel) return;
    rw[0] = make_rsrc(p.moe_table[e].codes, 0x80000000u);
    so[0] = p.s_off0;
    zo[0] = p.z_off0;
    if constexpr (DUAL) {
      rw[1] = make_rsrc(p.moe_table1[e].codes, 0x80000000u);
      so[1] = p.s_off1;
      zo[1] = p.z_off1;
    }
  } else if constexpr (MOE) {
    moe_y = blockIdx.y;
    moe_row = (moe_y * p.moe_sel_mul) >> 16;
    const uint32_t sel = moe_y - moe_row * p.moe_nsel;
    const int e = p.moe_id[(long long)moe_row * p.moe_ids_stride + sel];  // wave-uniform: scalar loads
    if (p.moe_w) moe_wsc = p.moe_w[(long long)moe_row * p.moe_w_stride + sel];
    if (e < 0 || e >= p.moe_n) {  // an out-of-range id: a zero PRODUCT for the row (the reference would assert), through the epilogue of section 6
      const KArgs cz = late_args();
      const int colz = int(T) * 16 + nn;
      if (w == 0 && g == 0 && colz < cz->mat[0].n) {
        float v = 0.f;
        if constexpr (!DUAL) {  // (fused gate / up: silu(0) * up = 0)
          const float dv = cz->d ? cz->d[size_t(moe_y) * cz->moe_d_stride + colz] : 0.f;
          v = epi_apply(v, dv, cz->epilogue);
        }
        float* cr = cz->mat[0].c + size_t(moe_y) * cz->moe_c_stride;
        cr[colz] = v;
        if (cz->mat[0].c16) cz->mat[0].c16[colz] = (_Float16)v;
      }
      return;
    }
    rw[0] = make_rsrc(p.moe_table[e].codes, 0x80000000u);
    so[0] = p.s_off0;
    zo[0] = p.z_off0;
    if constexpr (DUAL) {  // gate and up of the SAME expert, out of the two groups' tables
      rw[1] = make_rsrc(p.moe_table1[e].codes, 0x80000000u);
      so[1] = p.s_off1;
      zo[1] = p.z_off1;
    }
  } else if constexpr (DUAL) {
    rw[0] = make_rsrc(p.wbase0, 0x80000000u);
    rw[1] = make_rsrc(p.wbase1, 0x80000000u);
    so[0] = p.s_off0, so[1] = p.s_off1;
    zo[0] = p.z_off0, zo[1] = p.z_off1;
  } else if constexpr (MSEGX) {
    // all three matrices' bases and offsets come with the one batch of argument loads and are SELECTED (a lookup by
    // index in the argument segment would be a second, dependent round trip in front of the first weight request)
    sg = int(T >= p.tb1) + int(T >= p.tb2);
    const uint8_t* wb = sg == 0 ? p.mat[0].wbase : (sg == 1 ? p.mat[1].wbase : p.mat[2].wbase);
    rw[0] = make_rsrc(wb, 0x80000000u);
    so[0] = sg == 0 ? p.mat[0].s_off : (sg == 1 ? p.mat[1].s_off : p.mat[2].s_off);
    if constexpr (ASYM) zo[0] = sg == 0 ? p.mat[0].z_off : (sg == 1 ? p.mat[1].z_off : p.mat[2].z_off);
    else zo[0] = 0;
    tl = T - (sg == 0 ? 0u : (sg == 1 ? p.tb1 : p.tb2));
    if constexpr (MSEGP) {  // pair u of the matrix -> its first tile (the second lies pair_tiles further on); both streams share the descriptor
      tl += (tl / p.pair_tiles) * p.pair_tiles;
      rw[1] = rw[0], so[1] = so[0], zo[1] = zo[0];
    }
  } else {
    rw[0] = make_rsrc(p.wbase0, 0x80000000u);
    so[0] = p.s_off0;
    zo[0] = p.z_off0;
  }
  uint32_t tile_q[NQ], tile_c[NQ];
#pragma unroll
  for (int q = 0; q < NQ; q++) {
    const uint32_t tlq = (MSEGP && q) ? tl + p.pair_tiles : tl;
    tile_q[q] = tlq * ks * p.qstride;
    tile_c[q] = tlq * p.srows;
  }
  const uint32_t voff_q = l * 16, voff_s = nn * SBYTES, voff_z = nn * SPS;  // the only per-lane address parts
  const I4Consts i4c = {0x000f000fu, 0x00f000f0u, 0x64006400u};

  // this wave's private ring: up to PF slots, a slot = image of one record {1024 B codes | 16 x SBYTES scales | 16 x SPS
  // zero points}; slot i holds the record of item i (mod PF)
  constexpr uint32_t SLOT = 1024u + 16u * SBYTES + (ASYM ? 16u * SPS : 0u);
  constexpr int OPS = ASYM ? 3 : 2;  // requests per record
  static_assert(OPS * PF + kGvMaxRows * 2 <= 63, "vmcnt is a 6-bit counter (ring + the carried norm's pieces)");
  const LdsPtr ring = (LdsPtr)(smem) + p.ring_off + w * p.ring_stride;
  const uint32_t ring_lane = uint32_t(reinterpret_cast<uintptr_t>(ring)) + uint32_t(l) * 16u;  // LDS byte address
  const uint32_t ring_corr = uint32_t(reinterpret_cast<uintptr_t>(ring)) + 1024u + uint32_t(nn) * SBYTES;

  // item = (k-step s, matrix q = slot % NQ): codes (64 lanes x 16 B), then its scale row (SBYTES lanes x 16 B), then its
  // zero-point row (SPS lanes x 16 B), all non-temporal HBM -> LDS
  auto issue = [&](auto slot_c, uint32_t s) {
    constexpr int slot = decltype(slot_c)::value;
    constexpr int q = slot % NQ;
#if defined(__HIP_DEVICE_COMPILE__)  // (the host pass of hipcc cannot type-check this builtin and would drop the kernel stub)
    const uint32_t crow = tile_c[q] + ((s * p.srow_mul) >> p.srow_shift);
    const LdsPtr dst = ring + slot * SLOT;
    if (!PL || uint32_t(l) < p.pl_lanes)  // (a native record is shorter than 64 x 16 bytes)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rw[q], reinterpret_cast<__attribute__((address_space(3))) void*>(dst), 16, voff_q,
                                               tile_q[q] + s * p.qstride, 0, 2);
    if (l < SBYTES)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rw[q], reinterpret_cast<__attribute__((address_space(3))) void*>(dst + 1024), 16,
                                               voff_q, so[q] + crow * p.sstride, 0, 2);
    if constexpr (ASYM) {
      if (l < SPS)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rw[q], reinterpret_cast<__attribute__((address_space(3))) void*>(dst + 1024 + 16 * SBYTES),
                                                 16, voff_q, zo[q] + crow * p.zstride, 0, 2);
    }
#endif
  };
  // wait until at most `younger` RECORDS requested after the one about to be consumed are still in flight
  auto wait_records = [&](uint32_t younger) {
    if (younger == uint32_t(PF - 1)) {  // steady state first
      wait_vmcnt<OPS * (PF - 1)>();
      return;
    }
    [&]<int... K>(std::integer_sequence<int, K...>) {
      (void)((younger == uint32_t(K) ? (wait_vmcnt<OPS * K>(), true) : false) || ...);
    }(std::make_integer_sequence<int, PF + 1>{});
  };

  // ---- 1. activations requested first (small, and they must be in LDS before the first MFMA): fp16 rows go
  //      HBM/L2 -> LDS directly in 1 KiB pieces, piece c of row r by wave (r * pieces + c) % NW; LDS row r holds
  //      ks * KSTEP halves (columns >= K read as zero through the descriptor: k-step padding) ----
  const int rows = R1 ? 1 : GRP ? grp_rows : min(p.m, kGvMaxRows);  // (GRP: p.m is what the host sized LDS for)
  floatx4 areg[A32 ? kGvA32Regs : 1];
  if constexpr (A32) {
    // fp32 rows: 1 KiB pieces (256 columns) by wave (r * pieces + c) % NW again, at most kGvA32Regs per wave (host)
    // the descriptor make_rsrc() builds, as four words for the asm operand: base, stride 0, bytes, flags
    uint64_t abase = reinterpret_cast<uint64_t>(p.a);
    if constexpr (MOE) abase += uint64_t(moe_row) * p.moe_a_stride * 4u;  // the pair's token row (the workgroup stages this one row)
    const uint4v ra_words = {uint32_t(abase), uint32_t(abase >> 32) & 0xffffu,
                             uint32_t(rows - 1) * uint32_t(p.lda) * 4u + uint32_t(p.k) * 4u, 0x00020000u};
    const uint32_t row_bytes = ks * uint32_t(KSTEP) * 4u;
    const uint32_t pieces = (row_bytes + 1023u) >> 10;
    const uint32_t total = uint32_t(rows) * pieces;
    uint32_t r = 0, c = w;  // piece u = w + i * NW is (row r, column piece c): stepped, not divided
#pragma unroll
    for (int i = 0; i < kGvA32Regs; i++) {
      const uint32_t u = w + (uint32_t(i) << p.nw_log2);
      areg[i] = floatx4{0.f, 0.f, 0.f, 0.f};
      if (u < total) {
        if constexpr (!R1)
          while (c >= pieces) c -= pieces, r++;
#if defined(__HIP_DEVICE_COMPILE__)
        // columns >= K of the last k-step come back as zero through the descriptor
        // by hand: hipcc does not count LDS-DMA requests, so for a load it knows of it waits for everything in flight
        // (vmcnt(0): the whole ring) before the first use; wait_records() below is this load's wait
        asm volatile("buffer_load_dwordx4 %0, %1, %2, %3 offen"
                     : "=v"(areg[i])
                     : "v"(voff_q), "s"(ra_words), "s"(r * uint32_t(p.lda) * 4u + (c << 10))
                     : "memory");
#endif
        c += NW;
      }
    }
  } else {
    const void* a_rows = p.a;
    if constexpr (GRP) a_rows = static_cast<const _Float16*>(p.a) + size_t(grp_first) * uint32_t(p.lda);  // the chunk's rows are contiguous
    const Rsrc ra = make_rsrc(a_rows, uint32_t(rows - 1) * uint32_t(p.lda) * AEL + uint32_t(p.k) * AEL);
    const uint32_t row_bytes = ks * uint32_t(KSTEP) * AEL;
    const uint32_t pieces = (row_bytes + 1023u) >> 10;
    const uint32_t total = uint32_t(rows) * pieces;
    const LdsPtr al = (LdsPtr)(smem);
    for (uint32_t u = w; u < total; u += NW) {
      uint32_t r = 0, c = u;
      if (rows > 1) {
        r = u / pieces;
        c = u - r * pieces;
      }
      const uint32_t left = row_bytes - (c << 10);  // bytes of the row from this piece on
#if defined(__HIP_DEVICE_COMPILE__)
      if (uint32_t(l) * 16u < left)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, reinterpret_cast<__attribute__((address_space(3))) void*>(al + r * p.row_stride * 2u + (c << 10)),
                                                 16, voff_q, r * uint32_t(p.lda) * AEL + (c << 10), 0, 0);
#endif
    }
    if constexpr (I8S) {  // the rows' activation scales + zero points: one span, 1 KiB pieces, read zero past its end
      const Rsrc rc = make_rsrc(p.i8_corr, p.i8_span);
      for (uint32_t u = w; u < ((p.i8_span + 1023u) >> 10); u += NW) {
#if defined(__HIP_DEVICE_COMPILE__)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rc, reinterpret_cast<__attribute__((address_space(3))) void*>(al + p.ssq_off + (u << 10)), 16,
                                                 voff_q, u << 10, 0, 0);
#endif
      }
    }
  }
  __builtin_amdgcn_sched_barrier(0);

  // ---- 2. fill the ring: k-steps w, w + NW, ... of the tile belong to wave w ----
  const uint32_t first = w;
  const uint32_t nst = first < ks ? (ks - first + NW - 1) >> p.nw_log2 : 0u;
  NS_FOR_SLOTS({ if (uint32_t(i / NQ) < nst) issue(ic, first + ((i / NQ) << p.nw_log2)); })
  __builtin_amdgcn_sched_barrier(0);
  NS_GSTAMP(1);

  // ---- 2b. carried norm (consumer side): the rows' partial sums of squares, in_parts floats per row, go to LDS as
  //      1 KiB pieces too — requested AFTER the ring so that nothing is added in front of the first weight request
  //      (its arguments are fetched here, late); only the epilogue reads them.  The requesting wave waits a little
  //      more strictly for its first records (a piece counts as one more request in flight), that is all.  With up
  //      to 16 rows x pieces the 6-bit request counter cannot overflow: PF x OPS + 16 <= 63 is asserted below.
  //      The epilogue's arguments are requested here as well, one more batch of scalar loads behind the ring fill: they touch
  //      argument lines the prologue has not, and fetched at the tail (as they were up to round 13) that scalar-cache miss sat
  //      between the last record and the reduction barrier of every launch, with the whole workgroup and the next kernel
  //      behind it.  They are pinned in SGPRs below, after the activation wait — a wait that exists anyway — and consumed
  //      after the loop (7-8 more SGPRs through it, 14-16 with the carried norm's words: the one-row fp16 forms of a decode chain
  //      have 57-64, below the 80 that eight 4-wave workgroups per CU allow; docs/kernels/gemv.md lists the forms above it).
  const KArgs mid = late_args();
  const auto* mp = &mid->mat[MSEGX ? sg : 0];  // indexed scalar loads
  int ncols = mp->n;
  float* cbase = mp->c;
  _Float16* c16 = mp->c16;
  int ldc = mid->ldc, epi = mid->epilogue;
  int ldd = 0;
  const float* dptr = nullptr;
  float* c2 = nullptr;
  if constexpr (DUAL) {
    c2 = mid->c2;
  } else {
    dptr = mid->d;
    ldd = mid->ldd;
  }
  uint32_t moe_cs = 0, moe_ds = 0;
  if constexpr (MOE) moe_cs = mid->moe_c_stride, moe_ds = mid->moe_d_stride;
  const float* in_ssq = nullptr;
  uint32_t in_parts = 0, ssq_off = 0;
  float in_eps = 0.f, in_inv = 0.f;
  const float* ogamma = nullptr;
  float* ossq = nullptr;
  uint32_t ostride = 0;
  int rope_on_arg = 0;
  if constexpr (EXT) {
    in_ssq = mid->in_ssq;
    in_parts = mid->in_parts;
    ssq_off = mid->ssq_off;
    in_eps = mid->in_eps, in_inv = mid->in_inv_size;
    ogamma = mid->out_gamma;
    ossq = mid->out_ssq;
    ostride = mid->out_stride;
    if constexpr (MSEG) rope_on_arg = mid->rope.on;
  }
  if (EXT && in_ssq && w == 0) {  // wave 0 finishes the tile: it fetches them itself and needs no barrier to read them
    const uint32_t in_stride = late_args()->in_stride;
    const uint32_t spieces = (in_parts * 4u + 1023u) >> 10;
    const Rsrc rs = make_rsrc(in_ssq, (uint32_t(rows - 1) * in_stride + in_parts) * 4u);
    const LdsPtr al = (LdsPtr)(smem);
    for (uint32_t u = 0; u < uint32_t(rows) * spieces; u++) {
      const uint32_t r = u / spieces, c = u - r * spieces;
      const uint32_t left = in_parts * 4u - (c << 10);
#if defined(__HIP_DEVICE_COMPILE__)
      if (uint32_t(l) * 16u < left)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, reinterpret_cast<__attribute__((address_space(3))) void*>(al + ssq_off + (u << 10)),
                                                 16, voff_q, r * in_stride * 4u + (c << 10), 0, 0);
#endif
    }
  }
  __builtin_amdgcn_sched_barrier(0);

  // ---- 3. this wave's activation pieces (the oldest requests in its queue) have landed once only its ring
  //      requests are left in flight ----
  wait_records(min(nst * uint32_t(NQ), uint32_t(PF)));
  // the epilogue arguments of 2b: in SGPRs from here on (without the pins hipcc sinks each load to its first use, behind the stream)
  asm volatile("" : "+s"(ncols), "+s"(cbase), "+s"(c16), "+s"(ldc), "+s"(epi));
  if constexpr (DUAL) asm volatile("" : "+s"(c2));
  else asm volatile("" : "+s"(dptr), "+s"(ldd));
  if constexpr (MOE) asm volatile("" : "+s"(moe_cs), "+s"(moe_ds));
  if constexpr (EXT) asm volatile("" : "+s"(in_eps), "+s"(in_inv), "+s"(ogamma), "+s"(ossq), "+s"(ostride), "+s"(rope_on_arg));
  if constexpr (A32) {
#pragma unroll
    for (int i = 0; i < kGvA32Regs; i++) asm volatile("" : "+v"(areg[i]));  // not to be read above the wait
    const uint32_t row_bytes = ks * uint32_t(KSTEP) * 4u;
    const uint32_t pieces = (row_bytes + 1023u) >> 10;
    const uint32_t total = uint32_t(rows) * pieces;
    uint32_t r = 0, c = w;
    if constexpr (I8Q) {
      const uint32_t lds0q = uint32_t(reinterpret_cast<uintptr_t>((LdsPtr)(smem)));
      const uint32_t lpb = 1u << (p.i8_bshift - 2u);  // lanes per k-block (4 columns per lane): 8 .. 64
      const uint32_t k_bytes = uint32_t(p.k) * 4u;
#pragma unroll
      for (int i = 0; i < kGvA32Regs; i++) {
        const uint32_t u = w + (uint32_t(i) << p.nw_log2);
        if (u < total) {  // (wave-uniform)
          if constexpr (!R1)
            while (c >= pieces) c -= pieces, r++;
          const floatx4 v = areg[i];
          float maxval = 1.17549435e-38f /* FLT_MIN: a full block, kernel_ref.h:1832 */, minval = 0.f;
#pragma unroll
          for (int e = 0; e < 4; e++) {
            maxval = v[e] > maxval ? v[e] : maxval;  // std::max(f, maxval): a NaN in f keeps maxval
            minval = v[e] < minval ? v[e] : minval;
          }
          // the k-block's lanes combine max / min (order-independent).  Up to 16 lanes by DPP — quad swaps, then the mirror of the
          // 8-lane half, then of the 16-lane row: no LDS operation, for which hipcc would first drain every LDS-DMA request of the ring —
          // wider blocks by ds_bpermute on top
          auto dpp = [](float x, auto ctrl) {
            return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), decltype(ctrl)::value, 0xf, 0xf, false));
          };
          auto combine = [&](float om, float on) {
            maxval = om > maxval ? om : maxval;
            minval = on < minval ? on : minval;
          };
          combine(dpp(maxval, std::integral_constant<int, 0xB1>{}), dpp(minval, std::integral_constant<int, 0xB1>{}));    // quad_perm [1,0,3,2]
          combine(dpp(maxval, std::integral_constant<int, 0x4E>{}), dpp(minval, std::integral_constant<int, 0x4E>{}));    // quad_perm [2,3,0,1]
          combine(dpp(maxval, std::integral_constant<int, 0x141>{}), dpp(minval, std::integral_constant<int, 0x141>{}));  // row_half_mirror: 8 lanes
          if (lpb > 8u) combine(dpp(maxval, std::integral_constant<int, 0x140>{}), dpp(minval, std::integral_constant<int, 0x140>{}));  // row_mirror: 16
#pragma unroll
          for (uint32_t d = 16; d < 64u; d <<= 1) {
            if (d < lpb) {  // (wave-uniform)
              const float om = __shfl_xor(maxval, int(d), 64), on = __shfl_xor(minval, int(d), 64);
              combine(om, on);
            }
          }
          const float scale = __fdiv_rn(__fsub_rn(maxval, minval), 255.f);
          const int zp = x86_cast_f32_u8(__fdiv_rn(__fsub_rn(0.f, minval), scale));
          const float rscale = __fdiv_rn(1.f, scale), zpf = float(zp);
          uint32_t codes = 0;
#pragma unroll
          for (int e = 0; e < 4; e++)
            codes |= uint32_t(x86_cast_f32_u8(__fadd_rn(zpf, float(x86_cvt_round_int(__fmul_rn(v[e], rscale)))))) << (8 * e);
          const uint32_t col_b = (c << 10) + uint32_t(l) * 16u;  // byte offset of this lane's four columns in the fp32 row
          if (col_b < k_bytes) {  // (K is a multiple of the k-block: a block's lanes are live or dead together)
            // by hand: for a visible LDS store hipcc would first wait for every LDS-DMA request in flight (the whole ring)
            asm volatile("ds_write_b32 %0, %1" ::"v"(lds0q + r * p.row_stride * 2u + (col_b >> 2)), "v"(codes) : "memory");
            if ((uint32_t(l) & (lpb - 1u)) == 0u) {
              const uint32_t kb = (col_b >> 2) >> p.i8_bshift;
              asm volatile("ds_write_b32 %0, %1" ::"v"(lds0q + p.ssq_off + (r * p.i8_nblk + kb) * 4u), "v"(scale) : "memory");
              asm volatile("ds_write_b8 %0, %1" ::"v"(lds0q + p.ssq_off + uint32_t(rows) * p.i8_nblk * 4u + r * p.i8_nblk + kb), "v"(uint32_t(zp)) : "memory");
            }
          }
          c += NW;
        }
      }
    } else {
#pragma unroll
    for (int i = 0; i < kGvA32Regs; i++) {
      const uint32_t u = w + (uint32_t(i) << p.nw_log2);
      if (u < total) {
        while (c >= pieces) c -= pieces, r++;
        const half2_t lo = half2_t{(_Float16)areg[i][0], (_Float16)areg[i][1]};
        const half2_t hi = half2_t{(_Float16)areg[i][2], (_Float16)areg[i][3]};
        const uint32_t dst = uint32_t(reinterpret_cast<uintptr_t>((LdsPtr)(smem))) + r * p.row_stride * 2u + (c << 9) + uint32_t(l) * 8u;
        // by hand: for a visible LDS store hipcc would first wait for every LDS-DMA request in flight (the whole ring)
        if ((c << 10) + uint32_t(l) * 16u < row_bytes)
          asm volatile("ds_write_b64 %0, %1" ::"v"(dst), "v"((uint64_t(as_u32(hi)) << 32) | as_u32(lo)) : "memory");
        c += NW;
      }
    }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  }
  // workgroup barrier over the staged activations, written by hand: for __syncthreads() hipcc first waits for every
  // LDS-DMA request in flight (it cannot know that the rings are wave-private), i.e. for the whole ring to land
  asm volatile("s_barrier" ::: "memory");
  NS_GSTAMP(2);

  // A-fragment LDS offset of this lane (rows >= m are clamped: their output rows are discarded)
  const uint32_t aoff = R1 ? uint32_t(8 * g) : uint32_t(min(nn, rows - 1)) * p.row_stride + 8 * g;
  floatx4 acc[NQ];
#pragma unroll
  for (int q = 0; q < NQ; q++) acc[q] = floatx4{0.f, 0.f, 0.f, 0.f};
  float acc1[NQ];  // R1: row 0 of column nn (every lane group holds it: all A rows of the fragment are row 0); I8S: this lane's k-slots
#pragma unroll
  for (int q = 0; q < NQ; q++) acc1[q] = 0.f;

  float accr[NQ][4];  // I8S: rows 0..3 of column nn, this lane's k-slots
#pragma unroll
  for (int q = 0; q < NQ; q++)
#pragma unroll
    for (int r = 0; r < 4; r++) accr[q][r] = 0.f;
  const uint32_t i8_rsb = p.row_stride * 2u;  // I8S: bytes per staged row of codes
  auto compute = [&](auto slot_c, uint32_t s) {
    constexpr int slot = decltype(slot_c)::value;
    constexpr int q = slot % NQ;
#if defined(NS_GV_ABL) && NS_GV_ABL == 1  // timing ablation (diagnostic builds): the stream alone, no record is decoded or multiplied
    (void)s;
    return;
#endif
    if constexpr (I8S) {
      Corr cr;
      {
        typedef __attribute__((address_space(3))) const uint32_t* L32;
        const uint32_t ca = ring_corr + uint32_t(slot) * SLOT;
        if constexpr (SBYTES == 2) {
          cr.s[0] = *reinterpret_cast<__attribute__((address_space(3))) const uint16_t*>(ca);
        } else {
#pragma unroll
          for (int t = 0; t < Corr::NW32; t++) cr.s[t] = reinterpret_cast<L32>(ca)[t];
        }
        if constexpr (ASYM) {
          const uint32_t za = uint32_t(reinterpret_cast<uintptr_t>(ring)) + uint32_t(slot) * SLOT + 1024u + 16u * SBYTES + uint32_t(nn) * SPS;
          if constexpr (SPS == 4)
            cr.z[0] = *reinterpret_cast<L32>(za);
          else if constexpr (SPS == 2)
            cr.z[0] = *reinterpret_cast<__attribute__((address_space(3))) const uint16_t*>(za);
          else
            cr.z[0] = *reinterpret_cast<__attribute__((address_space(3))) const uint8_t*>(za);
        }
      }
      float sc[4], zp[4];
      corr_decode<SPS, SK, ASYM, NJ>(cr, sc, zp);
      const uint4v qvv = *reinterpret_cast<const __attribute__((address_space(3))) uint4v*>(ring_lane + uint32_t(slot) * SLOT);
      const uint32_t xw[4] = {qvv.x, qvv.y, qvv.z, qvv.w};
      constexpr int BIAS = KIND == WK_INT4 ? 8 : 128;
      const uint32_t lds0 = uint32_t(reinterpret_cast<uintptr_t>((LdsPtr)(smem)));
      const uint32_t kbase = s * uint32_t(KSTEP);
      const uint32_t i8_sbase = lds0 + p.ssq_off;                            // [rows][nblk] fp32 scales
      const uint32_t i8_zbase = i8_sbase + uint32_t(rows) * p.i8_nblk * 4u;  // [rows][nblk] u8 zero points
      // the record's weight side, once for all rows: codes as bytes (k ascending), their sums, zero points + bias, k-blocks
      uint32_t u0[NJ], u1[NJ], kb[NJ];
      int su[NJ], zbq[NJ];
#pragma unroll
      for (int j = 0; j < NJ; j++) {
        if constexpr (KIND == WK_INT4) {
          const uint32_t t0 = xw[j] & 0x0f0f0f0fu, t1 = (xw[j] >> 4) & 0x0f0f0f0fu;  // codes 0,4,1,5 and 2,6,3,7
          u0[j] = __builtin_amdgcn_perm(t1, t0, 0x06040200u);
          u1[j] = __builtin_amdgcn_perm(t1, t0, 0x07050301u);
        } else {
          u0[j] = xw[2 * j] ^ 0x80808080u, u1[j] = xw[2 * j + 1] ^ 0x80808080u;  // raw int8 -> q + 128
        }
        su[j] = int(__builtin_amdgcn_udot4(u0[j], 0x01010101u, __builtin_amdgcn_udot4(u1[j], 0x01010101u, 0u, false), false));
        zbq[j] = (ASYM ? int(zp[j]) : 0) + BIAS;
        kb[j] = min((kbase + 32u * uint32_t(j)) >> p.i8_bshift, p.i8_nblk - 1u);  // (slices past K: clamped, never used)
      }
      if constexpr (R1) {
        // One row: no row loop.  A full k-step (every wave's k-steps but possibly its last) runs without the per-slice test; only a partial
        // last k-step takes the guarded copy.  Integer algebra in 32 bits with 24-bit multiplies: codes <= 255, so sa, su <= 8 * 255 = 2040,
        // za <= 255, zbq = zero point + bias <= 255, |su - 8 zbq| <= 2040 — every operand fits 12 bits, every product 23, and
        //   isum = dot - zbq sa - za su + 8 za zbq = dot + (-zbq) sa + za (8 zbq - su)
        // is two multiply-adds per slice with the weight side's two factors made once per record.  Exact, hence the same integer.
        int nzb[NJ], nsu[NJ];
#pragma unroll
        for (int j = 0; j < NJ; j++) nzb[j] = -zbq[j], nsu[j] = 8 * zbq[j] - su[j];
        const uint32_t aaddr = lds0 + kbase + 8u * uint32_t(g);
        auto row0 = [&](auto guard_c, auto wide_c) {
          constexpr bool GUARD = decltype(guard_c)::value, WIDE = decltype(wide_c)::value;
          uint64_t av[4] = {0, 0, 0, 0};
          uint32_t zau[4] = {0, 0, 0, 0}, asu[4] = {0, 0, 0, 0};
          // LDS reads by hand (see the general form below)
          if constexpr (WIDE) {
            // 32-column activation k-blocks: the record's slices are consecutive blocks — their scales are NJ contiguous words, their
            // zero points NJ contiguous bytes (both aligned: kbase / 32 is a multiple of NJ)
            const uint32_t sa0 = i8_sbase + (kbase >> 5) * 4u, za0 = i8_zbase + (kbase >> 5);
            if constexpr (NJ == 4) {
              uint4v sv;
              uint32_t zw;
              asm volatile(
                  "ds_read_b64 %0, %6\n\tds_read_b64 %1, %6 offset:32\n\tds_read_b64 %2, %6 offset:64\n\tds_read_b64 %3, %6 offset:96\n\t"
                  "ds_read_b128 %4, %7\n\tds_read_b32 %5, %8\n\ts_waitcnt lgkmcnt(0)"
                  : "=&v"(av[0]), "=&v"(av[1]), "=&v"(av[2]), "=&v"(av[3]), "=&v"(sv), "=&v"(zw)
                  : "v"(aaddr), "v"(sa0), "v"(za0)
                  : "memory");
              asu[0] = sv.x, asu[1] = sv.y, asu[2] = sv.z, asu[3] = sv.w;
#pragma unroll
              for (int j = 0; j < 4; j++) zau[j] = (zw >> (8 * j)) & 0xffu;
            } else {
              uint64_t sv;
              uint32_t zw;
              asm volatile(
                  "ds_read_b64 %0, %4\n\tds_read_b64 %1, %4 offset:32\n\tds_read_b64 %2, %5\n\tds_read_u16 %3, %6\n\ts_waitcnt lgkmcnt(0)"
                  : "=&v"(av[0]), "=&v"(av[1]), "=&v"(sv), "=&v"(zw)
                  : "v"(aaddr), "v"(sa0), "v"(za0)
                  : "memory");
              asu[0] = uint32_t(sv), asu[1] = uint32_t(sv >> 32);
              zau[0] = zw & 0xffu, zau[1] = zw >> 8;
            }
          } else if constexpr (NJ == 4) {
            asm volatile(
                "ds_read_b64 %0, %12\n\tds_read_b64 %1, %12 offset:32\n\tds_read_b64 %2, %12 offset:64\n\tds_read_b64 %3, %12 offset:96\n\t"
                "ds_read_u8 %4, %13\n\tds_read_u8 %5, %14\n\tds_read_u8 %6, %15\n\tds_read_u8 %7, %16\n\t"
                "ds_read_b32 %8, %17\n\tds_read_b32 %9, %18\n\tds_read_b32 %10, %19\n\tds_read_b32 %11, %20\n\ts_waitcnt lgkmcnt(0)"
                : "=&v"(av[0]), "=&v"(av[1]), "=&v"(av[2]), "=&v"(av[3]), "=&v"(zau[0]), "=&v"(zau[1]), "=&v"(zau[2]), "=&v"(zau[3]),
                  "=&v"(asu[0]), "=&v"(asu[1]), "=&v"(asu[2]), "=&v"(asu[3])
                : "v"(aaddr), "v"(i8_zbase + kb[0]), "v"(i8_zbase + kb[1]), "v"(i8_zbase + kb[2]), "v"(i8_zbase + kb[3]), "v"(i8_sbase + kb[0] * 4u),
                  "v"(i8_sbase + kb[1] * 4u), "v"(i8_sbase + kb[2] * 4u), "v"(i8_sbase + kb[3] * 4u)
                : "memory");
          } else {
            asm volatile(
                "ds_read_b64 %0, %6\n\tds_read_b64 %1, %6 offset:32\n\tds_read_u8 %2, %7\n\tds_read_u8 %3, %8\n\t"
                "ds_read_b32 %4, %9\n\tds_read_b32 %5, %10\n\ts_waitcnt lgkmcnt(0)"
                : "=&v"(av[0]), "=&v"(av[1]), "=&v"(zau[0]), "=&v"(zau[1]), "=&v"(asu[0]), "=&v"(asu[1])
                : "v"(aaddr), "v"(i8_zbase + kb[0]), "v"(i8_zbase + kb[1]), "v"(i8_sbase + kb[0] * 4u), "v"(i8_sbase + kb[1] * 4u)
                : "memory");
          }
#pragma unroll
          for (int j = 0; j < NJ; j++) {
            if (!GUARD || kbase + 32u * uint32_t(j) < uint32_t(p.k)) {  // wave-uniform: a 32-deep slice lies inside K or outside
              const uint32_t avx = uint32_t(av[j]), avy = uint32_t(av[j] >> 32);
              const int dot = int(__builtin_amdgcn_udot4(avx, u0[j], __builtin_amdgcn_udot4(avy, u1[j], 0u, false), false));
              const int sa = int(__builtin_amdgcn_udot4(avx, 0x01010101u, __builtin_amdgcn_udot4(avy, 0x01010101u, 0u, false), false));
              const int isum = __mul24(int(zau[j]), nsu[j]) + (__mul24(nzb[j], sa) + dot);
              // the general form's  accr += float(isum) * (asu * sc)  is contracted into one FMA per slice; written out here, because left
              // as an expression the vectorizer pairs the slices' products into v_pk_mul_f32 + separate adds (another rounding)
              acc1[q] = __builtin_fmaf(float(isum), __builtin_bit_cast(float, asu[j]) * sc[j], acc1[q]);
            }
          }
        };
        if (kbase + uint32_t(KSTEP) <= uint32_t(p.k)) {
          if (p.i8_bshift == 5u)
            row0(std::false_type{}, std::true_type{});
          else
            row0(std::false_type{}, std::false_type{});
        } else {
          row0(std::true_type{}, std::false_type{});
        }
        return;
      }
#pragma unroll
      for (int r = 0; r < 4; r++) {
        if (r < rows) {
          // LDS reads by hand, one batch per row and record: for a visible LDS read hipcc waits for EVERY LDS-DMA request in
          // flight (vmcnt(0): the whole ring) — it cannot know that the rings and the staged activations do not overlap
          uint64_t av[4] = {0, 0, 0, 0};
          uint32_t zau[4] = {0, 0, 0, 0}, asu[4] = {0, 0, 0, 0};
          const uint32_t aaddr = lds0 + uint32_t(r) * i8_rsb + kbase + 8u * uint32_t(g);
          const uint32_t zrow = i8_zbase + uint32_t(r) * p.i8_nblk, srow = i8_sbase + uint32_t(r) * p.i8_nblk * 4u;
          if constexpr (NJ == 4) {
            asm volatile(
                "ds_read_b64 %0, %12\n\tds_read_b64 %1, %12 offset:32\n\tds_read_b64 %2, %12 offset:64\n\tds_read_b64 %3, %12 offset:96\n\t"
                "ds_read_u8 %4, %13\n\tds_read_u8 %5, %14\n\tds_read_u8 %6, %15\n\tds_read_u8 %7, %16\n\t"
                "ds_read_b32 %8, %17\n\tds_read_b32 %9, %18\n\tds_read_b32 %10, %19\n\tds_read_b32 %11, %20\n\ts_waitcnt lgkmcnt(0)"
                : "=&v"(av[0]), "=&v"(av[1]), "=&v"(av[2]), "=&v"(av[3]), "=&v"(zau[0]), "=&v"(zau[1]), "=&v"(zau[2]), "=&v"(zau[3]),
                  "=&v"(asu[0]), "=&v"(asu[1]), "=&v"(asu[2]), "=&v"(asu[3])
                : "v"(aaddr), "v"(zrow + kb[0]), "v"(zrow + kb[1]), "v"(zrow + kb[2]), "v"(zrow + kb[3]), "v"(srow + kb[0] * 4u),
                  "v"(srow + kb[1] * 4u), "v"(srow + kb[2] * 4u), "v"(srow + kb[3] * 4u)
                : "memory");
          } else {
            asm volatile(
                "ds_read_b64 %0, %6\n\tds_read_b64 %1, %6 offset:32\n\tds_read_u8 %2, %7\n\tds_read_u8 %3, %8\n\t"
                "ds_read_b32 %4, %9\n\tds_read_b32 %5, %10\n\ts_waitcnt lgkmcnt(0)"
                : "=&v"(av[0]), "=&v"(av[1]), "=&v"(zau[0]), "=&v"(zau[1]), "=&v"(asu[0]), "=&v"(asu[1])
                : "v"(aaddr), "v"(zrow + kb[0]), "v"(zrow + kb[1]), "v"(srow + kb[0] * 4u), "v"(srow + kb[1] * 4u)
                : "memory");
          }
#pragma unroll
          for (int j = 0; j < NJ; j++) {
            if (kbase + 32u * uint32_t(j) < uint32_t(p.k)) {  // wave-uniform: a 32-deep slice lies inside K or outside
              const uint32_t avx = uint32_t(av[j]), avy = uint32_t(av[j] >> 32);
              const int za = int(zau[j]);
              const int dot = int(__builtin_amdgcn_udot4(avx, u0[j], __builtin_amdgcn_udot4(avy, u1[j], 0u, false), false));
              const int sa = int(__builtin_amdgcn_udot4(avx, 0x01010101u, __builtin_amdgcn_udot4(avy, 0x01010101u, 0u, false), false));
              const int isum = dot - zbq[j] * sa - za * su[j] + 8 * za * zbq[j];
              accr[q][r] += float(isum) * (__builtin_bit_cast(float, asu[j]) * sc[j]);
            }
          }
        }
      }
      return;
    }
    const _Float16* abase = a_lds + s * KSTEP + aoff;
    // the record's scales / zero points of column nn and the lane's 16 B of codes, out of the ring slot
    Corr cr;
    {
      typedef __attribute__((address_space(3))) const uint32_t* L32;
      const uint32_t ca = ring_corr + uint32_t(slot) * SLOT;
      if constexpr (SBYTES == 2) {
        cr.s[0] = *reinterpret_cast<__attribute__((address_space(3))) const uint16_t*>(ca);
      } else {
#pragma unroll
        for (int t = 0; t < Corr::NW32; t++) cr.s[t] = reinterpret_cast<L32>(ca)[t];
      }
      if constexpr (ASYM) {
        const uint32_t za = uint32_t(reinterpret_cast<uintptr_t>(ring)) + uint32_t(slot) * SLOT + 1024u + 16u * SBYTES + uint32_t(nn) * SPS;
        if constexpr (SPS == 4)
          cr.z[0] = *reinterpret_cast<L32>(za);
        else if constexpr (SPS == 2)
          cr.z[0] = *reinterpret_cast<__attribute__((address_space(3))) const uint16_t*>(za);
        else
          cr.z[0] = *reinterpret_cast<__attribute__((address_space(3))) const uint8_t*>(za);
      }
    }
    float sc[4], zp[4];
    corr_decode<SPS, SK, ASYM, NJ>(cr, sc, zp);
    uint32_t xw[4];
    if constexpr (!PL) {
      const uint4v qvv = *reinterpret_cast<const __attribute__((address_space(3))) uint4v*>(ring_lane + uint32_t(slot) * SLOT);
      xw[0] = qvv.x, xw[1] = qvv.y, xw[2] = qvv.z, xw[3] = qvv.w;
    } else {
      // the lane's plane words out of the slot (layouts: repack_planes_kernel), assembled into the container words
      typedef const __attribute__((address_space(3))) uint32_t* L32;
      typedef const __attribute__((address_space(3))) uint16_t* L16;
      typedef uint32_t uint2v __attribute__((ext_vector_type(2)));
      const uint32_t rec = uint32_t(reinterpret_cast<uintptr_t>(ring)) + uint32_t(slot) * SLOT;
      const uint32_t bits = p.pl_bits;  // wave-uniform
      if constexpr (KIND == WK_INT4) {
        uint32_t a0 = 0, a1 = 0, cw = 0;
        if (bits >= 2) {
          const uint2v av = *reinterpret_cast<const __attribute__((address_space(3))) uint2v*>(rec + 8u * uint32_t(l));
          a0 = av.x, a1 = av.y;
        }
        if (bits != 2) cw = *reinterpret_cast<L32>(rec + (bits == 3 ? 512u : 0u) + 4u * uint32_t(l));
        // the 1-bit plane's bit goes to nibble bit 0 (S1) or 2 (S3): one shift + one and-or per word
        const uint32_t cm = bits == 3 ? 0x44444444u : 0x11111111u;
        const uint32_t c0 = bits == 3 ? cw << 2 : cw, c1 = bits == 3 ? cw << 1 : cw >> 1, c2 = bits == 3 ? cw : cw >> 2,
                       c3 = bits == 3 ? cw >> 1 : cw >> 3;
        xw[0] = and_or(c0, cm, a0 & 0x33333333u);
        xw[1] = and_or(c1, cm, (a0 >> 2) & 0x33333333u);
        xw[2] = and_or(c2, cm, a1 & 0x33333333u);
        xw[3] = and_or(c3, cm, (a1 >> 2) & 0x33333333u);
      } else {
        const uint2v nv = *reinterpret_cast<const __attribute__((address_space(3))) uint2v*>(rec + 8u * uint32_t(l));
        const uint32_t pw = *reinterpret_cast<L32>(rec + 512u + 4u * uint32_t(l));
        // S5: bit 4 of byte b of word d sits at bit 8 b + d of the plane word; S6: bits 4..5 at 8 b + 2 d
        const uint32_t pm = bits == 5 ? 0x10101010u : 0x30303030u;
        const uint32_t st = bits == 5 ? 1u : 2u;
        xw[0] = and_or(pw << 4, pm, nv.x & 0x0f0f0f0fu);
        xw[1] = and_or(pw << (4u - st), pm, (nv.x >> 4) & 0x0f0f0f0fu);
        xw[2] = and_or(pw << (4u - 2u * st), pm, nv.y & 0x0f0f0f0fu);
        xw[3] = and_or(bits == 5 ? pw << 1 : pw >> 2, pm, (nv.y >> 4) & 0x0f0f0f0fu);
      }
    }
    half8_t bq[NJ];
    float full = 0.f;  // PL: the codes are the stored ones (q + 2^(bits-1)); widened records were re-biased at load
    if constexpr (PL) full = float(1u << (p.pl_bits - 1u));
#pragma unroll
    for (int j = 0; j < NJ; j++) {
      if constexpr (KIND == WK_INT4) {
        const _Float16 zl = PL ? (_Float16)(-1024.f - full - zp[j]) : (_Float16)(-1032.f - zp[j]);
        const _Float16 zh = PL ? (_Float16)(-64.f - full - zp[j]) : (_Float16)(-72.f - zp[j]);
        bq[j] = cvt_i4x8(xw[j], i4c, half2_t{zl, zl}, half2_t{zh, zh});
      } else if constexpr (KIND == WK_INT8) {
        if constexpr (PL) {
          const _Float16 zo8 = (_Float16)(-1024.f - full - zp[j]);
          bq[j] = cvt_u8x8(xw[2 * j], xw[2 * j + 1], half2_t{zo8, zo8});
        } else {
          const _Float16 zo8 = (_Float16)(-1152.f - zp[j]);
          bq[j] = cvt_i8x8(xw[2 * j], xw[2 * j + 1], half2_t{zo8, zo8});
        }
      } else if constexpr (KIND == WK_F8) {
        bq[j] = cvt_f8x8(xw[2 * j], xw[2 * j + 1], p.f8);
      } else {
        bq[j] = cvt_f4x8(xw[j], p.lut);
      }
    }
    floatx4 dd[NJ];
#pragma unroll
    for (int j = 0; j < NJ; j++) {
      const half8_t afrag = *reinterpret_cast<const half8_t*>(abase + 32 * j);
      dd[j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(afrag, bq[j], floatx4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
    }
    if constexpr (R1) {
      // element 0 is the live one; the whole result stays alive behind its MFMA — otherwise hipcc hands the other three registers to
      // something else while the MFMA is still in flight (docs/kernels/experiments.md, finding (a))
#pragma unroll
      for (int j = 0; j < NJ; j++) asm volatile("" : "+v"(dd[j]));
#pragma unroll
      for (int j = 0; j < NJ; j++) acc1[q] += dd[j][0] * sc[j];
    } else {
#pragma unroll
      for (int j = 0; j < NJ; j++) acc[q] += dd[j] * sc[j];
    }
  };

  // ---- 4. stream: consume the oldest record, refill its slot with the record PF items ahead ----
  constexpr int SPR = PF / NQ;  // k-steps per round
  const uint32_t rounds = (nst + SPR - 1) / SPR;
  const uint32_t nitems = nst * NQ;
  for (uint32_t r = 0; r < rounds; r++) {
    NS_FOR_SLOTS({
      const uint32_t ord = r * SPR + i / NQ;  // ordinal of the k-step among this wave's
      if (ord < nst) {
        const uint32_t t = r * PF + i;  // ordinal of the item
        wait_records(min(nitems - t - 1, uint32_t(PF - 1)));
        compute(ic, first + (ord << p.nw_log2));
        __builtin_amdgcn_sched_barrier(0);
        if (t == 0) { NS_GSTAMP(3); }  /* first record consumed */
        if (ord + SPR < nst) issue(ic, first + ((ord + SPR) << p.nw_log2));
        __builtin_amdgcn_sched_barrier(0);
      }
    })
  }
  NS_GSTAMP(4);

  if constexpr (I8S && R1) {
#pragma unroll
    for (int q = 0; q < NQ; q++) {
      float v = acc1[q];
      v += __shfl_xor(v, 16, 64);
      v += __shfl_xor(v, 32, 64);
      acc1[q] = g == 0 ? v : 0.f;
    }
  } else if constexpr (I8S) {  // the four k-slots of a column live in lanes nn, nn + 16, nn + 32, nn + 48; rows 0..3 = lane group 0's
#pragma unroll
    for (int q = 0; q < NQ; q++) {
      float t[4];
#pragma unroll
      for (int r = 0; r < 4; r++) {
        float v = accr[q][r];
        v += __shfl_xor(v, 16, 64);
        v += __shfl_xor(v, 32, 64);
        t[r] = v;
      }
      acc[q] = g == 0 ? floatx4{t[0], t[1], t[2], t[3]} : floatx4{0.f, 0.f, 0.f, 0.f};
    }
  }
  // ---- 5. cross-wave reduction: every wave writes its partial sums over ITS OWN ring, wave 0 adds them in wave order ----
  floatx4* red = reinterpret_cast<floatx4*>(smem + p.ring_off);
  const uint32_t kRedWave = p.ring_stride / 16;  // floatx4 per wave region (>= NQ KiB, checked by the host)
  float* red1 = reinterpret_cast<float*>(smem + p.ring_off);  // R1: one float per lane and stream, same wave regions
  const uint32_t kRedWave1 = p.ring_stride / 4;
#pragma unroll
  for (int q = 0; q < NQ; q++) {
    if constexpr (R1)
      red1[w * kRedWave1 + q * 64 + l] = acc1[q];
    else
      red[w * kRedWave + q * 64 + l] = acc[q];
  }
  // (the epilogue's arguments have been in SGPRs since section 3; only what rare paths read — the RoPE words, the overflow
  // flags — is still fetched here, through the argument pointer)
  [[maybe_unused]] const KArgs cold = late_args();
  if constexpr (MOE) {  // the pair's output row (and the row of its epilogue operand)
    cbase += size_t(moe_y) * moe_cs;
    if (dptr) dptr += size_t(moe_y) * moe_ds;
  }
  if constexpr (GRP) {  // row r of the chunk is gathered position grp_first + r, of the fp32 output and of the fp16 one (either may be absent)
    if (cbase) cbase += size_t(grp_first) * ldc;
    if (c16) c16 += size_t(grp_first) * ldc;
  }
  // Wave 0 finishes the tile.  Everything its epilogue has to FETCH (the epilogue operand, the next norm's weight, the
  // RoPE table entry) is requested before the workgroup barrier, so the round trips overlap the wait for the slowest
  // wave instead of following it (each is 1-2 us at the tail of a 5-12 us launch).
  const int col = int(tl) * 16 + nn;
  const bool col_ok = col < ncols;
  float dvp[4] = {0.f, 0.f, 0.f, 0.f};
  float gam = 1.f;
  float2 cs[4];
  int rope_head = 0, rope_e = 0, rope_half = 0;
  bool rope_on = false;
  _Float16* rope_cache = nullptr;
  float* rope_cell = nullptr;
  long long rope_sl = 0;
  // carried norm, consumer side: A was gamma * x, not yet normalised; the row's 1 / rms scales the finished dot
  // products (ne_compute_forward_rms_norm_f32, ne_layers.c: scale = 1 / sqrtf(mean + eps)).  Per row the 64 lanes add
  // the staged partial sums in a fixed order (lane-strided, then a butterfly).
  float rscale[4] = {1.f, 1.f, 1.f, 1.f};
  if (w == 0) {
    if constexpr (!DUAL) {
      if (dptr && col_ok) {
#pragma unroll
        for (int rr = 0; rr < RR; rr++)
          if (4 * g + rr < p.m) dvp[rr] = dptr[size_t(4 * g + rr) * ldd + col];
      }
    }
    if constexpr (EXT) {
      if (ogamma && col_ok) gam = ogamma[col];
      if constexpr (MSEG) {
        rope_on = rope_on_arg != 0;
        if (rope_on) {
          const int hs = cold->rope.head_size;
          rope_head = col / hs;
          rope_e = col - rope_head * hs;
          if (sg < 2) {
#pragma unroll
            for (int rr = 0; rr < RR; rr++) cs[rr] = cold->rope.cos_sin[min(4 * g + rr, rows - 1) * (hs >> 1) + (rope_e >> 1)];
          }
          rope_sl = cold->rope.c_sl;
          const long long kk = cold->rope.kmove ? (long long)*cold->rope.kmove : 0ll;  // tokens since the plan was captured
          rope_cache = (sg == 1 ? cold->rope.kc : cold->rope.vc) + ((long long)cold->rope.n_past + kk * cold->rope.kd_pos) * rope_sl +
                       (long long)rope_head * cold->rope.c_head + rope_e;
          if (sg > 0 && cold->rope.k32)
            rope_cell = sg == 1 ? cold->rope.k32 + kk * cold->rope.k32_tok + rope_head * cold->rope.k32_head + rope_e * cold->rope.k32_dim
                                : cold->rope.v32 + kk * cold->rope.v32_tok + rope_head * cold->rope.v32_head + rope_e * cold->rope.v32_dim;
        }
      }
      if constexpr (MSEGP) {  // (always with the epilogue on: launch_gemv) col is the pair's first element, e < head_size / 2
        const int hs = cold->rope.head_size;
        rope_half = hs >> 1;
        rope_head = col / hs;
        rope_e = col - rope_head * hs;
        if (sg < 2) {
#pragma unroll
          for (int rr = 0; rr < 4; rr++) cs[rr] = cold->rope.cos_sin[min(4 * g + rr, rows - 1) * rope_half + rope_e];
        }
        rope_sl = cold->rope.c_sl;
        rope_cache = (sg == 1 ? cold->rope.kc : cold->rope.vc) + (long long)cold->rope.n_past * rope_sl + (long long)rope_head * cold->rope.c_head + rope_e;
      }
      if (in_ssq) {  // wave 0 requested the pieces itself and has waited for all its requests (last record: vmcnt 0)
        const uint32_t ssq_ld = ((in_parts * 4u + 1023u) >> 10) << 8;  // floats per staged row
        const float* sl = reinterpret_cast<const float*>(smem + ssq_off);
        for (int row = 0; row < rows; row++) {
          float t = 0.f;
          for (uint32_t j = uint32_t(l); j < in_parts; j += 64u) t += sl[uint32_t(row) * ssq_ld + j];
#pragma unroll
          for (int o = 1; o < 64; o <<= 1) t += __shfl_xor(t, o, 64);
          const float r = 1.0f / sqrtf(t * in_inv + in_eps);
          if ((row >> 2) == g) {
#pragma unroll
            for (int rr = 0; rr < 4; rr++)
              if ((row & 3) == rr) rscale[rr] = r;
          }
        }
      }
    }
  }
  __syncthreads();
  NS_GSTAMP(5);  // reduction barrier passed
  if (w == 0) {
    // Every wave's partial sums are requested before the first add — one LDS round trip for any wave count (as a run-time loop
    // the 2- and 4-wave launches paid one dependent round trip per wave) — and added in wave order 0 .. NW - 1 onto +0, as always:
    // the same bits (and 0 + (-0) stays +0).
    floatx4 sum[NQ];
#pragma unroll
    for (int q = 0; q < NQ; q++) sum[q] = floatx4{0.f, 0.f, 0.f, 0.f};
    auto reduce = [&](auto n_c) {
      constexpr int N = decltype(n_c)::value;
#pragma unroll
      for (int q = 0; q < NQ; q++) {
        if constexpr (R1) {
          float t[N];
#pragma unroll
          for (int ww = 0; ww < N; ww++) t[ww] = red1[uint32_t(ww) * kRedWave1 + q * 64 + l];
#pragma unroll
          for (int ww = 0; ww < N; ww++) sum[q][0] += t[ww];
        } else if constexpr (N <= 4) {
          floatx4 t[N];
#pragma unroll
          for (int ww = 0; ww < N; ww++) t[ww] = red[uint32_t(ww) * kRedWave + q * 64 + l];
#pragma unroll
          for (int ww = 0; ww < N; ww++) sum[q] += t[ww];
        } else {
          // four floats per lane and wave: 16 waves at once are 64 registers more than the rest of the kernel needs (96 instead of 41 VGPRs:
          // fewer workgroups per CU).  The run-time loop of before: hipcc unrolls it by eight with the reads pipelined
          for (uint32_t ww = 0; ww < NW; ww++) sum[q] += red[ww * kRedWave + q * 64 + l];
        }
      }
    };
    switch (p.nw_log2) {  // NW is a power of two <= 16 (gemv_plan)
      case 0: reduce(std::integral_constant<int, 1>{}); break;
      case 1: reduce(std::integral_constant<int, 2>{}); break;
      case 2: reduce(std::integral_constant<int, 4>{}); break;
      case 3: reduce(std::integral_constant<int, 8>{}); break;
      default: reduce(std::integral_constant<int, 16>{}); break;
    }
    // ---- 6. epilogue: lane (nn, g) holds rows 4g .. 4g+3 of column nn (R1: row 0 alone, live in lane group 0) ----
#pragma unroll
    for (int rr = 0; rr < RR; rr++) {
      const int row = 4 * g + rr;
      const bool ok = col_ok && row < (GRP ? rows : p.m);  // (GRP: the chunk's rows; p.m is the most a chunk has)
      float v = sum[0][rr] * rscale[rr];
      if constexpr (MSEGP) {
        // ne_rope (mode 2, NeoX) on q and k, then the kv-cache append: x0 = column e < head_size / 2, x1 = column e + head_size / 2 of the
        // head; rope_qkv_append_kernel's arithmetic (ns_quant.hip), every product and sum rounded on its own
        float y0 = v, y1 = sum[1][rr] * rscale[rr];
        if (sg < 2) neox_rotate(v, y1, cs[rr].x, cs[rr].y, &y0, &y1);
        if (ok) {
          if (sg > 0) {
            rope_cache[(long long)row * rope_sl] = (_Float16)y0;
            rope_cache[(long long)row * rope_sl + rope_half] = (_Float16)y1;
          }
          cbase[size_t(row) * ldc + col] = y0;
          cbase[size_t(row) * ldc + col + rope_half] = y1;
        }
        continue;
      }
      if constexpr (MSEG && EXT) {
        if (rope_on) {
          // ne_rope (mode 0) on q and k, then the kv-cache append (models/llama/llama.cpp:232-262): the arithmetic of
          // rope_qkv_append_kernel (ns_quant.hip), separately rounded multiplies; (cos, sin) from the per-token table
          // (evaluating cosf / sinf here — argument reduction for angles up to the context length — cost 12 us per
          // launch, profiles/r02n)
          const float vp = __shfl_xor(v, 1, 64);  // the pair's other element (same tile: 16 | even head_size)
          if (sg < 2)
            v = (rope_e & 1) ? __fadd_rn(__fmul_rn(vp, cs[rr].y), __fmul_rn(v, cs[rr].x))
                             : __fsub_rn(__fmul_rn(v, cs[rr].x), __fmul_rn(vp, cs[rr].y));
          if (ok && sg > 0) {
            rope_cache[(long long)row * rope_sl] = (_Float16)v;
            if (rope_cell && row == 0) {
              *rope_cell = v;
              if (fabsf(v) > 65504.f && cold->rope.ovf) __hip_atomic_store(cold->rope.ovf, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            }
          }
        }
      }
      if (ok) {
        if constexpr (DUAL) {
          // tmp1 = act(A*W1) ; tmp2 = (A*W3) * tmp1   (neural_speed/core/layers/ip_fusion_ffn.cpp:364-406)
          const float t1 = (epi == 5) ? epi_silu(v) : epi_gelu(v);
          if (c2) c2[size_t(row) * ldc + col] = t1;
          v = sum[1][rr] * rscale[rr] * t1;
        } else {
          const float dv = dvp[rr];
          if constexpr (MOE) v *= moe_wsc;  // the routing weight: out (+)= w * (h . W_down)
          v = epi_apply(v, dv, epi);
        }
        if (!GRP || cbase) cbase[size_t(row) * ldc + col] = v;
        // carried norm, producer side: the shadow the NEXT operator streams is gamma * v (its norm's weight), the
        // normalisation itself follows from the partial sums below
        if (c16) c16[size_t(row) * ldc + col] = (_Float16)(v * gam);
        if constexpr (EXT) {
          if (ogamma && fabsf(v * gam) > 65504.f && cold->out_ovf) __hip_atomic_store(cold->out_ovf, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
      }
      if (EXT && ossq) {  // sum of squares of this tile's 16 columns of row `row`, fixed order
        float t = ok ? v * v : 0.f;
        t += __shfl_xor(t, 1, 64);
        t += __shfl_xor(t, 2, 64);
        t += __shfl_xor(t, 4, 64);
        t += __shfl_xor(t, 8, 64);
        if (nn == 0 && row < p.m) ossq[size_t(row) * ostride + tl] = t;
      }
    }
  }
  NS_GSTAMP(6);
#ifdef NS_TRACE
  if ((threadIdx.x & 63) == 0 && blockIdx.x < 4096)  // where the wave ran: XCC_ID (reg 20) and HW_ID (reg 4)
    p.trace[(size_t(blockIdx.x) * 16 + (threadIdx.x >> 6)) * 8 + 7] =
        (uint64_t(__builtin_amdgcn_s_getreg((31 << 11) | 20)) << 32) | uint32_t(__builtin_amdgcn_s_getreg((31 << 11) | 4));
#endif
}

// ============================================================================================================
// host side: the ladder from a launch's run-time format and mode to its instantiation.  The if constexpr guards decide
// WHICH instantiations exist (launch_gemv, ns_gemv_host.cpp, prepares the GemvParams and picks the slice)
// ============================================================================================================
// one instantiation's launch (launch_lds, ns_launch.h: its dynamic LDS limit is raised once, at its first launch)
template <int KIND, int SPS, int SK, bool ASYM, int MODE, int XV, bool PL, bool R1>
static hipError_t gv_launch(dim3 g, dim3 b, size_t lds, hipStream_t st, const GemvParams& p) {
  return launch_lds<gemv_kernel<KIND, SPS, SK, ASYM, MODE, XV, PL, R1>>(int(kGvMaxLds), g, b, lds, st, p);
}
template <int KIND, int SPS, int SK, bool ASYM>
static hipError_t launch_gemv_planes(const GemvParams& p, int mode, int grid, int nw, size_t lds, hipStream_t st) {
  if constexpr ((KIND == WK_INT4 || KIND == WK_INT8) && SK != SK_F16) {
    const dim3 g(grid), b(nw * 64);
    const bool ext = p.in_ssq || p.out_gamma || p.out_ssq || p.rope.on;
    const bool a32 = (mode & kGvModeA32) != 0;
    mode &= 3;
#define NS_GVP(MODEV, EXTV) return gv_launch<KIND, SPS, SK, ASYM, MODEV, EXTV, true, false>(g, b, lds, st, p);
#define NS_GVP_M(MODEV)                                                              \
  {                                                                                 \
    if (ext) NS_GVP(MODEV, 1) else if (a32) NS_GVP(MODEV, 2) else NS_GVP(MODEV, 0)   \
  }
    if (mode == GV_DUAL)
      NS_GVP_M(GV_DUAL)
    else if (mode == GV_MSEG)
      NS_GVP_M(GV_MSEG)
    else
      NS_GVP_M(GV_PLAIN)
#undef NS_GVP_M
#undef NS_GVP
  } else {
    return hipErrorNotSupported;
  }
}
// the one-row form (R1) exists for these instantiations; every other launch of one row takes the general form
constexpr bool gemv_has_rows1(int kind, int mode, int xv) {
  return (kind == WK_INT4 || kind == WK_INT8) && (mode == GV_PLAIN || mode == GV_DUAL || mode == GV_MSEG) && (xv == 0 || xv == 1 || xv == 3 || xv == 5);
}

template <int KIND, int SPS, int SK, bool ASYM>
static hipError_t launch_gemv_k(const GemvParams& p, int mode, int grid, int nw, size_t lds, hipStream_t st, int grid_y) {
  if (mode & kGvModePlanes) return launch_gemv_planes<KIND, SPS, SK, ASYM>(p, mode & ~kGvModePlanes, grid, nw, lds, st);
  const dim3 g(grid, grid_y), b(nw * 64);  // (grid_y > 1: expert-indexed launches only, launch_gemv)
  const bool r1 = p.m == 1 && gemv_rows1();
  const bool ext = p.in_ssq || p.out_gamma || p.out_ssq || p.rope.on;
  const bool a32 = (mode & kGvModeA32) != 0;  // never together with ext (launch_gemv)
  const bool i8s = (mode & kGvModeI8) != 0;
  const bool moe = (mode & kGvModeMoe) != 0, grp = (mode & kGvModeGrp) != 0;
  mode &= ~(kGvModeA32 | kGvModeI8 | kGvModeMoe | kGvModeGrp);
  if (moe || grp) {
    if constexpr (KIND == WK_F8) return hipErrorNotSupported;
    if (mode != GV_PLAIN && mode != GV_DUAL) return hipErrorNotSupported;
  }
  if constexpr (KIND != WK_INT4 && KIND != WK_INT8)
    if (i8s) return hipErrorNotSupported;
#define NS_GV_LAUNCH(MODEV)                                                                                     \
  {                                                                                                             \
    if (grp) NS_GV_LAUNCH_GRP(MODEV) else if (moe) NS_GV_LAUNCH_MOE(MODEV) else if (ext) NS_GV_LAUNCH_E(MODEV, 1) else if (i8s && a32) NS_GV_LAUNCH_I8Q(MODEV) else if (a32) NS_GV_LAUNCH_E(MODEV, 2) else if (i8s) NS_GV_LAUNCH_I8(MODEV)    \
    else NS_GV_LAUNCH_E(MODEV, 0)                                                                               \
  }
#define NS_GV_LAUNCH_MOE(MODEV)                                                                                  \
  {                                                                                                             \
    if constexpr (KIND != WK_F8 && (MODEV == GV_PLAIN || MODEV == GV_DUAL)) NS_GV_LAUNCH_E(MODEV, 4)            \
  }
#define NS_GV_LAUNCH_GRP(MODEV)                                                                                  \
  {                                                                                                             \
    if constexpr (KIND != WK_F8 && (MODEV == GV_PLAIN || MODEV == GV_DUAL))                                     \
      return gv_launch<KIND, SPS, SK, ASYM, MODEV, 6, false, false>(g, b, lds, st, p);                          \
  }
#define NS_GV_LAUNCH_I8Q(MODEV)                                                                                  \
  {                                                                                                             \
    if constexpr (KIND == WK_INT4 || KIND == WK_INT8) NS_GV_LAUNCH_E(MODEV, 5)                                  \
  }
#define NS_GV_LAUNCH_I8(MODEV)                                                                                   \
  {                                                                                                             \
    if constexpr (KIND == WK_INT4 || KIND == WK_INT8) NS_GV_LAUNCH_E(MODEV, 3)                                  \
  }
#define NS_GV_LAUNCH_E(MODEV, EXTV)                                                                             \
  {                                                                                                             \
    if constexpr (gemv_has_rows1(KIND, MODEV, EXTV))                                                            \
      if (r1) return gv_launch<KIND, SPS, SK, ASYM, MODEV, EXTV, false, true>(g, b, lds, st, p);                \
    return gv_launch<KIND, SPS, SK, ASYM, MODEV, EXTV, false, false>(g, b, lds, st, p);                         \
  }
  if (mode == GV_MSEGP) {  // the NeoX RoPE epilogue's pair mode: one instantiation per format (XV = 1)
    if (moe || grp || i8s || a32 || !p.rope.on) return hipErrorNotSupported;
    NS_GV_LAUNCH_E(GV_MSEGP, 1)
  } else if (mode == GV_DUAL)
    NS_GV_LAUNCH(GV_DUAL)
  else if (mode == GV_MSEG)
    NS_GV_LAUNCH(GV_MSEG)
  else
    NS_GV_LAUNCH(GV_PLAIN)
#undef NS_GV_LAUNCH
#undef NS_GV_LAUNCH_E
#undef NS_GV_LAUNCH_I8
#undef NS_GV_LAUNCH_I8Q
#undef NS_GV_LAUNCH_MOE
#undef NS_GV_LAUNCH_GRP
  return hipGetLastError();
}

// ---- this object's slice ----
#define NS_GV_PASTE_(a, b) a##b
#define NS_GV_PASTE(a, b) NS_GV_PASTE_(a, b)
#define NS_GV_SLICE_FN(prefix) NS_GV_PASTE(NS_GV_PASTE(NS_GV_PASTE(prefix, NS_GEMV_KIND), _), NS_GEMV_SPS)
constexpr int kGvSliceKind = NS_GV_PASTE(WK_, NS_GEMV_KIND);

hipError_t NS_GV_SLICE_FN(launch_gemv_)(const GemvParams& p, uint32_t scale_dt, bool asym, int mode, int grid, int nw, size_t lds,
                                        hipStream_t st, int grid_y) {
  return with_scales<kGvSliceKind>(scale_dt, asym, [&](auto sk_c, auto asym_c) {
    return launch_gemv_k<kGvSliceKind, NS_GEMV_SPS, sk_c, asym_c>(p, mode, grid, nw, lds, st, grid_y);
  });
}
void NS_GV_SLICE_FN(touch_gemv_)() {  // (an instantiation every slice has)
  hipFuncAttributes fa;
  (void)hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(gemv_kernel<kGvSliceKind, NS_GEMV_SPS, SK_F32, false, GV_PLAIN, 0>));
  (void)hipGetLastError();
}
}  // namespace ns

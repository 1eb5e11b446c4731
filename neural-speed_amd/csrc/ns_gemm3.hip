// ns_gemm3.hip — prefill / large-M GEMM, third generation (the product):  C[M][N] = A[M][K] * dequant(W), optionally fused QKV (+ RoPE + kv-cache
// append) or gate/up pairs.  ns_gemm_plan.cpp decides the tile form, ns_gemm.cpp launches; what the GEMM files share is in ns_gemm.h.
// Reference semantics: w = (code - zp) * scale, fp32 accumulate (bestla/bestla/kernel_ref.h:1027-1127 dequant,
// bestla_wrapper.h LauncherBase GEMM loop); A rounded to fp16 (north_star: fp16 activations).
#include <hip/hip_runtime.h>

#include <type_traits>

#include "ns_gemm.h"
#include "ns_launch.h"

namespace ns {

// ================================================================================================================
// gemm3_kernel — third generation.  What bounded gemm2_kernel was the LDS pipe, not the matrix cores
// (profiles/r01i: SQ_VALU_MFMA_BUSY 0.39): every chunk the workgroup WROTE 16 KiB of A and 16 KiB of dequantised B
// with ds_write_b128 (~79 B/clk, MI355X_MICROARCH.md LDS table) and read both back.  Here
//   * A (fp16) goes HBM/L2 -> LDS by DMA (buffer_load ... lds, 16 B per lane): no staging registers, no ds_write.  The
//     image is row-major [256 rows][64 halves] with the 16-byte pieces of a row XOR-ed by (row >> 1) & 7 — applied on
//     the SOURCE address of the DMA (the LDS side of a DMA is lane-linear) and on the fragment reads — so every
//     ds_read_b128 lane group covers all 64 banks once;
//   * B never touches LDS: each wave loads the raw records of ITS four column tiles straight into registers (16 B per
//     lane = one record = 128 deep for 4-bit codes) and dequantises them into MFMA B fragments itself.  A record is
//     shared by the two waves that split the rows (one extra L1/L2 hit), in exchange the workgroup moves 1/4 of the
//     LDS bytes and no LDS writes at all;
//   * workgroup tile 256 x 128, four waves of 128 x 64 (8 x 4 accumulator tiles: 12 fragment reads feed 32 MFMAs per
//     32-deep slice), two 32 KiB A stages -> two workgroups per CU, whose waves fill each other's dequantisation
//     and barrier bubbles.
// Synchronisation per 64-deep chunk: s_waitcnt vmcnt(0) (the wave's own DMA of this chunk, issued one chunk ago, has
// landed) -> s_barrier (everybody's has, and everybody is done reading the other stage) -> issue the DMA of the next
// chunk into the other stage -> multiply this chunk.
// BM: rows of the workgroup tile.  256: waves 2 (rows) x 2 (columns), wave tile 128 x 64.  128: waves 1 x 4, wave tile 128 x 32
// — the same MFMA : dequantisation ratio, half the A stage (three workgroups per CU), twice the tiles: for outputs with
// few tiles (4096 wide at 2048 rows: 256 of the tall tiles, one per CU) instead of a K split and its reduction pass.
// TALL (BM = 256 only): waves 1 x 4 like BM = 128, but 256 rows each — wave tile 256 x 32: the dequantisation of a B fragment
// (the VALU work of the loop) is shared by 16 row fragments instead of 8, the same 128 accumulator registers per lane
template <int KIND, int SPS, int SK, bool ASYM, int BM, bool TALL = false, bool DUAL = false>
__global__ __launch_bounds__(256, (BM == 256 ? 2 : 3)) void gemm3_kernel(const Gemm2Params p) {  // (128- / 64-row tiles: three workgroups per CU = three waves per SIMD, at most 168 registers)
  static_assert(!TALL || BM == 256, "the tall wave tile is a 256-row workgroup tile");
  static_assert(!DUAL || (BM <= 128 && !kG3M32), "gate/up pairs: waves 1 x 4 with two column tiles each");
  constexpr bool SQ = BM == 256 && !TALL;       // waves 2 x 2
  constexpr int MI = (SQ ? 128 : BM) / 16;      // row fragments (16 rows) per wave
  constexpr int NIW = SQ ? 4 : 2;               // column tiles (16 wide) per wave
  constexpr int APW = BM / 32;                   // A DMA pieces (8 rows each) per wave and chunk
  constexpr Gemm3Lds kLds = gemm3_lds(KIND, SPS, SK, ASYM, BM, TALL);  // the LDS layout (ns_gemm.h)
  constexpr int kStage = kLds.stage;             // bytes of one A stage
  constexpr bool B8 = kind_is_8bit(KIND);       // 8-bit codes (int8, fp8): a record is 64 deep, two per 128-deep superstep
  constexpr int NJ = B8 ? 2 : 4;                // 32-deep slices per record
  constexpr int RPS = B8 ? 2 : 1;               // records per superstep (128 deep = chunks 2u, 2u + 1)
  constexpr int SBYTES = SPS * (SK == SK_F32 ? 4 : 2);
  constexpr bool M32 = kG3M32;
  static_assert(KIND != WK_F8 || (SK == SK_F32 && !ASYM && !M32 && !TALL), "fp8 weights: fp32 device scales, no zero points, the 16x16x32 loop");
  // VALU instructions the scheduler is asked to place behind each MFMA of a slice (interleave): the next slice's dequantisation is about
  // 18 VALU per B fragment for int8 / int4 codes and 34 for fp8 ones (cvt_f8x8: 7 per code pair + the packed multiply), for MI MFMAs
  constexpr int VPM = KIND == WK_F8 ? 4 : 2;
  constexpr int MB = MI / 2, NP = NIW / 2;       // 32-row / 32-column fragments of the wave tile (M32)
  using Corr = CorrRaw<SPS, SK, ASYM>;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  typedef __attribute__((address_space(3))) unsigned char* LdsPtr;

  const int tid = threadIdx.x;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l = tid & 63, nn = l & 15, g = l >> 4;
  const int wm = SQ ? (w >> 1) : 0, wn = SQ ? (w & 1) : w;
  const int xcd = blockIdx.x & 7, local = blockIdx.x >> 3;
  const int bn = xcd * p.cpx + local % p.cpx, bm = local / p.cpx;
  if (bn >= p.nbn) return;
  // fused QKV: the column block belongs to one of up to three matrices (indexed scalar loads of its pointers)
  int sg = 0;
  if (p.nseg > 1) sg = int(bn >= p.seg_bn0[1]) + int(p.nseg > 2 && bn >= p.seg_bn0[2]);
  const int bnl = p.nseg > 1 ? bn - p.seg_bn0[sg] : bn;  // column block inside its matrix
  const int n_cols = p.nseg > 1 ? p.seg_n[sg] : p.n;
  float* const c_out = p.nseg > 1 ? p.seg_c[sg] : p.c;
  _Float16* const c16_out = p.nseg > 1 ? p.seg_c16[sg] : p.c16;
  // the weight's fp16-range factors (scales are multiplied by spre before the fp16 product, results by spost): per matrix in a fused launch
  const float spre_ = p.nseg > 1 ? p.seg_spre[sg] : p.spre, spost_ = p.nseg > 1 ? p.seg_spost[sg] : p.spost;
  // gate/up pairs: the up matrix (column tile ni = 1 of the wave) has range factors of its own
  const float spre_up = DUAL ? p.seg_spre[1] : spre_, spost_up = DUAL ? p.seg_spost[1] : spost_;
  const int tile0 = DUAL ? bnl * 4 + w : bnl * kG3Tiles + wn * NIW, row0 = bm * BM;  // DUAL: the tile of BOTH matrices (output columns 16 tile0 ..)

  const Rsrc rq = p.nseg > 1 ? make_rsrc(p.seg_codes[sg], p.seg_codes_bytes[sg]) : make_rsrc(p.codes, p.codes_bytes);
  const Rsrc rs = p.nseg > 1 ? make_rsrc(p.seg_scales[sg], p.seg_scales_bytes[sg]) : make_rsrc(p.scales, p.scales_bytes);
  const Rsrc rz = p.nseg > 1 ? make_rsrc(p.seg_zps[sg], p.seg_zps_bytes[sg]) : make_rsrc(p.zps, p.zps_bytes);
  // DUAL: the up matrix (LDS tile slot 2 w + 1 of the wave; slot 2 w is the gate tile)
  const Rsrc rq2 = DUAL ? make_rsrc(p.codes2, p.codes_bytes) : rq;
  const Rsrc rs2 = DUAL ? make_rsrc(p.scales2, p.scales_bytes) : rs;
  const Rsrc rz2 = DUAL ? make_rsrc(p.zps2, p.zps_bytes) : rz;
  const Rsrc ra = make_rsrc(p.a16, uint32_t(p.m) * uint32_t(p.lda16) * 2u);  // rows >= m read as zeros
  const I4Consts i4c = {0x000f000fu, 0x00f000f0u, 0x64006400u};

  floatx4 acc[M32 ? 1 : MI][M32 ? 1 : NIW];
  floatx16 acc32[M32 ? MB : 1][M32 ? NP : 1];
  if constexpr (M32) {
#pragma unroll
    for (int mb = 0; mb < MB; mb++)
#pragma unroll
      for (int pp = 0; pp < NP; pp++)
#pragma unroll
        for (int r = 0; r < 16; r++) acc32[mb][pp][r] = 0.f;
  } else {
#pragma unroll
    for (int mi = 0; mi < MI; mi++)
#pragma unroll
      for (int ni = 0; ni < NIW; ni++) acc[mi][ni] = floatx4{0.f, 0.f, 0.f, 0.f};
  }

  // ---- A: DMA of chunk c into a stage.  Wave w, request i covers rows (8 w + i) * 8 .. + 7; lane l writes LDS piece
  //      l & 7 of row l >> 3 of them and therefore FETCHES piece (l & 7) ^ ((row >> 1) & 7) ----
  const uint32_t lrow = uint32_t(l >> 3);
  uint32_t a_voff[2];  // (row >> 1) & 7 = 4 * (i & 1) + (l >> 4): two per-lane source offsets, for even and odd i
#pragma unroll
  for (int par = 0; par < 2; par++)
    a_voff[par] = (uint32_t(row0) + uint32_t(w) * uint32_t(APW * 8) + lrow) * uint32_t(p.lda16) * 2u +
                  ((uint32_t(l & 7) ^ (uint32_t(4 * par) + uint32_t(l >> 4))) << 4);
  const uint32_t a_istride = 8u * uint32_t(p.lda16) * 2u;  // source bytes between consecutive requests of a wave
  auto issue_a_piece = [&](int c, int stage, int i) {
#if defined(__HIP_DEVICE_COMPILE__)
    const LdsPtr dst = (LdsPtr)(smem) + stage * kStage + (w * APW + i) * 1024;
    __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, reinterpret_cast<__attribute__((address_space(3))) void*>(dst), 16,
                                             a_voff[i & 1], uint32_t(c) * (kG3KC * 2) + uint32_t(i) * a_istride, 0, 0);
#endif
  };
  auto issue_a = [&](int c, int stage) {
#pragma unroll
    for (int i = 0; i < APW; i++) issue_a_piece(c, stage, i);
  };
  // fragment read offsets of this lane: row wm * 128 + mi * 16 + nn, piece (4 jj + g) ^ ((nn >> 1) & 7)
  uint32_t a_roff[2];
#pragma unroll
  for (int jj = 0; jj < 2; jj++)
    a_roff[jj] = uint32_t(wm * 128 + nn) * 128u + ((uint32_t(4 * jj + g) ^ uint32_t((nn >> 1) & 7)) << 4);
  // M32: lane (row l & 31, k half l >> 5) of the 32 x 16 operand kk (0..3 inside the 64-deep chunk) reads piece 2 kk + half of
  // its row, swizzled like every piece by (row >> 1) & 7
  uint32_t a_roff32[4];
#pragma unroll
  for (int kk = 0; kk < 4; kk++)
    a_roff32[kk] = uint32_t(wm * 128 + (l & 31)) * 128u + ((uint32_t(2 * kk + (l >> 5)) ^ uint32_t(((l & 31) >> 1) & 7)) << 4);

  // ---- B: raw records + their scale / zero-point rows of the workgroup's 8 column tiles for one 128-deep superstep,
  //      HBM -> LDS by DMA as well (an ordinary load in this loop would make hipcc drain every DMA in flight at its
  //      first use — measured: s_waitcnt vmcnt(0) right behind the issue).  ONE B stage: the waves copy their records
  //      into registers at the start of the superstep, the DMA of the next superstep refills the stage one chunk later.
  //      Wave w fetches tiles 2w, 2w + 1. ----
  constexpr uint32_t kBCodes = kLds.codes;   // [tile][record][64 lanes x 16 B]
  constexpr uint32_t kBScal = kLds.scal;     // [record][tile][16 columns x SBYTES]
  constexpr uint32_t kBZp = kLds.zp;
  unsigned char* const b_lds = smem + kG3Stages * kStage;
  const uint32_t btile0 = DUAL ? uint32_t(bnl * 4 + w) : uint32_t(bnl * kG3Tiles + 2 * w);
  // scale rows: 16 * SBYTES bytes per (tile, row) = SBYTES lanes of 16 B; lanes [0, 2 * SBYTES) cover the wave's two tiles
  // (DUAL: the two slots are the same tile of two matrices — one request per matrix, lanes [0, SBYTES) each)
  const uint32_t s_lane_tile = DUAL ? 0u : uint32_t(l) / uint32_t(SBYTES), s_lane_piece = uint32_t(l) % uint32_t(SBYTES);
  const uint32_t s_voff = (btile0 + s_lane_tile) * uint32_t(p.srows) * p.sstride + s_lane_piece * 16u;
  const uint32_t z_lane_tile = DUAL ? 0u : uint32_t(l) / uint32_t(SPS), z_lane_piece = uint32_t(l) % uint32_t(SPS);
  const uint32_t z_voff = (btile0 + z_lane_tile) * uint32_t(p.srows) * p.zstride + z_lane_piece * 16u;
  auto issue_b = [&](int u) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
    for (int r = 0; r < RPS; r++) {
      const uint32_t s = uint32_t(min(u * RPS + r, p.ksteps - 1));
#pragma unroll
      for (int t = 0; t < 2; t++) {
        const LdsPtr dst = (LdsPtr)(b_lds) + ((2 * w + t) * RPS + r) * 1024;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(DUAL && t ? rq2 : rq, reinterpret_cast<__attribute__((address_space(3))) void*>(dst), 16, uint32_t(l) * 16u,
                                                 ((btile0 + (DUAL ? 0u : uint32_t(t))) * uint32_t(p.ksteps) + s) * p.qstride, 0, 0);
      }
      const uint32_t srow = (s * uint32_t(p.srow_mul)) >> p.srow_shift;
      if constexpr (DUAL) {
        if (l < SBYTES) {
#pragma unroll
          for (int t = 0; t < 2; t++) {
            const LdsPtr dst = (LdsPtr)(b_lds) + kBCodes + (r * kG3Tiles + 2 * w + t) * (16 * SBYTES);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(t ? rs2 : rs, reinterpret_cast<__attribute__((address_space(3))) void*>(dst), 16, s_voff,
                                                     srow * p.sstride, 0, 0);
          }
        }
        if constexpr (ASYM) {
          if (l < SPS) {
#pragma unroll
            for (int t = 0; t < 2; t++) {
              const LdsPtr dst = (LdsPtr)(b_lds) + kBCodes + kBScal + (r * kG3Tiles + 2 * w + t) * (16 * SPS);
              __builtin_amdgcn_raw_ptr_buffer_load_lds(t ? rz2 : rz, reinterpret_cast<__attribute__((address_space(3))) void*>(dst), 16, z_voff,
                                                       srow * p.zstride, 0, 0);
            }
          }
        }
      } else {
        if (l < 2 * SBYTES) {
          const LdsPtr dst = (LdsPtr)(b_lds) + kBCodes + (r * kG3Tiles + 2 * w) * (16 * SBYTES);
          __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, reinterpret_cast<__attribute__((address_space(3))) void*>(dst), 16, s_voff,
                                                   srow * p.sstride, 0, 0);
        }
        if constexpr (ASYM) {
          if (l < 2 * SPS) {
            const LdsPtr dst = (LdsPtr)(b_lds) + kBCodes + kBScal + (r * kG3Tiles + 2 * w) * (16 * SPS);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rz, reinterpret_cast<__attribute__((address_space(3))) void*>(dst), 16, z_voff,
                                                     srow * p.zstride, 0, 0);
          }
        }
      }
    }
#endif
  };
  struct BRec {
    uint32_t q[NIW][4 * RPS];
    Corr c[NIW][RPS];
  };
  // M32: per PAIR of column tiles pp a lane holds, of the tile its column l & 31 lies in, the two record lanes it is an operand
  // lane of — (k slot 2 e + (l >> 5), column l & 15), e = 0, 1 — and that column's scales / zero points
  struct BRec32 {
    uint32_t q[NP > 0 ? NP : 1][2][4 * RPS];
    Corr c[NP > 0 ? NP : 1][RPS];
  };
  auto read_b32 = [&](BRec32& b) {
#pragma unroll
    for (int pp = 0; pp < NP; pp++) {
      const int t = wn * NIW + 2 * pp + ((l >> 4) & 1);
#pragma unroll
      for (int r = 0; r < RPS; r++) {
#pragma unroll
        for (int e = 0; e < 2; e++) {
          const uint4v v = *reinterpret_cast<const uint4v*>(b_lds + (t * RPS + r) * 1024 + ((2 * e + (l >> 5)) * 16 + nn) * 16);
          b.q[pp][e][4 * r + 0] = v.x, b.q[pp][e][4 * r + 1] = v.y, b.q[pp][e][4 * r + 2] = v.z, b.q[pp][e][4 * r + 3] = v.w;
        }
        const unsigned char* sp = b_lds + kBCodes + ((r * kG3Tiles + t) * 16 + nn) * SBYTES;
        if constexpr (SBYTES == 16) {
          const uint4v sv = *reinterpret_cast<const uint4v*>(sp);
          b.c[pp][r].s[0] = sv.x, b.c[pp][r].s[1] = sv.y, b.c[pp][r].s[2] = sv.z, b.c[pp][r].s[3] = sv.w;
        } else if constexpr (SBYTES == 8) {
          b.c[pp][r].s[0] = reinterpret_cast<const uint32_t*>(sp)[0];
          b.c[pp][r].s[1] = reinterpret_cast<const uint32_t*>(sp)[1];
        } else if constexpr (SBYTES == 4) {
          b.c[pp][r].s[0] = *reinterpret_cast<const uint32_t*>(sp);
        } else {
          b.c[pp][r].s[0] = *reinterpret_cast<const uint16_t*>(sp);
        }
        if constexpr (ASYM) {
          const unsigned char* zp = b_lds + kBCodes + kBScal + ((r * kG3Tiles + t) * 16 + nn) * SPS;
          if constexpr (SPS == 4)
            b.c[pp][r].z[0] = *reinterpret_cast<const uint32_t*>(zp);
          else if constexpr (SPS == 2)
            b.c[pp][r].z[0] = *reinterpret_cast<const uint16_t*>(zp);
          else
            b.c[pp][r].z[0] = *zp;
        }
      }
    }
  };
  // LDS -> registers: this wave's four column tiles (wn * 4 + ni)
  auto read_b = [&](BRec& b) {
#pragma unroll
    for (int ni = 0; ni < NIW; ni++) {
      const int t = wn * NIW + ni;
#pragma unroll
      for (int r = 0; r < RPS; r++) {
        const uint4v v = *reinterpret_cast<const uint4v*>(b_lds + (t * RPS + r) * 1024 + l * 16);
        b.q[ni][4 * r + 0] = v.x, b.q[ni][4 * r + 1] = v.y, b.q[ni][4 * r + 2] = v.z, b.q[ni][4 * r + 3] = v.w;
        const unsigned char* sp = b_lds + kBCodes + ((r * kG3Tiles + t) * 16 + nn) * SBYTES;
        if constexpr (SBYTES == 16) {
          const uint4v sv = *reinterpret_cast<const uint4v*>(sp);
          b.c[ni][r].s[0] = sv.x, b.c[ni][r].s[1] = sv.y, b.c[ni][r].s[2] = sv.z, b.c[ni][r].s[3] = sv.w;
        } else if constexpr (SBYTES == 8) {
          b.c[ni][r].s[0] = reinterpret_cast<const uint32_t*>(sp)[0];
          b.c[ni][r].s[1] = reinterpret_cast<const uint32_t*>(sp)[1];
        } else if constexpr (SBYTES == 4) {
          b.c[ni][r].s[0] = *reinterpret_cast<const uint32_t*>(sp);
        } else {
          b.c[ni][r].s[0] = *reinterpret_cast<const uint16_t*>(sp);
        }
        if constexpr (ASYM) {
          const unsigned char* zp = b_lds + kBCodes + kBScal + ((r * kG3Tiles + t) * 16 + nn) * SPS;
          if constexpr (SPS == 4)
            b.c[ni][r].z[0] = *reinterpret_cast<const uint32_t*>(zp);
          else if constexpr (SPS == 2)
            b.c[ni][r].z[0] = *reinterpret_cast<const uint16_t*>(zp);
          else
            b.c[ni][r].z[0] = *zp;
        }
      }
    }
  };

  // B fragments of 32-deep slice t (0..3) of the superstep held in `b`: codes -> fp16 (code - zp) * scale
  auto dequant = [&](const BRec& b, auto tc, half8_t (&bf)[NIW]) {
    constexpr int t = decltype(tc)::value;
    constexpr int h = t >> 1, jj = t & 1;
#pragma unroll
    for (int ni = 0; ni < NIW; ni++) {
      // 4-bit: word t of the one record; 8-bit: record h, words 2 jj, 2 jj + 1
      float sc[4], zp[4];
      corr_decode<SPS, SK, ASYM, NJ>(b.c[ni][B8 ? h : 0], sc, zp);
      constexpr int js = B8 ? jj : t;  // slice inside its record
      half8_t v;
      if constexpr (KIND == WK_INT4) {
        const _Float16 zl = (_Float16)(-1032.f - zp[js]), zh = (_Float16)(-72.f - zp[js]);
        v = cvt_i4x8(b.q[ni][js], i4c, half2_t{zl, zl}, half2_t{zh, zh});
      } else if constexpr (KIND == WK_INT8) {
        const _Float16 zo = (_Float16)(-1152.f - zp[js]);
        v = cvt_i8x8(b.q[ni][4 * h + 2 * jj], b.q[ni][4 * h + 2 * jj + 1], half2_t{zo, zo});
      } else if constexpr (KIND == WK_F8) {
        // exact bit-level conversion of the reference's encoding (no zero, no subnormals, no NaN: NOT the hardware's OCP fp8); E5M2's
        // exponent-field-0 codes become fp16 subnormals, which the packed multiply below and the MFMA both keep (fp16 denormals are on)
        v = cvt_f8x8(b.q[ni][4 * h + 2 * jj], b.q[ni][4 * h + 2 * jj + 1], p.f8);
      } else {
        v = cvt_f4x8(b.q[ni][js], p.lut);
      }
      const _Float16 sh = (_Float16)(sc[js] * (DUAL && ni ? spre_up : spre_));
      bf[ni] = v * half8_t{sh, sh, sh, sh, sh, sh, sh, sh};
    }
  };
  auto load_af = [&](int stage, int jj, half8_t (&af)[MI]) {
    const unsigned char* a_lds = smem + stage * kStage + a_roff[jj];
#pragma unroll
    for (int mi = 0; mi < MI; mi++) af[mi] = *reinterpret_cast<const half8_t*>(a_lds + mi * (16 * 128));
  };
  // one slice: 32 MFMAs; each A fragment is reloaded for the NEXT slice (stage / jj given) as soon as its four MFMAs are
  // issued — in place, so the next slice's fragments cost no registers beyond this slice's
  // `after(mi)`: hook behind the four MFMAs of fragment row mi — the DMA requests of the next chunk are issued there,
  // one per row, instead of in a burst behind the barrier (a request costs ~60 cycles of issue among MFMAs, 100-185 in a
  // phase that already carries fragment reads, MI355X_MICROARCH.md; 8 of them in front of the MFMAs stall every wave)
  auto mma = [&](half8_t (&af)[MI], const half8_t (&bf)[NIW], auto reload, int stage, int jj, auto&& after) {
    const unsigned char* nxt = smem + stage * kStage + a_roff[jj];
#pragma unroll
    for (int mi = 0; mi < MI; mi++) {
#pragma unroll
      for (int ni = 0; ni < NIW; ni++)
        acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[mi], bf[ni], acc[mi][ni], 0, 0, 0);
      if constexpr (decltype(reload)::value) af[mi] = *reinterpret_cast<const half8_t*>(nxt + mi * (16 * 128));
      after(mi);
    }
  };
  auto nothing = [](int) {};
  // ask the scheduler to spread the preparation of the NEXT slice (8 fragment reads, ~60 VALU of dequantisation) between
  // this slice's 32 MFMAs instead of in front of them: one wave then keeps its matrix pipe busy on its own
  auto interleave = [&](auto vpm, auto ds, auto dma) {
    constexpr int valu_per_mfma = decltype(vpm)::value;
#pragma unroll
    for (int i = 0; i < MI * NIW; i++) {
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                                            // 1 MFMA
      if (decltype(ds)::value && (i & (NIW - 1)) == NIW - 1) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);   // 1 LDS read
      if (decltype(dma)::value && (i & (NIW - 1)) == 1 && i / NIW < APW) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);  // 1 DMA request
      if (valu_per_mfma) __builtin_amdgcn_sched_group_barrier(0x002, valu_per_mfma, 0);             // VALU
    }
  };
  // ---- M32 forms of the same four steps ----
  auto dequant32 = [&](const BRec32& b, auto tc, half8_t (&bf)[NP > 0 ? NP : 1][2]) {
    constexpr int t = decltype(tc)::value;
    constexpr int h = t >> 1, jj = t & 1;
#pragma unroll
    for (int pp = 0; pp < NP; pp++) {
      float sc[4], zp[4];
      corr_decode<SPS, SK, ASYM, NJ>(b.c[pp][B8 ? h : 0], sc, zp);
      constexpr int js = B8 ? jj : t;
      const _Float16 sh = (_Float16)(sc[js] * spre_);
#pragma unroll
      for (int e = 0; e < 2; e++) {
        half8_t v;
        if constexpr (KIND == WK_INT4) {
          const _Float16 zl = (_Float16)(-1032.f - zp[js]), zh = (_Float16)(-72.f - zp[js]);
          v = cvt_i4x8(b.q[pp][e][js], i4c, half2_t{zl, zl}, half2_t{zh, zh});
        } else if constexpr (KIND == WK_INT8) {
          const _Float16 zo = (_Float16)(-1152.f - zp[js]);
          v = cvt_i8x8(b.q[pp][e][4 * h + 2 * jj], b.q[pp][e][4 * h + 2 * jj + 1], half2_t{zo, zo});
        } else {
          v = cvt_f4x8(b.q[pp][e][js], p.lut);
        }
        bf[pp][e] = v * half8_t{sh, sh, sh, sh, sh, sh, sh, sh};
      }
    }
  };
  auto load_af32 = [&](int stage, int jj, half8_t (&af)[MB > 0 ? MB : 1][2]) {
#pragma unroll
    for (int e = 0; e < 2; e++) {
      const unsigned char* a_lds = smem + stage * kStage + a_roff32[2 * jj + e];
#pragma unroll
      for (int mb = 0; mb < MB; mb++) af[mb][e] = *reinterpret_cast<const half8_t*>(a_lds + mb * (32 * 128));
    }
  };
  // one 32-deep slice = two 16-deep operand sets e: (MB x NP) v_mfma_f32_32x32x16_f16 each; operand (mb, e) is reloaded in place
  // for the next slice behind its NP instructions, `after` is called MI times like in the 16x16x32 loop
  auto mma32 = [&](half8_t (&af)[MB > 0 ? MB : 1][2], const half8_t (&bf)[NP > 0 ? NP : 1][2], auto reload, int stage, int jj, auto&& after) {
#pragma unroll
    for (int e = 0; e < 2; e++) {
      const unsigned char* nxt = smem + stage * kStage + a_roff32[2 * jj + e];
#pragma unroll
      for (int mb = 0; mb < MB; mb++) {
#pragma unroll
        for (int pp = 0; pp < NP; pp++)
          acc32[mb][pp] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[mb][e], bf[pp][e], acc32[mb][pp], 0, 0, 0);
        if constexpr (decltype(reload)::value) af[mb][e] = *reinterpret_cast<const half8_t*>(nxt + mb * (32 * 128));
        after(e * MB + mb);
      }
    }
  };
  auto interleave32 = [&](auto vpm, auto ds, auto dma) {
    constexpr int valu_per_mfma = decltype(vpm)::value;
#pragma unroll
    for (int i = 0; i < 2 * MB * NP; i++) {
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                                                   // 1 MFMA (twice the work of a 16x16x32)
      if (decltype(ds)::value && (i % NP) == NP - 1) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);    // 1 LDS read
      if (decltype(dma)::value && (i % NP) == 0 && i / NP < APW) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);  // 1 DMA request
      if (valu_per_mfma) __builtin_amdgcn_sched_group_barrier(0x002, 2 * valu_per_mfma, 0);                // VALU
    }
  };
  using T_ = std::true_type;
  using F_ = std::false_type;

  // chunk range of this workgroup (split-K: an even number of chunks per split, so supersteps never straddle)
  const int cbeg = p.ksplit > 1 ? int(blockIdx.y) * p.cps : 0;
  const int cend = p.ksplit > 1 ? min(p.nchunks, cbeg + p.cps) : p.nchunks;
  const int ubeg = cbeg >> 1, uend = (cend + 1) >> 1;

  if constexpr (M32) {
    BRec32 breg;
    half8_t af[MB > 0 ? MB : 1][2], bf0[NP > 0 ? NP : 1][2], bf1[NP > 0 ? NP : 1][2];
    issue_a(cbeg, 0);
    issue_b(ubeg);
    for (int u = ubeg; u < (p.diag == 2 ? ubeg + 1 : uend); u++) {
      const int c0 = 2 * u;
      // ---- chunk 2u (A stage 0): this superstep's records move to registers ----
      // __syncthreads() = s_waitcnt vmcnt(0) lgkmcnt(0) + s_barrier here (hipcc drains the DMAs in flight before a
      // barrier): the wave's own DMAs — A(2u), B(u) — have landed, then everybody's have, and everybody is done with A
      // stage 1.
      __syncthreads();
      read_b32(breg);
      load_af32(0, 0, af);
      dequant32(breg, std::integral_constant<int, 0>{}, bf0);
      __builtin_amdgcn_sched_barrier(0);
      // slice 0 multiplies while slice 1 is prepared and the next chunk's A image is requested piece by piece
      // (requested unconditionally: past the last chunk the pieces land in a stage nobody reads — the source offsets stay
      // inside the buffer descriptor or read as zeros — and the loop body stays one straight-line block to schedule)
      const bool more1 = c0 + 1 < cend;
      dequant32(breg, std::integral_constant<int, 1>{}, bf1);
      mma32(af, bf0, T_{}, 0, 1, [&](int mi) {
        if (mi < APW) issue_a_piece(c0 + 1, 1, mi);
      });
      interleave32(std::integral_constant<int, 2>{}, T_{}, T_{});
      __builtin_amdgcn_sched_barrier(0);
      // slice 1 multiplies while slice 2's B fragments are prepared (its A image is behind the next barrier)
      dequant32(breg, std::integral_constant<int, 2>{}, bf0);
      mma32(af, bf1, F_{}, 0, 0, nothing);
      interleave32(std::integral_constant<int, 2>{}, F_{}, F_{});
      __builtin_amdgcn_sched_barrier(0);
      // ---- chunk 2u + 1 (A stage 1) ----
      if (more1) {
        __syncthreads();  // A(2u + 1) has landed; everybody has copied B(u) and left A stage 0
        if (u + 1 < uend) issue_b(u + 1);
        load_af32(1, 0, af);
        __builtin_amdgcn_sched_barrier(0);
        dequant32(breg, std::integral_constant<int, 3>{}, bf1);
        mma32(af, bf0, T_{}, 1, 1, [&](int mi) {
          if (mi < APW) issue_a_piece(c0 + 2, 0, mi);
        });
        interleave32(std::integral_constant<int, 2>{}, T_{}, T_{});
        __builtin_amdgcn_sched_barrier(0);
        mma32(af, bf1, F_{}, 0, 0, nothing);
      }
    }
  } else {
    BRec breg;
    half8_t af[MI], bf0[NIW], bf1[NIW];
    issue_a(cbeg, 0);
    issue_b(ubeg);
    for (int u = ubeg; u < (p.diag == 2 ? ubeg + 1 : uend); u++) {
      const int c0 = 2 * u;
      // ---- chunk 2u (A stage 0): this superstep's records move to registers ----
      // __syncthreads() = s_waitcnt vmcnt(0) lgkmcnt(0) + s_barrier here (hipcc drains the DMAs in flight before a
      // barrier): the wave's own DMAs — A(2u), B(u) — have landed, then everybody's have, and everybody is done with A
      // stage 1.
      __syncthreads();
      read_b(breg);
      load_af(0, 0, af);
      dequant(breg, std::integral_constant<int, 0>{}, bf0);
      __builtin_amdgcn_sched_barrier(0);
      // slice 0 multiplies while slice 1 is prepared and the next chunk's A image is requested piece by piece
      // (requested unconditionally: past the last chunk the pieces land in a stage nobody reads — the source offsets stay
      // inside the buffer descriptor or read as zeros — and the loop body stays one straight-line block to schedule)
      const bool more1 = c0 + 1 < cend;
      dequant(breg, std::integral_constant<int, 1>{}, bf1);
      mma(af, bf0, T_{}, 0, 1, [&](int mi) {
        if (mi < APW) issue_a_piece(c0 + 1, 1, mi);
      });
      interleave(std::integral_constant<int, VPM>{}, T_{}, T_{});
      __builtin_amdgcn_sched_barrier(0);
      // slice 1 multiplies while slice 2's B fragments are prepared (its A image is behind the next barrier)
      dequant(breg, std::integral_constant<int, 2>{}, bf0);
      mma(af, bf1, F_{}, 0, 0, nothing);
      interleave(std::integral_constant<int, VPM>{}, F_{}, F_{});
      __builtin_amdgcn_sched_barrier(0);
      // ---- chunk 2u + 1 (A stage 1) ----
      if (more1) {
        __syncthreads();  // A(2u + 1) has landed; everybody has copied B(u) and left A stage 0
        if (u + 1 < uend) issue_b(u + 1);
        load_af(1, 0, af);
        __builtin_amdgcn_sched_barrier(0);
        dequant(breg, std::integral_constant<int, 3>{}, bf1);
        mma(af, bf0, T_{}, 1, 1, [&](int mi) {
          if (mi < APW) issue_a_piece(c0 + 2, 0, mi);
        });
        interleave(std::integral_constant<int, VPM>{}, T_{}, T_{});
        __builtin_amdgcn_sched_barrier(0);
        mma(af, bf1, F_{}, 0, 0, nothing);
      }
    }
  }

  // ---- epilogue: through LDS, so that C leaves in whole rows.  A lane of the MFMA layout holds column nn of rows
  //      4g .. 4g + 3: storing from there writes 64-byte (fp32) and 32-byte (fp16 shadow) pieces — 50 MB per 2048 x 4096
  //      output at a fraction of the HBM write rate, a third of the whole GEMM's time at K = 4096.  Each wave parks half
  //      of its 128 x 64 tile (64 rows, padded to 68 floats: conflict-free ds_write_b32) in the stage memory, reads it
  //      back as float4 along the rows and stores 256-byte runs; the operator is applied on the way out, in a plain loop
  //      (nothing below indexes the accumulators dynamically — with the switch inside the unrolled accumulator loops hipcc
  //      kept all 128 accumulator registers in scratch memory, a store behind every MFMA of the main loop). ----
  const int epi = p.epilogue;
  // ---- the cross-wave form of that epilogue (round 5; waves 1 x 4).  Measured on the 7B shapes at 2048 rows (profiles/r05a_prefill_probe.txt):
  //      with the stores skipped a 11008-wide GEMM takes 184 us, with the fp32 stores 187, with fp32 + the fp16 shadow 205 — the shadow left
  //      each wave as 8-byte stores in 64-byte runs (half a memory line).  Here the four waves park their 64-row halves side by side
  //      (row = the workgroup tile's whole width), each wave then owns 16 of the 64 rows: fp32 leaves as float4 per lane in 512-byte
  //      runs (256 for gate/up pairs), the fp16 shadow in a second read-back as 16-byte stores (8 columns per lane) in 256-byte runs
  //      (128).  DUAL: gate and up of one (row, column) sit in the same lane, the product is formed before parking. ----
  if constexpr (!SQ && !M32) {
    if (p.wide && p.ksplit <= 1) {
      constexpr int PC = NIW * 16;               // parked columns per wave (DUAL: 16 gate + 16 up)
      constexpr int WROW = 4 * PC + 4;           // floats per parked row (ds_write_b32 of the MFMA layout stays conflict-free)
      constexpr int OC = DUAL ? 16 : PC;         // output columns per wave
      constexpr int W = 4 * OC;                  // output columns of the workgroup tile
      constexpr int LA = W / 4, RA = 64 / LA, IA = 16 / RA;  // fp32 pass: lanes per row, rows per wave instruction, iterations
      constexpr int LB = W / 8, RB = 64 / LB, IB = 16 / RB;  // fp16 pass
      float* parkw = reinterpret_cast<float*>(smem);
      const int colb = bnl * W;  // first output column of the tile inside its matrix
      const bool full = colb + W <= n_cols;
      const bool al = (p.ldc & 7) == 0 && (!c_out || (reinterpret_cast<uintptr_t>(c_out) & 15) == 0) &&
                      (!c16_out || (reinterpret_cast<uintptr_t>(c16_out) & 15) == 0) &&
                      (!p.d || ((p.ldd & 3) == 0 && (reinterpret_cast<uintptr_t>(p.d) & 15) == 0)) &&
                      (!DUAL || !p.c2 || (reinterpret_cast<uintptr_t>(p.c2) & 15) == 0);
      const bool use_d = !DUAL && p.d && epi >= 1 && epi <= 3;
      typedef _Float16 half8o_t __attribute__((ext_vector_type(8)));
      // parked column of output column oc: the wave that multiplied it, then its place among that wave's columns
      auto pcol = [&](int oc) { return DUAL ? (oc >> 4) * PC + (oc & 15) : oc; };
      // one float4 of finished outputs at (parked row pr, output columns oc .. oc + 3); DUAL: act(gate) * up, gate4 = act(gate)
      auto out4 = [&](int pr, int oc, int row, float4* gate4) {
        const float* q = parkw + pr * WROW + pcol(oc);
        float4 v = *reinterpret_cast<const float4*>(q);
        if constexpr (DUAL) {
          const float4 u = *reinterpret_cast<const float4*>(q + 16);
          v = float4{epi_apply(v.x, 0.f, epi), epi_apply(v.y, 0.f, epi), epi_apply(v.z, 0.f, epi), epi_apply(v.w, 0.f, epi)};
          if (gate4) *gate4 = v;
          v = float4{v.x * u.x, v.y * u.y, v.z * u.z, v.w * u.w};
        } else {
          float4 dv = {0.f, 0.f, 0.f, 0.f};
          if (use_d) dv = *reinterpret_cast<const float4*>(p.d + size_t(row) * p.ldd + colb + oc);
          v = float4{epi_apply(v.x, dv.x, epi), epi_apply(v.y, dv.y, epi), epi_apply(v.z, dv.z, epi), epi_apply(v.w, dv.w, epi)};
        }
        return v;
      };
#pragma unroll
      for (int hh = 0; hh < MI / 4; hh++) {
        __syncthreads();  // every wave is done with the A stages / with the previous read-back
#pragma unroll
        for (int mi = 0; mi < 4; mi++)
#pragma unroll
          for (int ni = 0; ni < NIW; ni++)
#pragma unroll
            for (int r = 0; r < 4; r++)
              parkw[(mi * 16 + 4 * g + r) * WROW + w * PC + ni * 16 + nn] = acc[4 * hh + mi][ni][r] * (DUAL && ni ? spost_up : spost_);
        __syncthreads();
        if (p.diag == 1) continue;
        const int rb = row0 + hh * 64 + w * 16;  // this wave's 16 rows of the half
        if (full && al) {
          if (c_out || (DUAL && p.c2)) {
            for (int it = 0; it < IA; it++) {
              const int rl = it * RA + l / LA, row = rb + rl, oc = (l % LA) * 4;
              if (row >= p.m) continue;
              float4 gate4;
              const float4 v = out4(w * 16 + rl, oc, row, &gate4);
              if (c_out) *reinterpret_cast<float4*>(c_out + size_t(row) * p.ldc + colb + oc) = v;
              if constexpr (DUAL) {
                if (p.c2) *reinterpret_cast<float4*>(p.c2 + size_t(row) * p.ldc + colb + oc) = gate4;
              }
            }
          }
          if (c16_out) {
            for (int it = 0; it < IB; it++) {
              const int rl = it * RB + l / LB, row = rb + rl, oc = (l % LB) * 8;
              if (row >= p.m) continue;
              const float4 v0 = out4(w * 16 + rl, oc, row, nullptr), v1 = out4(w * 16 + rl, oc + 4, row, nullptr);
              *reinterpret_cast<half8o_t*>(c16_out + size_t(row) * p.ldc + colb + oc) =
                  half8o_t{(_Float16)v0.x, (_Float16)v0.y, (_Float16)v0.z, (_Float16)v0.w, (_Float16)v1.x, (_Float16)v1.y, (_Float16)v1.z, (_Float16)v1.w};
            }
          }
        } else {  // ragged right edge or unaligned outputs: element by element, row-major over the wave's 16 x W part
          for (int e = l; e < 16 * W; e += 64) {
            const int rl = e / W, oc = e % W, row = rb + rl, col = colb + oc;
            if (row >= p.m || col >= n_cols) continue;
            const float* q = parkw + (w * 16 + rl) * WROW + pcol(oc);
            float v = q[0];
            if constexpr (DUAL) {
              v = epi_apply(v, 0.f, epi);
              if (p.c2) p.c2[size_t(row) * p.ldc + col] = v;
              v *= q[16];
            } else {
              v = epi_apply(v, use_d ? p.d[size_t(row) * p.ldd + col] : 0.f, epi);
            }
            if (c_out) c_out[size_t(row) * p.ldc + col] = v;
            if (c16_out) c16_out[size_t(row) * p.ldc + col] = (_Float16)v;
          }
        }
      }
      return;
    }
  }
  if constexpr (DUAL) return;  // (gate/up launches always take the cross-wave epilogue)
  constexpr int kCols = NIW * 16;     // columns of the wave tile
  constexpr int kRowF = kCols + 4;    // floats per parked row
  constexpr int kLpr = kCols / 4;     // lanes per row in the float4 read-back
  float* park = reinterpret_cast<float*>(smem) + w * (64 * kRowF);
  const int colw = tile0 * 16;  // first column of this wave's 64
  const bool vec4 = (p.ldc & 3) == 0 && (reinterpret_cast<uintptr_t>(c_out) & 15) == 0 && colw + kCols <= n_cols &&
                    (p.ksplit > 1 ? (p.n & 3) == 0 && (reinterpret_cast<uintptr_t>(p.part) & 15) == 0 : true) &&
                    (!p.d || ((p.ldd & 3) == 0 && (reinterpret_cast<uintptr_t>(p.d) & 15) == 0)) &&
                    (!c16_out || (reinterpret_cast<uintptr_t>(c16_out) & 7) == 0);
  __syncthreads();  // every wave is done with the A stages
#pragma unroll
  for (int hh = 0; hh < MI / 4; hh++) {
    if constexpr (M32) {  // C of v_mfma_f32_32x32x16: lane (column l & 31, half l >> 5), register r -> row (r & 3) + 8 (r >> 2) + 4 half
#pragma unroll
      for (int mbl = 0; mbl < 2; mbl++)
#pragma unroll
        for (int pp = 0; pp < NP; pp++)
#pragma unroll
          for (int r = 0; r < 16; r++)
            park[(mbl * 32 + (r & 3) + 8 * (r >> 2) + 4 * (l >> 5)) * kRowF + pp * 32 + (l & 31)] = acc32[2 * hh + mbl][pp][r] * spost_;
    } else {
#pragma unroll
      for (int mi = 0; mi < 4; mi++)
#pragma unroll
        for (int ni = 0; ni < NIW; ni++)
#pragma unroll
          for (int r = 0; r < 4; r++) park[(mi * 16 + 4 * g + r) * kRowF + ni * 16 + nn] = acc[4 * hh + mi][ni][r] * spost_;
    }
    // (LDS operations of one wave complete in order: no barrier between its own writes and reads)
    // NeoX RoPE (rope_on == 2): a lane's partner columns, head_size / 2 further on or back, were parked by another lane and for
    // head sizes 64 / 128 by another wave — workgroup barriers around the park, outside everything that depends on the row
    const bool neox = p.rope_on == 2;
    if (neox) __syncthreads();
    const int rbase = row0 + wm * 128 + hh * 64;
    if (p.diag == 1) continue;
    if (vec4) {
      for (int it = 0; it < kLpr; it++) {
        const int rl = it * (64 / kLpr) + l / kLpr, row = rbase + rl, col = colw + (l % kLpr) * 4;
        if (row >= p.m) continue;
        float4 v = *reinterpret_cast<const float4*>(park + rl * kRowF + (l % kLpr) * 4);
        if (p.ksplit > 1) {  // raw partial; the operator is applied by gemm2_reduce_kernel
          *reinterpret_cast<float4*>(p.part + (size_t(blockIdx.y) * p.m + row) * p.n + col) = v;
          continue;
        }
        if (p.rope_on) {  // fused QKV + RoPE + cache append: rope_qkv_append_tab_kernel's arithmetic on the four columns (two adjacent pairs) of this lane
          typedef _Float16 half4r_t __attribute__((ext_vector_type(4)));
          const int hd = col / p.rope_hs, dcol = col - hd * p.rope_hs;
          if (neox) {
            // pairs (e, e + head_size / 2), head_size 32 / 64 / 128: the head lies inside this 128-column block, the partner four columns in
            // the same parked row of wave (partner column / wave columns) — rope_qkv_append_tab_kernel's NeoX branch, products and sums rounded one by one
            if (sg < 2) {
#pragma clang fp contract(off)
              const int half = p.rope_hs >> 1, e = dcol & (half - 1);
              const int wc = (wn * kCols + (l % kLpr) * 4) ^ half;  // the partner's column in the workgroup tile
              const float* pw = reinterpret_cast<const float*>(smem) + (w - wn + wc / kCols) * (64 * kRowF) + rl * kRowF + (wc % kCols);
              const float4 o = *reinterpret_cast<const float4*>(pw);
              const float2* tp = p.rope_tab + (size_t(row) * size_t(half) + size_t(e));
              const float4 c01 = *reinterpret_cast<const float4*>(tp), c23 = *reinterpret_cast<const float4*>(tp + 2);
              const bool lo = dcol < half;  // this lane holds x0 (and writes y0 = x0 c - x1 s) or x1 (y1 = x0 s + x1 c)
              const float4 xa = lo ? v : o, xb = lo ? o : v;
              const float a0 = xa.x * (lo ? c01.x : c01.y), a1 = xa.y * (lo ? c01.z : c01.w), a2 = xa.z * (lo ? c23.x : c23.y), a3 = xa.w * (lo ? c23.z : c23.w);
              const float b0 = xb.x * (lo ? c01.y : c01.x), b1 = xb.y * (lo ? c01.w : c01.z), b2 = xb.z * (lo ? c23.y : c23.x), b3 = xb.w * (lo ? c23.w : c23.z);
              v.x = lo ? a0 - b0 : a0 + b0, v.y = lo ? a1 - b1 : a1 + b1, v.z = lo ? a2 - b2 : a2 + b2, v.w = lo ? a3 - b3 : a3 + b3;
            }
          } else if (sg < 2) {
#pragma clang fp contract(off)  // (rope_kernel's products and sums are rounded one by one: ns_quant.hip is built with -ffp-contract=off, this file is not)
            const float4 cs = *reinterpret_cast<const float4*>(p.rope_tab + (size_t(row) * size_t(p.rope_hs >> 1) + size_t(dcol >> 1)));
            const float x0 = v.x, x1 = v.y, x2 = v.z, x3 = v.w;
            // (plain operators: hipcc's __fmul_rn / __fadd_rn are inline x * y / x + y carrying their header's contraction mode, which fuses them here)
            const float p0 = x0 * cs.x, p1 = x1 * cs.y, p2 = x0 * cs.y, p3 = x1 * cs.x, p4 = x2 * cs.z, p5 = x3 * cs.w, p6 = x2 * cs.w, p7 = x3 * cs.z;
            v.x = p0 - p1, v.y = p2 + p3, v.z = p4 - p5, v.w = p6 + p7;
          }
          if (sg > 0) {
            _Float16* cell = (sg == 1 ? p.rope_kc : p.rope_vc) + (long long)(p.rope_npast + row) * p.rope_csl + (long long)hd * p.rope_chead + dcol;
            *reinterpret_cast<half4r_t*>(cell) = half4r_t{(_Float16)v.x, (_Float16)v.y, (_Float16)v.z, (_Float16)v.w};
          }
          if (c_out) *reinterpret_cast<float4*>(c_out + size_t(row) * p.ldc + col) = v;
          continue;
        }
        float4 dv = {0.f, 0.f, 0.f, 0.f};
        if (p.d && epi >= 1 && epi <= 3) dv = *reinterpret_cast<const float4*>(p.d + size_t(row) * p.ldd + col);
        v = float4{epi_apply(v.x, dv.x, epi), epi_apply(v.y, dv.y, epi), epi_apply(v.z, dv.z, epi), epi_apply(v.w, dv.w, epi)};
        if (c_out) *reinterpret_cast<float4*>(c_out + size_t(row) * p.ldc + col) = v;
        if (c16_out) {
          typedef _Float16 half4_t __attribute__((ext_vector_type(4)));
          *reinterpret_cast<half4_t*>(c16_out + size_t(row) * p.ldc + col) =
              half4_t{(_Float16)v.x, (_Float16)v.y, (_Float16)v.z, (_Float16)v.w};
        }
      }
    } else {
      for (int it = 0; it < 64 * kCols / 64; it++) {  // 64 elements per step, row-major over the 64 x kCols half tile
        const int e = it * 64 + l, rl = e / kCols, cl = e % kCols;
        const int row = rbase + rl, col = colw + cl;
        if (row >= p.m || col >= n_cols) continue;
        float v = park[rl * kRowF + cl];
        if (p.ksplit > 1) {
          p.part[(size_t(blockIdx.y) * p.m + row) * p.n + col] = v;
          continue;
        }
        const float dv = (p.d && epi >= 1 && epi <= 3) ? p.d[size_t(row) * p.ldd + col] : 0.f;
        v = epi_apply(v, dv, epi);
        if (c_out) c_out[size_t(row) * p.ldc + col] = v;
        if (c16_out) c16_out[size_t(row) * p.ldc + col] = (_Float16)v;
      }
    }
    if (neox && hh + 1 < MI / 4) __syncthreads();  // every wave has read its partners before the next half is parked
  }
}

template <int KIND, int SPS, int SK, bool ASYM, int BM, bool TALL, bool DUAL>
static hipError_t launch_gemm3_k(const GemmPlan& pl, hipStream_t st) {
  return launch_gemm_reduce(launch_lds<gemm3_kernel<KIND, SPS, SK, ASYM, BM, TALL, DUAL>>(int(kG3Stages * kG3StageBytes + kG3BStageMax), pl.grid, dim3(256), pl.lds, st, pl.p), pl.p, st);
}
// gemm3_kernel for the plan's format (with_format, ns_launch.h) and tile form (BM, TALL, DUAL: p.bm3, p.tall3, p.dual)
hipError_t launch_gemm3_plan(const GemmPlan& pl, hipStream_t st) {
  const Gemm2Params& p = pl.p;
  return with_format(pl.kind, pl.sps, pl.scale_dt, pl.asym, [&](auto kind_c, auto sps_c, auto sk_c, auto asym_c) {
    constexpr int KIND = kind_c, SPS = sps_c, SK = sk_c;
    constexpr bool ASYM = asym_c;
    auto tile = [&](auto bm_c, auto tall_c, auto dual_c) { return launch_gemm3_k<KIND, SPS, SK, ASYM, bm_c, tall_c, dual_c>(pl, st); };
    constexpr std::true_type yes;
    constexpr std::false_type no;
    if (p.dual) {  // gate/up pairs: the 1 x 4 wave tiles only
      if (p.bm3 == 64) return tile(int_c<64>{}, no, yes);
      return tile(int_c<128>{}, no, yes);
    }
    if (p.bm3 == 64) return tile(int_c<64>{}, no, no);  // calls of at most 64 rows: a quarter / half of the 128-row tile's MFMA work is padding otherwise
    if (p.bm3 == 128) return tile(int_c<128>{}, no, no);
    if constexpr (KIND == WK_INT4)
      if (p.tall3) return tile(int_c<256>{}, yes, no);
    return tile(int_c<256>{}, no, no);
  });
}

void touch_gemm_module() {
  hipFuncAttributes fa;
  (void)hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(gemm3_kernel<WK_INT4, 4, SK_BF16, false, 128, false, false>));
  (void)hipGetLastError();
}
}  // namespace ns

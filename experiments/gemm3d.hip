// gemm3d.hip — gemm3_kernel with a deep pipeline for one workgroup per CU: measured slower than gemm3_kernel on every int4 shape
// (profiles/r02q_gemm3_vs_gemm3d.txt) and taken out of the product.  Not built.  See experiments/README.md for how it hooked in:
// it lived in the prefill GEMM's translation unit behind NS_WITH_GEMM3D, beside gemm3_kernel, and shared its constants (ns_gemm.h today).
// ================================================================================================================
// gemm3d_kernel — gemm3_kernel with a DEEP pipeline, for one workgroup per CU.  gemm3_kernel relies on a second
// workgroup on the CU to cover its memory latency (each chunk's DMA is issued one chunk ahead): with 256 output tiles
// on 256 CUs (every 4096-wide GEMM at 2048 rows) a chunk took 1.4 us, 30 % matrix-core utilisation, and splitting K to
// get the second workgroup costs a reduction pass as long as a third of the GEMM (profiles/r02q).  Here
//   * eight waves: the four 128 x 64 wave tiles twice, wave group wk multiplying 32-deep slice wk of every 64-deep
//     chunk (two waves per SIMD from ONE workgroup; the halves are added through LDS at the end);
//   * four A stages (three for 8-bit codes, whose B stages are twice as large): the DMA of chunk c + 3 is issued while
//     chunk c is multiplied; two B stages, a superstep's records arrive a chunk before they are needed;
//   * counted waits: s_waitcnt vmcnt(n) leaves the younger chunks' DMAs in flight across the barrier (raw s_barrier —
//     __syncthreads() would drain them).  Per wave a chunk's batch is 4 A requests, an odd chunk's batch also the NB
//     requests of the next superstep's B records; requests retire in order, so before chunk c only the batches younger
//     than the one that carried A(c) — and, before an odd chunk, B(u + 1) — may still be in flight.
constexpr int kG3dThreads = 512;
template <int KIND, int SPS, int SK, bool ASYM>
__global__ __launch_bounds__(kG3dThreads, 1) void gemm3d_kernel(const Gemm2Params p) {
  constexpr bool B8 = KIND == WK_INT8;
  constexpr int NJ = B8 ? 2 : 4;
  constexpr int RPS = B8 ? 2 : 1;
  constexpr int SBYTES = SPS * (SK == SK_F32 ? 4 : 2);
  constexpr int NS = B8 ? 3 : 4;   // A stages
  constexpr int D = NS - 1;        // chunks of A in flight ahead of the one being multiplied
  constexpr int NB = RPS * (2 + (ASYM ? 1 : 0));  // B requests per wave and superstep
  using Corr = CorrRaw<SPS, SK, ASYM>;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  typedef __attribute__((address_space(3))) unsigned char* LdsPtr;

  const int tid = threadIdx.x;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l = tid & 63, nn = l & 15, g = l >> 4;
  const int wk = w >> 2, wm = (w >> 1) & 1, wn = w & 1;
  const int xcd = blockIdx.x & 7, local = blockIdx.x >> 3;
  const int bn = xcd * p.cpx + local % p.cpx, bm = local / p.cpx;
  if (bn >= p.nbn) return;
  const int tile0 = bn * kG3Tiles + wn * 4, row0 = bm * kG3BM;

  const Rsrc rq = make_rsrc(p.codes, p.codes_bytes);
  const Rsrc rs = make_rsrc(p.scales, p.scales_bytes);
  const Rsrc rz = make_rsrc(p.zps, p.zps_bytes);
  const Rsrc ra = make_rsrc(p.a16, uint32_t(p.m) * uint32_t(p.lda16) * 2u);  // rows >= m read as zeros
  const I4Consts i4c = {0x000f000fu, 0x00f000f0u, 0x64006400u};

  floatx4 acc[8][4];
#pragma unroll
  for (int mi = 0; mi < 8; mi++)
#pragma unroll
    for (int ni = 0; ni < 4; ni++) acc[mi][ni] = floatx4{0.f, 0.f, 0.f, 0.f};

  // ---- A: wave w, request i (0..3) covers rows (4 w + i) * 8 .. + 7 of the 256; same XOR image as gemm3_kernel ----
  const uint32_t lrow = uint32_t(l >> 3);
  uint32_t a_voff[2];
#pragma unroll
  for (int par = 0; par < 2; par++)
    a_voff[par] = (uint32_t(row0) + uint32_t(w) * 32u + lrow) * uint32_t(p.lda16) * 2u +
                  ((uint32_t(l & 7) ^ (uint32_t(4 * par) + uint32_t(l >> 4))) << 4);
  const uint32_t a_istride = 8u * uint32_t(p.lda16) * 2u;
  auto issue_a = [&](int c, int stage) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const LdsPtr dst = (LdsPtr)(smem) + stage * kG3StageBytes + (w * 4 + i) * 1024;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, reinterpret_cast<__attribute__((address_space(3))) void*>(dst), 16,
                                               a_voff[i & 1], uint32_t(c) * (kG3KC * 2) + uint32_t(i) * a_istride, 0, 0);
    }
#endif
  };
  // this wave multiplies slice wk of a chunk: fragment of row wm * 128 + mi * 16 + nn, piece (4 wk + g) ^ ((nn >> 1) & 7)
  const uint32_t a_roff = uint32_t(wm * 128 + nn) * 128u + ((uint32_t(4 * wk + g) ^ uint32_t((nn >> 1) & 7)) << 4);

  // ---- B: two stages of {records, scale rows, zero-point rows} of the 8 column tiles; wave w fetches tile w ----
  constexpr uint32_t kBCodes = kG3Tiles * RPS * 1024u;
  constexpr uint32_t kBScal = kG3Tiles * RPS * 16u * SBYTES;
  constexpr uint32_t kBZp = ASYM ? kG3Tiles * RPS * 16u * SPS : 0u;
  constexpr uint32_t kBStage = kBCodes + kBScal + kBZp;
  unsigned char* const b_lds0 = smem + NS * kG3StageBytes;
  const uint32_t btile = uint32_t(bn * kG3Tiles + w);
  const uint32_t s_voff = btile * uint32_t(p.srows) * p.sstride + uint32_t(l) * 16u;  // lanes < SBYTES
  const uint32_t z_voff = btile * uint32_t(p.srows) * p.zstride + uint32_t(l) * 16u;  // lanes < SPS
  auto issue_b = [&](int u) {
#if defined(__HIP_DEVICE_COMPILE__)
    const LdsPtr bs = (LdsPtr)(b_lds0) + (u & 1) * kBStage;
#pragma unroll
    for (int r = 0; r < RPS; r++) {
      const uint32_t s = uint32_t(min(u * RPS + r, p.ksteps - 1));
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rq, reinterpret_cast<__attribute__((address_space(3))) void*>(bs + (w * RPS + r) * 1024), 16,
                                               uint32_t(l) * 16u, (btile * uint32_t(p.ksteps) + s) * p.qstride, 0, 0);
      const uint32_t srow = (s * uint32_t(p.srow_mul)) >> p.srow_shift;
      if (l < SBYTES)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, reinterpret_cast<__attribute__((address_space(3))) void*>(bs + kBCodes + (r * kG3Tiles + w) * (16 * SBYTES)),
                                                 16, s_voff, srow * p.sstride, 0, 0);
      if constexpr (ASYM) {
        if (l < SPS)
          __builtin_amdgcn_raw_ptr_buffer_load_lds(rz, reinterpret_cast<__attribute__((address_space(3))) void*>(bs + kBCodes + kBScal + (r * kG3Tiles + w) * (16 * SPS)),
                                                   16, z_voff, srow * p.zstride, 0, 0);
      }
    }
#endif
  };
  // a wave keeps, per column tile, only the words of ITS two slices of the superstep (t = wk and 2 + wk)
  struct BRec {
    uint32_t q[4][B8 ? 4 : 2];  // 4-bit: words wk, 2 + wk of the record; 8-bit: words 2 wk, 2 wk + 1 of records 0 and 1
    Corr c[4][RPS];
  };
  auto read_b = [&](int u, BRec& b) {
    const unsigned char* bs = b_lds0 + (u & 1) * kBStage;
#pragma unroll
    for (int ni = 0; ni < 4; ni++) {
      const int t = wn * 4 + ni;
#pragma unroll
      for (int r = 0; r < RPS; r++) {
        const unsigned char* rec = bs + (t * RPS + r) * 1024 + l * 16;
        if constexpr (B8) {
          b.q[ni][2 * r + 0] = reinterpret_cast<const uint32_t*>(rec)[2 * wk];
          b.q[ni][2 * r + 1] = reinterpret_cast<const uint32_t*>(rec)[2 * wk + 1];
        } else {
          b.q[ni][0] = reinterpret_cast<const uint32_t*>(rec)[wk];
          b.q[ni][1] = reinterpret_cast<const uint32_t*>(rec)[2 + wk];
        }
        const unsigned char* sp = bs + kBCodes + ((r * kG3Tiles + t) * 16 + nn) * SBYTES;
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
          const unsigned char* zp = bs + kBCodes + kBScal + ((r * kG3Tiles + t) * 16 + nn) * SPS;
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
  // B fragments of this wave's slice of chunk h (0 / 1) of the superstep in `b`
  auto dequant = [&](const BRec& b, auto hc, half8_t (&bf)[4]) {
    constexpr int h = decltype(hc)::value;
#pragma unroll
    for (int ni = 0; ni < 4; ni++) {
      float sc[4], zp[4];
      corr_decode<SPS, SK, ASYM, NJ>(b.c[ni][B8 ? h : 0], sc, zp);
      // slice inside its record: 4-bit t = 2 h + wk; 8-bit wk.  wk is wave-uniform but not a compile-time constant:
      // select with it instead of indexing
      const float s_sel = B8 ? (wk ? sc[1] : sc[0]) : (wk ? sc[2 * h + 1] : sc[2 * h]);
      const float z_sel = B8 ? (wk ? zp[1] : zp[0]) : (wk ? zp[2 * h + 1] : zp[2 * h]);
      half8_t v;
      if constexpr (KIND == WK_INT4) {
        const _Float16 zl = (_Float16)(-1032.f - z_sel), zh = (_Float16)(-72.f - z_sel);
        v = cvt_i4x8(b.q[ni][h], i4c, half2_t{zl, zl}, half2_t{zh, zh});
      } else if constexpr (KIND == WK_INT8) {
        const _Float16 zo = (_Float16)(-1152.f - z_sel);
        v = cvt_i8x8(b.q[ni][2 * h], b.q[ni][2 * h + 1], half2_t{zo, zo});
      } else {
        v = cvt_f4x8(b.q[ni][h], p.lut);
      }
      const _Float16 sh = (_Float16)(s_sel * p.spre);
      bf[ni] = v * half8_t{sh, sh, sh, sh, sh, sh, sh, sh};
    }
  };
  auto load_af = [&](int stage, half8_t (&af)[8]) {
    const unsigned char* a_lds = smem + stage * kG3StageBytes + a_roff;
#pragma unroll
    for (int mi = 0; mi < 8; mi++) af[mi] = *reinterpret_cast<const half8_t*>(a_lds + mi * (16 * 128));
  };
  auto mma = [&](const half8_t (&af)[8], const half8_t (&bf)[4]) {
#pragma unroll
    for (int mi = 0; mi < 8; mi++)
#pragma unroll
      for (int ni = 0; ni < 4; ni++)
        acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[mi], bf[ni], acc[mi][ni], 0, 0, 0);
  };
  auto wait_vm = [&](auto nc) { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(decltype(nc)::value) : "memory"); };
  using IC0 = std::integral_constant<int, 0>;
  using IC1 = std::integral_constant<int, 1>;

  // chunk range (split-K: an even number of chunks per split)
  const int cbeg = p.ksplit > 1 ? int(blockIdx.y) * p.cps : 0;
  const int cend = p.ksplit > 1 ? min(p.nchunks, cbeg + p.cps) : p.nchunks;
  const int ubeg = cbeg >> 1, uend = (cend + 1) >> 1;

  // ---- prologue: B(first), A(first D chunks); then the first superstep's B is read after a full drain ----
  issue_b(ubeg);
#pragma unroll
  for (int d = 0; d < D; d++)
    if (cbeg + d < cend) issue_a(cbeg + d, d % NS);
  BRec bcur, bnxt;
  half8_t af[8], bfa[4], bfb[4];
  wait_vm(IC0{});
  asm volatile("s_barrier" ::: "memory");
  read_b(ubeg, bcur);
  if (ubeg + 1 < uend) issue_b(ubeg + 1);  // in the steady state B(u + 1) is issued at the top of chunk 2u - 1
  dequant(bcur, IC0{}, bfa);
  if (p.diag >= 5) {  // diagnostics: operands that no longer come from LDS / the dequantiser
    dequant(bcur, IC1{}, bfb);
    load_af(0, af);
  }
  // The B fragments of a chunk are always prepared during the MFMAs of the chunk before it (bfa: even chunks, bfb: odd
  // chunks), so that behind a barrier only the A fragment reads stand in front of the matrix cores; the scheduler is
  // asked to put the fragment reads first and then to alternate MFMAs with the dequantisation's VALU work.
  auto interleave = [&]() {
    __builtin_amdgcn_sched_group_barrier(0x100, 8, 0);  // the 8 A fragment reads
#pragma unroll
    for (int i = 0; i < 32; i++) {
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // 1 MFMA
      __builtin_amdgcn_sched_group_barrier(0x002, 3, 0);  // up to 3 VALU
    }
  };
  // from here on, at the top of chunk c the batches in flight are those issued at the tops of chunks c - 1, c - 2, ...
  for (int u = ubeg; u < uend; u++) {
    const int c0 = 2 * u;
    // ================= even chunk c0 =================
    {
      const int c = c0;
      if (c > cbeg) {
        // A(c) came with the batch of chunk c - D; younger batches: chunk c - 1 (odd: 4 + NB) [and c - 2 (even: 4) when D = 3]
        if (c + D + 2 >= cend) wait_vm(IC0{});  // the last chunks: the younger batches are no longer full ones
        else if constexpr (D == 3) wait_vm(std::integral_constant<int, 8 + NB>{});
        else wait_vm(std::integral_constant<int, 4 + NB>{});
        if (p.diag != 7) asm volatile("s_barrier" ::: "memory");
      }
      if (c + D < cend && p.diag < 4) issue_a(c + D, (c - cbeg + D) % NS);
      __builtin_amdgcn_sched_barrier(0);
      if (p.diag != 3) {
        if (p.diag < 6) load_af((c - cbeg) % NS, af);
        if (p.diag < 5) dequant(bcur, IC1{}, bfb);  // for the odd chunk of this superstep
        mma(af, bfa);
        interleave();
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    // ================= odd chunk c0 + 1 =================
    if (c0 + 1 < cend) {
      const int c = c0 + 1;
      // A(c) and B(u + 1) (batch of chunk c - 2) must have landed; younger: the batch of chunk c - 1 (even: 4 requests)
      if (c + D + 2 >= cend) wait_vm(IC0{});
      else wait_vm(std::integral_constant<int, 4>{});
      if (p.diag != 7) asm volatile("s_barrier" ::: "memory");
      if (c + D < cend && p.diag < 4) issue_a(c + D, (c - cbeg + D) % NS);
      if (u + 2 < uend && p.diag < 4) issue_b(u + 2);
      if (u + 1 < uend) read_b(u + 1, bnxt);
      __builtin_amdgcn_sched_barrier(0);
      if (p.diag != 3) {
        if (p.diag < 6) load_af((c - cbeg) % NS, af);
        if (u + 1 < uend && p.diag < 5) dequant(bnxt, IC0{}, bfa);  // for the even chunk of the next superstep
        mma(af, bfb);
        interleave();
      }
      __builtin_amdgcn_sched_barrier(0);
      bcur = bnxt;
    }
  }

  // ---- the two slice halves are added through LDS: wave group 1 parks its accumulators, group 0 adds them ----
  __syncthreads();
  {
    floatx4* park4 = reinterpret_cast<floatx4*>(smem) + (w & 3) * (32 * 64) + l;
    if (wk == 1) {
#pragma unroll
      for (int mi = 0; mi < 8; mi++)
#pragma unroll
        for (int ni = 0; ni < 4; ni++) park4[(mi * 4 + ni) * 64] = acc[mi][ni];
    }
    __syncthreads();
    if (wk == 0) {
#pragma unroll
      for (int mi = 0; mi < 8; mi++)
#pragma unroll
        for (int ni = 0; ni < 4; ni++) acc[mi][ni] += park4[(mi * 4 + ni) * 64];
    }
    __syncthreads();
  }
  if (wk != 0) return;

  // ---- epilogue of wave group 0: through LDS in whole rows (see gemm3_kernel) ----
  constexpr int kRowF = 68;
  float* park = reinterpret_cast<float*>(smem) + w * (64 * kRowF);
  const int colw = tile0 * 16;
  const bool vec4 = (p.ldc & 3) == 0 && (reinterpret_cast<uintptr_t>(p.c) & 15) == 0 && colw + 64 <= p.n &&
                    (p.ksplit > 1 ? (p.n & 3) == 0 && (reinterpret_cast<uintptr_t>(p.part) & 15) == 0 : true) &&
                    (!p.d || ((p.ldd & 3) == 0 && (reinterpret_cast<uintptr_t>(p.d) & 15) == 0)) &&
                    (!p.c16 || (reinterpret_cast<uintptr_t>(p.c16) & 7) == 0);
  const int epi = p.epilogue;
#pragma unroll
  for (int hh = 0; hh < 2; hh++) {
#pragma unroll
    for (int mi = 0; mi < 4; mi++)
#pragma unroll
      for (int ni = 0; ni < 4; ni++)
#pragma unroll
        for (int r = 0; r < 4; r++) park[(mi * 16 + 4 * g + r) * kRowF + ni * 16 + nn] = acc[4 * hh + mi][ni][r] * p.spost;
    const int rbase = row0 + wm * 128 + hh * 64;
    if (p.diag == 1) continue;
    if (vec4) {
      for (int it = 0; it < 16; it++) {
        const int rl = it * 4 + (l >> 4), row = rbase + rl, col = colw + (l & 15) * 4;
        if (row >= p.m) continue;
        float4 v = *reinterpret_cast<const float4*>(park + rl * kRowF + (l & 15) * 4);
        if (p.ksplit > 1) {
          *reinterpret_cast<float4*>(p.part + (size_t(blockIdx.y) * p.m + row) * p.n + col) = v;
          continue;
        }
        float4 dv = {0.f, 0.f, 0.f, 0.f};
        if (p.d && epi >= 1 && epi <= 3) dv = *reinterpret_cast<const float4*>(p.d + size_t(row) * p.ldd + col);
        v = float4{epi_apply(v.x, dv.x, epi), epi_apply(v.y, dv.y, epi), epi_apply(v.z, dv.z, epi), epi_apply(v.w, dv.w, epi)};
        *reinterpret_cast<float4*>(p.c + size_t(row) * p.ldc + col) = v;
        if (p.c16) {
          typedef _Float16 half4_t __attribute__((ext_vector_type(4)));
          *reinterpret_cast<half4_t*>(p.c16 + size_t(row) * p.ldc + col) =
              half4_t{(_Float16)v.x, (_Float16)v.y, (_Float16)v.z, (_Float16)v.w};
        }
      }
    } else {
      for (int it = 0; it < 64; it++) {
        const int row = rbase + it, col = colw + l;
        if (row >= p.m || col >= p.n) continue;
        float v = park[it * kRowF + l];
        if (p.ksplit > 1) {
          p.part[(size_t(blockIdx.y) * p.m + row) * p.n + col] = v;
          continue;
        }
        const float dv = (p.d && epi >= 1 && epi <= 3) ? p.d[size_t(row) * p.ldd + col] : 0.f;
        v = epi_apply(v, dv, epi);
        p.c[size_t(row) * p.ldc + col] = v;
        if (p.c16) p.c16[size_t(row) * p.ldc + col] = (_Float16)v;
      }
    }
  }
}

template <int KIND, int SPS, int SK, bool ASYM>
static hipError_t launch_gemm3d_k(const Gemm2Params& p, dim3 grid, hipStream_t st) {
  constexpr int rps = KIND == WK_INT8 ? 2 : 1;
  constexpr int ns = KIND == WK_INT8 ? 3 : 4;
  constexpr int sbytes = SPS * (SK == SK_F32 ? 4 : 2);
  const size_t ldsd = size_t(ns) * kG3StageBytes + 2 * size_t(kG3Tiles) * rps * (1024 + 16 * sbytes + (ASYM ? 16 * SPS : 0));
  return gemm2_reduce(launch_lds<gemm3d_kernel<KIND, SPS, SK, ASYM>>(160 * 1024, grid, dim3(kG3dThreads), ldsd, st, p), p, st);
}

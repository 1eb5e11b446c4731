// ns_gemvs.h — what the files of the small-batch streaming kernel share (internal).  ns_gemvs.hip holds gemvs_kernel, gemvs_finalize_kernel
// and their two launch functions.  Host: ns_gemvs_plan.cpp decides a launch (gemvs_plan: a pure function, checked on the CPU by
// tests/test_stream_plan.py), ns_gemvs.cpp reads the tunables, takes scratch and launches what the plan says.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>

#include "ns_common.h"
#include "ns_dev.h"
#include "ns_gemv.h"

namespace ns {

#ifndef NS_GVS_PF
#define NS_GVS_PF 2
#endif
constexpr int kGsPF = NS_GVS_PF;        // records each streaming wave keeps in flight (with up to 15 waves per CU; deeper
                                        // rings measured no faster from 12 waves on and cost LDS, profiles/r04b_ablation.txt)
constexpr int kGsR = 2;                 // reduction slots (tiles whose partial sums may be pending in LDS)
constexpr int kGsMaxRows = 16;
constexpr int kGsMaxNS = 15;            // streaming waves (+ the service wave = 16 waves = 1024 threads)
constexpr size_t kGsMaxLds = 160 * 1024;
constexpr uint32_t kGsCtlBytes = 32;    // LDS control words: cnt[kGsR] at 0, done at 16
constexpr uint32_t kGsTblBytes = 32 * 1024;  // f4 pair table: 256 entries x 32 bank copies x 4 B, at LDS offset 0
constexpr uint32_t kGsSpinLimit = 1u << 22;  // polls of an LDS word before a wave gives up (about 0.2 s)
constexpr uint32_t kGsTicketCap = 1u << 16;  // tile units an in-launch split-K finish has tickets for

using GvsMat = GemvMat;  // one matrix of a launch: the same 40 bytes, looked up by index in the kernel-argument segment
static_assert(sizeof(GvsMat) == 40, "GvsMat is addressed by index in the kernel-argument segment");

enum GvsMode { GS_PLAIN = 0, GS_DUAL = 1, GS_MSEG = 2 };

struct GvsParams {
  // ---- hot: the prologue's words ----
  const uint8_t* wb0;
  const uint8_t* wb1;
  const uint8_t* wb2;
  const void* a;            // activations, fp16 [m][lda]
  uint32_t so0, so1, so2;   // scale offsets of the matrices
  uint32_t zo0, zo1, zo2;   // zero-point offsets (asymmetric only)
  uint32_t ks;              // k-steps per tile (whole K)
  uint32_t ksl;             // k-steps per slice
  uint32_t s_log2;          // log2(slices): workgroup b streams slice b & (S - 1) of tile group b >> s_log2
  uint32_t qstride, sstride, zstride;
  uint32_t srows, srow_mul, srow_shift;
  uint32_t tb1, tb2;        // first tile of matrices 1 and 2 of a fused QKV launch (2^32 - 1: absent)
  uint32_t ntiles;          // tile units of the launch (dual: tile pairs)
  uint32_t tg_count;        // tile groups = workgroups per slice; group t streams tiles t, t + tg_count, ...
  uint32_t tiles_base, tiles_rem;  // ntiles = tiles_base * tg_count + tiles_rem
  uint32_t ns;              // streaming waves
  int m, k, lda;
  uint32_t row_stride;      // halves per staged row
  uint32_t ctl_off, red_off, ring_off, ring_stride;
  uint32_t red_wave, red_slot;  // bytes of partial sums per wave / per slot
  uint32_t a_off;           // LDS offset of the staged activations (behind the f4 pair table when there is one)
  uint32_t a_bytes;         // bytes of the staged activations (rows x row_stride halves)
  uint32_t lut16[8];        // f4: the 16 table values as fp16, two per word
  const void* tbl_img;      // f4: the 32 KB pair table as a device image (round 5: fetched by LDS-DMA beside the activations instead of
                            // ~1.4 us of VALU per launch); nullptr: the waves build it (the image did not exist yet at capture time)
  // ---- cold ----
  GvsMat mat[3];
  float* c2;
  const float* d;
  int ldc, ldd, epilogue;
  float* slab;              // split-K: [slice][tile unit][q][64 lanes][4] fp32 partial sums
  uint32_t* tickets;        // split-K finished inside the launch: one counter per tile unit (zero between launches); nullptr:
                            // the partial sums are added by gemvs_finalize_kernel
  uint32_t slab_bytes;
  F4Lut lut;
  F8Consts f8;
#ifdef NS_TRACE
  unsigned long long* trace;
#endif
};

// split-K, second pass: one wave per tile unit adds the slices' partial sums in slice order and applies the epilogue
struct GvsFinParams {
  const float* slab;
  uint32_t slices, ntiles, nq;
  uint32_t tb1, tb2;
  int m;
  GvsMat mat[3];
  float* c2;
  const float* d;
  int ldc, ldd, epilogue;
};

// gemvs_kernel's dynamic LDS, stated once: [f4 pair table | A | control words | kGsR reduction slots | one ring per streaming wave], every
// region 16-byte aligned (a_bytes, red_slot and ring_stride are multiples of 16)
struct GvsLds {
  size_t a_off, ctl_off, red_off, ring_off, bytes;
};
constexpr GvsLds gvs_lds(bool table, size_t a_bytes, size_t red_slot, int ns, size_t ring_stride) {
  const size_t a_off = table ? kGsTblBytes : 0, ctl = a_off + a_bytes, red = ctl + kGsCtlBytes, ring = red + size_t(kGsR) * red_slot;
  return {a_off, ctl, red, ring, ring + size_t(ns) * ring_stride};
}
static_assert(gvs_lds(true, 0, 0, 0, 0).bytes == kGsTblBytes + kGsCtlBytes && gvs_lds(true, 0, 0, 0, 0).bytes < kGsMaxLds, "the fixed regions fit");

// ---- the launch decision as a value (ns_gemvs_plan.cpp) -------------------------------------------------------------------------------------
// Every switch the decision reads.  gvs_knobs() (ns_gemvs.cpp) fills it from ns_hip_set_tuning's atomics and the environment.
struct GvsKnobs {
  int gvs = 1;           // "gvs" / NS_GVS: 0 off, 1 by shape, 2 always from one row, 3 always from two rows
  int gvs_slices = 0;    // "gvs_slices" / NS_GVS_SLICES, "gvs_waves" / NS_GVS_WAVES, "gvs_grid" / NS_GVS_GRID: force the decomposition
  int gvs_waves = 0;     //   (K slices, streaming waves, workgroups; 0 = by shape)
  int gvs_grid = 0;
  int gvs_table = -1;    // "gvs_table" / NS_GVS_TABLE: the f4 pair table -1 by size, 0 never, 1 always
  int gvs_finalize = 1;  // "gvs_finalize" / NS_GVS_FINALIZE: 1 = gemvs_finalize_kernel adds the slices, 0 = the tile's owner inside the launch
  bool table_dma = true; // NS_GVS_TABLE_DMA (A-B runs): the pair table arrives as a device image; the launcher consumes it
};
// What a launch needs; nothing is decided after it.  Null in p and f: what the launcher owns — p.a when `convert`, p.slab / f.slab,
// p.tickets, p.tbl_img, p.trace.
struct GvsPlan {
  hipError_t refusal = hipErrorNotSupported;  // hipSuccess: launch; hipErrorNotSupported: gemv_kernel serves the call
  int kind = 0, sps = 0;                      // the format the kernel is instantiated for (with_format, ns_launch.h)
  uint32_t scale_dt = 0;
  bool asym = false;
  int mode = GS_PLAIN;
  GvsParams p;
  GvsFinParams f;              // of the second launch, when slab_bytes != 0 and the launcher got no tickets
  int grid = 0, nwaves = 0;    // workgroups = tile groups x slices; waves per workgroup = p.ns + the service wave
  size_t lds = 0;              // dynamic LDS bytes (gvs_lds)
  bool convert = false;        // an fp32 -> fp16 pass over A comes first: cvt_bytes of scratch, rows of p.k halves
  size_t cvt_bytes = 0;
  size_t slab_bytes = 0;       // split-K partial sums (0: one slice)
  bool want_tickets = false;   // the in-launch finish: kGsTicketCap zeroed words
  bool want_table_image = false;
  double cost = 0;             // of the chosen candidate, in bytes a workgroup moves
};
// refused: *why says what the call lacks.  cus: the device's compute units.  Pointers are only compared with null and looked at for alignment.
GvsPlan gemvs_plan(const SmallMArgs& a, const GvsKnobs& knobs, int cus, std::string* why);

// ---- launches of a plan (ns_gemvs.hip) --------------------------------------------------------------------------------------------------------
hipError_t launch_gemvs_plan(const GvsPlan& pl, hipStream_t st);      // gemvs_kernel of the plan's format and mode
hipError_t launch_gemvs_finalize(const GvsPlan& pl, hipStream_t st);  // gemvs_finalize_kernel of the plan's mode

}  // namespace ns

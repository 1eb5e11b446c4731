// ns_device_mha.hip — ns_hip_mha_f32_device_layout: attention over the reference device backend's fp32 kv cache, K [batch][heads][n_ctx][head_size],
// V [batch][heads][head_size][n_ctx] (ne_bestla_sycl.cpp:592-880; llama.cpp:241-285 lays the cache out like that).  Three servers, chosen by
// mha_f32_plan (ns_device_plan.h): this library's tuned attention kernels on the fp16 mirror of the cache (ns_route.h; the converters that
// feed the mirror are here), and two kernels that read the fp32 cache itself — mha_f32_split_kernel, the context split over workgroups, and
// mha_f32_kernel, one workgroup per (head, query row, batch): scores, soft-max in LDS, P*V; HBM-bound on the kv stream, written for
// correctness first.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "../../include/ns_bestla.h"
#include "ns_common.h"
#include "ns_device.h"
#include "ns_launch.h"
#include "ns_route.h"
#include "ns_route_op.h"

namespace ns {

// q [batch][seq][heads][hs] (contiguous), k [batch][heads_kv][n_ctx][hs], v [batch][heads_kv][hs][n_ctx], o like q.
// masked: key j is visible to query row iq when j <= iq + (seq_all - seq)  (ne_bestla_sycl.cpp:633-644)
__global__ __launch_bounds__(256) void mha_f32_kernel(const float* q, const float* k, const float* v, float* o, int seq, int seq_all,
                                                      int heads, int heads_kv, int hs, int n_ctx, float scale, int masked) {
  extern __shared__ float sm[];  // [seq_all] scores, then [256] reduction scratch
  float* sc = sm;
  float* red = sm + ((seq_all + 3) & ~3);
  const int ih = blockIdx.x, iq = blockIdx.y, ib = blockIdx.z;
  const int hkv = ih / (heads / heads_kv);
  const int t = threadIdx.x;
  const float* qp = q + ((size_t(ib) * seq + iq) * heads + ih) * hs;
  const float* kp = k + (size_t(ib) * heads_kv + hkv) * size_t(n_ctx) * hs;
  const float* vp = v + (size_t(ib) * heads_kv + hkv) * size_t(hs) * n_ctx;
  const int visible = masked ? min(seq_all, iq + (seq_all - seq) + 1) : seq_all;
  // ---- scores: a quarter-wave (16 lanes) per key, lanes split the head dimension (coalesced 64-byte reads of K) ----
  const int sub = t & 15, grp = t >> 4;  // 16 keys in flight per workgroup pass
  float mx = -INFINITY;
  for (int j0 = 0; j0 < visible; j0 += 16) {
    const int j = j0 + grp;
    float s = 0.f;
    if (j < visible) {
      const float* kr = kp + size_t(j) * hs;
      for (int e = sub; e < hs; e += 16) s += qp[e] * kr[e];
    }
    s += __shfl_xor(s, 1, 64);
    s += __shfl_xor(s, 2, 64);
    s += __shfl_xor(s, 4, 64);
    s += __shfl_xor(s, 8, 64);
    s *= scale;
    if (j < visible) {
      if (sub == 0) sc[j] = s;
      mx = fmaxf(mx, s);
    }
  }
  red[t] = mx;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (t < w) red[t] = fmaxf(red[t], red[t + w]);
    __syncthreads();
  }
  mx = red[0];
  __syncthreads();
  float sum = 0.f;
  for (int j = t; j < visible; j += 256) {
    const float e = expf(sc[j] - mx);
    sc[j] = e;
    sum += e;
  }
  red[t] = sum;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (t < w) red[t] += red[t + w];
    __syncthreads();
  }
  const float inv = 1.f / red[0];
  __syncthreads();
  // ---- P * V: V is [hs][n_ctx]: a quarter-wave per output element walks the keys (coalesced reads along n_ctx) ----
  for (int e0 = 0; e0 < hs; e0 += 16) {
    const int e = e0 + grp;
    float acc = 0.f;
    if (e < hs) {
      const float* vr = vp + size_t(e) * n_ctx;
      for (int j = sub; j < visible; j += 16) acc += sc[j] * vr[j];
    }
    acc += __shfl_xor(acc, 1, 64);
    acc += __shfl_xor(acc, 2, 64);
    acc += __shfl_xor(acc, 4, 64);
    acc += __shfl_xor(acc, 8, 64);
    if (e < hs && sub == 0) o[((size_t(ib) * seq + iq) * heads + ih) * hs + e] = acc * inv;
  }
}

// The same attention with the context split over workgroups (round 4): one workgroup per (128-key range, head, query row) instead
// of one per (head, query row) — at 2048 cached positions the single-workgroup form has 32 workgroups stream 2 MB of fp32 K / V
// each.  Scores: a quarter-wave per key, the lane's DPL = head_size / 16 dims as 16-byte loads, all 8 keys of the quarter-wave
// requested before the first is used; softmax over the range in LDS; P.V: a quarter-wave per head dim walks its 128 keys of the
// TRANSPOSED V (8 consecutive per lane).  Partials (max, sum, unnormalised output) go to a per-stream workspace,
// mha_f32_merge_kernel combines them (one launch more; a single range writes the output itself).  kMhaKS keys per workgroup: ns_device_plan.h.
// stores / loads past every cache (sc0 sc1): partial results cross XCDs inside one launch (as ns_attn_decode.hip st_through / ld_through)
__device__ __forceinline__ void dev_st_through(float* p, float v) {
  __hip_atomic_store(reinterpret_cast<uint32_t*>(p), __builtin_bit_cast(uint32_t, v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ float dev_ld_through(const float* p) {
  return __builtin_bit_cast(float, __hip_atomic_load(reinterpret_cast<const uint32_t*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM));
}
typedef float dfloat4 __attribute__((ext_vector_type(4)));
template <int DPL>
__global__ __launch_bounds__(256) void mha_f32_split_kernel(const float* q, const float* k, const float* v, float* o, float* ws, int nsplit,
                                                            int seq, int seq_all, int heads, int heads_kv, int n_ctx, float scale,
                                                            int masked, const int* __restrict__ kmove, int kdelta, uint32_t* tickets = nullptr,
                                                            _Float16* o16 = nullptr) {
  constexpr int HS = 16 * DPL;
  // replayed device route (ns_common.h Affine): the context length moves with the graph's token counter; the grid and the partials'
  // layout are those of the longest context (nsplit = ranges of n_ctx), ranges past the live length leave at once and the merge
  // (always launched then) reads the live ones only
  if (kmove) {
    seq_all += kdelta * *kmove;
    if (int(blockIdx.x) * kMhaKS >= seq_all) return;
  }
  __shared__ float sc[kMhaKS];
  __shared__ float red[4];
  const int split = blockIdx.x, ih = blockIdx.y, bq = blockIdx.z, ib = bq / seq, iq = bq % seq;
  const int hkv = ih / (heads / heads_kv);
  const int t = threadIdx.x, sub = t & 15, grp = t >> 4, w = t >> 6;
  const float* qp = q + (size_t(bq) * heads + ih) * HS + sub * DPL;
  const float* kp = k + (size_t(ib) * heads_kv + hkv) * size_t(n_ctx) * HS;
  const float* vp = v + (size_t(ib) * heads_kv + hkv) * size_t(HS) * n_ctx;
  const int visible = masked ? min(seq_all, iq + (seq_all - seq) + 1) : seq_all;
  const int j0 = split * kMhaKS, j1 = min(visible, j0 + kMhaKS);
  float* wp = ws + ((size_t(bq) * heads + ih) * nsplit + split) * (2 + HS);
  if (j0 >= j1) {  // a range past this row's causal extent
    if (t == 0) wp[0] = -INFINITY, wp[1] = 0.f;
    return;
  }
  dfloat4 qv[DPL / 4];
#pragma unroll
  for (int c = 0; c < DPL / 4; c++) qv[c] = *reinterpret_cast<const dfloat4*>(qp + 4 * c);
  // ---- scores ----
  dfloat4 kv[kMhaKS / 16][DPL / 4];
#pragma unroll
  for (int i = 0; i < kMhaKS / 16; i++) {
    const int j = min(j0 + grp + 16 * i, j1 - 1);
#pragma unroll
    for (int c = 0; c < DPL / 4; c++) kv[i][c] = *reinterpret_cast<const dfloat4*>(kp + size_t(j) * HS + sub * DPL + 4 * c);
  }
  float mx = -INFINITY;
#pragma unroll
  for (int i = 0; i < kMhaKS / 16; i++) {
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < DPL / 4; c++)
#pragma unroll
      for (int e = 0; e < 4; e++) s += qv[c][e] * kv[i][c][e];
    s += __shfl_xor(s, 1, 64);
    s += __shfl_xor(s, 2, 64);
    s += __shfl_xor(s, 4, 64);
    s += __shfl_xor(s, 8, 64);
    s = j0 + grp + 16 * i < j1 ? s * scale : -INFINITY;
    if (sub == 0) sc[grp + 16 * i] = s;
    mx = fmaxf(mx, s);
  }
#pragma unroll
  for (int off = 16; off < 64; off <<= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
  if ((t & 63) == 0) red[w] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));  // finite: j0 < j1
  float pe = 0.f;
  if (t < kMhaKS) {
    pe = expf(sc[t] - mx);  // exp(-inf) = 0 past the range
    sc[t] = pe;
  }
  float sum = pe;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) sum += __shfl_xor(sum, off, 64);
  __syncthreads();  // red[] read by everybody, sc[] complete
  if ((t & 63) == 0) red[w] = sum;
  // ---- P . V over the transposed V: lane sub takes keys j0 + 8 sub .. + 7 of head dim grp + 16 i ----
  const bool v16 = (n_ctx & 3) == 0 && (reinterpret_cast<uintptr_t>(v) & 15) == 0;
  float pv[8];
#pragma unroll
  for (int e = 0; e < 8; e++) pv[e] = sc[8 * sub + e];
  const int jl = j0 + 8 * sub;
  float part[DPL];
#pragma unroll
  for (int i = 0; i < DPL; i++) {
    const float* vr = vp + size_t(grp + 16 * i) * n_ctx + jl;
    float acc = 0.f;
    if (v16 && jl + 8 <= j1) {
      const dfloat4 a = *reinterpret_cast<const dfloat4*>(vr), b2 = *reinterpret_cast<const dfloat4*>(vr + 4);
#pragma unroll
      for (int e = 0; e < 4; e++) acc += pv[e] * a[e] + pv[4 + e] * b2[e];
    } else {
#pragma unroll
      for (int e = 0; e < 8; e++)
        if (jl + e < j1) acc += pv[e] * vr[e];  // (cache cells past the range are not read: they may hold anything)
    }
    part[i] = acc;
  }
#pragma unroll
  for (int i = 0; i < DPL; i++) {
    float acc = part[i];
    acc += __shfl_xor(acc, 1, 64);
    acc += __shfl_xor(acc, 2, 64);
    acc += __shfl_xor(acc, 4, 64);
    acc += __shfl_xor(acc, 8, 64);
    part[i] = acc;
  }
  __syncthreads();
  const float l = red[0] + red[1] + red[2] + red[3];
  // replayed route with tickets (round 5): no merge launch — the live ranges of a (row, head) draw a self-resetting ticket once their
  // partials are out (stores and loads past the per-XCD L2s), the last one combines them in range order: the sums mha_f32_merge_kernel forms.
  // A single live range (contexts up to 128 keys) writes the output row itself.
  const int live = kmove ? (seq_all + kMhaKS - 1) / kMhaKS : nsplit;  // (seq_all already moved above)
  if (tickets && live == 1) {
    if (sub == 0) {
      float* op = o + (size_t(bq) * heads + ih) * HS;
#pragma unroll
      for (int i = 0; i < DPL; i++) {
        const float y = part[i] / l;
        op[grp + 16 * i] = y;
        if (o16) o16[(size_t(bq) * heads + ih) * HS + grp + 16 * i] = (_Float16)y;
      }
    }
    return;
  }
  if (sub == 0) {
    if (nsplit == 1 && !kmove) {
      float* op = o + (size_t(bq) * heads + ih) * HS;
#pragma unroll
      for (int i = 0; i < DPL; i++) op[grp + 16 * i] = part[i] / l;
    } else if (tickets) {
#pragma unroll
      for (int i = 0; i < DPL; i++) dev_st_through(wp + 2 + grp + 16 * i, part[i]);
      if (t == 0) dev_st_through(wp, mx), dev_st_through(wp + 1, l);
    } else {
#pragma unroll
      for (int i = 0; i < DPL; i++) wp[2 + grp + 16 * i] = part[i];
      if (t == 0) wp[0] = mx, wp[1] = l;
    }
  }
  if (!tickets) return;
  __shared__ uint32_t drawn_s;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  uint32_t* tk = tickets + size_t(bq) * heads + ih;
  if (t == 0) drawn_s = __hip_atomic_fetch_add(tk, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __syncthreads();
  if (drawn_s != uint32_t(live - 1)) return;
  if (t == 0) __hip_atomic_store(tk, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // zero again for the next token
  if (t < HS) {
    const float* wq = ws + (size_t(bq) * heads + ih) * nsplit * (2 + HS);
    float mb = -INFINITY;
    for (int s2 = 0; s2 < live; s2++) mb = fmaxf(mb, dev_ld_through(wq + size_t(s2) * (2 + HS)));
    float lb = 0.f, ab = 0.f;
    for (int s2 = 0; s2 < live; s2++) {
      const float ms = dev_ld_through(wq + size_t(s2) * (2 + HS));
      const float c = ms != -INFINITY ? expf(ms - mb) : 0.f;
      lb += dev_ld_through(wq + size_t(s2) * (2 + HS) + 1) * c;
      if (ms != -INFINITY) ab += dev_ld_through(wq + size_t(s2) * (2 + HS) + 2 + t) * c;
    }
    const float y = ab / lb;
    o[(size_t(bq) * heads + ih) * HS + t] = y;
    if (o16) o16[(size_t(bq) * heads + ih) * HS + t] = (_Float16)y;
  }
}
// one workgroup of head_size threads per (query row, head): combine the ranges' (max, sum, output) in range order
__global__ void mha_f32_merge_kernel(const float* ws, float* o, int nsplit, int hs, int seq_all, const int* __restrict__ kmove, int kdelta, _Float16* o16) {
  const size_t row = blockIdx.x;  // (batch * seq + iq) * heads + head
  const int t = threadIdx.x;
  const float* wp = ws + row * nsplit * (2 + hs);
  if (kmove) nsplit = (seq_all + kdelta * *kmove + kMhaKS - 1) / kMhaKS;  // the live ranges of a layout made for the longest context
  float mb = -INFINITY;
  for (int s2 = 0; s2 < nsplit; s2++) mb = fmaxf(mb, wp[size_t(s2) * (2 + hs)]);
  float lb = 0.f, ab = 0.f;
  for (int s2 = 0; s2 < nsplit; s2++) {
    const float ms = wp[size_t(s2) * (2 + hs)];
    const float c = ms != -INFINITY ? expf(ms - mb) : 0.f;
    lb += wp[size_t(s2) * (2 + hs) + 1] * c;
    if (ms != -INFINITY) ab += wp[size_t(s2) * (2 + hs) + 2 + t] * c;  // (an empty range wrote no output columns)
  }
  const float y = ab / lb;
  o[row * hs + t] = y;
  if (o16) o16[row * hs + t] = (_Float16)y;  // (replayed route: the projection behind it streams fp16 activations)
}

// ---- the fp16 mirror's converters (round 5 made them for prompt-sized calls — the kernels above serve one query row per workgroup, a 1500-token prompt
//      re-read its whole K / V once per row: 184 ms through the reference's unchanged model_eval — round 6 feeds every call shape from them, ns_route.h) ----
// K [heads][n_ctx][hs] fp32 -> fp16 [heads][out_ctx][hs], positions lo .. hi of every head, 4 elements per thread (out_ctx = n_ctx: the mirror)
__global__ void mha_k_to_f16_kernel(const float* __restrict__ k, _Float16* __restrict__ out, int heads, int n_ctx, int out_ctx, int lo, int hi, int hs,
                                    uint32_t* overflow) {
  const size_t per_head = size_t(hi - lo) * hs / 4;
  const size_t gid = size_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (gid >= per_head * heads) return;
  const size_t h = gid / per_head, e = size_t(lo) * hs + (gid - h * per_head) * 4;
  const dfloat4 v = *reinterpret_cast<const dfloat4*>(k + h * size_t(n_ctx) * hs + e);
  typedef _Float16 dhalf4 __attribute__((ext_vector_type(4)));
  if (overflow && fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3]))) > 65504.f)
    __hip_atomic_store(overflow, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  *reinterpret_cast<dhalf4*>(out + h * size_t(out_ctx) * hs + e) = dhalf4{(_Float16)v[0], (_Float16)v[1], (_Float16)v[2], (_Float16)v[3]};
}
// V [heads][hs][n_ctx] fp32 (transposed) -> fp16 [heads][out_ctx][hs], positions lo .. hi: 32 x 32 tiles through LDS (reads run along the positions, writes along the head dims)
__global__ __launch_bounds__(256) void mha_vt_to_f16_kernel(const float* __restrict__ v, _Float16* __restrict__ out, int n_ctx, int out_ctx, int lo, int hi, int hs,
                                                            uint32_t* overflow) {
  __shared__ float tile[32][33];
  const int h = blockIdx.z, j0 = lo + blockIdx.x * 32, d0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  const float* src = v + size_t(h) * hs * n_ctx;
  bool big = false;
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const int d = d0 + ty + 8 * r, j = j0 + tx;
    const float x = (d < hs && j < hi) ? src[size_t(d) * n_ctx + j] : 0.f;
    big = big || fabsf(x) > 65504.f;
    tile[ty + 8 * r][tx] = x;
  }
  if (big && overflow) __hip_atomic_store(overflow, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __syncthreads();
  _Float16* dst = out + size_t(h) * out_ctx * hs;
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const int j = j0 + ty + 8 * r, d = d0 + tx;
    if (j < hi && d < hs) dst[size_t(j) * hs + d] = (_Float16)tile[tx][ty + 8 * r];
  }
}

namespace {
int fail(const char* what) {
  set_error(what);
  return -1;
}
MhaF32Knobs mha_f32_knobs() {
  static const bool no_split = getenv("NS_MHA_NO_SPLIT") != nullptr;
  static const bool inl_off = getenv("NS_MHA_INLAUNCH") && atoi(getenv("NS_MHA_INLAUNCH")) == 0;
  MhaF32Knobs kn;
  kn.kv16 = kv16_enabled(), kn.no_split = no_split, kn.inlaunch_off = inl_off;
  return kn;
}

// mha_f32_split_kernel's one launch: the lane's DPL = head_size / 16 dims
void launch_mha_split(int head_size, dim3 grid, hipStream_t st, const float* q, const float* k, const float* v, float* o, float* ws, int nsplit, int seq,
                      int seq_all, int heads, int heads_kv, int n_ctx, float scale, int masked, const Affine& aff, uint32_t* tickets, _Float16* o16) {
  const auto go = [&](auto dpl) {
    hipLaunchKernelGGL(mha_f32_split_kernel<decltype(dpl)::value>, grid, dim3(256), 0, st, q, k, v, o, ws, nsplit, seq, seq_all, heads, heads_kv, n_ctx, scale,
                       masked, aff.k, int(aff.delta), tickets, o16);
  };
  if (head_size == 64) go(std::integral_constant<int, 4>{});
  else if (head_size == 128) go(std::integral_constant<int, 8>{});
  else go(std::integral_constant<int, 16>{});
}

// the first server: positions the mirror lacks are converted (KvMirrorTable::convert_from), then this library's attention kernels read it
int mha_on_mirror(KvMirrorRec* mir, int slot0, const MhaF32Plan& p, const MhaF32Facts& f, const Affine& aff, const float* dQ, const float* dK, const float* dV,
                  float* dO, float scale, hipStream_t st) {
  const int batch = f.batch, seq = f.seq, seq_all = f.seq_all, heads = f.heads, heads_kv = f.heads_kv, head_size = f.head_size, n_ctx = f.n_ctx;
  _Float16 *k16 = static_cast<_Float16*>(mir->k16) + size_t(slot0) * mir->slot_elems(), *v16 = static_cast<_Float16*>(mir->v16) + size_t(slot0) * mir->slot_elems();
  if (!aff.k) {  // (a replayed step's captured cache writes store into the mirror themselves)
    const int lo = KvMirrorTable::convert_from(mir, slot0, batch, seq, seq_all, f.executing);
    if (lo < seq_all) {
      const int hb = batch * heads_kv, npos = seq_all - lo;
      const size_t units = size_t(hb) * npos * head_size / 4;
      uint32_t* ovf = kvm_overflow_word();
      hipLaunchKernelGGL(mha_k_to_f16_kernel, dim3(unsigned((units + 255) / 256)), dim3(256), 0, st, dK, k16, hb, n_ctx, n_ctx, lo, seq_all, head_size, ovf);
      hipLaunchKernelGGL(mha_vt_to_f16_kernel, dim3(unsigned((npos + 31) / 32), unsigned((head_size + 31) / 32), unsigned(hb)), dim3(256), 0, st, dV, v16,
                         n_ctx, n_ctx, lo, seq_all, head_size, ovf);
      if (hipGetLastError() != hipSuccess) {
        (void)kvm_note_foreign_write(dK, 1);  // (nothing was converted: the mirror starts over)
        return fail("mha_f32: fp16 mirror conversion launch failed");
      }
    }
  }
  attn_fp32_fp16_fp16_fp32_fwd_args_t a;
  memset(&a, 0, sizeof(a));
  a.Q = const_cast<float*>(dQ), a.K = reinterpret_cast<uint16_t*>(k16), a.V = reinterpret_cast<uint16_t*>(v16), a.dst = dO;
  a.Q_sc = a.K_sc = a.V_sc = a.dst_sc = 1.f;
  a.QK_scale = scale;
  a.attn_flags = f.masked ? NS_ATTN_FLAG_IS_CAUSAL : NS_ATTN_FLAG_NONE;
  a.batch_size = batch, a.head_num = heads, a.heads_kv = heads_kv, a.head_size = head_size, a.sl_q = seq, a.sl_kv = seq_all;
  a.step_q_bs = seq * heads * head_size, a.step_q_head_num = head_size, a.step_q_sl = heads * head_size;
  a.step_k_bs = heads_kv * n_ctx * head_size, a.step_k_head_num = n_ctx * head_size, a.step_k_sl = head_size, a.step_k_head_size = 1;
  a.step_v_bs = a.step_k_bs, a.step_v_head_num = a.step_k_head_num, a.step_v_sl = head_size, a.step_v_head_size = 1;
  a.step_dst_bs = a.step_q_bs, a.step_dst_head_num = head_size, a.step_dst_sl = heads * head_size;
  if (aff.k) g_affine.cap = n_ctx, g_affine.inlaunch = p.mirror_inlaunch;  // (launch_attn reads the moving length from g_affine; the cache's capacity bounds it)
  // (an fp16 copy of the output rows for the projection behind the attention: asked for by a replayed plan and by a window's prompt evaluation)
  const int rc = ns_hip_attn_fp32_fp16_fp16_fp32_forward_h(&a, p.mirror_o16 ? g_mha_out16 : nullptr, st);
  g_mha_out16_written = rc == 0 && p.mirror_o16 && g_mha_out16 != nullptr;
  return rc;
}
}  // namespace
}  // namespace ns

extern "C" int ns_hip_mha_f32_device_layout(const float* dQ, const float* dK, const float* dV, float* dO, int batch, int seq, int seq_all, int heads,
                                            int heads_kv, int head_size, int n_ctx, float scale, int masked, void* stream) {
  using namespace ns;
  if (!dQ || !dK || !dV || !dO || batch < 1 || seq < 1 || seq_all < seq || heads < 1 || heads_kv < 1 || heads % heads_kv || head_size < 1 ||
      n_ctx < seq_all)
    return fail("mha_f32: invalid argument");
  if (route_hook(stream)) return route_submit(route_op_mha(dQ, dK, dV, dO, batch, seq, seq_all, heads, heads_kv, head_size, n_ctx, scale, masked));
  if (ns_hip_lazy_flush() != 0) return -1;
  g_mha_out16_written = false;
  const Affine aff = g_affine;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const MhaF32Knobs kn = mha_f32_knobs();
  const auto aligned16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  MhaF32Facts f;
  f.batch = batch, f.seq = seq, f.seq_all = seq_all, f.heads = heads, f.heads_kv = heads_kv, f.head_size = head_size, f.n_ctx = n_ctx, f.masked = masked != 0;
  f.q16 = aligned16(dQ), f.k16 = aligned16(dK), f.v16 = aligned16(dV), f.moving = aff.k != nullptr, f.executing = route_executing();
  if (kn.kv16) {
    attn_shape_t shp;
    memset(&shp, 0, sizeof(shp));
    shp.batch_size = batch, shp.head_num = heads, shp.heads_kv = heads_kv, shp.head_size = head_size, shp.sl_q = seq, shp.sl_kv = seq_all;
    f.attn_supported = bestla_fusion_attn_fp32_fp16_fp16_fp32_support(&shp);
  }
  const MhaF32Plan p = mha_f32_plan(f, kn);

  int slot0 = 0;
  if (KvMirrorRec* mir = p.mirror.offered() ? kvm_get(dK, dV, batch, heads_kv, head_size, n_ctx, &slot0) : nullptr)
    return mha_on_mirror(mir, slot0, p, f, aff, dQ, dK, dV, dO, scale, st);

  if (p.split.error) return fail(p.split.error);
  float* ws = p.split.offered() ? static_cast<float*>(stream_scratch(st, p.partials_bytes, SLOT_MHA_PARTIALS)) : nullptr;
  if (ws) {
    for (int r0 = 0; r0 < seq; r0 += p.chunk) {
      const MhaChunk c = p.chunk_at(r0);
      const float* q_c = dQ + size_t(r0) * heads * head_size;
      float* o_c = dO + size_t(r0) * heads * head_size;
      // (tickets: sized by ns_route.cpp before the capture; without memory for them the merge launch)
      uint32_t* tickets = c.tickets ? static_cast<uint32_t*>(stream_scratch_zeroed(st, kMhaTicketBytes, SLOT_MHA_TICKETS)) : nullptr;
      _Float16* o16 = c.o16 ? static_cast<_Float16*>(g_mha_out16) : nullptr;
      launch_mha_split(head_size, dim3(unsigned(c.ns_c), unsigned(heads), unsigned(batch * c.nr)), st, q_c, dK, dV, o_c, ws, c.ns_c, c.nr, c.sa, heads, heads_kv,
                       n_ctx, scale, masked, aff, tickets, tickets ? o16 : nullptr);
      if (c.merge || (c.tickets && !tickets))
        hipLaunchKernelGGL(mha_f32_merge_kernel, dim3(unsigned(size_t(batch) * c.nr * heads)), dim3(unsigned(head_size)), 0, st, ws, o_c, c.ns_c, head_size, c.sa,
                           aff.k, int(aff.delta), o16);
    }
    return hipGetLastError() == hipSuccess ? 0 : fail("mha_f32: launch failed");
  }

  if (p.whole.error) return fail(p.whole.error);
  if (launch_lds<mha_f32_kernel>(kMhaWholeLds, dim3(heads, seq, batch), dim3(256), p.lds, st, dQ, dK, dV, dO, seq, seq_all, heads, heads_kv, head_size, n_ctx,
                                 scale, masked) != hipSuccess)
    return fail("mha_f32: launch failed, or the LDS limit it needs could not be raised");
  return 0;
}

// ns_moe_router.hip — the router's tail of a Mixtral-style layer on the device: ns_hip_moe_route / ns_hip_moe_route_f, one launch of
// moe_route_kernel, and the fp16 exponential table it looks its soft_max up in (built on the host like the reference's).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <mutex>

#include "ns_api_int.h"
#include "ns_dev.h"
#include "ns_moe.h"

namespace ns {
namespace {
// ---- the router's tail (ns_hip_moe_route): soft_max -> top_k -> get_rows -> sum_rows -> div of the reference graph in one launch ----
// One wave per token row, lane e holds expert e (n_expert <= 64).  The arithmetic is the reference's operation by operation
// (ne_compute_forward_soft_max_f32, ne_layers.c:8887-8954): fp16(x - max) looked up in table_exp_f16, the values summed in double (at most
// 64 fp16 values: exact, so the butterfly's order does not matter), float(1.0 / sum) multiplied in fp32; the selected probabilities summed in
// double in selection order, the sum stored as float (sum_rows) and divided in fp32 (ne_vec_div_f32).  Selection: n_used rounds of a wave-wide
// arg-max on (probability, lower index first) — the reference's std::sort leaves ties unspecified, here the lower expert index wins.
constexpr int kRouteWaves = 4;
__global__ __launch_bounds__(kRouteWaves * 64) void moe_route_kernel(const float* __restrict__ logits, int ld, int m, int n_expert, int n_used,
                                                                     const uint16_t* __restrict__ exp_table, int32_t* __restrict__ ids, int ids_stride,
                                                                     float* __restrict__ weights, int w_stride, float* __restrict__ probs, int raw) {
  const int row = blockIdx.x * kRouteWaves + int(threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= m) return;  // (wave-uniform)
  const bool on = lane < n_expert;
  const float ninf = -__builtin_inff();
  const float x = on ? logits[size_t(row) * ld + lane] : ninf;
  float mx = x;  // ne_vec_max_f32
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float y = __shfl_xor(mx, o, 64);
    mx = y > mx ? y : mx;
  }
  float val = 0.f;
  if (on && x != ninf) {
    const _Float16 h = (_Float16)__fsub_rn(x, mx);  // NE_FP32_TO_FP16: round to nearest even
    val = f16_bits_to_f32(exp_table[__builtin_bit_cast(unsigned short, h)]);
  }
  double sum = double(val);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
  if (mx == ninf) sum = double(n_expert);  // (all logits -inf: the reference's start value; every probability is 0)
  const float inv = float(1.0 / sum);
  const float pr = __fmul_rn(val, inv);  // ne_vec_scale_f32
  if (probs && on) probs[size_t(row) * ld + lane] = pr;
  // top-k: key = (probability bits, 63 - lane) — non-negative floats order like their bits; a NaN (outside the contract) counts as 0,
  // lanes beyond n_expert and lanes already taken as -1, so the ids are distinct and in range whatever the row holds
  long long key = on ? ((long long)(pr != pr ? 0u : (__builtin_bit_cast(uint32_t, pr) & 0x7fffffffu)) << 32) | (long long)(63 - lane) : -1ll;
  int my_id = 0;
  float my_p = 0.f;
  for (int r = 0; r < n_used; r++) {
    long long best = key;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const long long y = __shfl_xor(best, o, 64);
      best = y > best ? y : best;
    }
    const int win = 63 - int(best & 63);
    const float pw = __shfl(pr, win, 64);
    if (lane == r) my_id = win, my_p = pw;
    if (lane == win) key = -1ll;
  }
  double wsum = 0.0;  // sum_rows: double accumulator, in selection order
  for (int r = 0; r < n_used; r++) wsum += double(__shfl(my_p, r, 64));
  const float wsf = float(wsum);
  if (lane < n_used) {
    ids[size_t(row) * ids_stride + lane] = my_id;
    weights[size_t(row) * w_stride + lane] = raw ? my_p : __fdiv_rn(my_p, wsf);  // (raw: grok.cpp:293-299, no sum_rows / div)
  }
}

}  // namespace

// the router's exponential table: table_exp_f16 of the reference (ne_layers.c:745), fp16(expf(fp16 -> fp32(code))) for every code, made by
// the HOST's expf like the reference's and uploaded once per device
static uint16_t f32_to_f16_bits(float f) {  // round to nearest even, subnormals kept (what F16C's conversion and ne_compute_fp32_to_fp16 do)
  uint32_t x;
  memcpy(&x, &f, 4);
  const uint32_t sign = (x >> 16) & 0x8000u;
  x &= 0x7fffffffu;
  if (x >= 0x7f800000u) return uint16_t(sign | (x > 0x7f800000u ? 0x7e00u : 0x7c00u));
  if (x >= 0x477ff000u) return uint16_t(sign | 0x7c00u);  // rounds to 65536 and beyond
  if (x < 0x38800000u) {                                   // below 2^-14: a subnormal half, in units of 2^-24
    if (x < 0x33000000u) return uint16_t(sign);          // below 2^-25: zero (2^-25 itself is a tie to even = zero)
    const int e = int(x >> 23);                           // 102 .. 112
    const uint32_t man = (x & 0x7fffffu) | 0x800000u;     // value = man * 2^(e - 150)
    const int shift = 126 - e;                            // half units: man >> shift
    uint32_t h = man >> shift;
    const uint32_t rem = man & ((1u << shift) - 1u), halfway = 1u << (shift - 1);
    if (rem > halfway || (rem == halfway && (h & 1u))) h++;
    return uint16_t(sign | h);
  }
  uint32_t h = ((x - 0x38000000u) >> 13);
  const uint32_t rem = x & 0x1fffu;
  if (rem > 0x1000u || (rem == 0x1000u && (h & 1u))) h++;
  return uint16_t(sign | h);
}
static float f16_bits_to_f32_host(uint16_t h) {
  const uint32_t sign = uint32_t(h & 0x8000u) << 16, e = (h >> 10) & 31u, man = h & 0x3ffu;
  uint32_t x;
  if (e == 31u) {
    x = sign | 0x7f800000u | (man << 13);
  } else if (e) {
    x = sign | ((e + 112u) << 23) | (man << 13);
  } else {
    float f = float(man) * 5.9604644775390625e-8f;  // man * 2^-24, exact
    memcpy(&x, &f, 4);
    x |= sign;
  }
  float f;
  memcpy(&f, &x, 4);
  return f;
}
static std::mutex g_exp_table_mutex;
static uint16_t* g_exp_table[64];
const uint16_t* moe_exp_table(bool build) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) {
    (void)hipGetLastError();
    set_error("moe_route: no current device for the exponential table");
    return nullptr;
  }
  std::lock_guard<std::mutex> lock(g_exp_table_mutex);
  if (g_exp_table[dev] || !build) return g_exp_table[dev];
  std::vector<uint16_t> host(65536);
  for (uint32_t i = 0; i < 65536u; i++) host[i] = f32_to_f16_bits(expf(f16_bits_to_f32_host(uint16_t(i))));
  uint16_t* d = nullptr;
  if (hipMalloc((void**)&d, host.size() * 2) != hipSuccess || hipMemcpy(d, host.data(), host.size() * 2, hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipGetLastError();
    if (d) (void)hipFree(d);
    set_error("moe_route: allocating the exponential table failed");
    return nullptr;
  }
  g_exp_table[dev] = d;
  return d;
}

}  // namespace ns

using namespace ns;

extern "C" {

int ns_hip_moe_route(const float* dLogits, int ld_logits, int m, int n_expert, int n_used, int32_t* dIds, int ids_stride, float* dWeights,
                     int w_stride, float* dProbs, void* stream) {
  return ns_hip_moe_route_f(dLogits, ld_logits, m, n_expert, n_used, dIds, ids_stride, dWeights, w_stride, dProbs, 0, stream);
}

int ns_hip_moe_route_f(const float* dLogits, int ld_logits, int m, int n_expert, int n_used, int32_t* dIds, int ids_stride, float* dWeights,
                       int w_stride, float* dProbs, int flags, void* stream) {
  if (!have_device()) return -1;
  if (flags & ~NS_MOE_ROUTE_RAW_WEIGHTS) return moe_fail("moe_route: unknown flag bits (NS_MOE_ROUTE_RAW_WEIGHTS is the only flag)");
  if (n_used < 1 || n_used > 8 || n_expert < n_used || n_expert > 64 || m < 1)
    return moe_fail("moe_route: need 1 <= n_used <= 8, n_used <= n_expert <= 64 and at least one row");
  if (!dLogits || !dIds || !dWeights || ld_logits < n_expert || ids_stride < n_used || w_stride < n_used)
    return moe_fail("moe_route: bad argument (null pointer, or a row stride shorter than its row)");
  hipStream_t st = (hipStream_t)stream;
  const bool capturing = stream_is_capturing(st);
  const uint16_t* table = moe_exp_table(!capturing);  // (a synchronous upload: never inside a capture)
  if (!table) {
    if (capturing) set_error("moe_route: the exponential table is not built yet - call ns_hip_warm_up, create an expert group or route once before capturing");
    return -1;
  }
  hipLaunchKernelGGL(moe_route_kernel, dim3(unsigned((m + kRouteWaves - 1) / kRouteWaves)), dim3(kRouteWaves * 64), 0, st, dLogits, ld_logits, m,
                     n_expert, n_used, table, dIds, ids_stride, dWeights, w_stride, dProbs, (flags & NS_MOE_ROUTE_RAW_WEIGHTS) ? 1 : 0);
  return hip_ok(hipGetLastError(), "moe_route launch") ? 0 : -1;
}

}  // extern "C"

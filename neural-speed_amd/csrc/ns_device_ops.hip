// ns_device_ops.hip — the element-wise nodes of the reference's device backend that have kernels of their own: ne's broadcasting add / mul
// over four strided dimensions (ns_hip_binary_nd_f32; ne_bestla_sycl.cpp:174-295) and the lazy norm / silu peephole in front of the multiply
// (ns_hip_lazy_*).  Which kernel, and what a multiply makes of a recorded node: binary_plan / lazy_mul_plan (ns_device_plan.h).
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdlib>

#include "../../include/ns_bestla.h"
#include "ns_common.h"
#include "ns_device.h"
#include "ns_route_op.h"

namespace ns {

struct NdArgs {
  long long ne0[4];      // extents of src0 / dst
  long long nb0[4];      // byte strides of src0
  long long ne1[4];      // extents of src1 (each 1 or ne0[i]: broadcast by modulo, as the reference does)
  long long nb1[4];
  long long nbd[4];
};
__global__ __launch_bounds__(256) void nd_binary_kernel(const char* a, const char* b, char* d, NdArgs g, long long total, int op) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const long long i0 = i % g.ne0[0];
  i /= g.ne0[0];
  const long long i1 = i % g.ne0[1];
  i /= g.ne0[1];
  const long long i2 = i % g.ne0[2];
  const long long i3 = i / g.ne0[2];
  const float x = *reinterpret_cast<const float*>(a + i3 * g.nb0[3] + i2 * g.nb0[2] + i1 * g.nb0[1] + i0 * g.nb0[0]);
  const float y = *reinterpret_cast<const float*>(b + (i3 % g.ne1[3]) * g.nb1[3] + (i2 % g.ne1[2]) * g.nb1[2] + (i1 % g.ne1[1]) * g.nb1[1] +
                                                  (i0 % g.ne1[0]) * g.nb1[0]);
  *reinterpret_cast<float*>(d + i3 * g.nbd[3] + i2 * g.nbd[2] + i1 * g.nbd[1] + i0 * g.nbd[0]) = op ? x * y : x + y;
}

// the common shapes of those nodes — dense tensors of one shape (residual adds, silu(x) * up) or a dense tensor with a row vector (mul by the norm weight) —
// without the per-element index arithmetic: four elements per thread (round 5: a prompt's 192 such launches took 29.7 us each on 1500 x 4096 floats)
__global__ __launch_bounds__(256) void dense_binary_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ d, long long total4,
                                                           int bcols4, int op) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total4) return;
  typedef float nfloat4 __attribute__((ext_vector_type(4)));
  const nfloat4 x = reinterpret_cast<const nfloat4*>(a)[i];
  const nfloat4 y = reinterpret_cast<const nfloat4*>(b)[bcols4 ? i % bcols4 : i];
  reinterpret_cast<nfloat4*>(d)[i] = op ? x * y : x + y;
}

/* ---- lazy peephole of the device route (round 4).  The reference's graph runs node by node: rms_norm, then the multiply by the norm
 * weight; silu(gate), then the multiply by up — four launches per layer that are two.  The glue hands rms_norm and silu to
 * ns_hip_lazy_*; they are RECORDED, not launched.  The next call decides: a multiply that consumes the recorded result (the
 * llama graph always does) runs ONE kernel that writes BOTH tensors — the recorded node's own output and the product, bit for bit
 * what the two kernels write, so every tensor of the graph keeps its contents whatever else reads it; anything else (another
 * operator from the glue, a GEMM, a copy, a synchronisation) first launches the recorded node as it stands (ns_hip_lazy_flush).
 * One recorded node at most; the reference's executor issues device nodes from one thread. ---- */
namespace {
struct LazyNode {
  int kind = 0;  // 0 none, 1 rms norm, 2 silu
  const float* src = nullptr;
  float* dst = nullptr;
  int rows = 0, cols = 0;
  float eps = 0.f;
  size_t n = 0;
  hipStream_t st = nullptr;
};
LazyNode g_lazy;
std::atomic<int> g_lazy_on{-1};  // NS_DEV_LAZY=0: every node launches as it comes (A/B)
bool lazy_on() {
  int v = g_lazy_on.load();
  if (v < 0) {
    const char* e = getenv("NS_DEV_LAZY");
    v = e ? atoi(e) != 0 : 1;
    g_lazy_on.store(v);
  }
  return v != 0;
}
int fail(const char* what) {
  set_error(what);
  return -1;
}
int lazy_flush_impl() {
  const LazyNode n = g_lazy;
  g_lazy.kind = 0;
  hipError_t e = hipSuccess;
  if (n.kind == 1) e = launch_rmsnorm(n.rows, n.cols, true, n.eps, n.src, n.dst, n.st, nullptr, nullptr);
  if (n.kind == 2) e = launch_silu(n.src, n.dst, n.n, n.st);
  return e == hipSuccess ? 0 : fail("device route: launching a deferred node failed");
}
}  // namespace
}  // namespace ns

extern "C" {
using namespace ns;

int ns_hip_lazy_flush(void) { return g_lazy.kind ? lazy_flush_impl() : 0; }
int ns_hip_lazy_rms_norm(int rows, int cols, float eps, const float* dIn, float* dOut, void* stream) {
  if (route_hook(stream)) return route_submit(route_op_rms_norm(dIn, dOut, rows, cols, eps));
  if (ns_hip_lazy_flush() != 0) return -1;
  if (!dIn || !dOut || rows < 0 || cols < 1) return fail("lazy rms_norm: invalid argument");
  if (!rows) return 0;  // no rows: nothing to record, like ns_hip_lazy_silu with n == 0
  g_lazy = LazyNode{1, dIn, dOut, rows, cols, eps, size_t(rows) * cols, static_cast<hipStream_t>(stream)};
  return lazy_on() ? 0 : ns_hip_lazy_flush();
}
int ns_hip_lazy_silu(const float* dSrc, float* dDst, size_t n, void* stream) {
  if (route_hook(stream)) return route_submit(route_op_silu(dSrc, dDst, (long long)n));
  if (ns_hip_lazy_flush() != 0) return -1;
  if (n && (!dSrc || !dDst)) return fail("lazy silu: null argument");
  if (!n) return 0;
  g_lazy = LazyNode{2, dSrc, dDst, 0, 0, 0.f, n, static_cast<hipStream_t>(stream)};
  return lazy_on() ? 0 : ns_hip_lazy_flush();
}
/* the multiply node: fused with the recorded node when it consumes it, else the recorded node first and the plain kernel */
int ns_hip_lazy_mul(const float* dA, const float* dB, float* dDst, const long long ne0[4], const long long nb0[4], const long long ne1[4],
                    const long long nb1[4], const long long nbd[4], void* stream) {
  if (route_hook(stream)) return route_submit(route_op_binary(RK_MUL, dA, dB, dDst, ne0, nb0, ne1, nb1, nbd));
  const LazyNode n = g_lazy;
  LazyNodeFacts nf;
  nf.kind = n.kind, nf.src = n.src, nf.dst = n.dst, nf.cols = n.cols, nf.n = n.n, nf.same_stream = n.st == static_cast<hipStream_t>(stream);
  const LazyMul how = lazy_mul_plan(nf, dA, dB, dDst, ne0, nb0, ne1, nb1, nbd);
  if (how == LAZY_NORM_MUL) {
    g_lazy.kind = 0;
    if (launch_rmsnorm_mul2(n.rows, n.cols, true, n.eps, n.src, n.dst, dB, dDst, n.st) != hipSuccess) return fail("device route: norm . weight launch failed");
    return 0;
  }
  if (how == LAZY_SILU_FIRST || how == LAZY_SILU_SECOND) {
    g_lazy.kind = 0;
    const bool first = how == LAZY_SILU_FIRST;
    if (launch_silu_mul2(n.src, first ? dB : dA, n.dst, dDst, n.n, first ? 1 : 0, n.st) != hipSuccess) return fail("device route: silu . up launch failed");
    return 0;
  }
  if (ns_hip_lazy_flush() != 0) return -1;
  return ns_hip_binary_nd_f32(1, dA, dB, dDst, ne0, nb0, ne1, nb1, nbd, stream);
}

/* ---- kernels behind the tensor-level functions of glue/ne_bestla_hip_device.c ---- */
int ns_hip_binary_nd_f32(int is_mul, const float* dA, const float* dB, float* dDst, const long long ne0[4], const long long nb0[4],
                         const long long ne1[4], const long long nb1[4], const long long nbd[4], void* stream) {
  if (route_hook(stream)) return route_submit(route_op_binary(is_mul ? RK_MUL : RK_ADD, dA, dB, dDst, ne0, nb0, ne1, nb1, nbd));
  if (ns_hip_lazy_flush() != 0) return -1;
  if (!dA || !dB || !dDst) return fail("binary_nd: null argument");
  NdArgs g;
  long long total = 1;
  for (int i = 0; i < 4; i++) {
    g.ne0[i] = ne0[i], g.nb0[i] = nb0[i], g.ne1[i] = ne1[i] > 0 ? ne1[i] : 1, g.nb1[i] = nb1[i], g.nbd[i] = nbd[i];
    total *= ne0[i];
  }
  if (total <= 0) return 0;
  static const bool dense_off = getenv("NS_DENSE_BINARY") && atoi(getenv("NS_DENSE_BINARY")) == 0;  // diagnostics
  const bool aligned16 = ((reinterpret_cast<uintptr_t>(dA) | reinterpret_cast<uintptr_t>(dB) | reinterpret_cast<uintptr_t>(dDst)) & 15) == 0;
  const BinaryPlan p = binary_plan(ne0, nb0, ne1, nb1, nbd, aligned16, dense_off);
  if (p.dense) {
    const long long total4 = total / 4;
    hipLaunchKernelGGL(dense_binary_kernel, dim3(unsigned((total4 + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), dA, dB, dDst, total4, p.bcols4,
                       is_mul ? 1 : 0);
  } else {
    hipLaunchKernelGGL(nd_binary_kernel, dim3(unsigned((total + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), reinterpret_cast<const char*>(dA),
                       reinterpret_cast<const char*>(dB), reinterpret_cast<char*>(dDst), g, total, is_mul ? 1 : 0);
  }
  return hipGetLastError() == hipSuccess ? 0 : fail("binary_nd: launch failed");
}
}  // extern "C"

// ns_moe_group.hip — moe_pair_sort_kernel: the pair layout and the chunk lists of the block entries' device-grouped pass (ns_moe.cpp:
// ffn_device_grouped), made ON THE DEVICE so that nothing is read back and the pass can be captured.  What it writes is, element for element,
// what moe_chunk_plan (ns_moe_plan.cpp) computes on the host for the same ids: tests/test_gpu_moe_ffn_device.py compares the two.
#include <hip/hip_runtime.h>

#include "ns_moe.h"
#include "ns_moe_plan.h"

namespace ns {
namespace {

// One workgroup, one thread per (token row, selection) pair p = t * n_used + i (P = m * n_used <= kMoeDevMaxPairs).  A stable counting sort by
// expert WITHOUT a histogram and without atomics: every thread counts, over the P keys in LDS, the good pairs of a smaller expert (`below` =
// its group's offset), the pairs of its own expert in front of it (`before` = its rank in the group) and all of its own expert (`same` = the
// group's count).  Its gathered position is below + before — the (row, selection) order inside a group is the thread order, whatever the
// hardware schedules first.  An id outside [0, n_as) has key -1, is in no group and gets pos = -1.
// A chunk list (one per chunk size R: the gate / up launch's and the down launch's) holds, for e ascending and c = 0 .. ceil(count[e] / R) - 1,
// {e, offset[e] + c R, min(R, count[e] - c R)}.  The pair of rank c R of a group is the chunk's HEAD and writes it, at index = heads of
// smaller experts + c: a second pass over the head flags in LDS.  list[0] is the count; the slots behind it, up to the host's bound, read {-1, 0, 0}.
__global__ __launch_bounds__(kMoeDevMaxPairs) void moe_pair_sort_kernel(MoeDevSort a) {
  __shared__ int32_t key[kMoeDevMaxPairs];
  __shared__ uint8_t head[kMoeDevMaxPairs];  // bit 0: head of a gate / up chunk, bit 1: of a down chunk
  const int p = threadIdx.x, P = a.pairs;
  int t = 0, e = -1;
  if (p < P) {
    t = p / a.n_used;
    const int32_t v = a.ids[size_t(t) * a.ids_stride + (p - t * a.n_used)];
    e = (v >= 0 && v < a.n_as) ? v : -1;
    key[p] = e;
  }
  __syncthreads();
  int below = 0, before = 0, same = 0, total = 0;
  for (int q = 0; q < P; q++) {
    const int32_t k = key[q];  // (every lane reads the same word: a broadcast)
    total += k >= 0;
    below += k >= 0 && k < e;
    same += k == e;
    before += k == e && q < p;
  }
  const bool good = p < P && e >= 0;
  const int r_gu = a.r_gu, r_dn = a.r_dn;
  if (p < P) head[p] = good ? uint8_t((before % r_gu == 0 ? 1 : 0) | (before % r_dn == 0 ? 2 : 0)) : uint8_t(0);
  if (p < P) {
    const int j = good ? below + before : -1;
    a.pos[p] = j;
    if (good) a.src_row[j] = t;
    if (p >= total) a.src_row[p] = -1;  // (positions total .. P - 1: written by exactly these threads, the good pairs write below total)
  }
  __syncthreads();
  int heads_gu = 0, heads_dn = 0, first_gu = 0, first_dn = 0;  // heads in all / in the groups of smaller experts
  for (int q = 0; q < P; q++) {
    const int h = head[q];
    const bool smaller = key[q] < e;  // (a head has a good key)
    heads_gu += h & 1;
    heads_dn += h >> 1;
    first_gu += (h & 1) && smaller;
    first_dn += (h >> 1) && smaller;
  }
  auto write = [&](int32_t* list, int R, int slots, int heads, int first, bool is_head) {
    if (p == 0) list[0] = heads;
    if (is_head) {
      const int c = before / R, at = first + c;
      if (at < slots) {  // (always: moe_chunk_slots bounds the heads of every table)
        list[1 + 3 * at] = e;
        list[2 + 3 * at] = below + c * R;
        list[3 + 3 * at] = min(R, same - c * R);
      }
    }
    for (int s = heads + p; s < slots; s += blockDim.x) list[1 + 3 * s] = -1, list[2 + 3 * s] = 0, list[3 + 3 * s] = 0;
  };
  write(a.chunks_gu, r_gu, a.slots_gu, heads_gu, first_gu, good && (head[p] & 1));
  write(a.chunks_dn, r_dn, a.slots_dn, heads_dn, first_dn, good && (head[p] & 2));
}

}  // namespace

hipError_t launch_moe_pair_sort(const MoeDevSort& a, hipStream_t st) {
  if (a.pairs < 1 || a.pairs > kMoeDevMaxPairs || a.n_used < 1 || a.r_gu < 1 || a.r_dn < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(moe_pair_sort_kernel, dim3(1), dim3(unsigned((a.pairs + 63) / 64 * 64)), 0, st, a);
  return hipGetLastError();
}

}  // namespace ns

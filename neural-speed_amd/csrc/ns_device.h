// ns_device.h — what the pieces of the reference's device backend share (internal): ns_device.hip (device, queue, memory, copy and sync
// entries), ns_device_load.cpp (weight load path, bestla_device_f32f32_forward), ns_device_ops.hip (binary nodes, lazy norm / silu
// peephole), ns_device_mha.hip (device-layout attention), ns_device_kvm.cpp (the fp16 kv mirrors: its API for the route is ns_route.h).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/ns_bestla.h"
#include "ns_device_plan.h"

namespace ns {

// what bestla_device_load_storage leaves in the tensor object behind a device-resident BTLA weight
// (ne_layers.c:946-949 reserves bestla_device_storage_size() bytes there).  It starts with a word no BTLA blob can start
// with (a blob's first field is its size, bestla_storage.h:250-317): the host-pointer entry points (_support, forward)
// recognise a blob by that field and refuse this struct instead of parsing it.
struct DeviceStorage {
  uint64_t not_a_blob;  // 0xffffffffffffffff
  uint64_t magic;       // "NSHIPDEV"
  ns_weight* w;
  int n, k;
  uint64_t reserved[4];
};
constexpr uint64_t kDevMagic = 0x564544504948534eull;

struct Device {
  hipStream_t stream;
  int id;
};

// ns_device_load.cpp: completes every pending weight load, if there is one (one synchronisation of the load stream per model)
void finish_pending_loads_if_any();
// ns_device_kvm.cpp: the mirror that holds the `slots` cache slots starting at (dK, dV), made (and older, overlapping ones dropped) when
// there is none; nullptr without device memory for it
KvMirrorRec* kvm_get(const float* dK, const float* dV, int slots, int heads_kv, int hs, int n_ctx, int* slot0);

}  // namespace ns

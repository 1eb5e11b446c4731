// ns_device_kvm.cpp — the fp16 mirrors of the reference's fp32 device kv cache (ns_route.h says why and how they stay coherent): the
// process-wide table (its records and rules: KvMirrorTable, ns_device_plan.h), the device memory of the mirrors, the overflow word and the
// switch.  Not guarded by a mutex: the reference's executor issues device nodes from one thread.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdlib>
#include <cstring>

#include "ns_common.h"
#include "ns_device.h"
#include "ns_route.h"

namespace ns {
namespace {
KvMirrorTable g_table;
uint32_t* g_kvm_overflow = nullptr;
std::atomic<int> g_kv16{-1};

void kvm_drop(KvMirrorRec* m) {
  (void)hipFree(m->k16);
  (void)hipFree(m->v16);
  g_table.erase(m);
}
}  // namespace

KvMirrorRec* kvm_get(const float* dK, const float* dV, int slots, int heads_kv, int hs, int n_ctx, int* slot0) {
  if (KvMirrorRec* m = g_table.lookup(dK, dV, slots, heads_kv, hs, n_ctx, slot0)) return m;
  for (KvMirrorRec* old : g_table.evicted_by(dK, dV, slots, heads_kv, hs, n_ctx)) kvm_drop(old);
  const size_t bytes16 = size_t(slots) * heads_kv * n_ctx * hs * 2;
  void *k16 = nullptr, *v16 = nullptr;
  if (hipMalloc(&k16, bytes16) != hipSuccess || hipMalloc(&v16, bytes16) != hipSuccess) {
    (void)hipGetLastError();
    (void)hipFree(k16);
    return nullptr;
  }
  *slot0 = 0;
  return g_table.add(dK, dV, slots, heads_kv, hs, n_ctx, k16, v16);
}

bool kv16_enabled() {
  int v = g_kv16.load();
  if (v < 0) {
    const char* e = getenv("NS_DEVICE_KV");
    v = (e && (!strcmp(e, "f32") || !strcmp(e, "fp32") || !strcmp(e, "0"))) ? 0 : 1;
    g_kv16.store(v);
  }
  return v != 0;
}
void kv16_set(int on) { g_kv16.store(on < 0 ? -1 : (on != 0)); }
uint32_t* kvm_overflow_word() {
  if (!g_kvm_overflow) {
    if (hipHostMalloc(reinterpret_cast<void**>(&g_kvm_overflow), 64, hipHostMallocDefault) != hipSuccess) {
      (void)hipGetLastError();
      g_kvm_overflow = nullptr;
      return nullptr;
    }
    *g_kvm_overflow = 0;
  }
  return g_kvm_overflow;
}
bool kvm_overflowed() { return g_kvm_overflow && *reinterpret_cast<volatile uint32_t*>(g_kvm_overflow) != 0; }
void kvm_overflow_reset() {
  if (g_kvm_overflow) *reinterpret_cast<volatile uint32_t*>(g_kvm_overflow) = 0;
}
bool kvm_args_for_cell(const void* cell, KvMirrorArgs* out) {
  KvMirrorCell c;
  if (!g_table.args_for_cell(cell, &c)) return false;
  out->base32 = c.base32, out->m16 = static_cast<_Float16*>(c.m16), out->elems = c.elems;
  out->n_ctx = c.n_ctx, out->hs = c.hs, out->transposed = c.transposed, out->overflow = kvm_overflow_word();
  return true;
}
bool kvm_note_foreign_write(const void* dst, size_t bytes) { return g_table.note_foreign_write(dst, bytes); }
void kvm_set_valid(const void* k32, int valid) { g_table.set_valid(k32, valid); }
bool kvm_for_producer(const void* k32, const void* v32, int heads_kv, int hs, int n_ctx, int n_past, int m, _Float16** k16, _Float16** v16) {
  if (!KvMirrorTable::producer_admits(kv16_enabled(), n_ctx, n_past, m)) return false;
  int slot0 = 0;
  KvMirrorRec* mir = kvm_get(static_cast<const float*>(k32), static_cast<const float*>(v32), 1, heads_kv, hs, n_ctx, &slot0);
  if (!mir) return false;
  *k16 = static_cast<_Float16*>(mir->k16) + size_t(slot0) * mir->slot_elems(), *v16 = static_cast<_Float16*>(mir->v16) + size_t(slot0) * mir->slot_elems();
  KvMirrorTable::producer_rows(mir, slot0, n_past, m);
  return true;
}
void kvm_clear() {
  while (KvMirrorRec* m = g_table.newest()) kvm_drop(m);
}

}  // namespace ns

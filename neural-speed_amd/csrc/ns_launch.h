// ns_launch.h — host-side helpers shared by the kernel launchers of libns_hip.so: the ladder from a weight's run-time format to the
// template arguments its kernels are instantiated for, and the launch of a kernel whose dynamic LDS limit has to be raised first.
// No kernel is launched from here on its own account.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "ns_common.h"

namespace ns {

template <int V>
using int_c = std::integral_constant<int, V>;

// The format rule, stated once.  It decides which instantiations of the matrix kernels exist:
//   INT4 and F4 take 4, 2 or 1 scales per k-step record, INT8 and F8 take 2 or 1; any other sps means 1
//   F4 and F8 have no zero points
//   F8 scales are always fp32 (E8M0 shared exponents are expanded at load); elsewhere any scale_dt but fp32 / fp16 means bf16
//   any kind but INT4 / INT8 / F8 means F4
// A launcher that lacks some of these formats refuses them with an if constexpr inside f, so that nothing else is instantiated.

// f(sk_c, asym_c) for the scale type and zero-point presence of a weight of kind KIND; returns what f returns
template <int KIND, class F>
auto with_scales(uint32_t scale_dt, bool asym, F&& f) {
  if constexpr (KIND == WK_F8) {
    return f(int_c<SK_F32>{}, std::false_type{});
  } else {
    auto by_dt = [&](auto asym_c) {
      if (scale_dt == DT_F32) return f(int_c<SK_F32>{}, asym_c);
      if (scale_dt == DT_F16) return f(int_c<SK_F16>{}, asym_c);
      return f(int_c<SK_BF16>{}, asym_c);
    };
    if constexpr (KIND != WK_F4)
      if (asym) return by_dt(std::true_type{});
    return by_dt(std::false_type{});
  }
}

// f(kind_c, sps_c, sk_c, asym_c) for a weight's (kind, sps, scale_dt, asym); returns what f returns
template <class F>
auto with_format(int kind, int sps, uint32_t scale_dt, bool asym, F&& f) {
  auto by_sps = [&](auto kind_c) {
    constexpr int KIND = decltype(kind_c)::value;
    auto scales = [&](auto sps_c) {
      return with_scales<KIND>(scale_dt, asym, [&](auto sk_c, auto asym_c) { return f(kind_c, sps_c, sk_c, asym_c); });
    };
    if constexpr (!kind_is_8bit(KIND))
      if (sps == 4) return scales(int_c<4>{});
    if (sps == 2) return scales(int_c<2>{});
    return scales(int_c<1>{});
  };
  switch (kind) {
    case WK_INT4: return by_sps(int_c<WK_INT4>{});
    case WK_INT8: return by_sps(int_c<WK_INT8>{});
    case WK_F8: return by_sps(int_c<WK_F8>{});
    default: return by_sps(int_c<WK_F4>{});
  }
}

// Launch of a kernel that may need more dynamic LDS than the 64 KiB a kernel gets by default: the limit of Kern is raised to max_lds
// once, at its first launch (Kern is a template argument, so the static below is per kernel).  If raising it failed, a launch that needs
// more than 64 KiB returns that error; one that fits is launched all the same (the failed call's error is taken off the thread's
// last-error slot at once, so that it is not reported for the launch).
template <auto Kern, class... A>
hipError_t launch_lds(int max_lds, dim3 grid, dim3 block, size_t lds, hipStream_t st, const A&... args) {
  static const hipError_t attr = [max_lds] {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kern), hipFuncAttributeMaxDynamicSharedMemorySize, max_lds);
    if (e != hipSuccess) (void)hipGetLastError();
    return e;
  }();
  if (attr != hipSuccess && lds > 64 * 1024) return attr;
  hipLaunchKernelGGL(Kern, grid, block, lds, st, args...);
  return hipGetLastError();
}
// a kernel as a type: what a generic lambda takes so that it can hand the kernel on to launch_lds as a template argument
template <auto Kern>
struct kernel_c {
  static constexpr auto value = Kern;
};

}  // namespace ns

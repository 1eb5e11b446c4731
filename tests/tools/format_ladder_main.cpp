// Program of tests/test_format_ladder.py: prints the template arguments with_format (neural-speed_amd/csrc/ns_launch.h) hands over for
// every combination of a weight's run-time format, one line each:  <kind> <sps> <scale_dt> <asym> -> <KIND> <SPS> <SK> <ASYM>
// Host code only: no HIP call is made.
#include <cstdio>

#include "ns_launch.h"

int main() {
  using namespace ns;
  const char* kind_name[] = {"INT4", "INT8", "F4", "F8"};  // enum WKind
  const char* sk_name[] = {"BF16", "F16", "F32"};          // enum ScaleKind
  const int kinds[] = {WK_INT4, WK_INT8, WK_F4, WK_F8};
  const int spss[] = {1, 2, 3, 4, 8};
  const struct {
    uint32_t dt;
    const char* name;
  } dts[] = {{DT_F32, "F32"}, {DT_F16, "F16"}, {DT_BF16, "BF16"}, {DT_F8_E8M0, "OTHER"}};
  for (int kind : kinds)
    for (int sps : spss)
      for (const auto& dt : dts)
        for (int asym = 0; asym < 2; asym++)
          with_format(kind, sps, dt.dt, asym != 0, [&](auto kind_c, auto sps_c, auto sk_c, auto asym_c) {
            printf("%s %d %s %d -> %s %d %s %d\n", kind_name[kind], sps, dt.name, asym, kind_name[kind_c()], int(sps_c()), sk_name[sk_c()],
                   int(asym_c()));
          });
  return 0;
}

// Prints what sup3r_amd/csrc/launch_shape.h computes for the inputs of
// tests/test_launch_shape_cpu.py, one result per line:
//   grid_for <n> <num_cu> <per_cu> <result>
//   persistent <min1> <slots> <items> <result>
//   tiles <N> <o0> <o1> <o2> <T> <t0> <t1> <t2> <total>
//   tiles2d <N> <o0> <o1> <T> <t0> <t1> <t2> <total>
// Plain C++17, no HIP:  g++ -std=c++17 -I sup3r_amd/csrc tests/launch_shape_main.cpp
#include <cstdio>
#include <initializer_list>

#include "launch_shape.h"

int main() {
  std::printf("block %d\n", kBlock);
  for (int num_cu : {256, 1})
    for (int per_cu : {8, 16}) {
      const int64_t cap = (int64_t)num_cu * per_cu;
      const int64_t ns[] = {0, 1, 255, 256, 257, cap * 256 - 1, cap * 256, cap * 256 + 1, (int64_t)1 << 40};
      for (int64_t n : ns)
        std::printf("grid_for %lld %d %d %d\n", (long long)n, num_cu, per_cu, grid_for(n, num_cu, per_cu));
    }
  // the default of per_cu
  std::printf("grid_for_default %d %d\n", grid_for((int64_t)1 << 40, 256), grid_for((int64_t)1 << 40, 1));
  for (int slots : {0, 1, 256})
    for (int items : {0, 1, 255, 256, 257}) {
      std::printf("persistent 0 %d %d %d\n", slots, items, persistent_grid(slots, items));
      std::printf("persistent 1 %d %d %d\n", slots, items, persistent_grid_min1(slots, items));
    }
  for (int T : {2, 4, 16})
    for (int N : {1, 3}) {
      const int ext[] = {1, T - 1, T, T + 1};
      for (int o0 : ext)
        for (int o1 : ext) {
          for (int o2 : ext) {
            const TileCounts tc = tile_counts(N, o0, T, o1, T, o2, T);
            std::printf("tiles %d %d %d %d %d %d %d %d %d\n", N, o0, o1, o2, T, tc.t0, tc.t1, tc.t2, tc.total);
          }
          const TileCounts tc = tile_counts(N, o0, T, o1, T);
          std::printf("tiles2d %d %d %d %d %d %d %d %d\n", N, o0, o1, T, tc.t0, tc.t1, tc.t2, tc.total);
        }
    }
  return 0;
}

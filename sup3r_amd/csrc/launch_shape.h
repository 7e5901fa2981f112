// Host arithmetic of launch shapes: how many workgroups a pass gets.  The one
// definition of each; no HIP, no s3_ctx (a plain C++ compiler compiles this
// header alone: tests/launch_shape_main.cpp).  common.h includes it.
#pragma once
#include <stdint.h>

// threads per workgroup of the streaming (grid-stride) passes
constexpr int kBlock = 256;

// grid of a grid-stride pass over n threads' worth of work: ceil(n / kBlock)
// blocks, at most per_cu per CU, at least 1
inline int grid_for(int64_t n, int num_cu, int per_cu = 8) {
  int64_t b = (n + kBlock - 1) / kBlock;
  const int64_t cap = (int64_t)num_cu * per_cu;
  if (b > cap) b = cap;
  if (b < 1) b = 1;
  return (int)b;
}

// tiles of a tiled launch: per axis, and in all (their product times N)
struct TileCounts {
  int t0, t1, t2;
  int total;
};

// extents o* (ConvGeom::O) in tiles of e*; a 2-D tiling leaves the third axis out
inline TileCounts tile_counts(int N, int o0, int e0, int o1, int e1, int o2 = 1, int e2 = 1) {
  TileCounts tc;
  tc.t0 = (o0 + e0 - 1) / e0;
  tc.t1 = (o1 + e1 - 1) / e1;
  tc.t2 = (o2 + e2 - 1) / e2;
  tc.total = N * tc.t0 * tc.t1 * tc.t2;
  return tc;
}

// grid of a persistent kernel: `slots` workgroups (num_cu / channel tiles),
// raised to 1, then limited to the n_items they share: 0 for no items
inline int persistent_grid(int slots, int n_items) {
  int grid = slots < 1 ? 1 : slots;
  if (grid > n_items) grid = n_items;
  return grid;
}

// ... the two clamps the other way round (the weights-stationary 2-D convs):
// 1 for no items
inline int persistent_grid_min1(int slots, int n_items) {
  int grid = slots > n_items ? n_items : slots;
  return grid < 1 ? 1 : grid;
}

// What the kernels over the arena of cropped masks share (measure.hip, skeleton.hip): the mapping of blocks to ME_CHUNK-pixel
// chunks of a crop through the groups table's block0 column, and the check of that table on its host copy before any launch.
#pragma once
#include "common.h"
#include "runtime.h"

namespace {

constexpr int ME_T = 256;
constexpr int ME_PX = 4;
constexpr int ME_CHUNK = ME_T * ME_PX;      // = disyolo_tile_compose_blocks' chunk (checked in measure_tables)
constexpr int ME_SIDE = 32767;              // the largest box side: 2 * ME_SIDE^2 < 2^31

struct Crop {
  int g, bh, bw, area, p0;     // the group, its box, and the first pixel of this block's chunk
  size_t off;                  // the crop's first element in the arena's layout
};

// the last group whose first block is <= this block (groups without pixels own no block)
__device__ __forceinline__ Crop crop_of_block(const int* groups, int G) {
  int lo = 0, hi = G - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (groups[mid * 8 + 6] <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
  }
  const int* g = groups + lo * 8;
  Crop c;
  c.g = lo, c.bh = g[4] - g[2], c.bw = g[5] - g[3];
  c.area = c.bh * c.bw;
  c.p0 = ((int)blockIdx.x - g[6]) * ME_CHUNK;
  c.off = (size_t)g[7] * 16;
  return c;
}

__device__ __forceinline__ long long wave_sum_ll(long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}

// ---- the tables, checked on their host copy before any launch --------------------------------------------------------------
// what every entry point requires of groups [G,8] (columns 2..7 are read): a box with sides in 0 .. ME_SIDE, block0 = the sum
// of disyolo_tile_compose_blocks over the groups before, and crops that lie in the arena in table order without overlap
int measure_tables(const char* who, const int32_t* groups_host, int G, int64_t arena_bytes, int64_t* blocks_out, int* max_bw) {
  int64_t blocks = 0, end = 0;
  int widest = 0;
  for (int gi = 0; gi < G; ++gi) {
    const int32_t* g = groups_host + (size_t)gi * 8;
    const int64_t bh = (int64_t)g[4] - g[2], bw = (int64_t)g[5] - g[3];
    DY_REQUIRE(bh >= 0 && bw >= 0 && bh <= ME_SIDE && bw <= ME_SIDE,
               "%s: group %d: a box of %lld x %lld (the sides must be in 0 .. %d)", who, gi, (long long)bh, (long long)bw, ME_SIDE);
    const int64_t area = bh * bw;
    DY_REQUIRE(g[6] == blocks, "%s: group %d: block0 is %d, the plan gives %lld (disyolo_tile_compose_blocks)", who, gi, g[6],
               (long long)blocks);
    DY_REQUIRE(g[7] >= 0 && (int64_t)g[7] * 16 >= end && (int64_t)g[7] * 16 + area <= arena_bytes,
               "%s: group %d: its crop at %lld does not lie behind the one before it and inside the arena of %lld bytes", who, gi,
               (long long)g[7] * 16, (long long)arena_bytes);
    end = (int64_t)g[7] * 16 + area;
    blocks += disyolo_tile_compose_blocks(area);
    DY_REQUIRE(blocks < (1ll << 31), "%s: too many pixels for one launch", who);
    if (area > 0 && bw > widest) widest = (int)bw;
  }
  *blocks_out = blocks;
  if (max_bw) *max_bw = widest;
  return DISYOLO_OK;
}

#define ME_TABLES(who, max_bw)                                                                              \
  DY_REQUIRE(G >= 0 && arena_bytes >= 0, who ": bad args (G = %d, arena_bytes = %lld)", G, (long long)arena_bytes); \
  if (G == 0) return DISYOLO_OK;                                                                            \
  DY_REQUIRE(disyolo_tile_compose_blocks(ME_CHUNK) == 1 && disyolo_tile_compose_blocks(ME_CHUNK + 1) == 2,  \
             who ": the compose plan's chunk is not %d pixels", ME_CHUNK);                                  \
  int64_t blocks = 0;                                                                                       \
  {                                                                                                         \
    const int rc_ = measure_tables(who, groups_host, G, arena_bytes, &blocks, max_bw);                      \
    if (rc_ != DISYOLO_OK) return rc_;                                                                      \
  }                                                                                                         \
  if (blocks == 0) return DISYOLO_OK

}  // namespace

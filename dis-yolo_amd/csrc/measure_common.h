// What the kernels over the arena of cropped masks share (measure.hip, skeleton.hip, trace.hip, shape.hip, outline.hip): the
// mapping of blocks to ME_CHUNK-pixel chunks of a crop through the groups table's block0 column, the small device helpers, the
// layout of a branch row, and the entry points' preamble with the check of the groups table on its host copy before any launch.
// The labelling (union-find, flatten, link merge, row allocation) is in arena_labels.h.
#pragma once
#include "common.h"
#include "runtime.h"

namespace {

constexpr int ME_T = 256;
constexpr int ME_PX = 4;
constexpr int ME_CHUNK = ME_T * ME_PX;      // = disyolo_tile_compose_blocks' chunk (asserted by ME_PLAN)
constexpr int ME_SIDE = 32767;              // the largest box side: 2 * ME_SIDE^2 < 2^31

// a branch row of disyolo_skeleton_rows: SK_ROW int64 words, the last one 0 (skeleton.hip writes it; trace.hip reads n_end and
// n_attach)
constexpr int SK_ROW = 12;
enum { SK_GROUP = 0, SK_ROOT, SK_PX, SK_N_ORTH, SK_N_DIAG, SK_N_END, SK_N_ATTACH, SK_SUM_Q8, SK_MAX_D2, SK_MIN_D2, SK_SPUR };

struct Crop {
  int g, bh, bw, area, p0;     // the group, its box, and the first pixel of this block's chunk
  size_t off;                  // the crop's first element in the arena's layout
};

// the crop of a block of the plan: the last group whose first block is <= it (groups without pixels own no block)
__device__ __forceinline__ Crop crop_of(const int* groups, int G, int block) {
  int lo = 0, hi = G - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (groups[mid * 8 + 6] <= block) lo = mid; else hi = mid - 1;
  }
  const int* g = groups + lo * 8;
  Crop c;
  c.g = lo, c.bh = g[4] - g[2], c.bw = g[5] - g[3];
  c.area = c.bh * c.bw;
  c.p0 = (block - g[6]) * ME_CHUNK;
  c.off = (size_t)g[7] * 16;
  return c;
}
__device__ __forceinline__ Crop crop_of_block(const int* groups, int G) { return crop_of(groups, G, (int)blockIdx.x); }

// the offset of neighbour P(2+k) (N, NE, E, SE, S, SW, W, NW) in a crop of pitch bw
__device__ __forceinline__ int nb_offset(int k, int bw) {
  const int dy = (k == 0 || k == 1 || k == 7) ? -1 : (k >= 3 && k <= 5) ? 1 : 0;
  const int dx = (k >= 1 && k <= 3) ? 1 : (k >= 5) ? -1 : 0;
  return dy * bw + dx;
}

// floor(sqrt(65536 d2)): the half-width in 1/256 px, bit by bit in integers (d2 < 2^31: the root has 24 bits)
__device__ __forceinline__ unsigned isqrt_q8(int d2) {
  const unsigned long long v = (unsigned long long)(unsigned)d2 << 16;
  unsigned r = 0;
  for (int b = 23; b >= 0; --b) {
    const unsigned t = r | 1u << b;
    if ((unsigned long long)t * t <= v) r = t;
  }
  return r;
}

// butterflies over the wave's 64 lanes: every lane gets the result
__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ long long wave_sum_ll(long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ int wave_min_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ long long wave_max_ll(long long v) {
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

// The preamble of every entry point, in the two halves an entry may put checks of its own between (each entry refuses in the
// order it always did): ME_ARGS checks G and arena_bytes; ME_PLAN returns at once without groups, asserts the chunk, checks the
// tables and leaves the plan's `blocks` (and the widest crop where wanted).  Whether zero blocks means "return" or "still zero
// the counters" is the caller's: ME_TABLES is both halves and the return.
#define ME_ARGS(who) \
  DY_REQUIRE(G >= 0 && arena_bytes >= 0, who ": bad args (G = %d, arena_bytes = %lld)", G, (long long)arena_bytes)
#define ME_PLAN(who, max_bw)                                                                                \
  if (G == 0) return DISYOLO_OK;                                                                            \
  DY_REQUIRE(disyolo_tile_compose_blocks(ME_CHUNK) == 1 && disyolo_tile_compose_blocks(ME_CHUNK + 1) == 2,  \
             who ": the compose plan's chunk is not %d pixels", ME_CHUNK);                                  \
  int64_t blocks = 0;                                                                                       \
  {                                                                                                         \
    const int rc_ = measure_tables(who, groups_host, G, arena_bytes, &blocks, max_bw);                      \
    if (rc_ != DISYOLO_OK) return rc_;                                                                      \
  }
#define ME_TABLES(who, max_bw) \
  ME_ARGS(who);                \
  ME_PLAN(who, max_bw)         \
  if (blocks == 0) return DISYOLO_OK

// zero these bytes on the stream, or set the error and return DISYOLO_E_HIP
#define ME_ZERO(who, ptr, bytes, stream)                                                 \
  do {                                                                                   \
    const hipError_t e_ = hipMemsetAsync(ptr, 0, bytes, stream);                         \
    if (e_ != hipSuccess) {                                                              \
      disyolo_set_error(who ": hipMemsetAsync failed: %s", hipGetErrorString(e_));       \
      return DISYOLO_E_HIP;                                                              \
    }                                                                                    \
  } while (0)

}  // namespace

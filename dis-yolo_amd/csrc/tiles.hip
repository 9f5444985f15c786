// Tiled detection: the path around the network for an image larger than the net (dis-yolo_amd/tiles.py).
//
// The reference has no counterpart (calculate_test_map.py:149-176 letter-boxes the whole image to the net's size); the
// definition these kernels are held to is tests/tiles_ref.py.  Four launches per photograph beside the network's replays:
//   tile_gather      uint8 image -> f32 net inputs of a chunk of tiles (the letter box's arithmetic at scale 1)
//   tile_paste_bits  every kept detection's mask pasted into its tile as a BIT plane (paste_bit, one wave ballot per 64 px)
//   tile_seam_counts per candidate pair of instances of two overlapping tiles: |A n R|, |B n R|, |A n B| by popcount
//   tile_compose     per merged group: the OR of its members cropped to its box, and the owner map (integer atomicMax)
// and for tiled evaluation (evaluate.MAP.collect_tiled; defined by tests/tiles_eval_ref.py) one more per photograph:
//   tile_group_counts per (group, ground-truth instance) pair: |mask n gt| over the groups' arena bytes and cropped bit planes
// Every output is an integer or a bit and every sum an integer sum, so nothing depends on the order the lanes land in.
#include <vector>
#include "common.h"
#include "paste_bit.h"
#include "runtime.h"

namespace {

// ---- gather ---------------------------------------------------------------------------------------------------------------
// One thread per 4 consecutive floats of an output row (a row is 3 W floats, W % 32 == 0: 16-byte aligned quads that never
// straddle a row): 4 byte loads, one 16-byte store.  The store stream is the traffic: 12 bytes out per byte in.
__global__ __launch_bounds__(256) void tile_gather_kernel(const unsigned char* rgb, int h, int w, const int* origins, int T, int t0,
                                                          int nt, float* out, int H, int W) {
  const int rq = W * 3 / 4;                                   // quads per row
  const int64_t total = (int64_t)nt * H * rq;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int q = (int)(i % rq);
    const int64_t ry = i / rq;
    const int y = (int)(ry % H), tc = (int)(ry / H);
    const int t = t0 + tc;
    const bool live = t < T;                                  // a tile index at or beyond T is a whole pad tile
    const int y0 = live ? origins[2 * t] : 0, x0 = live ? origins[2 * t + 1] : 0;
    const int sy = y0 + y;
    const bool row_in = live && sy >= 0 && sy < h;
    float v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int e = 4 * q + k;
      const int x = e / 3, c = e - 3 * x;
      const int sx = x0 + x;
      unsigned char b = 127;
      if (row_in && sx >= 0 && sx < w) b = rgb[((size_t)sy * w + sx) * 3 + c];
      v[k] = (float)__ddiv_rn((double)b, 255.0);              // letterbox_kernel's division (detect.hip)
    }
    *reinterpret_cast<float4*>(out + (((size_t)tc * H + y) * W) * 3 + (size_t)4 * q) = make_float4(v[0], v[1], v[2], v[3]);
  }
}

// ---- paste into bit planes ------------------------------------------------------------------------------------------------
// planes[n][y][j] bit i = paste_bit of detection n at tile pixel (y, 32 j + i).  A wave owns 64 consecutive pixels of the
// flattened plane (W % 32 == 0, so each half of them lies in one row and is one word): one lane per pixel, one ballot, two
// word stores.  A crop rect that leaves the map gives an empty plane instead of a read outside the mask.
constexpr int TB_T = 256;

__global__ __launch_bounds__(TB_T) void tile_paste_bits_kernel(const float* masks, int mh, int mw, const int* rects, int H, int W,
                                                               int bpd, unsigned int* planes) {
  const int n = blockIdx.x / bpd;
  const int total = H * W;
  const int i = (blockIdx.x - n * bpd) * TB_T + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const int* r = rects + (size_t)n * 8;
  const bool crop_ok = r[0] >= 0 && r[1] >= 0 && r[2] <= mh && r[3] <= mw;
  bool bit = false;
  if (i < total && crop_ok) {
    const int y = i / W, x = i - y * W;
    bit = paste_bit(masks + (size_t)n * mh * mw, mw, r, y, x) != 0;
  }
  const unsigned long long b = __ballot(bit);
  if ((lane & 31) == 0 && i < total)
    planes[(size_t)n * (total / 32) + i / 32] = lane ? (unsigned int)(b >> 32) : (unsigned int)b;
}

// ---- seam counts ----------------------------------------------------------------------------------------------------------
// One wave per pair (a, b).  R = the two tiles' windows n the image.  The walk is on B's word grid: for B's word j of a row,
// A's 32 bits under it start at A-column s = 32 j + (xb0 - xa0) -- any sign, in general no multiple of 32 -- and come out of
// the funnel shift of A's words floor(s / 32) and floor(s / 32) + 1 by s mod 32; words outside A's plane are zero.  The first
// and the last word of a row are masked to R's columns.
__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(256) void tile_seam_counts_kernel(const int* pairs, int P, const int* inst_tile, const int* origins,
                                                               int h, int w, const unsigned int* planes, int H, int W, int* counts) {
  const int p = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (p >= P) return;                                         // (wave-uniform; the kernel has no barrier)
  const int a = pairs[2 * p], b = pairs[2 * p + 1];
  const int ta = inst_tile[a], tb = inst_tile[b];
  const int ya0 = origins[2 * ta], xa0 = origins[2 * ta + 1], yb0 = origins[2 * tb], xb0 = origins[2 * tb + 1];
  const int WW = W / 32;
  const int ry1 = max(max(ya0, yb0), 0), rx1 = max(max(xa0, xb0), 0);
  const int ry2 = min(min(ya0, yb0) + H, h), rx2 = min(min(xa0, xb0) + W, w);
  int na = 0, nb = 0, ni = 0;
  if (ry2 > ry1 && rx2 > rx1) {
    const int xl1 = rx1 - xb0, xl2 = rx2 - xb0;               // R's columns in B's plane: 0 <= xl1 < xl2 <= W
    const int j1 = xl1 >> 5, nj = ((xl2 - 1) >> 5) - j1 + 1;
    const int d = xb0 - xa0;
    const unsigned int* pa = planes + (size_t)a * H * WW;
    const unsigned int* pb = planes + (size_t)b * H * WW;
    const int items = (ry2 - ry1) * nj;
    for (int it = lane; it < items; it += 64) {
      const int yr = it / nj, j = j1 + (it - yr * nj);
      const int y = ry1 + yr;
      const int lo_bit = max(xl1 - 32 * j, 0), hi_bit = min(xl2 - 32 * j, 32);
      const unsigned int m = (hi_bit == 32 ? 0xffffffffu : ((1u << hi_bit) - 1u)) & ~((1u << lo_bit) - 1u);
      const unsigned int wb = pb[(size_t)(y - yb0) * WW + j];
      const int s = 32 * j + d;
      const int ja = s >> 5, sh = s & 31;
      const unsigned int* ra = pa + (size_t)(y - ya0) * WW;
      const unsigned int lo = (ja >= 0 && ja < WW) ? ra[ja] : 0u;
      const unsigned int hi = (ja + 1 >= 0 && ja + 1 < WW) ? ra[ja + 1] : 0u;
      const unsigned int wa = (unsigned int)((((unsigned long long)hi << 32) | lo) >> sh);
      na += __popc(wa & m);
      nb += __popc(wb & m);
      ni += __popc(wa & wb & m);
    }
  }
  na = wave_sum_i(na);
  nb = wave_sum_i(nb);
  ni = wave_sum_i(ni);
  if (lane == 0) {
    counts[3 * p] = na;
    counts[3 * p + 1] = nb;
    counts[3 * p + 2] = ni;
  }
}

// ---- compose --------------------------------------------------------------------------------------------------------------
// groups[g] = {m0, m1, y1, x1, y2, x2, block0, off16}: members[m0..m1) are the group's instances, the box is in image pixels,
// block0 the first block of the group's TC_CHUNK-pixel chunks, off16 * 16 its offset in the arena.  A block owns TC_CHUNK
// consecutive pixels of the box, a thread TC_PX of them TC_T apart, so that the lanes of a wave write neighbouring bytes of the
// arena and raise neighbouring words of owner: the OR of the members' bits goes to the arena, and a covered pixel raises owner
// to g + 1 (groups are in rank order, so the maximum is the LAST covering group: mask_paste_kernel's rule).
constexpr int TC_T = 256;
constexpr int TC_PX = 4;
constexpr int TC_CHUNK = TC_T * TC_PX;

__global__ __launch_bounds__(TC_T) void tile_compose_kernel(const int* groups, int G, const int* members, const int* inst_tile,
                                                            const int* origins, const unsigned int* planes, int H, int W, int w,
                                                            unsigned char* arena, int* owner) {
  int lo = 0, hi = G - 1;      // the last group whose first block is <= this block
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (groups[mid * 8 + 6] <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
  }
  const int* g = groups + lo * 8;
  const int m0 = g[0], m1 = g[1], y1 = g[2], x1 = g[3], bh = g[4] - y1, bw = g[5] - x1;
  const int64_t area = (int64_t)bh * bw;
  const int64_t chunk0 = ((int64_t)blockIdx.x - g[6]) * TC_CHUNK;
  const int WW = W / 32;
  unsigned char* out = arena + (size_t)g[7] * 16;
#pragma unroll
  for (int k = 0; k < TC_PX; ++k) {
    const int64_t p = chunk0 + k * TC_T + threadIdx.x;
    if (p >= area) break;
    const int y = y1 + (int)(p / bw), x = x1 + (int)(p % bw);
    unsigned int bit = 0;
    for (int mi = m0; mi < m1; ++mi) {
      const int n = members[mi];
      const int t = inst_tile[n];
      const int ly = y - origins[2 * t], lx = x - origins[2 * t + 1];
      if (ly >= 0 && ly < H && lx >= 0 && lx < W) bit |= (planes[((size_t)n * H + ly) * WW + (lx >> 5)] >> (lx & 31)) & 1u;
    }
    if (bit) atomicMax(&owner[(size_t)y * w + x], lo + 1);
    out[p] = (unsigned char)bit;
  }
}

// ---- group counts (tiled evaluation) --------------------------------------------------------------------------------------
// pairs[p] = {g, j, block0}: |mask_g n gt_j|, or with j = -1 the group's own pixel count.  The pair's rectangle is the
// group's box, cut to the ground-truth instance's box when there is one; a block takes GC_CHUNK consecutive pixels of the
// rectangle (row-major), a thread GC_PX of them GC_T apart, so that a wave reads 64 neighbouring bytes of the arena.  The two
// operands need no common alignment: a lane takes its pixel's byte of the group (origin x1_g) and its pixel's bit of the plane
// (origin x1_j, word (x - x1_j) / 32), the wave ballots "both set", and the popcounts are summed: one integer atomic per block.
// A pair gets one block per chunk up to GC_MAX_BLOCKS, which then stride over the chunks: a rectangle the size of the
// photograph still covers the device, but no more than GC_MAX_BLOCKS atomics land on its one count (adds to ONE address run
// at some 90 per microsecond: with a block per chunk a 12-Mpixel box spent its time there, not reading).
constexpr int GC_T = 256;
constexpr int GC_PX = 8;
constexpr int GC_CHUNK = GC_T * GC_PX;
constexpr int GC_MAX_BLOCKS = 1024;

__host__ __device__ inline int group_counts_blocks(int64_t area) {
  if (area <= 0) return 1;
  const int64_t chunks = (area + GC_CHUNK - 1) / GC_CHUNK;
  return chunks < GC_MAX_BLOCKS ? (int)chunks : GC_MAX_BLOCKS;
}

__global__ __launch_bounds__(GC_T) void tile_group_counts_kernel(const int* groups, const unsigned char* arena, const int* gt,
                                                                 const unsigned int* gt_bits, const int* pairs, int P, int* counts) {
  __shared__ int part[GC_T / 64];
  int lo = 0, hi = P - 1;      // the last pair whose first block is <= this block
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (pairs[mid * 3 + 2] <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
  }
  const int* pr = pairs + lo * 3;
  const int* g = groups + (size_t)pr[0] * 8;
  const int j = pr[1];
  const int gy1 = g[2], gx1 = g[3], bw = g[5] - gx1;
  int ry1 = gy1, rx1 = gx1, ry2 = g[4], rx2 = g[5];
  int jy1 = 0, jx1 = 0, pitch = 0;
  const unsigned int* plane = gt_bits;
  if (j >= 0) {
    const int* t = gt + (size_t)j * 8;
    jy1 = t[0], jx1 = t[1], pitch = t[5];
    ry1 = max(ry1, jy1), rx1 = max(rx1, jx1), ry2 = min(ry2, t[2]), rx2 = min(rx2, t[3]);
    plane = gt_bits + (size_t)t[6];
  }
  const int rw = rx2 - rx1;
  const unsigned int area = (ry2 > ry1 && rw > 0) ? (unsigned int)(ry2 - ry1) * (unsigned int)rw : 0u;     // < 2^31 (checked)
  const unsigned int nb = (unsigned int)group_counts_blocks(area);
  const unsigned char* mask = arena + (size_t)g[7] * 16;
  int n = 0;                   // (wave-uniform: every lane holds its wave's count)
  // (block-uniform trip count: every lane reaches every ballot.  chunk * GC_CHUNK < area + nb * GC_CHUNK < 2^31 + 2^21)
  for (unsigned int chunk = (unsigned int)blockIdx.x - (unsigned int)pr[2]; chunk * GC_CHUNK < area; chunk += nb) {
#pragma unroll
    for (int k = 0; k < GC_PX; ++k) {
      const unsigned int p = chunk * GC_CHUNK + k * GC_T + threadIdx.x;
      bool on = false;
      if (p < area) {
        const unsigned int yr = p / (unsigned int)rw;
        const int y = ry1 + (int)yr, x = rx1 + (int)(p - yr * (unsigned int)rw);
        on = mask[(size_t)(y - gy1) * bw + (x - gx1)] != 0;
        if (on && j >= 0) {
          const int c = x - jx1;
          on = (plane[(size_t)(y - jy1) * pitch + (c >> 5)] >> (c & 31)) & 1u;
        }
      }
      n += __popcll(__ballot(on));
    }
  }
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x == 0) {
    int s = 0;
#pragma unroll
    for (int wv = 0; wv < GC_T / 64; ++wv) s += part[wv];
    if (s) atomicAdd(&counts[lo], s);
  }
}

bool net_ok(int H, int W) { return H > 0 && W > 0 && W % 32 == 0; }

bool tiles_ok(const int32_t* origins_host, int T, int H, int W) {
  // an origin this far from zero could not belong to an image that one launch addresses; it keeps every sum below in int32
  for (int t = 0; t < T; ++t)
    for (int k = 0; k < 2; ++k)
      if (origins_host[2 * t + k] < -(1 << 28) || origins_host[2 * t + k] > (1 << 28)) return false;
  return true;
}

}  // namespace

extern "C" int disyolo_tile_gather(const uint8_t* rgb, int image_h, int image_w, const int32_t* origins, int T, int t0, int t1,
                                   float* out, int net_h, int net_w, void* stream) {
  DY_REQUIRE(rgb && origins && out && image_h > 0 && image_w > 0, "tile_gather: bad args");
  DY_REQUIRE(net_ok(net_h, net_w), "tile_gather: the net's width must be a positive multiple of 32 (got %d x %d)", net_h, net_w);
  DY_REQUIRE(T > 0 && t0 >= 0 && t1 > t0, "tile_gather: need T > 0 and 0 <= t0 < t1 (got T = %d, [%d, %d))", T, t0, t1);
  DY_RECORD_OR_RUN([=](void* s) { return disyolo_tile_gather(rgb, image_h, image_w, origins, T, t0, t1, out, net_h, net_w, s); });
  const int64_t total = (int64_t)(t1 - t0) * net_h * (net_w * 3 / 4);
  int64_t grid = (total + 255) / 256;
  if (grid > 256 * 64) grid = 256 * 64;
  hipLaunchKernelGGL(tile_gather_kernel, dim3((int)grid), dim3(256), 0, (hipStream_t)stream, rgb, image_h, image_w,
                     (const int*)origins, T, t0, t1 - t0, out, net_h, net_w);
  DY_CHECK_LAUNCH();
  return DISYOLO_OK;
}

extern "C" int disyolo_tile_paste_bits(const float* masks, int n, int map_h, int map_w, const int32_t* rects, int net_h, int net_w,
                                       uint32_t* planes, void* stream) {
  DY_REQUIRE(n >= 0 && map_h > 0 && map_w > 0, "tile_paste_bits: bad args");
  DY_REQUIRE(net_ok(net_h, net_w), "tile_paste_bits: the net's width must be a positive multiple of 32 (got %d x %d)", net_h,
             net_w);
  DY_REQUIRE((int64_t)net_h * net_w < (1ll << 30), "tile_paste_bits: net too large");
  if (n == 0) return DISYOLO_OK;
  DY_REQUIRE(masks && rects && planes, "tile_paste_bits: null pointer");
  const int bpd = ceil_div((int64_t)net_h * net_w, TB_T);
  DY_REQUIRE((int64_t)n * bpd < (1ll << 31), "tile_paste_bits: too many detections for one launch");
  DY_RECORD_OR_RUN([=](void* s) { return disyolo_tile_paste_bits(masks, n, map_h, map_w, rects, net_h, net_w, planes, s); });
  hipLaunchKernelGGL(tile_paste_bits_kernel, dim3(n * bpd), dim3(TB_T), 0, (hipStream_t)stream, masks, map_h, map_w,
                     (const int*)rects, net_h, net_w, bpd, (unsigned int*)planes);
  DY_CHECK_LAUNCH();
  return DISYOLO_OK;
}

static int tile_seam_counts_run(const int32_t* pairs, int P, const int32_t* inst_tile, const int32_t* origins, int image_h,
                                int image_w, const uint32_t* planes, int net_h, int net_w, int32_t* counts, void* stream) {
  DY_RECORD_OR_RUN([=](void* s) {
    return tile_seam_counts_run(pairs, P, inst_tile, origins, image_h, image_w, planes, net_h, net_w, counts, s);
  });
  hipLaunchKernelGGL(tile_seam_counts_kernel, dim3((P + 3) / 4), dim3(256), 0, (hipStream_t)stream, (const int*)pairs, P,
                     (const int*)inst_tile, (const int*)origins, image_h, image_w, (const unsigned int*)planes, net_h, net_w,
                     (int*)counts);
  DY_CHECK_LAUNCH();
  return DISYOLO_OK;
}

extern "C" int disyolo_tile_seam_counts(const int32_t* pairs_host, const int32_t* pairs, int P, const int32_t* inst_tile_host,
                                        const int32_t* inst_tile, int N, const int32_t* origins_host, const int32_t* origins,
                                        int T, int image_h, int image_w, const uint32_t* planes, int net_h, int net_w,
                                        int32_t* counts, void* stream) {
  DY_REQUIRE(P >= 0 && N >= 0 && T > 0 && image_h > 0 && image_w > 0, "tile_seam_counts: bad args");
  DY_REQUIRE(net_ok(net_h, net_w), "tile_seam_counts: the net's width must be a positive multiple of 32 (got %d x %d)", net_h,
             net_w);
  if (P == 0) return DISYOLO_OK;
  DY_REQUIRE(pairs_host && pairs && inst_tile_host && inst_tile && origins_host && origins && planes && counts,
             "tile_seam_counts: null pointer");
  // the host copies are what this call can check: every index the kernel follows
  DY_REQUIRE(tiles_ok(origins_host, T, net_h, net_w), "tile_seam_counts: tile origin out of range");
  for (int i = 0; i < N; ++i)
    DY_REQUIRE(inst_tile_host[i] >= 0 && inst_tile_host[i] < T, "tile_seam_counts: instance %d names tile %d of %d", i,
               inst_tile_host[i], T);
  for (int p = 0; p < P; ++p)
    DY_REQUIRE(pairs_host[2 * p] >= 0 && pairs_host[2 * p] < N && pairs_host[2 * p + 1] >= 0 && pairs_host[2 * p + 1] < N,
               "tile_seam_counts: pair %d = (%d, %d) is out of range (%d instances)", p, pairs_host[2 * p], pairs_host[2 * p + 1], N);
  return tile_seam_counts_run(pairs, P, inst_tile, origins, image_h, image_w, planes, net_h, net_w, counts, stream);
}

extern "C" int disyolo_tile_compose_blocks(int64_t area) { return area <= 0 ? 0 : (int)((area + TC_CHUNK - 1) / TC_CHUNK); }

static int tile_compose_run(const int32_t* groups, int G, int blocks, const int32_t* members, const int32_t* inst_tile,
                            const int32_t* origins, const uint32_t* planes, int net_h, int net_w, int image_h, int image_w,
                            uint8_t* arena, int32_t* owner, void* stream) {
  DY_RECORD_OR_RUN([=](void* s) {
    return tile_compose_run(groups, G, blocks, members, inst_tile, origins, planes, net_h, net_w, image_h, image_w, arena, owner, s);
  });
  if (hipMemsetAsync(owner, 0, (size_t)image_h * image_w * sizeof(int32_t), (hipStream_t)stream) != hipSuccess) {
    disyolo_set_error("tile_compose: hipMemsetAsync failed");
    return DISYOLO_E_HIP;
  }
  if (blocks == 0) return DISYOLO_OK;
  hipLaunchKernelGGL(tile_compose_kernel, dim3(blocks), dim3(TC_T), 0, (hipStream_t)stream, (const int*)groups, G,
                     (const int*)members, (const int*)inst_tile, (const int*)origins, (const unsigned int*)planes, net_h, net_w,
                     image_w, (unsigned char*)arena, (int*)owner);
  DY_CHECK_LAUNCH();
  return DISYOLO_OK;
}

extern "C" int disyolo_tile_compose(const int32_t* groups_host, const int32_t* groups, int G, const int32_t* members_host,
                                    const int32_t* members, int M, const int32_t* inst_tile_host, const int32_t* inst_tile, int N,
                                    const int32_t* origins_host, const int32_t* origins, int T, const uint32_t* planes, int net_h,
                                    int net_w, int image_h, int image_w, uint8_t* arena, int64_t arena_bytes, int32_t* owner,
                                    void* stream) {
  DY_REQUIRE(G >= 0 && M >= 0 && N >= 0 && T > 0 && image_h > 0 && image_w > 0 && owner, "tile_compose: bad args");
  DY_REQUIRE(net_ok(net_h, net_w), "tile_compose: the net's width must be a positive multiple of 32 (got %d x %d)", net_h, net_w);
  DY_REQUIRE((int64_t)image_h * image_w < (1ll << 31), "tile_compose: image too large");
  int64_t blocks = 0;
  if (G > 0) {
    DY_REQUIRE(groups_host && groups && members_host && members && inst_tile_host && inst_tile && origins_host && origins &&
                   planes && arena, "tile_compose: null pointer");
    DY_REQUIRE(tiles_ok(origins_host, T, net_h, net_w), "tile_compose: tile origin out of range");
    for (int i = 0; i < N; ++i)
      DY_REQUIRE(inst_tile_host[i] >= 0 && inst_tile_host[i] < T, "tile_compose: instance %d names tile %d of %d", i,
                 inst_tile_host[i], T);
    for (int i = 0; i < M; ++i)
      DY_REQUIRE(members_host[i] >= 0 && members_host[i] < N, "tile_compose: member %d = %d is out of range (%d instances)", i,
                 members_host[i], N);
    for (int gi = 0; gi < G; ++gi) {
      const int32_t* g = groups_host + (size_t)gi * 8;
      DY_REQUIRE(g[0] >= 0 && g[0] <= g[1] && g[1] <= M, "tile_compose: group %d: members [%d, %d) of %d", gi, g[0], g[1], M);
      DY_REQUIRE(g[2] >= 0 && g[2] <= g[4] && g[4] <= image_h && g[3] >= 0 && g[3] <= g[5] && g[5] <= image_w,
                 "tile_compose: group %d: box (%d, %d, %d, %d) leaves the %d x %d image", gi, g[2], g[3], g[4], g[5], image_h,
                 image_w);
      const int64_t area = (int64_t)(g[4] - g[2]) * (g[5] - g[3]);
      DY_REQUIRE(g[6] == blocks, "tile_compose: group %d: block0 is %d, the plan gives %lld (disyolo_tile_compose_blocks)", gi,
                 g[6], (long long)blocks);
      DY_REQUIRE(g[7] >= 0 && (int64_t)g[7] * 16 + (area + 15) / 16 * 16 <= arena_bytes,
                 "tile_compose: group %d does not fit the arena of %lld bytes", gi, (long long)arena_bytes);
      blocks += disyolo_tile_compose_blocks(area);
      DY_REQUIRE(blocks < (1ll << 31), "tile_compose: too many pixels for one launch");
    }
  }
  return tile_compose_run(groups, G, (int)blocks, members, inst_tile, origins, planes, net_h, net_w, image_h, image_w, arena, owner,
                          stream);
}

extern "C" int disyolo_tile_group_counts_blocks(int64_t area) { return group_counts_blocks(area); }

static int tile_group_counts_run(const int32_t* groups, const uint8_t* arena, const int32_t* gt, const uint32_t* gt_bits,
                                 const int32_t* pairs, int P, int blocks, int32_t* counts, void* stream) {
  DY_RECORD_OR_RUN([=](void* s) { return tile_group_counts_run(groups, arena, gt, gt_bits, pairs, P, blocks, counts, s); });
  if (hipMemsetAsync(counts, 0, (size_t)P * sizeof(int32_t), (hipStream_t)stream) != hipSuccess) {
    disyolo_set_error("tile_group_counts: hipMemsetAsync failed");
    return DISYOLO_E_HIP;
  }
  hipLaunchKernelGGL(tile_group_counts_kernel, dim3(blocks), dim3(GC_T), 0, (hipStream_t)stream, (const int*)groups,
                     (const unsigned char*)arena, (const int*)gt, (const unsigned int*)gt_bits, (const int*)pairs, P,
                     (int*)counts);
  DY_CHECK_LAUNCH();
  return DISYOLO_OK;
}

extern "C" int disyolo_tile_group_counts(const int32_t* groups_host, const int32_t* groups, int G, const uint8_t* arena,
                                         int64_t arena_bytes, const int32_t* gt_host, const int32_t* gt, int ng,
                                         const uint32_t* gt_bits, int64_t gt_words, const int32_t* pairs_host,
                                         const int32_t* pairs, int P, int image_h, int image_w, int32_t* counts, void* stream) {
  DY_REQUIRE(G >= 0 && ng >= 0 && P >= 0 && image_h > 0 && image_w > 0 && arena_bytes >= 0 && gt_words >= 0,
             "tile_group_counts: bad args");
  DY_REQUIRE((int64_t)image_h * image_w < (1ll << 31), "tile_group_counts: image too large");
  if (P == 0 || G == 0) return DISYOLO_OK;
  DY_REQUIRE(groups_host && groups && arena && pairs_host && pairs && counts, "tile_group_counts: null pointer");
  DY_REQUIRE(ng == 0 || (gt_host && gt && (gt_bits || gt_words == 0)), "tile_group_counts: null pointer");
  // the host copies are what this call can check: every index and offset the kernel follows
  for (int gi = 0; gi < G; ++gi) {
    const int32_t* g = groups_host + (size_t)gi * 8;
    DY_REQUIRE(g[2] >= 0 && g[2] <= g[4] && g[4] <= image_h && g[3] >= 0 && g[3] <= g[5] && g[5] <= image_w,
               "tile_group_counts: group %d: box (%d, %d, %d, %d) leaves the %d x %d image", gi, g[2], g[3], g[4], g[5], image_h,
               image_w);
    const int64_t area = (int64_t)(g[4] - g[2]) * (g[5] - g[3]);
    DY_REQUIRE(g[7] >= 0 && (int64_t)g[7] * 16 + area <= arena_bytes,
               "tile_group_counts: group %d does not fit the arena of %lld bytes", gi, (long long)arena_bytes);
  }
  for (int j = 0; j < ng; ++j) {
    const int32_t* t = gt_host + (size_t)j * 8;
    DY_REQUIRE(t[0] >= 0 && t[0] <= t[2] && t[2] <= image_h && t[1] >= 0 && t[1] <= t[3] && t[3] <= image_w,
               "tile_group_counts: ground truth %d: box (%d, %d, %d, %d) leaves the %d x %d image", j, t[0], t[1], t[2], t[3],
               image_h, image_w);
    const int64_t rows = t[2] - t[0], need = (t[3] - t[1] + 31) / 32;
    DY_REQUIRE(t[5] >= need && t[6] >= 0 && (int64_t)t[6] + rows * t[5] <= gt_words,
               "tile_group_counts: ground truth %d: pitch %d, offset %d do not hold its %lld x %d box in %lld words", j, t[5],
               t[6], (long long)rows, t[3] - t[1], (long long)gt_words);
  }
  int64_t blocks = 0;
  for (int p = 0; p < P; ++p) {
    const int32_t* pr = pairs_host + (size_t)p * 3;
    DY_REQUIRE(pr[0] >= 0 && pr[0] < G && pr[1] >= -1 && pr[1] < ng,
               "tile_group_counts: pair %d = (%d, %d) is out of range (%d groups, %d ground-truth instances)", p, pr[0], pr[1], G,
               ng);
    const int32_t* g = groups_host + (size_t)pr[0] * 8;
    int64_t rh = g[4] - g[2], rw = g[5] - g[3];
    if (pr[1] >= 0) {
      const int32_t* t = gt_host + (size_t)pr[1] * 8;
      rh = (int64_t)(g[4] < t[2] ? g[4] : t[2]) - (g[2] > t[0] ? g[2] : t[0]);
      rw = (int64_t)(g[5] < t[3] ? g[5] : t[3]) - (g[3] > t[1] ? g[3] : t[1]);
    }
    DY_REQUIRE(pr[2] == blocks, "tile_group_counts: pair %d: block0 is %d, the plan gives %lld (disyolo_tile_group_counts_blocks)",
               p, pr[2], (long long)blocks);
    blocks += disyolo_tile_group_counts_blocks(rh > 0 && rw > 0 ? rh * rw : 0);
    DY_REQUIRE(blocks < (1ll << 31), "tile_group_counts: too many pixels for one launch");
  }
  return tile_group_counts_run(groups, arena, gt, gt_bits, pairs, P, (int)blocks, counts, stream);
}

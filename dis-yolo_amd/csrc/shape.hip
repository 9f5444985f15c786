// The shape of an instance: moment sums, the tight box and the bit quads; the 8-connected parts; the extents along K directions
// (dis-yolo_amd/measure.py, instance_shapes).
//
// The reference has no counterpart; the definition these kernels are held to is tests/shape_ref.py, and everything in it is an
// integer: there is no float in this file.  The kernels read the [G,8] groups table as measure.hip does (measure_common.h): a
// block owns ME_CHUNK consecutive pixels of a crop, every per-pixel buffer lies in the arena's layout, and the elements between
// two crops are never read and never written.  A non-zero byte of the arena is foreground; everything outside a crop is
// background.
//   shape_sums_init     the [G,16] rows: zeros, and (bh, -1, bw, -1) for the tight box
//   shape_sums          per thread n, Sy, Sx, Syy, Sxx, Sxy, the box and the bit quads of the windows its pixels own (a pixel
//                       owns the 2x2 window it is the bottom-right of; the last column, the last row and the corner own the ones
//                       that reach into the ring), over 8 consecutive chunks of the plan; per group among them summed in the wave
//                       by shuffles, over the four waves in LDS, then one atomic per block and column
//   shape_parts_init    labels = the first pixel of the pixel's row run within its wave's 64 pixels (-1 off the foreground),
//                       px = 0
//   shape_parts_merge   the union-find of arena_labels.h over the 8-neighbour foreground: a part ends at its smallest index
//                       whatever the order of arrival.  A pair is merged from its upper (left) pixel, and only where the run
//                       structure does not already join it
//   labels_flatten      labels = the root of every foreground pixel (arena_labels.h)
//   shape_parts_count   px[root] += 1 per foreground pixel, summed per lane, then per wave and root first
//   shape_parts_roots   every root adds 1 to its group's n_parts and takes a max on largest_part_px, per wave first
//   shape_extents_init  the [G,K,2] rows (INT32_MAX, INT32_MIN)
//   shape_extents       the boundary pixels (foreground with a background 4-neighbour) of a block are listed in LDS; thread k
//                       projects the list onto direction k and issues at most two atomics, and none where the group's row
//                       already holds a value as good; a block without a boundary pixel returns at once
// No block waits for another: the retry loops of the merge are lock-free (arena_labels.h).  Integer atomics only: two runs give
// the same bits.
#include "arena_labels.h"

namespace {

constexpr int SH_COLS = 16;          // int64 words of a sums row: n, Sy, Sx, Syy, Sxx, Sxy, ymin, ymax, xmin, xmax, Q1, Q2, Q3, Q4, QD, 0
constexpr int SH_SUMS = 11;          // the columns that are sums, in the order acc[] holds them: 0 .. 5 and 10 .. 14
constexpr int SH_K_MAX = 360;
constexpr int SH_UNIT = 16384;       // a direction's (c, s) is a unit vector in 2^-14: |c x + s y| <= 16384 * 65532 < 2^31
constexpr int SH_WAVES = ME_T / 64;

// ---- sums ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(ME_T) void shape_sums_init_kernel(const int* groups, int G, long long* sums) {
  const int i = blockIdx.x * ME_T + threadIdx.x;
  if (i >= G * SH_COLS) return;
  const int* g = groups + (i / SH_COLS) * 8;
  const int q = i % SH_COLS;
  sums[i] = q == 6 ? g[4] - g[2] : q == 8 ? g[5] - g[3] : (q == 7 || q == 9) ? -1 : 0;
}

// the window with the pixels a b / c d: which of Q1, Q2, Q3, Q4, QD it counts for (none when empty)
__device__ __forceinline__ void quad(unsigned a, unsigned b, unsigned c, unsigned d, int* q) {
  const unsigned s = a + b + c + d;
  q[0] += s == 1, q[1] += s == 2 && a != d, q[2] += s == 3, q[3] += s == 4, q[4] += s == 2 && a == d;
}

struct ShapeAcc {
  long long m[5];                    // Sy, Sx, Syy, Sxx, Sxy
  int n, q[5];                       // n; Q1, Q2, Q3, Q4, QD
  int ymin, ymax, xmin, xmax;
  __device__ __forceinline__ void reset(int bh, int bw) {
    m[0] = m[1] = m[2] = m[3] = m[4] = 0;
    n = q[0] = q[1] = q[2] = q[3] = q[4] = 0;
    ymin = bh, ymax = -1, xmin = bw, xmax = -1;
  }
};

// what the block gathered for one group goes to the group's row: summed in the wave by shuffles, over the four waves in LDS, then
// one atomic per column -- and for the box only where it changes the row.  Called by all threads of the block.
__device__ __forceinline__ void shape_sums_flush(ShapeAcc& a, long long* row, long long (*ssum)[SH_SUMS], int (*sbox)[4]) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  // (a window is counted only when a pixel of it is set: a wave that saw nothing but background has nothing to add)
  const bool some = __ballot(a.n | a.q[0] | a.q[1] | a.q[2] | a.q[3] | a.q[4]) != 0ull;
  long long acc[SH_SUMS] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (some) {
    acc[0] = wave_sum_i(a.n);
#pragma unroll
    for (int i = 0; i < 5; ++i) acc[1 + i] = wave_sum_ll(a.m[i]);
#pragma unroll
    for (int i = 0; i < 5; ++i) acc[6 + i] = wave_sum_i(a.q[i]);
    a.ymin = wave_min_i(a.ymin), a.ymax = wave_max_i(a.ymax), a.xmin = wave_min_i(a.xmin), a.xmax = wave_max_i(a.xmax);
  }
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < SH_SUMS; ++i) ssum[wave][i] = acc[i];
    sbox[wave][0] = a.ymin, sbox[wave][1] = a.ymax, sbox[wave][2] = a.xmin, sbox[wave][3] = a.xmax;
  }
  __syncthreads();
  const int t = threadIdx.x;
  if (t < SH_SUMS) {
    long long v = 0;
#pragma unroll
    for (int w = 0; w < SH_WAVES; ++w) v += ssum[w][t];
    if (v) atomicAdd((unsigned long long*)&row[t < 6 ? t : t + 4], (unsigned long long)v);   // (every sum is >= 0)
  } else if (t < SH_SUMS + 4) {
    const int b = t - SH_SUMS;                                     // 0, 2: a minimum; 1, 3: a maximum
    int v = sbox[0][b];
#pragma unroll
    for (int w = 1; w < SH_WAVES; ++w) v = (b & 1) ? max(v, sbox[w][b]) : min(v, sbox[w][b]);
    const long long now = __hip_atomic_load(&row[6 + b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (b & 1) {
      if (v > now) __hip_atomic_fetch_max(&row[6 + b], (long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else if (v < now) {
      __hip_atomic_fetch_min(&row[6 + b], (long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  __syncthreads();                                                 // (the LDS rows are free for the next group)
}

// A block of the launch takes SH_WALK consecutive blocks of the plan and goes to a row once per group among them, not once per
// chunk: every atomic of a group lands in the one 128-byte line of its row, and with one flush per chunk the launch took the time
// those atomics queue there (profiles/shape_rate.txt).
// Sxx over a full crop of the largest box is 32767 * (32766 * 32767 * 65533 / 6) < 3.9e17 < 2^63, and no other sum is larger.
constexpr int SH_WALK = 8;

__global__ __launch_bounds__(ME_T) void shape_sums_kernel(const int* groups, int G, int blocks, const unsigned char* arena,
                                                          long long* sums) {
  __shared__ long long ssum[SH_WAVES][SH_SUMS];
  __shared__ int sbox[SH_WAVES][4];
  const int first = blockIdx.x * SH_WALK, last = min(first + SH_WALK, blocks);
  ShapeAcc a;
  int g = -1;
  for (int vb = first; vb < last; ++vb) {                           // (block-uniform)
    const Crop c = crop_of(groups, G, vb);
    if (c.g != g) {
      if (g >= 0) shape_sums_flush(a, sums + (size_t)g * SH_COLS, ssum, sbox);
      g = c.g;
      a.reset(c.bh, c.bw);
    }
    const unsigned char* s = arena + c.off;
    const int bh = c.bh, bw = c.bw;
#pragma unroll
    for (int k = 0; k < ME_PX; ++k) {
      const int p = c.p0 + k * ME_T + threadIdx.x;
      if (p >= c.area) break;
      const int y = p / bw, x = p - y * bw;
      const unsigned char* r = s + p;                  // (every neighbour is read from the crop, wherever the chunk begins)
      const unsigned d = r[0] != 0;
      const unsigned b = y > 0 && r[-bw] != 0, cc = x > 0 && r[-1] != 0, nw = y > 0 && x > 0 && r[-bw - 1] != 0;
      quad(nw, b, cc, d, a.q);
      const bool lastx = x == bw - 1, lasty = y == bh - 1;
      if (lastx) quad(b, 0, d, 0, a.q);
      if (lasty) quad(cc, d, 0, 0, a.q);
      if (lastx && lasty) quad(d, 0, 0, 0, a.q);
      if (d) {
        ++a.n;
        a.m[0] += y, a.m[1] += x, a.m[2] += (long long)y * y, a.m[3] += (long long)x * x, a.m[4] += (long long)x * y;
        a.ymin = min(a.ymin, y), a.ymax = max(a.ymax, y), a.xmin = min(a.xmin, x), a.xmax = max(a.xmax, x);
      }
    }
  }
  if (g >= 0) shape_sums_flush(a, sums + (size_t)g * SH_COLS, ssum, sbox);
}

// ---- parts: union-find -----------------------------------------------------------------------------------------------------
// A wave holds 64 consecutive pixels of the crop (the chunk begins at a multiple of ME_CHUNK): a foreground pixel starts at the
// first pixel of its row run within those 64, found from the wave's ballot, so a solid blob begins with chains of one step
// instead of one per pixel.  Such a start is a pixel of the same part with an index <= its own.
__global__ __launch_bounds__(ME_T) void shape_parts_init_kernel(const int* groups, int G, const unsigned char* arena, int* labels,
                                                                int* px) {
  const Crop c = crop_of_block(groups, G);
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int k = 0; k < ME_PX; ++k) {                                    // (no lane leaves the loop early: ballots)
    const int p = c.p0 + k * ME_T + threadIdx.x;
    const bool in = p < c.area;
    const bool fg = in && arena[c.off + p] != 0;
    const int x = in ? p % c.bw : 0;
    // a lane opens a run when it is foreground and the lane before it is not, or is the end of the row above, or there is none
    const unsigned long long fgs = __ballot(fg);
    const unsigned long long opens = __ballot(fg && (lane == 0 || x == 0 || !((fgs >> (lane - 1)) & 1ull)));
    if (!in) continue;
    int start = -1;
    if (fg) {
      const unsigned long long upto = opens & ((2ull << lane) - 1ull);   // (never empty: walking left from a foreground lane ends at one)
      start = p - (lane - (63 - __clzll((long long)upto)));
    }
    labels[c.off + p] = start;
    px[c.off + p] = 0;
  }
}

// Forward neighbours only.  E: the two pixels began under one start unless the right one opens a wave's 64 pixels.  S: when W and
// SW are foreground too and neither p nor S opens a wave, p ~ W and S ~ SW began joined and the pair (W, SW) is merged (or, by
// the same rule, left to a pair further left that is): nothing to do.  SW, SE: only when S is background -- a foreground S is
// joined to both along its row.
__global__ __launch_bounds__(ME_T) void shape_parts_merge_kernel(const int* groups, int G, const unsigned char* arena, int* labels) {
  const Crop c = crop_of_block(groups, G);
  const unsigned char* s = arena + c.off;
  int* L = labels + c.off;
  const int bh = c.bh, bw = c.bw;
#pragma unroll
  for (int k = 0; k < ME_PX; ++k) {
    const int p = c.p0 + k * ME_T + threadIdx.x;
    if (p >= c.area) break;
    if (!s[p]) continue;
    const int y = p / bw, x = p - y * bw;
    const bool w = x > 0, e = x + 1 < bw, so = y + 1 < bh;
    if (e && ((p + 1) & 63) == 0 && s[p + 1]) uf_union(L, p, p + 1);
    if (!so) continue;
    const unsigned char* r = s + p + bw;
    if (r[0]) {
      const bool joined = w && s[p - 1] && r[-1] && (p & 63) != 0 && ((p + bw) & 63) != 0;
      if (!joined) uf_union(L, p, p + bw);
    } else {
      if (w && r[-1]) uf_union(L, p, p + bw - 1);
      if (e && r[1]) uf_union(L, p, p + bw + 1);
    }
  }
}

// A lane first adds up its own consecutive pixels of one root; then the lanes of a wave that share a root add up (a leader per
// distinct root, found by ballot): a solid blob would otherwise queue every one of its pixels on one address.
__device__ __forceinline__ void wave_add_px(int* px, int root, int cnt, int lane) {
  unsigned long long todo = __ballot(root >= 0);
  while (todo) {                                                       // (wave-uniform: one turn per distinct root of the wave)
    const int leader = __ffsll((long long)todo) - 1;
    const int lr = __shfl(root, leader, 64);
    const bool mine = root == lr;
    todo &= ~__ballot(mine);
    const int total = wave_sum_i(mine ? cnt : 0);
    if (lane == leader) atomicAdd(&px[lr], total);
  }
}

// (a block of the launch takes SH_WALK consecutive blocks of the plan, as shape_sums does: a lane of a solid blob then brings 32
// pixels of one root to one atomic of its wave)
__global__ __launch_bounds__(ME_T) void shape_parts_count_kernel(const int* groups, int G, int blocks, const int* labels, int* px) {
  const int lane = threadIdx.x & 63;
  const int first = blockIdx.x * SH_WALK, last = min(first + SH_WALK, blocks);
  int pend = -1, cnt = 0, g = -1;                                      // this lane's pixels of one root, not yet added
  size_t off = 0;
  for (int vb = first; vb < last; ++vb) {                              // (block-uniform)
    const Crop c = crop_of(groups, G, vb);
    if (c.g != g) {                                                    // (a root is an index in its own crop)
      if (g >= 0 && __ballot(pend >= 0) != 0ull) wave_add_px(px + off, pend, cnt, lane);
      g = c.g, off = c.off, pend = -1, cnt = 0;
    }
#pragma unroll
    for (int k = 0; k < ME_PX; ++k) {                                  // (no lane leaves the loop early: ballots and shuffles)
      const int p = c.p0 + k * ME_T + threadIdx.x;
      const int root = p < c.area ? labels[c.off + p] : -1;
      const bool flush = pend >= 0 && root != pend;
      if (__ballot(flush) != 0ull) wave_add_px(px + c.off, flush ? pend : -1, cnt, lane);
      if (root == pend) cnt += root >= 0;
      else pend = root, cnt = root >= 0;
    }
  }
  if (g >= 0 && __ballot(pend >= 0) != 0ull) wave_add_px(px + off, pend, cnt, lane);
}

__global__ __launch_bounds__(ME_T) void shape_parts_roots_kernel(const int* groups, int G, const int* labels, const int* px,
                                                                 long long* parts) {
  const Crop c = crop_of_block(groups, G);
  int roots = 0, largest = 0;
#pragma unroll
  for (int k = 0; k < ME_PX; ++k) {
    const int p = c.p0 + k * ME_T + threadIdx.x;
    if (p >= c.area) break;
    if (labels[c.off + p] != p) continue;
    ++roots;
    largest = max(largest, px[c.off + p]);
  }
  if (__ballot(roots) == 0ull) return;                                 // (wave-uniform)
  roots = wave_sum_i(roots), largest = wave_max_i(largest);
  if ((threadIdx.x & 63) == 0) {
    atomicAdd((unsigned long long*)&parts[(size_t)c.g * 2], (unsigned long long)roots);
    atomicMax((unsigned long long*)&parts[(size_t)c.g * 2 + 1], (unsigned long long)largest);
  }
}

// ---- extents -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(ME_T) void shape_extents_init_kernel(int* pminmax, long long n) {
  const long long i = (long long)blockIdx.x * ME_T + threadIdx.x;
  if (i < n) pminmax[i] = (i & 1) ? (int)0x80000000 : 0x7fffffff;
}

// The block's boundary pixels are listed in LDS (in any order: a minimum does not depend on it); then thread k walks the list for
// direction k, every lane reading the same entry, and goes to its group's row only where it can change it.
__global__ __launch_bounds__(ME_T) void shape_extents_kernel(const int* groups, int G, const unsigned char* arena, const int* dirs,
                                                             int K, int* pminmax) {
  __shared__ int list[ME_CHUNK];                                       // y << 16 | x (both below 2^15)
  __shared__ int count;
  const Crop c = crop_of_block(groups, G);
  const unsigned char* s = arena + c.off;
  const int bh = c.bh, bw = c.bw, lane = threadIdx.x & 63;
  if (threadIdx.x == 0) count = 0;
  __syncthreads();
#pragma unroll
  for (int k = 0; k < ME_PX; ++k) {                                    // (no lane leaves the loop early: ballots and shuffles)
    const int p = c.p0 + k * ME_T + threadIdx.x;
    bool edge = false;
    int y = 0, x = 0;
    if (p < c.area && s[p]) {
      y = p / bw, x = p - y * bw;
      edge = !(y > 0 && y + 1 < bh && x > 0 && x + 1 < bw && s[p - bw] && s[p + bw] && s[p - 1] && s[p + 1]);
    }
    const unsigned long long m = __ballot(edge);
    if (m == 0ull) continue;                                           // (wave-uniform)
    const int leader = __ffsll((long long)m) - 1;
    int base = 0;
    if (lane == leader) base = atomicAdd(&count, __popcll(m));
    base = __shfl(base, leader, 64);
    if (edge) list[base + __popcll(m & ((1ull << lane) - 1ull))] = y << 16 | x;
  }
  __syncthreads();
  const int n = count;                                                 // (<= ME_CHUNK: a pixel is listed once)
  if (n == 0) return;
  int* row = pminmax + (size_t)c.g * K * 2;
  for (int k = threadIdx.x; k < K; k += ME_T) {
    const int ck = dirs[2 * k], sk = dirs[2 * k + 1];
    int lo = 0x7fffffff, hi = (int)0x80000000;
    for (int i = 0; i < n; ++i) {
      const int e = list[i];
      const int v = ck * (e & 0xffff) + sk * (e >> 16);
      lo = min(lo, v), hi = max(hi, v);
    }
    if (lo < __hip_atomic_load(&row[2 * k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&row[2 * k], lo);
    if (hi > __hip_atomic_load(&row[2 * k + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&row[2 * k + 1], hi);
  }
}

}  // namespace

static int shape_sums_run(const int32_t* groups, int G, int blocks, const uint8_t* arena, int64_t* sums, void* stream) {
  DY_RECORD_OR_RUN([=](void* s) { return shape_sums_run(groups, G, blocks, arena, sums, s); });
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(shape_sums_init_kernel, dim3((G * SH_COLS + ME_T - 1) / ME_T), dim3(ME_T), 0, st, (const int*)groups, G,
                     (long long*)sums);
  DY_CHECK_LAUNCH();
  if (blocks == 0) return DISYOLO_OK;
  hipLaunchKernelGGL(shape_sums_kernel, dim3((blocks + SH_WALK - 1) / SH_WALK), dim3(ME_T), 0, st, (const int*)groups, G, blocks,
                     (const unsigned char*)arena, (long long*)sums);
  DY_CHECK_LAUNCH();
  return DISYOLO_OK;
}

extern "C" int disyolo_shape_sums(const int32_t* groups_host, const int32_t* groups, int G, const uint8_t* arena, int64_t arena_bytes,
                                  int64_t* sums, void* stream) {
  DY_REQUIRE(G <= 0 || (groups_host && groups && arena && sums), "shape_sums: null pointer");
  ME_ARGS("shape_sums");
  DY_REQUIRE(G < (1 << 26), "shape_sums: G = %d (need < 2^26)", G);
  ME_PLAN("shape_sums", nullptr);
  // (groups without a pixel still get their empty row)
  return shape_sums_run(groups, G, (int)blocks, arena, sums, stream);
}

static int shape_parts_run(const int32_t* groups, int G, int blocks, const uint8_t* arena, int32_t* labels, int32_t* px, int64_t* parts,
                           void* stream) {
  DY_RECORD_OR_RUN([=](void* s) { return shape_parts_run(groups, G, blocks, arena, labels, px, parts, s); });
  hipStream_t st = (hipStream_t)stream;
  ME_ZERO("shape_parts", parts, (size_t)G * 2 * sizeof(int64_t), st);
  if (blocks == 0) return DISYOLO_OK;
  const int* g = (const int*)groups;
  const unsigned char* a = (const unsigned char*)arena;
  hipLaunchKernelGGL(shape_parts_init_kernel, dim3(blocks), dim3(ME_T), 0, st, g, G, a, (int*)labels, (int*)px);
  DY_CHECK_LAUNCH();
  hipLaunchKernelGGL(shape_parts_merge_kernel, dim3(blocks), dim3(ME_T), 0, st, g, G, a, (int*)labels);
  DY_CHECK_LAUNCH();
  hipLaunchKernelGGL(labels_flatten_kernel<>, dim3(blocks), dim3(ME_T), 0, st, g, G, (int*)labels);
  DY_CHECK_LAUNCH();
  hipLaunchKernelGGL(shape_parts_count_kernel, dim3((blocks + SH_WALK - 1) / SH_WALK), dim3(ME_T), 0, st, g, G, blocks,
                     (const int*)labels, (int*)px);
  DY_CHECK_LAUNCH();
  hipLaunchKernelGGL(shape_parts_roots_kernel, dim3(blocks), dim3(ME_T), 0, st, g, G, (const int*)labels, (const int*)px,
                     (long long*)parts);
  DY_CHECK_LAUNCH();
  return DISYOLO_OK;
}

extern "C" int disyolo_shape_parts(const int32_t* groups_host, const int32_t* groups, int G, const uint8_t* arena, int64_t arena_bytes,
                                   int32_t* labels, int32_t* px, int64_t* parts, void* stream) {
  DY_REQUIRE(G <= 0 || (groups_host && groups && arena && labels && px && parts), "shape_parts: null pointer");
  ME_ARGS("shape_parts");
  ME_PLAN("shape_parts", nullptr);
  // (groups without a pixel still get their zero row)
  return shape_parts_run(groups, G, (int)blocks, arena, labels, px, parts, stream);
}

static int shape_extents_run(const int32_t* groups, int G, int blocks, const uint8_t* arena, const int32_t* dirs, int K,
                             int32_t* pminmax, void* stream) {
  DY_RECORD_OR_RUN([=](void* s) { return shape_extents_run(groups, G, blocks, arena, dirs, K, pminmax, s); });
  hipStream_t st = (hipStream_t)stream;
  const long long n = (long long)G * K * 2;
  hipLaunchKernelGGL(shape_extents_init_kernel, dim3((unsigned)((n + ME_T - 1) / ME_T)), dim3(ME_T), 0, st, (int*)pminmax, n);
  DY_CHECK_LAUNCH();
  if (blocks == 0) return DISYOLO_OK;
  hipLaunchKernelGGL(shape_extents_kernel, dim3(blocks), dim3(ME_T), 0, st, (const int*)groups, G, (const unsigned char*)arena,
                     (const int*)dirs, K, (int*)pminmax);
  DY_CHECK_LAUNCH();
  return DISYOLO_OK;
}

extern "C" int disyolo_shape_extents(const int32_t* groups_host, const int32_t* groups, int G, const uint8_t* arena, int64_t arena_bytes,
                                     const int32_t* dirs_host, const int32_t* dirs, int K, int32_t* pminmax, void* stream) {
  DY_REQUIRE(G <= 0 || (groups_host && groups && arena && dirs_host && dirs && pminmax), "shape_extents: null pointer");
  ME_ARGS("shape_extents");
  DY_REQUIRE(G < (1 << 20), "shape_extents: G = %d (need < 2^20)", G);
  if (G == 0) return DISYOLO_OK;                                      // (no directions are asked of a call without groups)
  DY_REQUIRE(K >= 2 && K <= SH_K_MAX && K % 2 == 0, "shape_extents: K = %d directions (need an even number in 2 .. %d)", K, SH_K_MAX);
  for (int k = 0; k < K; ++k)
    DY_REQUIRE(dirs_host[2 * k] >= -SH_UNIT && dirs_host[2 * k] <= SH_UNIT && dirs_host[2 * k + 1] >= -SH_UNIT &&
                   dirs_host[2 * k + 1] <= SH_UNIT,
               "shape_extents: direction %d is (%d, %d) (need |c|, |s| <= %d)", k, dirs_host[2 * k], dirs_host[2 * k + 1], SH_UNIT);
  ME_PLAN("shape_extents", nullptr);
  // (groups without a pixel still get their (INT32_MAX, INT32_MIN) rows)
  return shape_extents_run(groups, G, (int)blocks, arena, dirs, K, pminmax, stream);
}

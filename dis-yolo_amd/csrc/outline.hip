// The outlines of an instance: the borders of its crop as closed loops of pixel sides, ordered, with their pixel chains and their
// corner rings (dis-yolo_amd/measure.py, instance_outlines).
//
// The definition these kernels are held to is tests/outline_ref.py; everything is an integer, and there is no float in this file.
// A boundary edge is (p, s): a foreground pixel and a side (0 = N, 1 = E, 2 = S, 3 = W) whose neighbour across it is background,
// walked clockwise.  Its successor -- the diagonal pixel ahead if it is foreground (a left turn), else the pixel ahead (straight),
// else the next side of p (a right turn) -- is a permutation of the edges, and its cycles are the borders.  So there is no walk:
// the edges are listed, every entry learns its successor by one lookup, and what a walk would have counted comes from pointer
// jumping over the list.  The kernels read the [G,8] groups table as measure.hip does (measure_common.h): a block owns ME_CHUNK
// consecutive pixels of a crop, per-pixel buffers lie in the arena's layout, the elements between two crops are never touched.
// An edge is known everywhere by its key in the arena, 4 (off + p) + s < 2^31.
//   outline_mark    per pixel the side mask and the pixel's first list entry; the entries of a wave's 64 pixels are counted by a
//                   shuffle scan and take their places by one atomic per wave on ctrl[0]; a list that would pass the capacity
//                   sets bit 0 of ctrl[2], and every later kernel returns at once when ctrl[2] is set
//   outline_next    per edge its successor's entry; the edge tells its successor whether that one opens a run of another owner
//                   pixel (a point of the chain) and whether it lies on another side (a corner of the ring) -- an entry has one
//                   predecessor, so one writer; the edge's term of the shoelace sum
//   outline_min     R rounds: (label, pointer) -> (min of the label and the pointed entry's, the pointed entry's pointer), between
//                   two buffers; with 2^R >= the longest loop every entry ends with its loop's smallest key
//   outline_cut     the entry in front of the key edge becomes the end of a list; the key edge takes a row by an atomic on ctrl[1]
//   outline_rank    R rounds of list ranking as trace_round does them: the sums over the entries from here to the end of the number
//                   of edges, of points, of corners, of the shoelace terms, and the smallest key of an E side
//   outline_rows    every entry: its loop's row, its index among the points and among the corners; the key edge writes the row --
//                   it holds the totals -- with the part from the shape's label arena, the loop met on the way west, and the run
//                   the chain starts with
//   outline_gather  (after the host has sorted the rows) every point and every corner goes to the place the plan gives its loop:
//                   one writer per output element, whatever the order of the list
// The only atomics are the two counters and the overflow bits: the sums come from the ranking, so two runs give the same rows up to
// their order, which the host sorts away.  No kernel allocates, synchronises or waits for another block.
#include "measure_common.h"

namespace {

constexpr int OL_ROW = 12;           // int64 words of a loop's row: instance, key, n_edges, n_points, n_corners, area2, part, west,
                                     // estart, heads, start, 0
constexpr int OL_PLAN = 8;           // int32 words of a loop's plan: point offset, corner offset, start, heads, bw, off, x1, y1
constexpr int OL_WORK = 10;          // int64 words of work per list entry: two (label, pointer) buffers and two of OlRank
constexpr long long OL_MAX_LIST = (1ll << 30) - 1;

struct alignas(16) OlRank {
  int ptr, se, sh, sc;               // the next entry not yet added (-1: none), edges, points, corners from here to the end
  long long area;                    // the shoelace terms from here to the end
  int emin, pad;                     // the smallest key of an E side from here to the end
};
static_assert(sizeof(OlRank) == 32, "OlRank");

__device__ __forceinline__ int ol_entry(const int* first, const unsigned char* sides, int key) {
  const int gp = key >> 2, s = key & 3;
  return first[gp] + __popc(sides[gp] & ((1u << s) - 1u));
}

// ---- the list ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(ME_T) void outline_mark_kernel(const int* groups, int G, const unsigned char* arena, int* first,
                                                            unsigned char* sides, int* ekey, int capacity, int* ctrl) {
  const Crop c = crop_of_block(groups, G);
  const unsigned char* s = arena + c.off;
  const int bh = c.bh, bw = c.bw, lane = threadIdx.x & 63;
#pragma unroll
  for (int k = 0; k < ME_PX; ++k) {                                    // (no lane leaves the loop early: ballots and shuffles)
    const int p = c.p0 + k * ME_T + threadIdx.x;
    const bool in = p < c.area;
    unsigned m = 0;
    if (in && s[p]) {
      const int y = p / bw, x = p - y * bw;
      m = (unsigned)!(y > 0 && s[p - bw]) | (unsigned)!(x + 1 < bw && s[p + 1]) << 1 | (unsigned)!(y + 1 < bh && s[p + bw]) << 2 |
          (unsigned)!(x > 0 && s[p - 1]) << 3;
    }
    const int cnt = __popc(m);
    int f = -1;
    if (__ballot(cnt) != 0ull) {                                       // (wave-uniform)
      int inc = cnt;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
      }
      const int total = __shfl(inc, 63, 64);
      int base = 0;
      if (lane == 63) {
        base = atomicAdd(&ctrl[0], total);                             // (< 4 * arena_bytes < 2^31 in all)
        if ((long long)base + total > capacity) atomicOr(&ctrl[2], 1);
      }
      base = __shfl(base, 63, 64);
      if (cnt && (long long)base + total <= capacity) f = base + inc - cnt;
    }
    if (!in) continue;
    first[c.off + p] = f;
    sides[c.off + p] = (unsigned char)m;
    if (f >= 0) {
      const int gk = 4 * (int)(c.off + p);
#pragma unroll
      for (int t = 0; t < 4; ++t)
        if (m >> t & 1u) ekey[f++] = gk + t;
    }
  }
}

__global__ __launch_bounds__(ME_T) void outline_next_kernel(const int* groups, int G, const unsigned char* arena, const int* first,
                                                            const unsigned char* sides, int* nxt, unsigned char* flag, int* aterm,
                                                            int2* lab, const int* ctrl) {
  if (ctrl[2]) return;
  const Crop c = crop_of_block(groups, G);
  const unsigned char* s = arena + c.off;
  const int* fi = first + c.off;
  const unsigned char* si = sides + c.off;
  const int bh = c.bh, bw = c.bw;
#pragma unroll
  for (int k = 0; k < ME_PX; ++k) {
    const int p = c.p0 + k * ME_T + threadIdx.x;
    if (p >= c.area) break;
    const unsigned m = si[p];
    if (!m) continue;
    const int y = p / bw, x = p - y * bw, f = fi[p];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      if (!(m >> t & 1u)) continue;
      const int e = f + __popc(m & ((1u << t) - 1u));
      const int fx = t == 0 ? 1 : t == 2 ? -1 : 0, fy = t == 1 ? 1 : t == 3 ? -1 : 0;      // the direction of travel
      const int ox = t == 1 ? 1 : t == 3 ? -1 : 0, oy = t == 0 ? -1 : t == 2 ? 1 : 0;      // the neighbour across the side
      int qx = x + fx + ox, qy = y + fy + oy, q = p, u = (t + 1) & 3;
      if (qx >= 0 && qx < bw && qy >= 0 && qy < bh && s[qy * bw + qx]) {
        q = qy * bw + qx, u = (t + 3) & 3;
      } else {
        qx = x + fx, qy = y + fy;
        if (qx >= 0 && qx < bw && qy >= 0 && qy < bh && s[qy * bw + qx]) q = qy * bw + qx, u = t;
      }
      const int fe = fi[q] + __popc(si[q] & ((1u << u) - 1u));
      nxt[e] = fe;
      flag[fe] = (unsigned char)((q != p) | (u != t) << 1);
      aterm[e] = t == 0 ? -y : t == 1 ? x + 1 : t == 2 ? y + 1 : -x;
      lab[e] = make_int2(4 * (int)(c.off + p) + t, fe);
    }
  }
}

// ---- the loops --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(ME_T) void outline_min_kernel(const int* ctrl, int capacity, const int2* src, int2* dst) {
  if (ctrl[2]) return;
  const int i = blockIdx.x * ME_T + threadIdx.x;
  if (i >= min(ctrl[0], capacity)) return;
  const int2 a = src[i], b = src[a.y];
  dst[i] = make_int2(min(a.x, b.x), b.y);
}

__global__ __launch_bounds__(ME_T) void outline_cut_kernel(int* ctrl, int capacity, const int* ekey, const int* nxt,
                                                           const unsigned char* flag, const int* aterm, const int2* lab, OlRank* rank,
                                                           int* eidx, int rows_capacity) {
  if (ctrl[2] & 1) return;
  const int i = blockIdx.x * ME_T + threadIdx.x;
  if (i >= min(ctrl[0], capacity)) return;
  const int l = lab[i].x, key = ekey[i], f = nxt[i], fl = flag[i];
  OlRank r;
  r.ptr = ekey[f] == l ? -1 : f;
  r.se = 1, r.sh = fl & 1, r.sc = fl >> 1 & 1;
  r.area = aterm[i];
  r.emin = (key & 3) == 1 ? key : 0x7fffffff;
  r.pad = 0;
  rank[i] = r;
  int row = -1;
  if (key == l) {
    row = atomicAdd(&ctrl[1], 1);
    if (row >= rows_capacity) atomicOr(&ctrl[2], 2), row = -1;
  }
  eidx[3 * (size_t)i] = row;
}

__global__ __launch_bounds__(ME_T) void outline_rank_kernel(const int* ctrl, int capacity, const OlRank* src, OlRank* dst) {
  if (ctrl[2]) return;
  const int i = blockIdx.x * ME_T + threadIdx.x;
  if (i >= min(ctrl[0], capacity)) return;
  OlRank a = src[i];
  if (a.ptr >= 0) {
    const OlRank b = src[a.ptr];
    a.se += b.se, a.sh += b.sh, a.sc += b.sc, a.area += b.area, a.emin = min(a.emin, b.emin), a.ptr = b.ptr;
  }
  dst[i] = a;
}

__global__ __launch_bounds__(ME_T) void outline_rows_kernel(const int* groups, int G, const unsigned char* arena, const int* part_labels,
                                                            const int* first, const unsigned char* sides, const unsigned char* flag,
                                                            const int2* lab, const OlRank* rank, const int* ctrl, int capacity,
                                                            int* eidx, long long* rows) {
  if (ctrl[2]) return;
  const int i = blockIdx.x * ME_T + threadIdx.x;
  if (i >= min(ctrl[0], capacity)) return;
  const int l = lab[i].x;
  const int k = ol_entry(first, sides, l);
  const OlRank tot = rank[k], me = rank[i];
  const int row = eidx[3 * (size_t)k];                                 // (written by outline_cut)
  eidx[3 * (size_t)i + 1] = tot.sh - me.sh;
  eidx[3 * (size_t)i + 2] = tot.sc - me.sc;
  if (i != k) {
    eidx[3 * (size_t)i] = row;
    return;
  }
  // the key edge: its sums are the loop's
  const int gp = l >> 2, s = l & 3;
  int lo = 0, hi = G - 1;                                              // the last group whose crop begins at or before gp
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if ((long long)groups[mid * 8 + 7] * 16 <= gp) lo = mid; else hi = mid - 1;
  }
  const int* g = groups + lo * 8;
  const int off = g[7] * 16, bw = g[5] - g[3], p = gp - off;
  const int y = p / bw, x = p - y * bw;
  // the run the chain starts with: the one that holds the key edge (an outer loop: a N side) or the smallest E side (a hole)
  const int es = s == 0 ? k : ol_entry(first, sides, tot.emin);
  const int m = tot.sh;
  int start = 0;
  if (m) {
    start = m - rank[es].sh + (flag[es] & 1) - 1;                      // the runs opened up to the start edge, less one
    if (start < 0) start = m - 1;                                      // (the start edge lies in the run that wraps around the cut)
  }
  long long west = -1;
  if (s == 0) {
    const unsigned char* r = arena + off + (size_t)y * bw;
    int qx = x - 1;
    while (qx >= 0 && !r[qx]) --qx;
    if (qx >= 0) west = lab[ol_entry(first, sides, 4 * (off + y * bw + qx) + 1)].x - 4 * off;
  }
  long long* o = rows + (size_t)row * OL_ROW;
  o[0] = lo, o[1] = l - 4 * off, o[2] = tot.se, o[3] = max(m, 1), o[4] = tot.sc, o[5] = tot.area, o[6] = part_labels[gp], o[7] = west;
  o[8] = tot.emin - 4 * off, o[9] = m, o[10] = start, o[11] = 0;
}

// ---- points and corners -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(ME_T) void outline_gather_kernel(const int* ctrl, int capacity, const int* ekey, const unsigned char* flag,
                                                              const int* eidx, const int* plan, int rows_capacity, int* points,
                                                              int n_points, int* corners, int n_corners) {
  if (ctrl[2]) return;
  const int i = blockIdx.x * ME_T + threadIdx.x;
  if (i >= min(ctrl[0], capacity)) return;
  const int row = eidx[3 * (size_t)i];
  if (row < 0 || row >= rows_capacity) return;
  const int* pl = plan + (size_t)row * OL_PLAN;
  const int m = pl[3], bw = pl[4], key = ekey[i], s = key & 3, fl = flag[i];
  const int p = (key >> 2) - pl[5];
  const int y = p / bw, x = p - y * bw;
  if ((fl & 1) || (m == 0 && s == 0)) {                                // (a loop without a change of owner is one pixel: one point)
    const int j = eidx[3 * (size_t)i + 1];
    const int pos = m ? (pl[2] - j + m) % m : 0;
    const long long at = (long long)pl[0] + pos;
    if (pos >= 0 && at >= 0 && at < n_points) points[2 * at] = x + pl[6], points[2 * at + 1] = y + pl[7];
  }
  if (fl & 2) {
    const long long at = (long long)pl[1] + eidx[3 * (size_t)i + 2];
    if (at >= 0 && at < n_corners) corners[2 * at] = x + (s == 1 || s == 2) + pl[6], corners[2 * at + 1] = y + (s >= 2) + pl[7];
  }
}

}  // namespace

#define OL_LIMITS(who)                                                                                                       \
  DY_REQUIRE(arena_bytes < (1ll << 29), who ": an arena of %lld bytes (an edge's key is 4 (off + p) + s: need 4 * arena_bytes < 2^31)", \
             (long long)arena_bytes);                                                                                        \
  DY_REQUIRE(capacity >= 0 && capacity <= OL_MAX_LIST, who ": a capacity of %lld list entries (need 0 .. 2^30 - 1)", (long long)capacity)

static int outline_edges_run(const int32_t* groups, int G, int blocks, const uint8_t* arena, int32_t* first, uint8_t* sides,
                             int32_t* ekey, int32_t* nxt, uint8_t* flag, int32_t* aterm, int capacity, int64_t* work, int32_t* ctrl,
                             void* stream) {
  DY_RECORD_OR_RUN([=](void* s) {
    return outline_edges_run(groups, G, blocks, arena, first, sides, ekey, nxt, flag, aterm, capacity, work, ctrl, s);
  });
  hipStream_t st = (hipStream_t)stream;
  ME_ZERO("outline_edges", ctrl, 4 * sizeof(int32_t), st);
  if (blocks == 0) return DISYOLO_OK;
  hipLaunchKernelGGL(outline_mark_kernel, dim3(blocks), dim3(ME_T), 0, st, (const int*)groups, G, (const unsigned char*)arena,
                     (int*)first, (unsigned char*)sides, (int*)ekey, capacity, (int*)ctrl);
  DY_CHECK_LAUNCH();
  if (capacity == 0) return DISYOLO_OK;
  hipLaunchKernelGGL(outline_next_kernel, dim3(blocks), dim3(ME_T), 0, st, (const int*)groups, G, (const unsigned char*)arena,
                     (const int*)first, (const unsigned char*)sides, (int*)nxt, (unsigned char*)flag, (int*)aterm, (int2*)work,
                     (const int*)ctrl);
  DY_CHECK_LAUNCH();
  return DISYOLO_OK;
}

// first int32 and sides uint8 lie in the arena's layout; ekey, nxt, aterm int32 and flag uint8 hold `capacity` list entries; work
// int64 holds OL_WORK words per entry (its first words take the labels the loops start from); ctrl int32 [4] = the entries listed,
// the rows taken, the overflow bits (1: the list, 2: the rows), 0
extern "C" int disyolo_outline_edges(const int32_t* groups_host, const int32_t* groups, int G, const uint8_t* arena, int64_t arena_bytes,
                                     int32_t* first, uint8_t* sides, int32_t* ekey, int32_t* nxt, uint8_t* flag, int32_t* aterm,
                                     int64_t capacity, int64_t* work, int64_t work_elems, int32_t* ctrl, void* stream) {
  DY_REQUIRE(G <= 0 || (groups_host && groups && arena && first && sides && ctrl && ((ekey && nxt && flag && aterm && work) || capacity == 0)),
             "outline_edges: null pointer");
  ME_ARGS("outline_edges");
  OL_LIMITS("outline_edges");
  DY_REQUIRE(work_elems >= OL_WORK * capacity, "outline_edges: work holds %lld words, %lld entries need %lld", (long long)work_elems,
             (long long)capacity, (long long)(OL_WORK * capacity));
  ME_PLAN("outline_edges", nullptr);
  // (groups without a pixel still get the zero counters)
  return outline_edges_run(groups, G, (int)blocks, arena, first, sides, ekey, nxt, flag, aterm, (int)capacity, work, ctrl, stream);
}

static int outline_loops_run(const int32_t* groups, int G, const uint8_t* arena, const int32_t* part_labels, const int32_t* first,
                             const uint8_t* sides, const int32_t* ekey, const int32_t* nxt, const uint8_t* flag, const int32_t* aterm,
                             int capacity, int rounds, int64_t* work, int32_t* eidx, int64_t* rows, int rows_capacity, int32_t* ctrl,
                             void* stream) {
  DY_RECORD_OR_RUN([=](void* s) {
    return outline_loops_run(groups, G, arena, part_labels, first, sides, ekey, nxt, flag, aterm, capacity, rounds, work, eidx, rows,
                             rows_capacity, ctrl, s);
  });
  hipStream_t st = (hipStream_t)stream;
  const unsigned lb = (unsigned)(((int64_t)capacity + ME_T - 1) / ME_T);
  int2* a0 = (int2*)work, *a1 = a0 + (size_t)capacity;
  OlRank* r0 = (OlRank*)(work + 2 * (size_t)capacity), *r1 = r0 + (size_t)capacity;
  const int* c = (const int*)ctrl;
  for (int r = 0; r < rounds; ++r) {
    hipLaunchKernelGGL(outline_min_kernel, dim3(lb), dim3(ME_T), 0, st, c, capacity, (const int2*)(r & 1 ? a1 : a0), r & 1 ? a0 : a1);
    DY_CHECK_LAUNCH();
  }
  const int2* lab = rounds & 1 ? a1 : a0;
  hipLaunchKernelGGL(outline_cut_kernel, dim3(lb), dim3(ME_T), 0, st, (int*)ctrl, capacity, (const int*)ekey, (const int*)nxt,
                     (const unsigned char*)flag, (const int*)aterm, lab, r0, (int*)eidx, rows_capacity);
  DY_CHECK_LAUNCH();
  for (int r = 0; r < rounds; ++r) {
    hipLaunchKernelGGL(outline_rank_kernel, dim3(lb), dim3(ME_T), 0, st, c, capacity, (const OlRank*)(r & 1 ? r1 : r0), r & 1 ? r0 : r1);
    DY_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(outline_rows_kernel, dim3(lb), dim3(ME_T), 0, st, (const int*)groups, G, (const unsigned char*)arena,
                     (const int*)part_labels, (const int*)first, (const unsigned char*)sides, (const unsigned char*)flag, lab,
                     (const OlRank*)(rounds & 1 ? r1 : r0), c, capacity, (int*)eidx, (long long*)rows);
  DY_CHECK_LAUNCH();
  return DISYOLO_OK;
}

// after disyolo_outline_edges on the same buffers, and disyolo_shape_parts' labels of the same arena: eidx int32 [capacity, 3] =
// per entry its loop's row, its index among the loop's points and among its corners; rows int64 [rows_capacity, 12], one per loop
// in the order the key edges arrived.  rounds: 2^rounds must reach the number of edges of the longest loop.
extern "C" int disyolo_outline_loops(const int32_t* groups_host, const int32_t* groups, int G, const uint8_t* arena, int64_t arena_bytes,
                                     const int32_t* part_labels, const int32_t* first, const uint8_t* sides, const int32_t* ekey,
                                     const int32_t* nxt, const uint8_t* flag, const int32_t* aterm, int64_t capacity, int rounds,
                                     int64_t* work, int64_t work_elems, int32_t* eidx, int64_t* rows, int64_t rows_capacity,
                                     int32_t* ctrl, void* stream) {
  DY_REQUIRE(G <= 0 || (groups_host && groups && arena && part_labels && first && sides && ctrl && (rows || rows_capacity == 0) &&
                        ((ekey && nxt && flag && aterm && work && eidx) || capacity == 0)),
             "outline_loops: null pointer");
  ME_ARGS("outline_loops");
  OL_LIMITS("outline_loops");
  DY_REQUIRE(work_elems >= OL_WORK * capacity, "outline_loops: work holds %lld words, %lld entries need %lld", (long long)work_elems,
             (long long)capacity, (long long)(OL_WORK * capacity));
  DY_REQUIRE(rows_capacity >= 0 && rows_capacity < (1ll << 31), "outline_loops: a capacity of %lld rows (need 0 .. 2^31 - 1)",
             (long long)rows_capacity);
  DY_REQUIRE(rounds >= 0 && rounds <= 31, "outline_loops: rounds = %d (need 0 .. 31)", rounds);
  ME_PLAN("outline_loops", nullptr);
  if (blocks == 0 || capacity == 0) return DISYOLO_OK;
  return outline_loops_run(groups, G, arena, part_labels, first, sides, ekey, nxt, flag, aterm, (int)capacity, rounds, work, eidx, rows,
                           (int)rows_capacity, ctrl, stream);
}

static int outline_gather_run(const int32_t* ekey, const uint8_t* flag, const int32_t* eidx, int capacity, const int32_t* ctrl,
                              const int32_t* plan, int rows_capacity, int32_t* points, int n_points, int32_t* corners, int n_corners,
                              void* stream) {
  DY_RECORD_OR_RUN([=](void* s) {
    return outline_gather_run(ekey, flag, eidx, capacity, ctrl, plan, rows_capacity, points, n_points, corners, n_corners, s);
  });
  hipLaunchKernelGGL(outline_gather_kernel, dim3((unsigned)(((int64_t)capacity + ME_T - 1) / ME_T)), dim3(ME_T), 0, (hipStream_t)stream,
                     (const int*)ctrl, capacity, (const int*)ekey, (const unsigned char*)flag, (const int*)eidx, (const int*)plan,
                     rows_capacity, (int*)points, n_points, (int*)corners, n_corners);
  DY_CHECK_LAUNCH();
  return DISYOLO_OK;
}

// after disyolo_outline_loops: plan int32 [rows_capacity, 8] per row of `rows` = where its points and its corners begin, the run
// its chain starts with, its heads (rows columns 10 and 9), and its crop's width, first arena element, x1 and y1; points int32
// [n_points, 2] and corners int32 [n_corners, 2] take (x, y) in the image
extern "C" int disyolo_outline_gather(const int32_t* groups_host, const int32_t* groups, int G, int64_t arena_bytes, const int32_t* ekey,
                                      const uint8_t* flag, const int32_t* eidx, int64_t capacity, const int32_t* ctrl,
                                      const int32_t* plan, int64_t rows_capacity, int32_t* points, int64_t n_points, int32_t* corners,
                                      int64_t n_corners, void* stream) {
  DY_REQUIRE(G <= 0 || (groups_host && groups && ctrl && ((ekey && flag && eidx) || capacity == 0) && (plan || rows_capacity == 0) &&
                        (points || n_points == 0) && (corners || n_corners == 0)),
             "outline_gather: null pointer");
  ME_ARGS("outline_gather");
  OL_LIMITS("outline_gather");
  DY_REQUIRE(rows_capacity >= 0 && rows_capacity < (1ll << 31), "outline_gather: a capacity of %lld rows (need 0 .. 2^31 - 1)",
             (long long)rows_capacity);
  DY_REQUIRE(n_points >= 0 && n_points <= OL_MAX_LIST && n_corners >= 0 && n_corners <= OL_MAX_LIST,
             "outline_gather: %lld points and %lld corners (need 0 .. 2^30 - 1)", (long long)n_points, (long long)n_corners);
  ME_PLAN("outline_gather", nullptr);
  if (blocks == 0 || capacity == 0 || rows_capacity == 0) return DISYOLO_OK;
  return outline_gather_run(ekey, flag, eidx, (int)capacity, ctrl, plan, (int)rows_capacity, points, (int)n_points, corners,
                            (int)n_corners, stream);
}

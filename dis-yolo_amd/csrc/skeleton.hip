// The graph of a skeleton: links, branches, per-branch rows and spur pruning (dis-yolo_amd/measure.py, skeleton_graph).
//
// The reference has no counterpart; the definition these kernels are held to is tests/skeleton_ref.py, and everything in it is
// an integer: there is no float in this file.  The kernels read the [G,8] groups table as measure.hip does (measure_common.h):
// a block owns ME_CHUNK consecutive pixels of a crop, every buffer lies in the arena's layout, one element per pixel, and the
// elements between two crops are never read and never written.
//   skeleton_classify   skel -> links: bit k of a pixel's byte = it is linked to its neighbour P(2+k) (N, NE, E, SE, S, SW, W, NW)
//   links_init          labels = the pixel's own index on P pixels (degree <= 2), -1 elsewhere          } arena_labels.h, with
//   links_merge         union-find over the links between two P pixels                                    } BranchPixels and
//   labels_flatten      labels = the root of every P pixel: its branch's smallest index                   } BranchRow below
//   roots_alloc         every root draws a row number from one counter and writes its row's head          }
//   skeleton_accum      every P pixel adds its integers to its branch's row (summed per wave and row first); J pixels add
//                       to the [G,4] junction table
//   skeleton_finish     the spur bit of every row from M2, and one flag per group that has a spur
//   skeleton_prune      deletes the pixels whose row is a spur
// No block waits for another: the retry loops of the merge are lock-free (arena_labels.h), and what one launch writes is read
// with plain loads only by later launches.
#include "arena_labels.h"

namespace {

constexpr int SK_M2_MAX = 2 * 32767;

__global__ __launch_bounds__(ME_T) void skeleton_classify_kernel(const int* groups, int G, const unsigned char* src,
                                                                 unsigned char* skel, unsigned char* links, int copy) {
  const Crop c = crop_of_block(groups, G);
  const unsigned char* s = src + c.off;
  const int bh = c.bh, bw = c.bw;
#pragma unroll
  for (int k = 0; k < ME_PX; ++k) {
    const int p = c.p0 + k * ME_T + threadIdx.x;
    if (p >= c.area) break;
    const int on = s[p] != 0;
    unsigned lk = 0;
    if (on) {
      const int y = p / bw, x = p - y * bw;
      const bool n = y > 0, so = y + 1 < bh, w = x > 0, e = x + 1 < bw;
      const unsigned char* r = s + p;
      const unsigned N = n && r[-bw], NE = n && e && r[1 - bw], E = e && r[1], SE = so && e && r[bw + 1];
      const unsigned S = so && r[bw], SW = so && w && r[bw - 1], W = w && r[-1], NW = n && w && r[-bw - 1];
      lk = N | (NE & !N & !E) << 1 | E << 2 | (SE & !E & !S) << 3 | S << 4 | (SW & !S & !W) << 5 | W << 6 | (NW & !N & !W) << 7;
    }
    links[c.off + p] = (unsigned char)lk;
    if (copy) skel[c.off + p] = (unsigned char)on;
  }
}

// ---- labels and rows: what arena_labels.h is told ----------------------------------------------------------------------------
// the P pixels: on the skeleton (an off pixel has no link either) with at most two links
struct BranchPixels {
  const unsigned char* skel;
  __device__ bool seed(size_t i, unsigned links) const { return skel[i] && member(links); }
  __device__ static bool member(unsigned links) { return __popc(links) <= 2; }
};

// ctrl int32 [1 + G]: word 0 = the row counter, which keeps counting beyond `capacity` without anything being written there;
// word 1 + g != 0 <=> group g has a spur.  junctions int64 [G, 4] = junction_px, jj_orth, jj_diag, n_branches.
struct BranchRow {
  static constexpr int WIDTH = SK_ROW;
  unsigned long long* junctions;
  __device__ void drawn(int g) const { atomicAdd(&junctions[(size_t)g * 4 + 3], 1ull); }
  __device__ static long long empty(int q) { return q == SK_MIN_D2 ? 0x7fffffffll : 0; }
};

// Most waves hold no skeleton pixel at all, and those of a wave that does mostly belong to one branch: the lanes of a wave
// that share a row add their integers up first (a leader per distinct row, found by ballot), and only the leader touches the
// row -- a handful of atomics per wave and row where a long branch would otherwise queue thousands on eight addresses.
__global__ __launch_bounds__(ME_T) void skeleton_accum_kernel(const int* groups, int G, const unsigned char* links,
                                                              const int* labels, const int* d2, const int* rowid,
                                                              unsigned long long* rows, int capacity,
                                                              unsigned long long* junctions) {
  const Crop c = crop_of_block(groups, G);
  const unsigned char* lk = links + c.off;
  const int lane = threadIdx.x & 63;
  int jpx = 0, jorth = 0, jdiag = 0;
#pragma unroll
  for (int k = 0; k < ME_PX; ++k) {                                    // (no lane leaves the loop early: ballots and shuffles)
    const int p = c.p0 + k * ME_T + threadIdx.x;
    int id = -1, orth = 0, diag = 0, attach = 0, ends = 0, d = 0;
    if (p < c.area) {
      const unsigned l = lk[p];
      const int root = labels[c.off + p];
      if (root < 0) {
        if (__popc(l) >= 3) {                                          // a junction pixel (anything else is off the skeleton)
          ++jpx;
#pragma unroll
          for (int b = 2; b <= 5; ++b)
            if ((l >> b & 1) && __popc(lk[p + nb_offset(b, c.bw)]) >= 3) (b & 1) ? ++jdiag : ++jorth;
        }
      } else {
        id = rowid[c.off + root];
        if (id >= capacity) id = -1;
#pragma unroll
        for (int b = 0; b < 8; ++b) {
          if (!(l >> b & 1)) continue;
          const bool toJ = __popc(lk[p + nb_offset(b, c.bw)]) >= 3;
          if (toJ || (b >= 2 && b <= 5)) (b & 1) ? ++diag : ++orth;
          attach += toJ;
        }
        const int deg = __popc(l);
        ends = deg == 1 ? 1 : deg == 0 ? 2 : 0;
        d = d2[c.off + p];
      }
    }
    unsigned long long todo = __ballot(id >= 0);
    while (todo) {                                                     // (wave-uniform: one turn per distinct row of the wave)
      const int leader = __ffsll((long long)todo) - 1;
      const int lid = __shfl(id, leader, 64);
      const bool mine = id == lid;
      todo &= ~__ballot(mine);
      const long long px = wave_sum_ll(mine ? 1 : 0), so = wave_sum_ll(mine ? orth : 0), sd = wave_sum_ll(mine ? diag : 0);
      const long long se = wave_sum_ll(mine ? ends : 0), sa = wave_sum_ll(mine ? attach : 0);
      const long long sq = wave_sum_ll(mine ? (long long)isqrt_q8(d) : 0);
      const int mx = wave_max_i(mine ? d : 0), mn = -wave_max_i(mine ? -d : -0x7fffffff);
      if (lane == leader) {
        unsigned long long* r = rows + (size_t)lid * SK_ROW;
        atomicAdd(&r[SK_PX], (unsigned long long)px);
        if (so) atomicAdd(&r[SK_N_ORTH], (unsigned long long)so);
        if (sd) atomicAdd(&r[SK_N_DIAG], (unsigned long long)sd);
        if (se) atomicAdd(&r[SK_N_END], (unsigned long long)se);
        if (sa) atomicAdd(&r[SK_N_ATTACH], (unsigned long long)sa);
        atomicAdd(&r[SK_SUM_Q8], (unsigned long long)sq);
        atomicMax(&r[SK_MAX_D2], (unsigned long long)mx);
        atomicMin(&r[SK_MIN_D2], (unsigned long long)mn);
      }
    }
  }
  const long long v[3] = {wave_sum_ll(jpx), wave_sum_ll(jorth), wave_sum_ll(jdiag)};
  if (lane == 0) {
#pragma unroll
    for (int q = 0; q < 3; ++q)
      if (v[q]) atomicAdd(&junctions[(size_t)c.g * 4 + q], (unsigned long long)v[q]);
  }
}

// a spur: n_end = 1, n_attach = 1 and 2 n_orth + 2 sqrt(2) n_diag + n_end < M2, i.e. t2 = M2 - 2 n_orth - n_end > 0 and
// 8 n_diag^2 < t2^2 (int64: n_diag < 2^30 and t2 <= M2 < 2^16)
__global__ __launch_bounds__(ME_T) void skeleton_finish_kernel(long long* rows, int capacity, int M2, int* ctrl) {
  const long long i = (long long)blockIdx.x * ME_T + threadIdx.x;
  if (i >= min(ctrl[0], capacity)) return;
  long long* r = rows + (size_t)i * SK_ROW;
  const long long t2 = (long long)M2 - 2 * r[SK_N_ORTH] - r[SK_N_END];
  const int spur = r[SK_N_END] == 1 && r[SK_N_ATTACH] == 1 && t2 > 0 && 8 * r[SK_N_DIAG] * r[SK_N_DIAG] < t2 * t2;
  r[SK_SPUR] = spur;
  if (spur) atomicOr(&ctrl[1 + (int)r[SK_GROUP]], 1);
}

__global__ __launch_bounds__(ME_T) void skeleton_prune_kernel(const int* groups, int G, const int* labels, const int* rowid,
                                                              const long long* rows, int capacity, unsigned char* skel) {
  const Crop c = crop_of_block(groups, G);
#pragma unroll
  for (int k = 0; k < ME_PX; ++k) {
    const int p = c.p0 + k * ME_T + threadIdx.x;
    if (p >= c.area) break;
    const int root = labels[c.off + p];
    if (root < 0) continue;
    const int id = rowid[c.off + root];
    if (id < capacity && rows[(size_t)id * SK_ROW + SK_SPUR]) skel[c.off + p] = 0;
  }
}

}  // namespace

static int skeleton_classify_run(const int32_t* groups, int G, int blocks, const uint8_t* src, uint8_t* skel, uint8_t* links,
                                 void* stream) {
  DY_RECORD_OR_RUN([=](void* s) { return skeleton_classify_run(groups, G, blocks, src, skel, links, s); });
  hipLaunchKernelGGL(skeleton_classify_kernel, dim3(blocks), dim3(ME_T), 0, (hipStream_t)stream, (const int*)groups, G,
                     (const unsigned char*)src, (unsigned char*)skel, (unsigned char*)links, src != skel ? 1 : 0);
  DY_CHECK_LAUNCH();
  return DISYOLO_OK;
}

extern "C" int disyolo_skeleton_classify(const int32_t* groups_host, const int32_t* groups, int G, int64_t arena_bytes,
                                         const uint8_t* src, uint8_t* skel, uint8_t* links, void* stream) {
  DY_REQUIRE(G <= 0 || (groups_host && groups && src && skel && links), "skeleton_classify: null pointer");
  ME_TABLES("skeleton_classify", nullptr);
  return skeleton_classify_run(groups, G, (int)blocks, src, skel, links, stream);
}

static int skeleton_label_run(const int32_t* groups, int G, int blocks, const uint8_t* skel, const uint8_t* links, int32_t* labels,
                              void* stream) {
  DY_RECORD_OR_RUN([=](void* s) { return skeleton_label_run(groups, G, blocks, skel, links, labels, s); });
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(links_init_kernel<BranchPixels>, dim3(blocks), dim3(ME_T), 0, st, (const int*)groups, G,
                     BranchPixels{(const unsigned char*)skel}, (const unsigned char*)links, (int*)labels);
  DY_CHECK_LAUNCH();
  hipLaunchKernelGGL(links_merge_kernel<BranchPixels>, dim3(blocks), dim3(ME_T), 0, st, (const int*)groups, G,
                     (const unsigned char*)links, (int*)labels);
  DY_CHECK_LAUNCH();
  hipLaunchKernelGGL(labels_flatten_kernel<LINKS_HALVE>, dim3(blocks), dim3(ME_T), 0, st, (const int*)groups, G, (int*)labels);
  DY_CHECK_LAUNCH();
  return DISYOLO_OK;
}

extern "C" int disyolo_skeleton_label(const int32_t* groups_host, const int32_t* groups, int G, int64_t arena_bytes,
                                      const uint8_t* skel, const uint8_t* links, int32_t* labels, void* stream) {
  DY_REQUIRE(G <= 0 || (groups_host && groups && skel && links && labels), "skeleton_label: null pointer");
  ME_TABLES("skeleton_label", nullptr);
  return skeleton_label_run(groups, G, (int)blocks, skel, links, labels, stream);
}

static int skeleton_rows_run(const int32_t* groups, int G, int blocks, const uint8_t* links, const int32_t* labels,
                             const int32_t* d2, int32_t* rowid, int64_t* rows, int capacity, int M2, int32_t* ctrl,
                             int64_t* junctions, void* stream) {
  DY_RECORD_OR_RUN([=](void* s) {
    return skeleton_rows_run(groups, G, blocks, links, labels, d2, rowid, rows, capacity, M2, ctrl, junctions, s);
  });
  hipStream_t st = (hipStream_t)stream;
  ME_ZERO("skeleton_rows", ctrl, (size_t)(G + 1) * sizeof(int32_t), st);
  ME_ZERO("skeleton_rows", junctions, (size_t)G * 4 * sizeof(int64_t), st);
  if (blocks == 0) return DISYOLO_OK;
  hipLaunchKernelGGL(roots_alloc_kernel<BranchRow>, dim3(blocks), dim3(ME_T), 0, st, (const int*)groups, G, (const int*)labels,
                     (int*)rowid, (long long*)rows, capacity, (int*)ctrl, BranchRow{(unsigned long long*)junctions});
  DY_CHECK_LAUNCH();
  hipLaunchKernelGGL(skeleton_accum_kernel, dim3(blocks), dim3(ME_T), 0, st, (const int*)groups, G, (const unsigned char*)links,
                     (const int*)labels, (const int*)d2, (const int*)rowid, (unsigned long long*)rows, capacity,
                     (unsigned long long*)junctions);
  DY_CHECK_LAUNCH();
  if (capacity > 0) {
    const unsigned row_blocks = (unsigned)(((int64_t)capacity + ME_T - 1) / ME_T);
    hipLaunchKernelGGL(skeleton_finish_kernel, dim3(row_blocks), dim3(ME_T), 0, st, (long long*)rows, capacity, M2, (int*)ctrl);
    DY_CHECK_LAUNCH();
  }
  return DISYOLO_OK;
}

extern "C" int disyolo_skeleton_rows(const int32_t* groups_host, const int32_t* groups, int G, int64_t arena_bytes,
                                     const uint8_t* links, const int32_t* labels, const int32_t* d2, int32_t* rowid,
                                     int64_t* rows, int64_t capacity, int M2, int32_t* ctrl, int64_t* junctions, void* stream) {
  DY_REQUIRE(G <= 0 || (groups_host && groups && links && labels && d2 && rowid && ctrl && junctions && (rows || capacity == 0)),
             "skeleton_rows: null pointer");
  ME_ARGS("skeleton_rows");
  DY_REQUIRE(capacity >= 0 && capacity < (1ll << 31), "skeleton_rows: a capacity of %lld rows (need 0 .. 2^31 - 1)",
             (long long)capacity);
  DY_REQUIRE(M2 >= 0 && M2 <= SK_M2_MAX, "skeleton_rows: M2 = %d (twice min_branch_px: need 0 .. %d)", M2, SK_M2_MAX);
  ME_PLAN("skeleton_rows", nullptr);
  // (groups without a pixel still get their zero flag and their zero junction row)
  return skeleton_rows_run(groups, G, (int)blocks, links, labels, d2, rowid, rows, (int)capacity, M2, ctrl, junctions, stream);
}

static int skeleton_prune_run(const int32_t* groups, int G, int blocks, const int32_t* labels, const int32_t* rowid,
                              const int64_t* rows, int capacity, uint8_t* skel, void* stream) {
  DY_RECORD_OR_RUN([=](void* s) { return skeleton_prune_run(groups, G, blocks, labels, rowid, rows, capacity, skel, s); });
  hipLaunchKernelGGL(skeleton_prune_kernel, dim3(blocks), dim3(ME_T), 0, (hipStream_t)stream, (const int*)groups, G,
                     (const int*)labels, (const int*)rowid, (const long long*)rows, capacity, (unsigned char*)skel);
  DY_CHECK_LAUNCH();
  return DISYOLO_OK;
}

extern "C" int disyolo_skeleton_prune(const int32_t* groups_host, const int32_t* groups, int G, int64_t arena_bytes,
                                      const int32_t* labels, const int32_t* rowid, const int64_t* rows, int64_t capacity,
                                      uint8_t* skel, void* stream) {
  DY_REQUIRE(G <= 0 || (groups_host && groups && labels && rowid && skel && (rows || capacity == 0)), "skeleton_prune: null pointer");
  DY_REQUIRE(capacity >= 0 && capacity < (1ll << 31), "skeleton_prune: a capacity of %lld rows (need 0 .. 2^31 - 1)",
             (long long)capacity);
  ME_TABLES("skeleton_prune", nullptr);
  return skeleton_prune_run(groups, G, (int)blocks, labels, rowid, rows, (int)capacity, skel, stream);
}

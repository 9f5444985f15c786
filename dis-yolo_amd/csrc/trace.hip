// The traced skeleton graph: junction clusters as nodes, every branch ordered from one end to the other, what its two ends are,
// and the gathers of the ordered profiles (dis-yolo_amd/measure.py, skeleton_trace).
//
// The reference has no counterpart; the definition these kernels are held to is tests/trace_ref.py, and everything in it is an
// integer: there is no float in this file.  The arena-wide kernels read the [G,8] groups table as skeleton.hip does
// (measure_common.h): a block owns ME_CHUNK consecutive pixels of a crop, every per-pixel buffer lies in the arena's layout, and
// the elements between two crops are never read and never written.  The P pixels (degree <= 2, the pixels of branches) are
// compacted once into a list of entries, in any order; everything after that sweeps the list, not the arena, and writes to
// places that do not depend on the list's order.
//   links_init / links_merge / labels_flatten   the union-find of skeleton_label (arena_labels.h) over the links between two J
//                       pixels (degree >= 3, NodePixels below): a node ends at its smallest index
//   roots_alloc         every node root draws a row (NodeRow below)
//   trace_node_accum    every J pixel adds its integers to its node's row
//   trace_compact       every P pixel draws a list index and writes its entry: where it is, its (at most two) in-branch
//                       neighbours and its (at most two) J neighbours, each in ascending link bit
//   trace_link          the doubled state (entry, direction): state 2 i + s of entry i moves on to its neighbour s; its successor
//                       is that neighbour's state that moves away from i.  A state without a neighbour ahead is a terminal; a
//                       loop is cut between its root and the root's neighbour with the larger index
//   trace_round         pointer jumping, one launch per round between two buffers: next = next[next], (steps, diagonal steps)
//                       added up in one 64-bit word.  After K rounds with 2^K >= px - 1 every state stands at its terminal
//   trace_final         rank = the steps to the branch's start (a path: its end with the smaller index; a loop: its root)
//   trace_edge          every end pixel (and every loop's root) writes its branch's edge slot, chosen by its rank
//   trace_gather        every P pixel writes its entry of the branch profile at offset[row] + rank and, when its branch is on
//                       its instance's trunk, of the trunk profile; the J pixels between two branches of a trunk come from the
//                       host's plan
//   trace_trunk_rows    one block per instance reduces its trunk profile: integer sums, the maximum with its first position
// No block waits for another and none reads what another block writes in the same launch, the union-find apart, whose retry
// loops are lock-free (arena_labels.h).
#include "arena_labels.h"

namespace {

constexpr int TR_NODE = 8;           // int64 words of a node row: group, root, px, sum_y, sum_x, max_d2, n_attach, 0
constexpr int TR_EDGE = 12;          // int64 words of an edge row: group, root, end0_kind, end0_id, end1_kind, end1_id, attach0_px,
                                     // attach1_px, end0_px, end1_px, inner_diag (rank_diag of the last pixel), last_rank (px - 1)
constexpr int TR_ENT = 12;           // int32 words of a list entry
enum { E_POS = 0, E_P, E_ROOT, E_NB0, E_NB1, E_ATT0, E_ATT1, E_FLAGS, E_ROW, E_GROUP, E_D2, E_BW };
constexpr int F_DIAG0 = 1, F_DIAG1 = 2, F_LOOP = 4;
constexpr int TR_SEG = 4;            // int32 words per branch row of the trunk plan: dest (-1: not on a trunk), reversed, base_orth,
                                     // base_diag
constexpr int TR_ATT = 6;            // int32 words of an attach entry of the trunk plan: pos, dest, y, x, cum_orth, cum_diag
constexpr int TR_PROF = 4;           // int32 words of a branch profile entry: y, x, d2, rank_diag
constexpr int TR_TPROF = 5;          // int32 words of a trunk profile entry: y, x, d2, cum_orth, cum_diag
constexpr int TR_TRUNK = 8;          // int64 words of a trunk row: px, sum_q8, max_d2, max_pos, max_y, max_x, cum_orth, cum_diag (last)

// ---- nodes: what arena_labels.h is told --------------------------------------------------------------------------------------
// the J pixels: three links or more (an off pixel has none)
struct NodePixels {
  __device__ bool seed(size_t, unsigned links) const { return member(links); }
  __device__ static bool member(unsigned links) { return __popc(links) >= 3; }
};

struct NodeRow {
  static constexpr int WIDTH = TR_NODE;
  __device__ void drawn(int) const {}
  __device__ static long long empty(int) { return 0; }
};

// (J pixels are few beside the arena: one atomic per pixel and column)
__global__ __launch_bounds__(ME_T) void trace_node_accum_kernel(const int* groups, int G, const unsigned char* links, const int* nlab,
                                                                const int* d2, const int* noderow, unsigned long long* nodes,
                                                                int capacity) {
  const Crop c = crop_of_block(groups, G);
  const unsigned char* lk = links + c.off;
#pragma unroll
  for (int k = 0; k < ME_PX; ++k) {
    const int p = c.p0 + k * ME_T + threadIdx.x;
    if (p >= c.area) break;
    const int root = nlab[c.off + p];
    if (root < 0) continue;
    const int id = noderow[c.off + root];
    if (id < 0 || id >= capacity) continue;
    const unsigned l = lk[p];
    int attach = 0;
#pragma unroll
    for (int b = 0; b < 8; ++b)
      if ((l >> b & 1) && __popc(lk[p + nb_offset(b, c.bw)]) <= 2) ++attach;
    unsigned long long* r = nodes + (size_t)id * TR_NODE;
    const int y = p / c.bw;
    atomicAdd(&r[2], 1ull);
    atomicAdd(&r[3], (unsigned long long)y);
    atomicAdd(&r[4], (unsigned long long)(p - y * c.bw));
    atomicMax(&r[5], (unsigned long long)d2[c.off + p]);
    if (attach) atomicAdd(&r[6], (unsigned long long)attach);
  }
}

// ---- the list of P pixels ----------------------------------------------------------------------------------------------------
// rank holds a P pixel's list index until trace_final writes its rank there; -1 off P in both maps from here on
__global__ __launch_bounds__(ME_T) void trace_compact_kernel(const int* groups, int G, const unsigned char* links, const int* labels,
                                                             const int* d2, const int* rowid, const long long* rows,
                                                             int rows_capacity, int* ents, int capacity, int* count, int* rank,
                                                             int* rank_diag) {
  const Crop c = crop_of_block(groups, G);
  const unsigned char* lk = links + c.off;
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int k = 0; k < ME_PX; ++k) {                                    // (no lane leaves the loop early: ballots and shuffles)
    const int p = c.p0 + k * ME_T + threadIdx.x;
    const bool in = p < c.area;
    const int root = in ? labels[c.off + p] : -1;
    const bool isP = root >= 0;
    const unsigned long long mask = __ballot(isP);
    int base = 0;
    if (mask) {
      const int leader = __ffsll((long long)mask) - 1;
      if (lane == leader) base = atomicAdd(count, __popcll(mask));
      base = __shfl(base, leader, 64);
    }
    if (!in) continue;
    int idx = -1;
    if (isP) {
      idx = base + __popcll(mask & ((1ull << lane) - 1ull));
      if (idx >= capacity) idx = -1;
    }
    rank[c.off + p] = idx;
    rank_diag[c.off + p] = -1;
    if (idx < 0) continue;
    const unsigned l = lk[p];
    int nb[2] = {-1, -1}, att[2] = {-1, -1}, nn = 0, na = 0, flags = 0;
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      if (!(l >> b & 1)) continue;
      const int q = p + nb_offset(b, c.bw);
      if (__popc(lk[q]) <= 2) {
        if (nn < 2) {
          nb[nn] = (int)c.off + q;
          if (b & 1) flags |= nn ? F_DIAG1 : F_DIAG0;
        }
        ++nn;
      } else {
        if (na < 2) att[na] = (int)c.off + q;
        ++na;
      }
    }
    const int id = rowid[c.off + root];
    if (id >= 0 && id < rows_capacity) {
      const long long* r = rows + (size_t)id * SK_ROW;
      if (r[SK_N_END] == 0 && r[SK_N_ATTACH] == 0) flags |= F_LOOP;                    // no end and no attachment: every pixel has two neighbours
    }
    int* e = ents + (size_t)idx * TR_ENT;
    e[E_POS] = (int)c.off + p, e[E_P] = p, e[E_ROOT] = root, e[E_NB0] = nb[0], e[E_NB1] = nb[1], e[E_ATT0] = att[0], e[E_ATT1] = att[1];
    e[E_FLAGS] = flags, e[E_ROW] = id, e[E_GROUP] = c.g, e[E_D2] = d2[c.off + p], e[E_BW] = c.bw;
  }
}

__device__ __forceinline__ int list_len(const int* count, int capacity) { return min(*count, capacity); }

__global__ __launch_bounds__(ME_T) void trace_link_kernel(const int* ents, const int* count, int capacity, const int* rank, int* nxt,
                                                          unsigned long long* val) {
  const int n = list_len(count, capacity);
  const int i = blockIdx.x * ME_T + threadIdx.x;
  if (i >= n) return;
  const int* e = ents + (size_t)i * TR_ENT;
  const int pos = e[E_POS], flags = e[E_FLAGS];
  const int rootpos = pos - e[E_P] + e[E_ROOT];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const int q = s ? e[E_NB1] : e[E_NB0];
    bool terminal = q < 0;
    int qi = -1;
    if (!terminal) {
      qi = rank[q];
      if (qi < 0 || qi >= n) terminal = true;                          // (cannot happen: the list holds every P pixel)
    }
    if (!terminal && (flags & F_LOOP)) {
      if (pos == rootpos) {
        terminal = q == max(e[E_NB0], e[E_NB1]);
      } else if (q == rootpos) {
        const int* r = ents + (size_t)qi * TR_ENT;
        terminal = pos == max(r[E_NB0], r[E_NB1]);
      }
    }
    if (terminal) {
      nxt[2 * i + s] = 2 * i + s, val[2 * i + s] = 0;
    } else {
      const int s2 = ents[(size_t)qi * TR_ENT + E_NB0] == pos ? 1 : 0;  // the neighbour's state that moves away from here
      nxt[2 * i + s] = 2 * qi + s2;
      val[2 * i + s] = 1ull << 32 | (unsigned long long)((flags >> s) & 1);
    }
  }
}

__global__ __launch_bounds__(ME_T) void trace_round_kernel(const int* count, int capacity, const int* nin, const unsigned long long* vin,
                                                           int* nout, unsigned long long* vout) {
  const int n2 = 2 * list_len(count, capacity);
  const int s = blockIdx.x * ME_T + threadIdx.x;
  if (s >= n2) return;
  const int t = nin[s];
  nout[s] = nin[t];
  vout[s] = vin[s] + vin[t];
}

__global__ __launch_bounds__(ME_T) void trace_final_kernel(const int* ents, const int* count, int capacity, const int* nxt,
                                                           const unsigned long long* val, int* rank, int* rank_diag) {
  const int n = list_len(count, capacity);
  const int i = blockIdx.x * ME_T + threadIdx.x;
  if (i >= n) return;
  const int* e = ents + (size_t)i * TR_ENT;
  const int pos = e[E_POS];
  const int e0 = ents[(size_t)(nxt[2 * i] >> 1) * TR_ENT + E_POS], e1 = ents[(size_t)(nxt[2 * i + 1] >> 1) * TR_ENT + E_POS];
  int s;
  if (e[E_FLAGS] & F_LOOP) s = e0 == pos - e[E_P] + e[E_ROOT] ? 0 : 1;
  else s = e0 <= e1 ? 0 : 1;                                          // (a single pixel: both its own, both 0 steps)
  const unsigned long long v = val[2 * i + s];
  rank[pos] = (int)(v >> 32);
  rank_diag[pos] = (int)(v & 0xffffffffull);
}

// ---- edges -------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void edge_end(long long* r, int slot, int att, int off, int p, const int* nlab) {
  r[2 + 2 * slot] = att >= 0 ? 1 : 0;
  r[3 + 2 * slot] = att >= 0 ? nlab[att] : p;
  r[6 + slot] = att >= 0 ? att - off : -1;
  r[8 + slot] = p;
}

__global__ __launch_bounds__(ME_T) void trace_edge_kernel(const int* ents, const int* count, int capacity, const int* rank,
                                                          const int* rank_diag, const int* nlab, long long* edges, int edges_capacity) {
  const int n = list_len(count, capacity);
  const int i = blockIdx.x * ME_T + threadIdx.x;
  if (i >= n) return;
  const int* e = ents + (size_t)i * TR_ENT;
  const int row = e[E_ROW], pos = e[E_POS], p = e[E_P], off = pos - p;
  if (row < 0 || row >= edges_capacity) return;
  long long* r = edges + (size_t)row * TR_EDGE;
  if (e[E_FLAGS] & F_LOOP) {
    if (p != e[E_ROOT]) return;
    const int last = max(e[E_NB0], e[E_NB1]);
    r[0] = e[E_GROUP], r[1] = p, r[2] = 2, r[3] = p, r[4] = 2, r[5] = p, r[6] = -1, r[7] = -1, r[8] = p, r[9] = last - off;
    r[10] = rank_diag[last], r[11] = rank[last];
    return;
  }
  if (e[E_NB1] >= 0) return;                                          // two in-branch neighbours: no end
  if (e[E_NB0] < 0) {                                                 // a single pixel is both ends
    r[0] = e[E_GROUP], r[1] = e[E_ROOT];
    edge_end(r, 0, e[E_ATT0], off, p, nlab);
    edge_end(r, 1, e[E_ATT1], off, p, nlab);
    r[10] = 0, r[11] = 0;
    return;
  }
  const int rk = rank[pos];
  if (rk == 0) {
    r[0] = e[E_GROUP], r[1] = e[E_ROOT];
    edge_end(r, 0, e[E_ATT0], off, p, nlab);
  } else {
    edge_end(r, 1, e[E_ATT0], off, p, nlab);
    r[10] = rank_diag[pos], r[11] = rk;
  }
}

// ---- profiles ----------------------------------------------------------------------------------------------------------------
// threads 0 .. n-1: the P pixels; threads capacity .. capacity + n_att - 1: the attach entries of the trunk plan
__global__ __launch_bounds__(ME_T) void trace_gather_kernel(const int* ents, const int* count, int capacity, const int* rank,
                                                            const int* rank_diag, const int* d2, long long arena_bytes,
                                                            const int* offsets, int n_rows, int* profile, const int* seg,
                                                            const long long* edges, const int* attach, int n_att, int* tprofile,
                                                            int tprofile_len) {
  const long long i = (long long)blockIdx.x * ME_T + threadIdx.x;
  if (i >= capacity) {
    const long long a = i - capacity;
    if (a >= n_att) return;
    const int* t = attach + (size_t)a * TR_ATT;
    if (t[0] < 0 || t[0] >= arena_bytes || t[1] < 0 || t[1] >= tprofile_len) return;
    int* o = tprofile + (size_t)t[1] * TR_TPROF;
    o[0] = t[2], o[1] = t[3], o[2] = d2[t[0]], o[3] = t[4], o[4] = t[5];
    return;
  }
  if (i >= list_len(count, capacity)) return;
  const int* e = ents + (size_t)i * TR_ENT;
  const int row = e[E_ROW], pos = e[E_POS];
  if (row < 0 || row >= n_rows) return;
  const int y = e[E_P] / e[E_BW], x = e[E_P] - y * e[E_BW];
  const int rk = rank[pos], rd = rank_diag[pos];
  const long long at = (long long)offsets[row] + rk;
  if (at >= 0 && at < capacity) {
    int* o = profile + (size_t)at * TR_PROF;
    o[0] = y, o[1] = x, o[2] = e[E_D2], o[3] = rd;
  }
  const int* sg = seg + (size_t)row * TR_SEG;
  if (sg[0] < 0) return;
  const long long* er = edges + (size_t)row * TR_EDGE;
  const int k = sg[1] ? (int)er[11] - rk : rk, dg = sg[1] ? (int)er[10] - rd : rd;
  const long long dest = (long long)sg[0] + k;
  if (dest < 0 || dest >= tprofile_len) return;
  int* o = tprofile + (size_t)dest * TR_TPROF;
  o[0] = y, o[1] = x, o[2] = e[E_D2], o[3] = sg[2] + (k - dg), o[4] = sg[3] + dg;
}

// one block per instance: tstart int32 [G + 1] = where its trunk profile begins.  The maximum with its first position is the
// maximum of (d2 << 32 | ~position)
__global__ __launch_bounds__(ME_T) void trace_trunk_rows_kernel(const int* tstart, const int* tprofile, int tprofile_len,
                                                                long long* trunkrows) {
  __shared__ long long ssum[ME_T / 64], skey[ME_T / 64];
  const int g = blockIdx.x;
  const int a = max(tstart[g], 0), b = min(tstart[g + 1], tprofile_len);
  long long sum = 0, key = -1;
  for (int i = a + (int)threadIdx.x; i < b; i += ME_T) {
    const int d = tprofile[(size_t)i * TR_TPROF + 2];
    sum += isqrt_q8(d);
    key = max(key, (long long)d << 32 | (long long)(0x7fffffff - (i - a)));
  }
  sum = wave_sum_ll(sum), key = wave_max_ll(key);
  if ((threadIdx.x & 63) == 0) ssum[threadIdx.x >> 6] = sum, skey[threadIdx.x >> 6] = key;
  __syncthreads();
  if (threadIdx.x != 0) return;
  for (int w = 1; w < ME_T / 64; ++w) sum += ssum[w], key = max(key, skey[w]);
  long long* r = trunkrows + (size_t)g * TR_TRUNK;
  if (b <= a) {
    for (int q = 0; q < TR_TRUNK; ++q) r[q] = 0;
    return;
  }
  const int at = 0x7fffffff - (int)(key & 0x7fffffffll);
  const int* m = tprofile + (size_t)(a + at) * TR_TPROF, *last = tprofile + (size_t)(b - 1) * TR_TPROF;
  r[0] = b - a, r[1] = sum, r[2] = key >> 32, r[3] = at, r[4] = m[0], r[5] = m[1], r[6] = last[3], r[7] = last[4];
}

constexpr long long TR_MAX_LIST = 1ll << 30;

}  // namespace

#define TR_ARENA(who)                                                                                                           \
  DY_REQUIRE(arena_bytes < (1ll << 31), who ": an arena of %lld elements (positions are int32: need < 2^31)", (long long)arena_bytes)

static int trace_nodes_run(const int32_t* groups, int G, int blocks, const uint8_t* links, const int32_t* d2, int32_t* node_labels,
                           int32_t* noderow, int64_t* nodes, int capacity, int32_t* ctrl, void* stream) {
  DY_RECORD_OR_RUN([=](void* s) { return trace_nodes_run(groups, G, blocks, links, d2, node_labels, noderow, nodes, capacity, ctrl, s); });
  hipStream_t st = (hipStream_t)stream;
  ME_ZERO("trace_nodes", ctrl, sizeof(int32_t), st);
  if (blocks == 0) return DISYOLO_OK;
  const int* g = (const int*)groups;
  const unsigned char* lk = (const unsigned char*)links;
  hipLaunchKernelGGL(links_init_kernel<NodePixels>, dim3(blocks), dim3(ME_T), 0, st, g, G, NodePixels{}, lk, (int*)node_labels);
  DY_CHECK_LAUNCH();
  hipLaunchKernelGGL(links_merge_kernel<NodePixels>, dim3(blocks), dim3(ME_T), 0, st, g, G, lk, (int*)node_labels);
  DY_CHECK_LAUNCH();
  hipLaunchKernelGGL(labels_flatten_kernel<LINKS_HALVE>, dim3(blocks), dim3(ME_T), 0, st, g, G, (int*)node_labels);
  DY_CHECK_LAUNCH();
  hipLaunchKernelGGL(roots_alloc_kernel<NodeRow>, dim3(blocks), dim3(ME_T), 0, st, g, G, (const int*)node_labels, (int*)noderow,
                     (long long*)nodes, capacity, (int*)ctrl, NodeRow{});
  DY_CHECK_LAUNCH();
  hipLaunchKernelGGL(trace_node_accum_kernel, dim3(blocks), dim3(ME_T), 0, st, g, G, lk, (const int*)node_labels, (const int*)d2,
                     (const int*)noderow, (unsigned long long*)nodes, capacity);
  DY_CHECK_LAUNCH();
  return DISYOLO_OK;
}

extern "C" int disyolo_trace_nodes(const int32_t* groups_host, const int32_t* groups, int G, int64_t arena_bytes, const uint8_t* links,
                                   const int32_t* d2, int32_t* node_labels, int32_t* noderow, int64_t* nodes, int64_t capacity,
                                   int32_t* ctrl, void* stream) {
  DY_REQUIRE(G <= 0 || (groups_host && groups && links && d2 && node_labels && noderow && ctrl && (nodes || capacity == 0)),
             "trace_nodes: null pointer");
  ME_ARGS("trace_nodes");
  DY_REQUIRE(capacity >= 0 && capacity < (1ll << 31), "trace_nodes: a capacity of %lld rows (need 0 .. 2^31 - 1)", (long long)capacity);
  ME_PLAN("trace_nodes", nullptr);
  // (groups without a pixel still get the zero counter)
  return trace_nodes_run(groups, G, (int)blocks, links, d2, node_labels, noderow, nodes, (int)capacity, ctrl, stream);
}

static int trace_rank_run(const int32_t* groups, int G, int blocks, const uint8_t* links, const int32_t* labels, const int32_t* d2,
                          const int32_t* rowid, const int64_t* rows, int rows_capacity, int32_t* ents, int capacity, int rounds,
                          int32_t* nxt, int64_t* val, int32_t* count, int32_t* rank, int32_t* rank_diag, void* stream) {
  DY_RECORD_OR_RUN([=](void* s) {
    return trace_rank_run(groups, G, blocks, links, labels, d2, rowid, rows, rows_capacity, ents, capacity, rounds, nxt, val, count,
                          rank, rank_diag, s);
  });
  hipStream_t st = (hipStream_t)stream;
  ME_ZERO("trace_rank", count, sizeof(int32_t), st);
  if (blocks == 0) return DISYOLO_OK;
  hipLaunchKernelGGL(trace_compact_kernel, dim3(blocks), dim3(ME_T), 0, st, (const int*)groups, G, (const unsigned char*)links,
                     (const int*)labels, (const int*)d2, (const int*)rowid, (const long long*)rows, rows_capacity, (int*)ents,
                     capacity, (int*)count, (int*)rank, (int*)rank_diag);
  DY_CHECK_LAUNCH();
  if (capacity == 0) return DISYOLO_OK;
  const unsigned lb = (unsigned)(((int64_t)capacity + ME_T - 1) / ME_T), sb = (unsigned)((2 * (int64_t)capacity + ME_T - 1) / ME_T);
  int* n0 = (int*)nxt, *n1 = n0 + 2 * (size_t)capacity;
  unsigned long long* v0 = (unsigned long long*)val, *v1 = v0 + 2 * (size_t)capacity;
  hipLaunchKernelGGL(trace_link_kernel, dim3(lb), dim3(ME_T), 0, st, (const int*)ents, (const int*)count, capacity, (const int*)rank,
                     n0, v0);
  DY_CHECK_LAUNCH();
  for (int r = 0; r < rounds; ++r) {
    hipLaunchKernelGGL(trace_round_kernel, dim3(sb), dim3(ME_T), 0, st, (const int*)count, capacity, (const int*)(r & 1 ? n1 : n0),
                       (const unsigned long long*)(r & 1 ? v1 : v0), r & 1 ? n0 : n1, r & 1 ? v0 : v1);
    DY_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(trace_final_kernel, dim3(lb), dim3(ME_T), 0, st, (const int*)ents, (const int*)count, capacity,
                     (const int*)(rounds & 1 ? n1 : n0), (const unsigned long long*)(rounds & 1 ? v1 : v0), (int*)rank, (int*)rank_diag);
  DY_CHECK_LAUNCH();
  return DISYOLO_OK;
}

extern "C" int disyolo_trace_rank(const int32_t* groups_host, const int32_t* groups, int G, int64_t arena_bytes, const uint8_t* links,
                                  const int32_t* labels, const int32_t* d2, const int32_t* rowid, const int64_t* rows,
                                  int64_t rows_capacity, int32_t* ents, int64_t capacity, int rounds, int32_t* nxt, int64_t* val,
                                  int32_t* count, int32_t* rank, int32_t* rank_diag, void* stream) {
  DY_REQUIRE(G <= 0 || (groups_host && groups && links && labels && d2 && rowid && count && rank && rank_diag &&
                        (rows || rows_capacity == 0) && ((ents && nxt && val) || capacity == 0)),
             "trace_rank: null pointer");
  ME_ARGS("trace_rank");
  TR_ARENA("trace_rank");
  DY_REQUIRE(capacity >= 0 && capacity <= TR_MAX_LIST, "trace_rank: a capacity of %lld list entries (need 0 .. 2^30)", (long long)capacity);
  DY_REQUIRE(rows_capacity >= 0 && rows_capacity < (1ll << 31), "trace_rank: a capacity of %lld rows (need 0 .. 2^31 - 1)",
             (long long)rows_capacity);
  DY_REQUIRE(rounds >= 0 && rounds <= 31, "trace_rank: rounds = %d (need 0 .. 31)", rounds);
  ME_PLAN("trace_rank", nullptr);
  return trace_rank_run(groups, G, (int)blocks, links, labels, d2, rowid, rows, (int)rows_capacity, ents, (int)capacity, rounds, nxt, val,
                        count, rank, rank_diag, stream);
}

static int trace_edges_run(const int32_t* ents, const int32_t* count, int capacity, const int32_t* rank, const int32_t* rank_diag,
                           const int32_t* node_labels, int64_t* edges, int edges_capacity, void* stream) {
  DY_RECORD_OR_RUN([=](void* s) { return trace_edges_run(ents, count, capacity, rank, rank_diag, node_labels, edges, edges_capacity, s); });
  hipLaunchKernelGGL(trace_edge_kernel, dim3((unsigned)(((int64_t)capacity + ME_T - 1) / ME_T)), dim3(ME_T), 0, (hipStream_t)stream,
                     (const int*)ents, (const int*)count, capacity, (const int*)rank, (const int*)rank_diag, (const int*)node_labels,
                     (long long*)edges, edges_capacity);
  DY_CHECK_LAUNCH();
  return DISYOLO_OK;
}

extern "C" int disyolo_trace_edges(const int32_t* groups_host, const int32_t* groups, int G, int64_t arena_bytes, const int32_t* ents,
                                   const int32_t* count, int64_t capacity, const int32_t* rank, const int32_t* rank_diag,
                                   const int32_t* node_labels, int64_t* edges, int64_t edges_capacity, void* stream) {
  DY_REQUIRE(G <= 0 || (groups_host && groups && count && rank && rank_diag && node_labels && (ents || capacity == 0) &&
                        (edges || edges_capacity == 0)),
             "trace_edges: null pointer");
  DY_REQUIRE(capacity >= 0 && capacity <= TR_MAX_LIST, "trace_edges: a capacity of %lld list entries (need 0 .. 2^30)", (long long)capacity);
  DY_REQUIRE(edges_capacity >= 0 && edges_capacity < (1ll << 31), "trace_edges: a capacity of %lld rows (need 0 .. 2^31 - 1)",
             (long long)edges_capacity);
  ME_TABLES("trace_edges", nullptr);
  TR_ARENA("trace_edges");
  if (capacity == 0) return DISYOLO_OK;
  return trace_edges_run(ents, count, (int)capacity, rank, rank_diag, node_labels, edges, (int)edges_capacity, stream);
}

static int trace_gather_run(int G, const int32_t* ents, const int32_t* count, int capacity, const int32_t* rank, const int32_t* rank_diag,
                            const int32_t* d2, int64_t arena_bytes, const int32_t* offsets, int n_rows, int32_t* profile,
                            const int32_t* seg, const int64_t* edges, const int32_t* attach, int n_attach, int32_t* tprofile,
                            int tprofile_len, const int32_t* tstart, int64_t* trunkrows, void* stream) {
  DY_RECORD_OR_RUN([=](void* s) {
    return trace_gather_run(G, ents, count, capacity, rank, rank_diag, d2, arena_bytes, offsets, n_rows, profile, seg, edges, attach,
                            n_attach, tprofile, tprofile_len, tstart, trunkrows, s);
  });
  hipStream_t st = (hipStream_t)stream;
  const int64_t threads = (int64_t)capacity + n_attach;
  if (threads > 0) {
    hipLaunchKernelGGL(trace_gather_kernel, dim3((unsigned)((threads + ME_T - 1) / ME_T)), dim3(ME_T), 0, st, (const int*)ents,
                       (const int*)count, capacity, (const int*)rank, (const int*)rank_diag, (const int*)d2, (long long)arena_bytes,
                       (const int*)offsets, n_rows, (int*)profile, (const int*)seg, (const long long*)edges, (const int*)attach,
                       n_attach, (int*)tprofile, tprofile_len);
    DY_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(trace_trunk_rows_kernel, dim3(G), dim3(ME_T), 0, st, (const int*)tstart, (const int*)tprofile, tprofile_len,
                     (long long*)trunkrows);
  DY_CHECK_LAUNCH();
  return DISYOLO_OK;
}

extern "C" int disyolo_trace_gather(const int32_t* groups_host, const int32_t* groups, int G, int64_t arena_bytes, const int32_t* ents,
                                    const int32_t* count, int64_t capacity, const int32_t* rank, const int32_t* rank_diag,
                                    const int32_t* d2, const int32_t* offsets, int64_t n_rows, int32_t* profile, const int32_t* seg,
                                    const int64_t* edges, const int32_t* attach, int64_t n_attach, int32_t* tprofile,
                                    int64_t tprofile_len, const int32_t* tstart, int64_t* trunkrows, void* stream) {
  DY_REQUIRE(G <= 0 || (groups_host && groups && count && rank && rank_diag && d2 && tstart && trunkrows &&
                        ((ents && profile) || capacity == 0) && ((offsets && seg && edges) || n_rows == 0) &&
                        (attach || n_attach == 0) && (tprofile || tprofile_len == 0)),
             "trace_gather: null pointer");
  DY_REQUIRE(capacity >= 0 && capacity <= TR_MAX_LIST, "trace_gather: a capacity of %lld list entries (need 0 .. 2^30)", (long long)capacity);
  DY_REQUIRE(n_rows >= 0 && n_rows < (1ll << 31), "trace_gather: %lld rows (need 0 .. 2^31 - 1)", (long long)n_rows);
  DY_REQUIRE(n_attach >= 0 && n_attach <= TR_MAX_LIST && tprofile_len >= 0 && tprofile_len <= TR_MAX_LIST,
             "trace_gather: a plan of %lld attach entries and %lld profile entries (need 0 .. 2^30 each)", (long long)n_attach,
             (long long)tprofile_len);
  ME_ARGS("trace_gather");
  TR_ARENA("trace_gather");
  ME_PLAN("trace_gather", nullptr);
  // (groups without a pixel still get their zero trunk row)
  return trace_gather_run(G, ents, count, (int)capacity, rank, rank_diag, d2, arena_bytes, offsets, (int)n_rows, profile, seg, edges, attach,
                          (int)n_attach, tprofile, (int)tprofile_len, tstart, trunkrows, stream);
}

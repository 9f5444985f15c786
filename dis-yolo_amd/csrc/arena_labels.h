// Labelling over the arena of cropped masks, for skeleton.hip (branches), trace.hip (nodes) and shape.hip (parts): the lock-free
// union-find, the flatten launch, the init and merge launches over the link bits of skeleton_classify, and the launch in which
// every root draws a row.  A label array lies in the arena's layout: within its crop a pixel's label is the index of a pixel of
// the same component (its parent), its own on a root, -1 off the set.
#pragma once
#include "measure_common.h"

namespace {

// ---- union-find ------------------------------------------------------------------------------------------------------------
// Within the merge and the flatten launch the label array is touched with agent-scope atomics only: a plain load could be
// served from another XCD's L2.  The invariant: a label never grows, and L[i] <= i always -- an init writes a pixel's own index
// or a smaller one of its component, and every later write is an atomic min with an ancestor.  So every walk ends at a root,
// however the writes of other threads fall between its loads.
__device__ __forceinline__ int uf_load(int* L, int i) { return __hip_atomic_load(L + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// Path halving on the way: a pixel met on the walk is hung under its grandparent, an ancestor with a smaller index, by the same
// atomic min -- on a solid blob the roots of the row runs would otherwise form chains as long as the blob is high.  The pixel
// written was seen with a parent below it, and labels never grow: it is no root and never becomes one, so halving never touches
// a root, and uf_union's "old == a" still means that a was one.  Halve = false is the plain walk, which writes nothing.
template <bool Halve = true>
__device__ __forceinline__ int uf_find(int* L, int i) {
  for (;;) {
    const int p = uf_load(L, i);
    if (p == i) return i;
    if (!Halve) { i = p; continue; }
    const int gp = uf_load(L, p);
    if (gp == p) return p;
    __hip_atomic_fetch_min(L + i, gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    i = gp;
  }
}

// The components over link bits are one-pixel-wide curves and junction clusters of a few pixels: after the merge from the upper
// (left) pixel their walks are short, and the second load and the atomic per step cost more than the shorter paths save
// (disyolo_skeleton_label 143 -> 166 us with halving, profiles/arena_refactor_rate.txt).  So links_merge and the flatten after it
// walk plainly; the parts of shape.hip, whose run roots chain down a solid blob, halve (819 -> 567 us on the disc).
constexpr bool LINKS_HALVE = false;

// The larger root is hung under the smaller one with an atomic min, so a component ends at its smallest index whatever the order
// of arrival.  No thread waits for another: every turn either succeeds or meets a label that another thread has made smaller, and
// labels are bounded below.
template <bool Halve = true>
__device__ __forceinline__ void uf_union(int* L, int a, int b) {
  for (;;) {
    a = uf_find<Halve>(L, a), b = uf_find<Halve>(L, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b, b = t; }
    const int old = __hip_atomic_fetch_min(L + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (old == a) return;            // a was a root and hangs under b now (halving never touches a root)
    a = old;                         // another thread hung a under `old` first: L[a] = min(old, b), and old is joined with b
  }
}

// labels = the root of every pixel of the set.  After this launch a label is the smallest index of its component whether the
// walks halved their paths or not: halving changes which ancestor a pixel points to on the way, never the root it ends at.
template <bool Halve = true>
__global__ __launch_bounds__(ME_T) void labels_flatten_kernel(const int* groups, int G, int* labels) {
  const Crop c = crop_of_block(groups, G);
  int* L = labels + c.off;
#pragma unroll
  for (int k = 0; k < ME_PX; ++k) {
    const int p = c.p0 + k * ME_T + threadIdx.x;
    if (p >= c.area) break;
    const int l = uf_load(L, p);
    if (l < 0 || l == p) continue;
    __hip_atomic_store(L + p, uf_find<Halve>(L, l), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (any ancestor is a valid parent)
  }
}

// ---- components over the link bits ------------------------------------------------------------------------------------------
// Set says which pixels are labelled: set.seed(i, links) for arena element i in the init, and Set::member(links) for a pixel
// known to lie on the skeleton (its own or a linked neighbour's byte) in the merge.
template <class Set>
__global__ __launch_bounds__(ME_T) void links_init_kernel(const int* groups, int G, Set set, const unsigned char* links, int* labels) {
  const Crop c = crop_of_block(groups, G);
#pragma unroll
  for (int k = 0; k < ME_PX; ++k) {
    const int p = c.p0 + k * ME_T + threadIdx.x;
    if (p >= c.area) break;
    labels[c.off + p] = set.seed(c.off + p, links[c.off + p]) ? p : -1;
  }
}

// a pair is merged from its upper (or, in a row, left) pixel: bits 2 .. 5 = E, SE, S, SW
template <class Set>
__global__ __launch_bounds__(ME_T) void links_merge_kernel(const int* groups, int G, const unsigned char* links, int* labels) {
  const Crop c = crop_of_block(groups, G);
  const unsigned char* lk = links + c.off;
  int* L = labels + c.off;
#pragma unroll
  for (int k = 0; k < ME_PX; ++k) {
    const int p = c.p0 + k * ME_T + threadIdx.x;
    if (p >= c.area) break;
    const unsigned l = lk[p];
    if ((l & 0x3c) == 0 || !Set::member(l)) continue;
#pragma unroll
    for (int b = 2; b <= 5; ++b) {
      if (!(l >> b & 1)) continue;
      const int q = p + nb_offset(b, c.bw);
      if (Set::member(lk[q])) uf_union<LINKS_HALVE>(L, p, q);
    }
  }
}

// ---- rows -------------------------------------------------------------------------------------------------------------------
// Every root draws a row number from the counter ctrl[0], which keeps counting beyond `capacity` without anything being written
// there, and writes its row's head: group, root, then Row::WIDTH - 2 words of Row::empty(column).  row.drawn(group) is whatever
// else a root does.
template <class Row>
__global__ __launch_bounds__(ME_T) void roots_alloc_kernel(const int* groups, int G, const int* labels, int* rowid, long long* rows,
                                                           int capacity, int* ctrl, Row row) {
  const Crop c = crop_of_block(groups, G);
#pragma unroll
  for (int k = 0; k < ME_PX; ++k) {
    const int p = c.p0 + k * ME_T + threadIdx.x;
    if (p >= c.area) break;
    if (labels[c.off + p] != p) continue;
    const int id = atomicAdd(&ctrl[0], 1);
    rowid[c.off + p] = id;
    row.drawn(c.g);
    if (id < capacity) {
      long long* r = rows + (size_t)id * Row::WIDTH;
      r[0] = c.g, r[1] = p;
#pragma unroll
      for (int q = 2; q < Row::WIDTH; ++q) r[q] = Row::empty(q);
    }
  }
}

}  // namespace

// Detection decode + filter and the inference-time position-sensitive mask assembly.
//
// Replaces interpret_output / filter_detections / clip_boxes_graph / val_test of
// yolo/yolo3_net_pos.py:465-628, 862-952 (the reference unrolls these per image in Python
// and runs tf.image.non_max_suppression per class through tf.map_fn).
#include <array>
#include <vector>
#include "common.h"
#include "paste_bit.h"
#include "runtime.h"

namespace {

struct ScaleInfo {
  const float* logits;  // [B,gh,gw,3,5+C]
  int gh, gw;
  int cand0;  // first candidate index of this scale inside an image
  float aw[3], ah[3];
};
struct DecodeParams {
  ScaleInfo sc[3];
  int B, H, W, C, NC;   // H x W = the net's input (net_h, net_w)
  const float* window;  // [B,4] y1,x1,y2,x2
  float4* boxes;        // [B][NC] (y1,x1,y2,x2)
  float* scores;        // [B][NC]
  int* classes;         // [B][NC]
};

__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }

// candidate order inside an image: scale (1/8, 1/16, 1/32 grids), then y, x, anchor (row-major)
// (yolo/yolo3_net_pos.py:527-542)
__global__ __launch_bounds__(256) void decode_score_kernel(DecodeParams p) {
  const int b = blockIdx.y;
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= p.NC) return;
  int s = 0;
  if (idx >= p.sc[1].cand0) s = 1;
  if (idx >= p.sc[2].cand0) s = 2;
  const ScaleInfo& si = p.sc[s];
  const int local = idx - si.cand0;
  const int a = local % 3;
  const int cell = local / 3;
  const int x = cell % si.gw, y = cell / si.gw;
  const int D = 5 + p.C;
  const float* t = si.logits + (((size_t)b * si.gh * si.gw + cell) * 3 + a) * D;
  const float conf = sigmoidf_(t[4]);
  // softmax max-probability and argmax (first maximum wins, tf.argmax)
  float mx = t[5];
  int arg = 0;
  for (int c = 1; c < p.C; ++c)
    if (t[5 + c] > mx) {
      mx = t[5 + c];
      arg = c;
    }
  float den = 0.f;
  for (int c = 0; c < p.C; ++c) den += expf(t[5 + c] - mx);
  const float score = conf * (1.f / den);
  // grid_factor = [gw, gh], net_factor = [net_w, net_h] (yolo/yolo3_net_pos.py:473-506)
  const float xc = ((float)x + sigmoidf_(t[0])) / (float)si.gw;
  const float yc = ((float)y + sigmoidf_(t[1])) / (float)si.gh;
  const float w = expf(t[2]) * si.aw[a] / (float)p.W;
  const float h = expf(t[3]) * si.ah[a] / (float)p.H;
  const float* win = p.window + b * 4;
  float4 bx;
  bx.x = fmaxf(fminf(yc - h / 2.f, win[2]), win[0]);
  bx.y = fmaxf(fminf(xc - w / 2.f, win[3]), win[1]);
  bx.z = fmaxf(fminf(yc + h / 2.f, win[2]), win[0]);
  bx.w = fmaxf(fminf(xc + w / 2.f, win[3]), win[1]);
  const size_t o = (size_t)b * p.NC + idx;
  p.boxes[o] = bx;
  p.scores[o] = score;
  p.classes[o] = arg;
}

// IoU as tf.image.non_max_suppression computes it (corner order normalised, empty box -> 0)
__device__ __forceinline__ float nms_iou(const float4& a, const float4& b) {
  const float ya1 = fminf(a.x, a.z), xa1 = fminf(a.y, a.w), ya2 = fmaxf(a.x, a.z), xa2 = fmaxf(a.y, a.w);
  const float yb1 = fminf(b.x, b.z), xb1 = fminf(b.y, b.w), yb2 = fmaxf(b.x, b.z), xb2 = fmaxf(b.y, b.w);
  const float aa = (ya2 - ya1) * (xa2 - xa1), ab = (yb2 - yb1) * (xb2 - xb1);
  if (aa <= 0.f || ab <= 0.f) return 0.f;
  const float iy1 = fmaxf(ya1, yb1), ix1 = fmaxf(xa1, xb1), iy2 = fminf(ya2, yb2), ix2 = fminf(xa2, xb2);
  const float inter = fmaxf(iy2 - iy1, 0.f) * fmaxf(ix2 - ix1, 0.f);
  return inter / (aa + ab - inter);
}

// Detection filter.  Stage 1: one block per (image, class): ordered compaction of the
// candidates with score > thr and arg-max class == c, then greedy NMS (IoU > nms_thr
// suppresses, at most max_det kept) as a repeated block-wide arg-max over the live list --
// exact for any number of candidates, never a truncated sort.  Stage 2: one block per image
// merges the per-class survivors: top max_det by score (ties: lower candidate index), zero
// padded.
//
// The live list sits in REGISTERS while it fits (<= NMS_K candidates per thread, 8,192 per
// block: score and box of list position q are held by thread q % NMS_T).  One
// round of the greedy loop is then ONE pass over a thread's slots -- suppress against the
// last winner and find the thread's best survivor in the same sweep -- and ONE barrier: the
// wave winners (score, position, box) go to LDS, double-buffered by round parity, and
// every thread picks the block winner from the 16 entries.  An untrained network passes
// thousands of candidates per class (random logits at 576^2: ~6,800 of 20,412); with the list
// in global memory a round cost 16 us (two dependent sweeps + two barriers), 30 rounds = 0.5 ms
// on the chain that holds up the mask subnet's backward pass; in registers a round is ~1 us.
// Longer lists (one class taking > 8,192 candidates) keep the global-memory form.  (The image-wide modes, one list per image
// whatever the class: nms_image_kernel below, 20 slots per thread.)
constexpr int NMS_T = 1024;
constexpr int NMS_K = 8;
constexpr int NMS_W = NMS_T / 64;
constexpr int NMS_CB = 8;             // compaction rounds per barrier
constexpr int MAX_KEEP = 512;  // >= num_class * max_det

__device__ __forceinline__ bool nms_better(float v2, int p2, float v, int p) { return v2 > v || (v2 == v && p2 < p); }

__device__ __forceinline__ int greedy_nms_global(int n, const int* list, const float4* boxes, float* live, float nms_thr,
                                                 int max_det, int* kept_idx, float* kept_sc, float* s_ws, int* s_wp) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  int nk = 0;
  for (int it = 0; it < max_det; ++it) {
    float bs = -1.f;
    int bp = 0x7fffffff;
    for (int q = tid; q < n; q += NMS_T) {
      const float v = live[q];
      if (v > bs) {  // ascending scan: lowest position wins among equal scores
        bs = v;
        bp = q;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float v2 = __shfl_xor(bs, o, 64);
      const int p2 = __shfl_xor(bp, o, 64);
      if (nms_better(v2, p2, bs, bp)) {
        bs = v2;
        bp = p2;
      }
    }
    if (lane == 0) {
      s_ws[wv] = bs;
      s_wp[wv] = bp;
    }
    __syncthreads();
    float wsc = s_ws[0];
    int wq = s_wp[0];
#pragma unroll
    for (int w = 1; w < NMS_W; ++w) {
      const float v2 = s_ws[w];
      const int p2 = s_wp[w];
      if (nms_better(v2, p2, wsc, wq)) {
        wsc = v2;
        wq = p2;
      }
    }
    if (!(wsc > 0.f)) break;  // nothing alive (live scores are > thr >= 0); uniform exit
    const float4 wb = boxes[list[wq]];
    if (tid == 0) {
      kept_idx[nk] = list[wq];
      kept_sc[nk] = wsc;
    }
    ++nk;
    for (int q = tid; q < n; q += NMS_T) {
      if (live[q] >= 0.f) {
        const float4 bx = boxes[list[q]];
        if (q == wq || nms_iou(bx, wb) > nms_thr) live[q] = -1.f;
      }
    }
    __syncthreads();
  }
  return nk;
}

// The greedy loop over one (image, class) list, shared by the kernel that compacts its own list (<= 16 classes) and the one
// that takes a segment of the bucketed list (more classes): list[0..n) holds candidate indices in ascending order, scores /
// boxes are the image's, live_glob has room for n floats.  All NMS_T threads of the block call it; kept_idx / kept_sc receive
// the survivors in selection order and the count is returned to every thread.  KMAX >= max_det: the winners' LDS list (64 is
// the instance of the entry points that take max_det <= 64, 256 = DISYOLO_MAX_DET the one of disyolo_detect_x).
template <int KMAX>
__device__ __forceinline__ int greedy_nms_block(const int n, const int* list, const float4* boxes, const float* scores,
                                                float* live_glob, const float nms_thr, const int max_det, int* kept_idx,
                                                float* kept_sc) {
  const int tid = threadIdx.x, wv = tid >> 6;
  __shared__ float s_ws[2][NMS_W];
  __shared__ int s_wp[2][NMS_W];
  __shared__ float4 s_wb[2][NMS_W];
  __shared__ int s_kidx[KMAX];
  __shared__ float s_ksc[KMAX];
  int nk = 0;
  if (n <= NMS_K * NMS_T) {
    float sc[NMS_K];
    float4 bx[NMS_K];
    float bs = -1.f;                 // this thread's best survivor: score, list position, box
    int bp = 0x7fffffff;
    float4 bb = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int k = 0; k < NMS_K; ++k) {
      const int q = tid + k * NMS_T;
      sc[k] = -1.f;
      bx[k] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (q < n) {
        const int i = list[q];
        sc[k] = scores[i];
        bx[k] = boxes[i];
      }
      const bool take = sc[k] > bs;  // ascending positions: the lowest wins among equal scores
      bs = take ? sc[k] : bs;
      bp = take ? q : bp;
      bb.x = take ? bx[k].x : bb.x;
      bb.y = take ? bx[k].y : bb.y;
      bb.z = take ? bx[k].z : bb.z;
      bb.w = take ? bx[k].w : bb.w;
    }
    for (int it = 0; it < max_det; ++it) {
      const int par = it & 1;
      float ws = bs;
      int wp = bp;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const float v2 = __shfl_xor(ws, o, 64);
        const int p2 = __shfl_xor(wp, o, 64);
        if (nms_better(v2, p2, ws, wp)) {
          ws = v2;
          wp = p2;
        }
      }
      if (wp == bp) {  // the wave winner's owner (a wave with nothing alive: every lane, the same values)
        s_ws[par][wv] = ws;
        s_wp[par][wv] = wp;
        s_wb[par][wv] = bb;
      }
      __syncthreads();
      float wsc = s_ws[par][0];
      int wq = s_wp[par][0], ww = 0;
#pragma unroll
      for (int w = 1; w < NMS_W; ++w) {
        const float v2 = s_ws[par][w];
        const int p2 = s_wp[par][w];
        if (nms_better(v2, p2, wsc, wq)) {
          wsc = v2;
          wq = p2;
          ww = w;
        }
      }
      if (!(wsc > 0.f)) break;  // nothing alive (live scores are > thr >= 0); uniform exit
      const float4 wb = s_wb[par][ww];
      if (tid == 0) {
        s_kidx[nk] = wq;          // list position; the candidate index is looked up once, after the loop
        s_ksc[nk] = wsc;
      }
      ++nk;
      // suppress against the winner and find this thread's best survivor, one sweep.  Branch-free on purpose: the nested
      // form "if (alive) { if (winner || iou > thr) kill; else if (better) take; }" came out of hipcc 7.2 never killing
      // on the IoU test (caught by the many-candidates known-answer test)
      bs = -1.f;
      bp = 0x7fffffff;
#pragma unroll
      for (int k = 0; k < NMS_K; ++k) {
        const int q = tid + k * NMS_T;
        const float iou = nms_iou(bx[k], wb);
        const bool kill = (q == wq) | (iou > nms_thr);
        sc[k] = kill ? -1.f : sc[k];            // (dead slots stay at -1)
        const bool take = sc[k] > bs;
        bs = take ? sc[k] : bs;
        bp = take ? q : bp;
        bb.x = take ? bx[k].x : bb.x;
        bb.y = take ? bx[k].y : bb.y;
        bb.z = take ? bx[k].z : bb.z;
        bb.w = take ? bx[k].w : bb.w;
      }
    }
    __syncthreads();
    if (tid < nk) {          // (nk <= max_det <= KMAX <= NMS_T)
      kept_idx[tid] = list[s_kidx[tid]];
      kept_sc[tid] = s_ksc[tid];
    }
  } else {
    for (int q = tid; q < n; q += NMS_T) live_glob[q] = scores[list[q]];
    __syncthreads();
    nk = greedy_nms_global(n, list, boxes, live_glob, nms_thr, max_det, kept_idx, kept_sc, s_ws[0], s_wp[0]);
  }
  return nk;
}

template <int KMAX>
__global__ __launch_bounds__(NMS_T) void nms_class_kernel(const float4* boxes, const float* scores, const int* classes,
                                                          int NC, int C, float thr, float nms_thr, int max_det,
                                                          int* list_g, float* live_g, int* kept_idx, float* kept_sc,
                                                          int* kept_n) {
  const int b = blockIdx.x / C, c = blockIdx.x - b * C, tid = threadIdx.x;
  const int lane = tid & 63, wv = tid >> 6;
  boxes += (size_t)b * NC;
  scores += (size_t)b * NC;
  classes += (size_t)b * NC;
  int* list = list_g + (size_t)blockIdx.x * NC;
  float* live_glob = live_g + (size_t)blockIdx.x * NC;
  kept_idx += (size_t)blockIdx.x * max_det;
  kept_sc += (size_t)blockIdx.x * max_det;
  __shared__ int s_wcnt[2][NMS_CB][NMS_W];
  // ---- ordered compaction: wave ballots; eight rounds of 1,024 candidates per barrier, their 16 loads in flight together
  //      (a round per barrier is a load round trip + a store drain each: 60 us for the 20 rounds of a 576^2 image even when
  //      nothing passes the threshold)
  int total = 0;
  for (int base = 0, bt = 0; base < NC; base += NMS_T * NMS_CB, ++bt) {
    bool f[NMS_CB];
    unsigned long long mask[NMS_CB];
#pragma unroll
    for (int j = 0; j < NMS_CB; ++j) {
      const int i = base + j * NMS_T + tid;
      const int ii = i < NC ? i : 0;
      const float sv = scores[ii];
      const int cv = classes[ii];
      f[j] = (i < NC) && (sv > thr) && (cv == c);
    }
#pragma unroll
    for (int j = 0; j < NMS_CB; ++j) {
      mask[j] = __ballot(f[j]);
      if (lane == 0) s_wcnt[bt & 1][j][wv] = __popcll(mask[j]);
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NMS_CB; ++j) {
      int off = total;
#pragma unroll
      for (int w = 0; w < NMS_W; ++w) {
        const int cw = s_wcnt[bt & 1][j][w];
        if (w < wv) off += cw;
        total += cw;
      }
      if (f[j]) list[off + __popcll(mask[j] & ((1ull << lane) - 1ull))] = base + j * NMS_T + tid;
    }
  }
  __syncthreads();  // list[] (global) written by this block, read below by all its threads
  const int nk = greedy_nms_block<KMAX>(total, list, boxes, scores, live_glob, nms_thr, max_det, kept_idx, kept_sc);
  if (tid == 0) kept_n[blockIdx.x] = nk;
}

// ---- image-wide filter: class-agnostic NMS (Method 2 of yolo/yolo3_net_pos.py:594-605) and NMS off (nms=False, :518, 585) ----
// One block per image compacts ALL candidates with score > thr in index order and runs the same greedy loop over that one
// list.  The selection order -- score descending, ties to the lower candidate index -- already is the top_k order of
// :608-612, so the block writes the rows, the zero padding and det_count itself: no merge launch.  "No NMS" is the same
// loop with nms_thr = +inf (no IoU is > +inf): max_det rounds of "take the best, retire it".
// The register form holds NMS_KA slots per thread: 20,480 candidates >= the 20,412 of a 576^2 image.  A slot costs 5
// VGPRs and a 1,024-thread block has 128 per lane, so 20 (100 VGPRs) is about what fits beside the sweep's own registers.
constexpr int NMS_KA = 20;
constexpr int NMS_KA_LD = 4;          // slots whose loads are in flight together while the list is read

// nms_class_kernel's ordered compaction without the class test, as a function: list[0..total) receives, in ascending order,
// the indices of the image's candidates with score > thr; total is returned to every thread.  list[] is global memory: the
// caller puts a barrier before the block reads it.  (That kernel keeps its own inlined copy: its code is left as measured.)
__device__ __forceinline__ int compact_above(const float* scores, const int NC, const float thr, int* list) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  __shared__ int s_wcnt[2][NMS_CB][NMS_W];
  int total = 0;
  for (int base = 0, bt = 0; base < NC; base += NMS_T * NMS_CB, ++bt) {
    bool f[NMS_CB];
    unsigned long long mask[NMS_CB];
#pragma unroll
    for (int j = 0; j < NMS_CB; ++j) {
      const int i = base + j * NMS_T + tid;
      const float sv = scores[i < NC ? i : 0];
      f[j] = (i < NC) && (sv > thr);
    }
#pragma unroll
    for (int j = 0; j < NMS_CB; ++j) {
      mask[j] = __ballot(f[j]);
      if (lane == 0) s_wcnt[bt & 1][j][wv] = __popcll(mask[j]);
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NMS_CB; ++j) {
      int off = total;
#pragma unroll
      for (int w = 0; w < NMS_W; ++w) {
        const int cw = s_wcnt[bt & 1][j][w];
        if (w < wv) off += cw;
        total += cw;
      }
      if (f[j]) list[off + __popcll(mask[j] & ((1ull << lane) - 1ull))] = base + j * NMS_T + tid;
    }
  }
  return total;
}

// min / max of two numbers as compare + select: fminf / fmaxf on a value the compiler has not produced itself (the winner
// out of LDS, a slot after the asm below) cost an extra canonicalising instruction and a register each
__device__ __forceinline__ float nms_lo(float a, float b) { return a < b ? a : b; }
__device__ __forceinline__ float nms_hi(float a, float b) { return a > b ? a : b; }

// greedy_nms_block for the image-wide list: the same rounds and the same one barrier, with the register form trimmed to
// what 20 slots leave room for.  A slot holds its score and its box with the corner order already normalised (nms_iou's
// min / max are idempotent, so the IoU is the same bit for bit); a thread tracks only score and slot of its best survivor,
// and the wave winner's owner picks that slot's box out of its registers with a select chain when it publishes it; the
// round's winner lives in scalar registers.  hipcc 7.2: 128 VGPRs, no spill, no scratch (-Rpass-analysis=kernel-resource-usage);
// each of these choices removed spills, so look at that report after touching the loop.  KMAX as in greedy_nms_block.
template <int KMAX>
__device__ __forceinline__ int greedy_nms_image(const int n, const int* list, const float4* boxes, const float* scores,
                                                float* live_glob, const float nms_thr, const int max_det, int* kept_idx,
                                                float* kept_sc) {
  const int tid = threadIdx.x, wv = __builtin_amdgcn_readfirstlane(tid >> 6);   // (wave-uniform: LDS addresses in scalars)
  __shared__ float s_ws[2][NMS_W];
  __shared__ int s_wp[2][NMS_W];
  __shared__ float4 s_wb[2][NMS_W];
  __shared__ int s_kidx[KMAX];
  __shared__ float s_ksc[KMAX];
  if (n > NMS_KA * NMS_T) {
    for (int q = tid; q < n; q += NMS_T) live_glob[q] = scores[list[q]];
    __syncthreads();
    return greedy_nms_global(n, list, boxes, live_glob, nms_thr, max_det, kept_idx, kept_sc, s_ws[0], s_wp[0]);
  }
  float sc[NMS_KA], y1[NMS_KA], x1[NMS_KA], y2[NMS_KA], x2[NMS_KA];
  float bs = -1.f;                   // this thread's best survivor: score and slot (list position tid + bk * NMS_T)
  int bk = -1;
#pragma unroll
  for (int k = 0; k < NMS_KA; ++k) {
    const int q = tid + k * NMS_T;
    sc[k] = -1.f;
    float4 bx = make_float4(0.f, 0.f, 0.f, 0.f);
    if (q < n) {
      const int i = list[q];
      sc[k] = scores[i];
      bx = boxes[i];
    }
    y1[k] = fminf(bx.x, bx.z);
    x1[k] = fminf(bx.y, bx.w);
    y2[k] = fmaxf(bx.x, bx.z);
    x2[k] = fmaxf(bx.y, bx.w);
    const bool take = sc[k] > bs;    // ascending positions: the lowest wins among equal scores
    bs = take ? sc[k] : bs;
    bk = take ? k : bk;
    if (k % NMS_KA_LD == NMS_KA_LD - 1) asm volatile("" ::: "memory");   // (bounds the loads in flight, and their registers)
  }
  int nk = 0;
  for (int it = 0; it < max_det; ++it) {
    const int par = it & 1;
    const int bp = bk < 0 ? 0x7fffffff : tid + bk * NMS_T;
    float ws = bs;
    int wp = bp;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float v2 = __shfl_xor(ws, o, 64);
      const int p2 = __shfl_xor(wp, o, 64);
      if (nms_better(v2, p2, ws, wp)) {
        ws = v2;
        wp = p2;
      }
    }
    if (wp == bp) {  // the wave winner's owner (a wave with nothing alive: every lane, the same values)
      float4 bb = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int k = 0; k < NMS_KA; ++k) {
        const bool mine = bk == k;
        bb.x = mine ? y1[k] : bb.x;
        bb.y = mine ? x1[k] : bb.y;
        bb.z = mine ? y2[k] : bb.z;
        bb.w = mine ? x2[k] : bb.w;
      }
      s_ws[par][wv] = ws;
      s_wp[par][wv] = wp;
      s_wb[par][wv] = bb;
    }
    __syncthreads();
    float wsc = s_ws[par][0];
    int wq = s_wp[par][0], ww = 0;
#pragma unroll
    for (int w = 1; w < NMS_W; ++w) {
      const float v2 = s_ws[par][w];
      const int p2 = s_wp[par][w];
      if (nms_better(v2, p2, wsc, wq)) {
        wsc = v2;
        wq = p2;
        ww = w;
      }
    }
    if (!(wsc > 0.f)) break;  // nothing alive (live scores are > thr >= 0); uniform exit
    // the block winner is the same in every lane: position and (normalised) box go to scalar registers, the vector ones
    // are all needed for the slots
    wq = __builtin_amdgcn_readfirstlane(wq);
    const float4 wbv = s_wb[par][ww];
    float4 wb;
    wb.x = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, wbv.x)));
    wb.y = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, wbv.y)));
    wb.z = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, wbv.z)));
    wb.w = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, wbv.w)));
    const float ab = (wb.z - wb.x) * (wb.w - wb.y);
    if (tid == 0) {
      s_kidx[nk] = wq;        // list position; the candidate index is looked up once, after the loop
      s_ksc[nk] = wsc;
    }
    ++nk;
    // suppress against the winner and find this thread's best survivor, one sweep, branch-free like greedy_nms_block's:
    // the IoU is nms_iou's, operation by operation, with its early "empty box -> 0" as a select
    const int dq = wq - tid;
    const int kq = (dq & (NMS_T - 1)) ? -1 : dq / NMS_T;   // the winner's slot in the thread that holds it
    bs = -1.f;
    bk = -1;
#pragma unroll
    for (int k = 0; k < NMS_KA; ++k) {
      // (no instruction: the slot's area is the same every round, and hoisted out of the round loop it would cost a
      //  sixth register per slot, which spills)
      asm volatile("" : "+v"(y2[k]), "+v"(x2[k]));
      const float aa = (y2[k] - y1[k]) * (x2[k] - x1[k]);
      const float inter = fmaxf(nms_lo(y2[k], wb.z) - nms_hi(y1[k], wb.x), 0.f) * fmaxf(nms_lo(x2[k], wb.w) - nms_hi(x1[k], wb.y), 0.f);
      const float quot = inter / (aa + ab - inter);
      const float iou = ((aa <= 0.f) | (ab <= 0.f)) ? 0.f : quot;
      const bool kill = (kq == k) | (iou > nms_thr);
      sc[k] = kill ? -1.f : sc[k];            // (dead slots stay at -1)
      const bool take = sc[k] > bs;
      bs = take ? sc[k] : bs;
      bk = take ? k : bk;
    }
  }
  __syncthreads();
  if (tid < nk) {
    kept_idx[tid] = list[s_kidx[tid]];
    kept_sc[tid] = s_ksc[tid];
  }
  return nk;
}

template <int KMAX>
__global__ __launch_bounds__(NMS_T) void nms_image_kernel(const float4* boxes, const float* scores, const int* classes,
                                                          int NC, float thr, float nms_thr, int max_det, int* list_g,
                                                          float* live_g, int* kept_idx, float* kept_sc, float* det,
                                                          int* det_count) {
  const int b = blockIdx.x, tid = threadIdx.x;
  boxes += (size_t)b * NC;
  scores += (size_t)b * NC;
  classes += (size_t)b * NC;
  int* list = list_g + (size_t)b * NC;
  kept_idx += (size_t)b * max_det;
  kept_sc += (size_t)b * max_det;
  det += (size_t)b * max_det * 6;
  const int total = compact_above(scores, NC, thr, list);
  __syncthreads();  // list[] (global) written by this block, read below by all its threads
  const int nk = greedy_nms_image<KMAX>(total, list, boxes, scores, live_g + (size_t)b * NC, nms_thr, max_det, kept_idx, kept_sc);
  __syncthreads();  // kept_idx / kept_sc (global) written by this block
  for (int e = tid; e < max_det * 6; e += NMS_T) {
    const int r = e / 6, f = e - r * 6;
    float v = 0.f;
    if (r < nk) {
      const int i = kept_idx[r];
      const float4 bx = boxes[i];
      v = f == 0 ? bx.x : f == 1 ? bx.y : f == 2 ? bx.z : f == 3 ? bx.w : f == 4 ? (float)classes[i] : kept_sc[r];
    }
    det[e] = v;
  }
  if (tid == 0) det_count[b] = nk;
}

// ---- more than 16 classes: one ordered pass per image buckets the candidates by class, the greedy loop runs per segment ----
// bucket_class_kernel, one block per image: pass 1 counts the candidates with score > thr per class (LDS histogram, integer
// adds), an exclusive scan gives the class offsets, pass 2 walks the candidates again in index order, NMS_T at a time, and
// scatters their indices: inside a wave the lanes of one class rank themselves with a ballot per distinct class, the waves'
// per-class counts go through LDS, so a class's segment stays in candidate-index order (ties are decided by position).
// Work and memory are B NC, whatever the class count.
constexpr int WD_MAXC = 80;

__global__ __launch_bounds__(NMS_T) void bucket_class_kernel(const float* scores, const int* classes, int NC, int C, float thr,
                                                             int* list_g, int* off_g) {
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  scores += (size_t)b * NC;
  classes += (size_t)b * NC;
  int* list = list_g + (size_t)b * NC;
  __shared__ int s_cur[WD_MAXC];            // next free position of each class
  __shared__ int s_wc[NMS_W][WD_MAXC];      // this tile's candidates per (wave, class)
  if (tid < C) s_cur[tid] = 0;
  for (int e = tid; e < NMS_W * WD_MAXC; e += NMS_T) (&s_wc[0][0])[e] = 0;
  __syncthreads();
  for (int i = tid; i < NC; i += NMS_T) {
    const int cv = classes[i];
    if (scores[i] > thr && cv >= 0 && cv < C) atomicAdd(&s_cur[cv], 1);
  }
  __syncthreads();
  if (tid == 0) {
    int o = 0;
    for (int c = 0; c < C; ++c) {
      const int n = s_cur[c];
      s_cur[c] = o;
      off_g[b * (WD_MAXC + 1) + c] = o;
      o += n;
    }
    for (int c = C; c <= WD_MAXC; ++c) off_g[b * (WD_MAXC + 1) + c] = o;
  }
  __syncthreads();
  for (int base = 0; base < NC; base += NMS_T) {
    const int i = base + tid;
    const int ii = i < NC ? i : 0;
    const int cv = classes[ii];
    const bool f = i < NC && scores[ii] > thr && cv >= 0 && cv < C;
    int rank = 0;
    unsigned long long todo = __ballot(f);
    while (todo) {                               // (wave-uniform) one round per distinct class among the wave's candidates
      const int c0 = __shfl(cv, __ffsll((long long)todo) - 1, 64);
      const unsigned long long m = __ballot(f && cv == c0);
      if (f && cv == c0) rank = __popcll(m & ((1ull << lane) - 1ull));
      if (lane == 0) s_wc[wv][c0] = __popcll(m);
      todo &= ~m;
    }
    __syncthreads();
    if (f) {
      int off = s_cur[cv] + rank;
      for (int w = 0; w < wv; ++w) off += s_wc[w][cv];
      list[off] = i;
    }
    __syncthreads();
    if (tid < C) {
      int n = 0;
#pragma unroll
      for (int w = 0; w < NMS_W; ++w) {
        n += s_wc[w][tid];
        s_wc[w][tid] = 0;
      }
      s_cur[tid] += n;
    }
    __syncthreads();
  }
}

template <int KMAX>
__global__ __launch_bounds__(NMS_T) void nms_segment_kernel(const float4* boxes, const float* scores, int NC, int C,
                                                            float nms_thr, int max_det, const int* list_g, const int* off_g,
                                                            float* live_g, int* kept_idx, float* kept_sc, int* kept_n) {
  const int b = blockIdx.x / C, c = blockIdx.x - b * C;
  const int o0 = off_g[b * (WD_MAXC + 1) + c], n = off_g[b * (WD_MAXC + 1) + c + 1] - o0;
  if (n <= 0) {                                  // (block-uniform) an empty class
    if (threadIdx.x == 0) kept_n[blockIdx.x] = 0;
    return;
  }
  const int nk = greedy_nms_block<KMAX>(n, list_g + (size_t)b * NC + o0, boxes + (size_t)b * NC, scores + (size_t)b * NC,
                                  live_g + (size_t)b * NC + o0, nms_thr, max_det, kept_idx + (size_t)blockIdx.x * max_det,
                                  kept_sc + (size_t)blockIdx.x * max_det);
  if (threadIdx.x == 0) kept_n[blockIdx.x] = nk;
}

// k-way merge of the classes' kept lists, each already in selection order (score descending, ties by lower candidate index):
// max_det rounds of "best head among the C lists" with the same tie rule; one wave per image, a lane holds the heads of
// classes lane and lane + 64.  Up to 80 * max_det survivors, none of them in LDS.
__global__ __launch_bounds__(64) void nms_merge_kway_kernel(const float4* boxes, const int* classes, int NC, int C,
                                                            int max_det, const int* kept_idx, const float* kept_sc,
                                                            const int* kept_n, float* det, int* det_count) {
  const int b = blockIdx.x, lane = threadIdx.x;
  boxes += (size_t)b * NC;
  classes += (size_t)b * NC;
  for (int r = lane; r < max_det * 6; r += 64) det[(size_t)b * max_det * 6 + r] = 0.f;
  __syncthreads();
  int hn[2], hp[2], hi[2];
  float hs[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int c = lane + 64 * j;
    hn[j] = c < C ? kept_n[b * C + c] : 0;
    hp[j] = 0;
    hs[j] = -1.f;
    hi[j] = 0x7fffffff;
    if (hn[j] > 0) {
      hs[j] = kept_sc[((size_t)b * C + c) * max_det];
      hi[j] = kept_idx[((size_t)b * C + c) * max_det];
    }
  }
  int nd = 0;
  for (; nd < max_det; ++nd) {
    const int mine = nms_better(hs[1], hi[1], hs[0], hi[0]) ? 1 : 0;
    float ws = mine ? hs[1] : hs[0];
    int wi = mine ? hi[1] : hi[0];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float v2 = __shfl_xor(ws, o, 64);
      const int p2 = __shfl_xor(wi, o, 64);
      if (nms_better(v2, p2, ws, wi)) {
        ws = v2;
        wi = p2;
      }
    }
    if (!(ws > 0.f)) break;                      // every list is used up (kept scores are > thr >= 0); uniform exit
    if (lane == 0) {
      float* o = det + ((size_t)b * max_det + nd) * 6;
      const float4 bx = boxes[wi];
      o[0] = bx.x;
      o[1] = bx.y;
      o[2] = bx.z;
      o[3] = bx.w;
      o[4] = (float)classes[wi];
      o[5] = ws;
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      if (hi[j] == wi && hs[j] > 0.f) {          // candidate indices are unique: exactly one head advances
        const int c = lane + 64 * j;
        ++hp[j];
        hs[j] = -1.f;
        hi[j] = 0x7fffffff;
        if (hp[j] < hn[j]) {
          hs[j] = kept_sc[((size_t)b * C + c) * max_det + hp[j]];
          hi[j] = kept_idx[((size_t)b * C + c) * max_det + hp[j]];
        }
      }
    }
  }
  if (lane == 0) det_count[b] = nd;
}

__global__ __launch_bounds__(64) void nms_merge_kernel(const float4* boxes, const int* classes, int NC, int C,
                                                       int max_det, const int* kept_idx, const float* kept_sc,
                                                       const int* kept_n, float* det, int* det_count) {
  const int b = blockIdx.x, tid = threadIdx.x;
  boxes += (size_t)b * NC;
  classes += (size_t)b * NC;
  __shared__ int s_idx[MAX_KEEP];
  __shared__ float s_sc[MAX_KEEP];
  __shared__ int s_off[17];
  if (tid == 0) {
    int o = 0;
    for (int c = 0; c < C; ++c) {
      s_off[c] = o;
      o += kept_n[b * C + c];
    }
    s_off[C] = o;
  }
  __syncthreads();
  const int nk = s_off[C];
  for (int c = 0; c < C; ++c) {
    const int cn = s_off[c + 1] - s_off[c];
    for (int k = tid; k < cn; k += 64) {
      s_idx[s_off[c] + k] = kept_idx[((size_t)b * C + c) * max_det + k];
      s_sc[s_off[c] + k] = kept_sc[((size_t)b * C + c) * max_det + k];
    }
  }
  for (int r = tid; r < max_det * 6; r += 64) det[(size_t)b * max_det * 6 + r] = 0.f;
  __syncthreads();
  for (int k = tid; k < nk; k += 64) {
    const float sc = s_sc[k];
    const int ix = s_idx[k];
    int rank = 0;
    for (int j = 0; j < nk; ++j) {
      const float sj = s_sc[j];
      if (sj > sc || (sj == sc && s_idx[j] < ix)) ++rank;
    }
    if (rank < max_det) {
      float* o = det + ((size_t)b * max_det + rank) * 6;
      const float4 bx = boxes[ix];
      o[0] = bx.x;
      o[1] = bx.y;
      o[2] = bx.z;
      o[3] = bx.w;
      o[4] = (float)classes[ix];
      o[5] = sc;
    }
  }
  if (tid == 0) det_count[b] = nk < max_det ? nk : max_det;
}

// bin edges of assemble_kmask_from_box (yolo/yolo3_net_pos.py:804-813) for a k x k grid:
// [int(lo), rint(lo + j*sub) for j = 1..k-1, int(hi)], sub = (hi - lo)/k, f32 math,
// rintf = round-half-to-even like tf.round.
template <int K>
__device__ __forceinline__ void bin_edges(float lo, float hi, int e[K + 1]) {
  const float sub = (hi - lo) / (float)K;
  e[0] = (int)lo;
#pragma unroll
  for (int j = 1; j < K; ++j) e[j] = (int)rintf(lo + (float)j * sub);
  e[K] = (int)hi;
}

// masks[b,r,y,x] = sigmoid(score[b,y,x,bin(y,x)]) inside the box, 0.5 outside (:925-928); score rows have k*k channels.
// The map is Hm x Wm: y-coordinates scale by Hm, x-coordinates by Wm (the reference's one `size` at Hm = Wm)
template <int K>
__global__ __launch_bounds__(256) void psroi_assemble_kernel(const float* score, const float* det, int B, int max_det,
                                                             int Hm, int Wm, float* masks, int* keep) {
  const int r = blockIdx.y, b = blockIdx.z;
  const float* d = det + ((size_t)b * max_det + r) * 6;
  const float szy = (float)Hm, szx = (float)Wm;
  const float y1 = rintf(d[0] * szy), x1 = rintf(d[1] * szx), y2 = rintf(d[2] * szy), x2 = rintf(d[3] * szx);
  const bool kp = (y2 - y1) > 0.f && (x2 - x1) > 0.f;
  if (blockIdx.x == 0 && threadIdx.x == 0) keep[b * max_det + r] = kp ? 1 : 0;
  int gy[K + 1], gx[K + 1];
  bin_edges<K>(y1, y2, gy);
  bin_edges<K>(x1, x2, gx);
  const int npx = Hm * Wm;
  float* out = masks + ((size_t)b * max_det + r) * npx;
  const float* sc = score + (size_t)b * npx * (K * K);
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < npx; i += gridDim.x * blockDim.x) {
    float v = 0.f;
    if (kp) {
      const int y = i / Wm, x = i - y * Wm;
      float logit = 0.f;
      if (y >= gy[0] && y < gy[K] && x >= gx[0] && x < gx[K]) {
        int by = 0, bx = 0;
#pragma unroll
        for (int j = 1; j < K; ++j) {
          by += y >= gy[j];
          bx += x >= gx[j];
        }
        logit = sc[(size_t)i * (K * K) + by * K + bx];
      }
      v = 1.f / (1.f + expf(-logit));
    }
    out[i] = v;
  }
}

// ---- evaluate(): mask post-processing (calculate_test_map.py:237-262) ----------------------
// One thread per image pixel walks the image's detections in order: inside a detection's
// destination rectangle it samples the cropped mask bilinearly with cv2.resize(INTER_LINEAR)
// semantics (pixel centres aligned, border taps clamped with weight 0, horizontal then vertical
// pass, every product and sum rounded to f32 separately -- no FMA, so the > 0.5 decision is the
// same as the host restatement's), writes the per-detection bit and keeps the class of the last
// covering detection for the merged class map.
// THE tap arithmetic and the > 0.5 decision of the paste, shared by the per-image and the batched kernel (and by the tiled
// paste of tiles.hip) so they cannot drift: paste_bit(m, size, r, y, x) of paste_bit.h
__global__ __launch_bounds__(256) void mask_paste_kernel(const float* masks, int n, int mh, int mw, const int* rects,
                                                         const int* classids, int H, int W, unsigned char* full,
                                                         unsigned char* merged) {
  const int64_t total = (int64_t)H * W;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int y = (int)(i / W), x = (int)(i - (int64_t)y * W);
    unsigned char mcls = 0;
    for (int k = 0; k < n; ++k) {
      const unsigned char bit = paste_bit(masks + (size_t)k * mh * mw, mw, rects + k * 8, y, x);
      if (full) full[(size_t)k * total + i] = bit;
      if (bit) mcls = (unsigned char)(classids[k] + 1);
    }
    merged[i] = mcls;
  }
}

// The test loop's paste for a whole batch in ONE launch (MAP.collect_batch): per image (job) the merged class map, the pasted
// pixel count of every detection, its intersection with every ground-truth instance of its class and -- with a true class map --
// the 4x4 confusion counts, without ever writing a full-resolution mask.  A block owns PB_CHUNK consecutive pixels of one job
// (found through the jobs' block0 prefix); a thread owns PB_PX of them, walks the job's detections in order with paste_bit and
// keeps the n <= 64 bits of a pixel in one 64-bit register.  Every count is an integer: wave ballot + popcount, one LDS add per
// wave, one global int32 add per block and non-zero counter -- the sums are the same whatever order the adds land in.  The
// ground-truth instances go through the LDS counters PB_GT at a time, so their number is not bounded.
// Bound by memory latency, not by bandwidth or arithmetic: a pixel reads ng ground-truth bytes and a few mask taps and writes one
// byte; the detection walk is a chain of uniform rect loads and a short dependent tap read per covering detection.
constexpr int PB_T = 256;
constexpr int PB_PX = 4;
constexpr int PB_CHUNK = PB_T * PB_PX;
constexpr int PB_GT = 32;
constexpr int PB_MAXN = 64;
constexpr int PB_MAXN_X = DISYOLO_MAX_DET;   // disyolo_mask_paste_iou_batch_x

// MAXN = 64 * NW detections per job: a pixel keeps NW cover words, word w for detections 64 w .. 64 w + 63.  The walk over
// the detections runs word after word, each word in ascending k, so it visits them in order across a word boundary: the
// last covering detection owns the pixel of the merged map whatever word it sits in.
template <int MAXN>
__global__ __launch_bounds__(PB_T) void mask_paste_iou_batch_kernel(const disyolo_paste_job* jobs, int njobs, int mh, int mw,
                                                                    unsigned long long* conf) {
  constexpr int NW = MAXN / 64;
  static_assert(MAXN % 64 == 0 && MAXN <= PB_T, "one thread per detection sets up and flushes the LDS counters");
  __shared__ unsigned int s_area[MAXN];
  __shared__ unsigned int s_inter[MAXN * PB_GT];
  __shared__ unsigned int s_conf[16];
  __shared__ int s_cls[MAXN];
  int lo = 0, hi = njobs - 1;      // the last job whose first block is <= this block
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (jobs[mid].block0 <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
  }
  const disyolo_paste_job j = jobs[lo];
  const int tid = threadIdx.x, lane = tid & 63;
  const int W = j.image_w, total = j.image_h * j.image_w, n = j.n, ng = j.ng;
  const int chunk0 = ((int)blockIdx.x - j.block0) * PB_CHUNK;
  if (tid < MAXN) {
    s_area[tid] = 0;
    s_cls[tid] = tid < n ? j.classids[tid] : -1;
  }
  if (tid < 16) s_conf[tid] = 0;
  __syncthreads();
  unsigned long long bits[PB_PX][NW];
#pragma unroll
  for (int p = 0; p < PB_PX; ++p) {
    const int i = chunk0 + p * PB_T + tid;
    const bool valid = i < total;
    const int y = valid ? i / W : 0, x = valid ? i - y * W : 0;
    unsigned char mcls = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      unsigned long long b = 0;
      const int kend = NW == 1 ? n : min(n, 64 * (w + 1));     // (one word: the plan holds n <= 64)
      for (int k = 64 * w; k < kend; ++k) {
        const int* r = j.rects + k * 8;
        unsigned char bit = 0;
        // (a crop that leaves the mh x mw mask would read outside `masks`: such a row pastes nothing)
        if (valid && r[0] >= 0 && r[1] >= 0 && r[2] <= mh && r[3] <= mw)
          bit = paste_bit(j.masks + (size_t)k * mh * mw, mw, r, y, x);
        if (bit) {
          b |= 1ull << (k - 64 * w);
          mcls = (unsigned char)(s_cls[k] + 1);
        }
        const int c = __popcll(__ballot(bit));
        if (lane == 0 && c) atomicAdd(&s_area[k], (unsigned)c);
      }
      bits[p][w] = b;
    }
    if (valid) {
      j.merged[i] = mcls;
      if (j.true_map) {
        const unsigned a = j.true_map[i];
        if (a < 4 && mcls < 4) atomicAdd(&s_conf[a * 4 + mcls], 1u);
      }
    }
  }
  __syncthreads();
  if (tid < n && s_area[tid]) atomicAdd(&j.counts[(size_t)tid * (1 + ng)], (int)s_area[tid]);
  if (j.true_map && tid < 16 && s_conf[tid]) atomicAdd(&conf[tid], (unsigned long long)s_conf[tid]);
  for (int g0 = 0; g0 < ng; g0 += PB_GT) {
    const int gn = min(PB_GT, ng - g0);
    for (int e = tid; e < n * PB_GT; e += PB_T) s_inter[e] = 0;
    __syncthreads();
    for (int gg = 0; gg < gn; ++gg) {
      const int gc = j.gt_class[g0 + gg];
      const unsigned char* gp = j.gt + (size_t)(g0 + gg) * total;
#pragma unroll
      for (int p = 0; p < PB_PX; ++p) {
        const int i = chunk0 + p * PB_T + tid;
        unsigned long long any = 0;
#pragma unroll
        for (int w = 0; w < NW; ++w) any |= bits[p][w];
        const bool on = any && i < total && gp[i];
#pragma unroll
        for (int w = 0; w < NW; ++w) {
          const unsigned long long m = on ? bits[p][w] : 0ull;
          if (__ballot(m != 0) == 0) continue;      // (wave-uniform)
          const int kend = NW == 1 ? n : min(n, 64 * (w + 1));     // (one word: the plan holds n <= 64)
          for (int k = 64 * w; k < kend; ++k) {
            if (s_cls[k] != gc) continue;           // (block-uniform)
            const int c = __popcll(__ballot((m >> (k - 64 * w)) & 1));
            if (lane == 0 && c) atomicAdd(&s_inter[k * PB_GT + gg], (unsigned)c);
          }
        }
      }
    }
    __syncthreads();
    for (int e = tid; e < n * PB_GT; e += PB_T) {
      const unsigned v = s_inter[e];
      if (v) atomicAdd(&j.counts[(size_t)(e / PB_GT) * (1 + ng) + 1 + g0 + (e % PB_GT)], (int)v);
    }
    __syncthreads();
  }
}


// image_read (calculate_test_map.py:149-176, utils/val_data.py:36-63): aspect-preserving bilinear
// resize of an RGB uint8 image (as float32, like cv2.resize(image.astype(float32), INTER_LINEAR))
// centred in an oh x ow letter box padded with 127, then / 255.  Same tap arithmetic as the mask
// paste above (aligned pixel centres, clamped border taps with weight 0, horizontal then vertical
// pass, float32 without FMA).  One thread per output pixel; the three channels together.
__global__ __launch_bounds__(256) void letterbox_kernel(const unsigned char* rgb, int H, int W, float* out, int oh, int ow,
                                                        int new_h, int new_w, int top, int left) {
  const int64_t total = (int64_t)oh * ow;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int y = (int)(i / ow), x = (int)(i - (int64_t)y * ow);
    float v[3] = {127.f, 127.f, 127.f};
    if (y >= top && y < top + new_h && x >= left && x < left + new_w) {
      float fx = (float)(((double)(x - left) + 0.5) * ((double)W / (double)new_w) - 0.5);
      float fy = (float)(((double)(y - top) + 0.5) * ((double)H / (double)new_h) - 0.5);
      int sx = (int)floorf(fx), sy = (int)floorf(fy);
      float ax = __fsub_rn(fx, (float)sx), ay = __fsub_rn(fy, (float)sy);
      if (sx < 0) { ax = 0.f; sx = 0; }
      if (sx >= W - 1) { ax = 0.f; sx = W - 1; }
      if (sy < 0) { ay = 0.f; sy = 0; }
      if (sy >= H - 1) { ay = 0.f; sy = H - 1; }
      const int sx1 = min(sx + 1, W - 1), sy1 = min(sy + 1, H - 1);
      const unsigned char* r0 = rgb + ((size_t)sy * W) * 3;
      const unsigned char* r1 = rgb + ((size_t)sy1 * W) * 3;
      const float bx = __fsub_rn(1.f, ax), by = __fsub_rn(1.f, ay);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float h0 = __fadd_rn(__fmul_rn((float)r0[sx * 3 + c], bx), __fmul_rn((float)r0[sx1 * 3 + c], ax));
        const float h1 = __fadd_rn(__fmul_rn((float)r1[sx * 3 + c], bx), __fmul_rn((float)r1[sx1 * 3 + c], ax));
        v[c] = __fadd_rn(__fmul_rn(h0, by), __fmul_rn(h1, ay));
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) out[i * 3 + c] = (float)__ddiv_rn((double)v[c], 255.0);   // new_image / 255.0 in float64 (a plain "/" is narrowed to an approximate f32 division)
  }
}

// 4x4 pixel confusion counts of two uint8 class maps (calculate_test_map.py:303-331): per-block LDS
// histogram, integer atomics into the caller's int64[16] accumulator (exact, order-independent)
__global__ __launch_bounds__(256) void confusion16_kernel(const unsigned char* t, const unsigned char* p, int64_t n,
                                                          unsigned long long* conf) {
  __shared__ unsigned int h[16];
  if (threadIdx.x < 16) h[threadIdx.x] = 0;
  __syncthreads();
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const unsigned a = t[i], b = p[i];
    if (a < 4 && b < 4) atomicAdd(&h[a * 4 + b], 1u);
  }
  __syncthreads();
  if (threadIdx.x < 16 && h[threadIdx.x]) atomicAdd(&conf[threadIdx.x], (unsigned long long)h[threadIdx.x]);
}

// the same counts for any number of labels (background + up to 80 classes): nlabel^2 LDS counters (26 KB at 81 labels)
constexpr int CONF_MAXL = 81;
__global__ __launch_bounds__(256) void confusion_n_kernel(const unsigned char* t, const unsigned char* p, int64_t n, int nl,
                                                          unsigned long long* conf) {
  __shared__ unsigned int h[CONF_MAXL * CONF_MAXL];
  for (int e = threadIdx.x; e < nl * nl; e += 256) h[e] = 0;
  __syncthreads();
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int a = t[i], b = p[i];
    if (a < nl && b < nl) atomicAdd(&h[a * nl + b], 1u);
  }
  __syncthreads();
  for (int e = threadIdx.x; e < nl * nl; e += 256)
    if (h[e]) atomicAdd(&conf[e], (unsigned long long)h[e]);
}

}  // namespace

// the workspace with room for `keep` (>= max_det) kept rows per (image, class)
static size_t detect_workspace_keep(int B, int H, int W, int num_class, int keep) {
  if (B <= 0 || H <= 0 || W <= 0 || H % 32 || W % 32) return 0;
  const size_t c1 = (size_t)(H / 32) * (W / 32);
  const size_t NC = 3 * (16 * c1 + 4 * c1 + c1);
  // boxes (16 B) + scores + classes, per-class list + live, per-class kept (idx, score, n)
  if (num_class <= 16)
    return (size_t)B * NC * (16 + 4 + 4) + (size_t)B * num_class * NC * 8 + (size_t)B * num_class * ((size_t)keep * 8 + 4) + 256;
  // the same prefix, ONE bucketed list + live per image, the class offsets, per-class kept (idx, score, n)
  return (size_t)B * NC * (16 + 4 + 4) + (size_t)B * NC * 8 + (size_t)B * (WD_MAXC + 1) * 4 +
         (size_t)B * num_class * ((size_t)keep * 8 + 4) + 256;
}

extern "C" size_t disyolo_detect_workspace_hw(int B, int H, int W, int num_class) {
  return detect_workspace_keep(B, H, W, num_class, 64);
}

// ... of disyolo_detect_x: the kept lists hold max_det rows, never fewer than the 64 of the other entry points
extern "C" size_t disyolo_detect_workspace_x(int B, int H, int W, int num_class, int max_det) {
  if (max_det <= 0 || max_det > DISYOLO_MAX_DET || num_class <= 0 || num_class > WD_MAXC) return 0;
  return detect_workspace_keep(B, H, W, num_class, max_det > 64 ? max_det : 64);
}

extern "C" size_t disyolo_detect_workspace(int B, int S, int num_class) {
  return disyolo_detect_workspace_hw(B, S, S, num_class);
}

extern "C" int disyolo_detect(const float* logits3, const float* logits2, const float* logits1, int B, int S,
                              int num_class, const float* anchors_host, const float* clip_window, float obj_thresh,
                              float nms_thresh, int max_det, float* detections, int32_t* det_count, void* workspace,
                              size_t workspace_bytes, void* stream) {
  return disyolo_detect_hw(logits3, logits2, logits1, B, S, S, num_class, anchors_host, clip_window, obj_thresh, nms_thresh,
                           max_det, detections, det_count, workspace, workspace_bytes, stream);
}

// the filter on a net of H x W pixels: head grids (H/8, W/8), (H/16, W/16), (H/32, W/32)
extern "C" int disyolo_detect_hw(const float* logits3, const float* logits2, const float* logits1, int B, int H, int W,
                                 int num_class, const float* anchors_host, const float* clip_window, float obj_thresh,
                                 float nms_thresh, int max_det, float* detections, int32_t* det_count, void* workspace,
                                 size_t workspace_bytes, void* stream) {
  return disyolo_detect_nms_hw(logits3, logits2, logits1, B, H, W, num_class, anchors_host, clip_window, obj_thresh,
                               nms_thresh, max_det, DISYOLO_NMS_PER_CLASS, detections, det_count, workspace, workspace_bytes,
                               stream);
}

extern "C" int disyolo_detect_list_capacity(void) { return NMS_KA * NMS_T; }

static int detect_run(const float* logits3, const float* logits2, const float* logits1, int B, int H, int W, int num_class,
                      const float* anchors_host, const float* clip_window, float obj_thresh, float nms_thresh, int max_det,
                      int nms_mode, float* detections, int32_t* det_count, void* workspace, size_t workspace_bytes,
                      void* stream, bool wide);

// ... with the choice of which candidates above the threshold survive (DISYOLO_NMS_*)
extern "C" int disyolo_detect_nms_hw(const float* logits3, const float* logits2, const float* logits1, int B, int H, int W,
                                     int num_class, const float* anchors_host, const float* clip_window, float obj_thresh,
                                     float nms_thresh, int max_det, int nms_mode, float* detections, int32_t* det_count,
                                     void* workspace, size_t workspace_bytes, void* stream) {
  return detect_run(logits3, logits2, logits1, B, H, W, num_class, anchors_host, clip_window, obj_thresh, nms_thresh, max_det,
                    nms_mode, detections, det_count, workspace, workspace_bytes, stream, false);
}

// ... with up to DISYOLO_MAX_DET rows per image: the winners' lists of the greedy loops hold 256, and up to 16 classes
// whose C * max_det kept rows pass the LDS rank merge's 512 go through the k-way merge of the longer class lists (its
// layout is nms_class_kernel's kept lists).  The workspace is disyolo_detect_workspace_x's.  max_det <= 64 launches the
// same kernel instances as disyolo_detect_nms_hw.
extern "C" int disyolo_detect_x(const float* logits3, const float* logits2, const float* logits1, int B, int H, int W,
                                int num_class, const float* anchors_host, const float* clip_window, float obj_thresh,
                                float nms_thresh, int max_det, int nms_mode, float* detections, int32_t* det_count,
                                void* workspace, size_t workspace_bytes, void* stream) {
  return detect_run(logits3, logits2, logits1, B, H, W, num_class, anchors_host, clip_window, obj_thresh, nms_thresh, max_det,
                    nms_mode, detections, det_count, workspace, workspace_bytes, stream, true);
}

static int detect_run(const float* logits3, const float* logits2, const float* logits1, int B, int H, int W, int num_class,
                      const float* anchors_host, const float* clip_window, float obj_thresh, float nms_thresh, int max_det,
                      int nms_mode, float* detections, int32_t* det_count, void* workspace, size_t workspace_bytes,
                      void* stream, bool wide) {
  DY_REQUIRE(nms_mode == DISYOLO_NMS_PER_CLASS || nms_mode == DISYOLO_NMS_AGNOSTIC || nms_mode == DISYOLO_NMS_NONE,
             "detect: nms_mode must be 0 (per class), 1 (class-agnostic) or 2 (none) (got %d)", nms_mode);
  DY_REQUIRE(logits3 && logits2 && logits1 && anchors_host && clip_window && detections && det_count,
             "detect: null pointer");
  DY_REQUIRE(B > 0 && H > 0 && W > 0 && H % 32 == 0 && W % 32 == 0 && num_class > 0 && num_class <= WD_MAXC,
             "detect: bad sizes");
  if (wide)
    DY_REQUIRE(max_det > 0 && max_det <= DISYOLO_MAX_DET, "detect_x: max_det must be in 1..%d (got %d)", DISYOLO_MAX_DET,
               max_det);
  else
    DY_REQUIRE(max_det > 0 && max_det <= 64 && (num_class > 16 || num_class * max_det <= MAX_KEEP),
               "detect: max_det must be <= 64");
  DY_REQUIRE(obj_thresh >= 0.f, "detect: obj_thresh must be >= 0");
  const int keep = wide && max_det > 64 ? max_det : 64;     // rows of a kept list in the workspace
  const size_t ws_need = detect_workspace_keep(B, H, W, num_class, keep);
  if (!workspace || workspace_bytes < ws_need) {
    disyolo_set_error("detect: workspace too small");
    return DISYOLO_E_WORKSPACE;
  }
  if (nms_mode != DISYOLO_NMS_PER_CLASS) {
    // decode results, ONE list + live per image, max_det kept (idx, score): inside what any class count's workspace holds
    const size_t NC = (size_t)3 * 21 * (H / 32) * (W / 32);
    DY_REQUIRE((size_t)B * NC * (16 + 4 + 4) + (size_t)B * NC * 8 + (size_t)B * max_det * 8 <= ws_need,
               "detect: the workspace does not hold an image-wide list");
  }
  {
    std::array<float, 18> anc;
    for (int i = 0; i < 18; ++i) anc[i] = anchors_host[i];
    DY_RECORD_OR_RUN([=](void* s) {
      return detect_run(logits3, logits2, logits1, B, H, W, num_class, anc.data(), clip_window, obj_thresh, nms_thresh,
                        max_det, nms_mode, detections, det_count, workspace, workspace_bytes, s, wide);
    });
  }
  DecodeParams p;
  const float* lg[3] = {logits3, logits2, logits1};
  const int div[3] = {8, 16, 32};
  int c0 = 0;
  for (int s = 0; s < 3; ++s) {
    p.sc[s].logits = lg[s];
    p.sc[s].gh = H / div[s];
    p.sc[s].gw = W / div[s];
    p.sc[s].cand0 = c0;
    c0 += p.sc[s].gh * p.sc[s].gw * 3;
    for (int a = 0; a < 3; ++a) {
      p.sc[s].aw[a] = anchors_host[(3 * s + a) * 2 + 0];
      p.sc[s].ah[a] = anchors_host[(3 * s + a) * 2 + 1];
    }
  }
  p.B = B; p.H = H; p.W = W; p.C = num_class; p.NC = c0;
  p.window = clip_window;
  char* ws = (char*)workspace;
  p.boxes = (float4*)ws;                  ws += (size_t)B * c0 * 16;
  p.scores = (float*)ws;                  ws += (size_t)B * c0 * 4;
  p.classes = (int*)ws;                   ws += (size_t)B * c0 * 4;
  hipStream_t st = (hipStream_t)stream;
  const bool k256 = max_det > 64;         // the instances with 256 winners per list
  if (nms_mode != DISYOLO_NMS_PER_CLASS) {
    int* list = (int*)ws;                 ws += (size_t)B * c0 * 4;
    float* live = (float*)ws;             ws += (size_t)B * c0 * 4;
    int* kept_idx = (int*)ws;             ws += (size_t)B * max_det * 4;
    float* kept_sc = (float*)ws;
    hipLaunchKernelGGL(decode_score_kernel, dim3(ceil_div(c0, 256), B), dim3(256), 0, st, p);
    DY_CHECK_LAUNCH();
    hipLaunchKernelGGL(k256 ? nms_image_kernel<256> : nms_image_kernel<64>, dim3(B), dim3(NMS_T), 0, st, p.boxes, p.scores, p.classes, c0, obj_thresh,
                       nms_mode == DISYOLO_NMS_NONE ? INFINITY : nms_thresh, max_det, list, live, kept_idx, kept_sc,
                       detections, det_count);
    DY_CHECK_LAUNCH();
    return DISYOLO_OK;
  }
  if (num_class > 16) {
    int* list = (int*)ws;                 ws += (size_t)B * c0 * 4;
    float* live = (float*)ws;             ws += (size_t)B * c0 * 4;
    int* off = (int*)ws;                  ws += (size_t)B * (WD_MAXC + 1) * 4;
    int* kept_idx = (int*)ws;             ws += (size_t)B * num_class * keep * 4;
    float* kept_sc = (float*)ws;          ws += (size_t)B * num_class * keep * 4;
    int* kept_n = (int*)ws;
    hipLaunchKernelGGL(decode_score_kernel, dim3(ceil_div(c0, 256), B), dim3(256), 0, st, p);
    DY_CHECK_LAUNCH();
    hipLaunchKernelGGL(bucket_class_kernel, dim3(B), dim3(NMS_T), 0, st, p.scores, p.classes, c0, num_class, obj_thresh,
                       list, off);
    DY_CHECK_LAUNCH();
    hipLaunchKernelGGL(k256 ? nms_segment_kernel<256> : nms_segment_kernel<64>, dim3(B * num_class), dim3(NMS_T), 0, st, p.boxes, p.scores, c0, num_class,
                       nms_thresh, max_det, list, off, live, kept_idx, kept_sc, kept_n);
    DY_CHECK_LAUNCH();
    hipLaunchKernelGGL(nms_merge_kway_kernel, dim3(B), dim3(64), 0, st, p.boxes, p.classes, c0, num_class, max_det,
                       kept_idx, kept_sc, kept_n, detections, det_count);
    DY_CHECK_LAUNCH();
    return DISYOLO_OK;
  }
  int* list = (int*)ws;                   ws += (size_t)B * num_class * c0 * 4;
  float* live = (float*)ws;               ws += (size_t)B * num_class * c0 * 4;
  int* kept_idx = (int*)ws;               ws += (size_t)B * num_class * keep * 4;
  float* kept_sc = (float*)ws;            ws += (size_t)B * num_class * keep * 4;
  int* kept_n = (int*)ws;
  hipLaunchKernelGGL(decode_score_kernel, dim3(ceil_div(c0, 256), B), dim3(256), 0, st, p);
  DY_CHECK_LAUNCH();
  hipLaunchKernelGGL(k256 ? nms_class_kernel<256> : nms_class_kernel<64>, dim3(B * num_class), dim3(NMS_T), 0, st, p.boxes, p.scores, p.classes, c0,
                     num_class, obj_thresh, nms_thresh, max_det, list, live, kept_idx, kept_sc, kept_n);
  DY_CHECK_LAUNCH();
  if (num_class * max_det <= MAX_KEEP)
    hipLaunchKernelGGL(nms_merge_kernel, dim3(B), dim3(64), 0, st, p.boxes, p.classes, c0, num_class, max_det, kept_idx,
                       kept_sc, kept_n, detections, det_count);
  else      // (disyolo_detect_x alone) more survivors than the rank merge's LDS holds
    hipLaunchKernelGGL(nms_merge_kway_kernel, dim3(B), dim3(64), 0, st, p.boxes, p.classes, c0, num_class, max_det,
                       kept_idx, kept_sc, kept_n, detections, det_count);
  DY_CHECK_LAUNCH();
  return DISYOLO_OK;
}

extern "C" int disyolo_psroi_assemble(const float* score, const float* detections, int B, int max_det, int map_size,
                                      int k, float* masks, int32_t* keep, void* stream) {
  return disyolo_psroi_assemble_hw(score, detections, B, max_det, map_size, map_size, k, masks, keep, stream);
}

extern "C" int disyolo_psroi_assemble_hw(const float* score, const float* detections, int B, int max_det, int map_h,
                                         int map_w, int k, float* masks, int32_t* keep, void* stream) {
  DY_REQUIRE(score && detections && masks && keep && B > 0 && max_det > 0 && map_h > 0 && map_w > 0 &&
                 (int64_t)map_h * map_w <= (1ll << 30),
             "psroi_assemble: bad args");
  DY_REQUIRE(k == 3 || k == 5 || k == 7, "psroi_assemble: k must be one of k = 3, 5, 7 (got %d)", k);
  DY_RECORD_OR_RUN([=](void* s) {
    return disyolo_psroi_assemble_hw(score, detections, B, max_det, map_h, map_w, k, masks, keep, s);
  });
  const int npx = map_h * map_w;
  int gx = ceil_div(npx, 256 * 4);
  if (gx < 1) gx = 1;
  auto kern = k == 3 ? psroi_assemble_kernel<3> : k == 5 ? psroi_assemble_kernel<5> : psroi_assemble_kernel<7>;
  hipLaunchKernelGGL(kern, dim3(gx, max_det, B), dim3(256), 0, (hipStream_t)stream, score, detections, B, max_det, map_h,
                     map_w, masks, keep);
  DY_CHECK_LAUNCH();
  return DISYOLO_OK;
}

extern "C" int disyolo_mask_paste(const float* masks, int n, int size, const int32_t* rects, const int32_t* classids,
                                  int image_h, int image_w, uint8_t* full_masks, uint8_t* merged, void* stream) {
  return disyolo_mask_paste_hw(masks, n, size, size, rects, classids, image_h, image_w, full_masks, merged, stream);
}

extern "C" int disyolo_mask_paste_hw(const float* masks, int n, int map_h, int map_w, const int32_t* rects,
                                     const int32_t* classids, int image_h, int image_w, uint8_t* full_masks, uint8_t* merged,
                                     void* stream) {
  DY_REQUIRE(merged && image_h > 0 && image_w > 0 && n >= 0 && map_h > 0 && map_w > 0, "mask_paste: bad args");
  DY_REQUIRE(n == 0 || (masks && rects && classids), "mask_paste: null pointer");
  DY_RECORD_OR_RUN([=](void* s) {
    return disyolo_mask_paste_hw(masks, n, map_h, map_w, rects, classids, image_h, image_w, full_masks, merged, s);
  });
  const int64_t total = (int64_t)image_h * image_w;
  int grid = (int)((total + 255) / 256);
  if (grid > 256 * 16) grid = 256 * 16;
  hipLaunchKernelGGL(mask_paste_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, masks, n, map_h, map_w, (const int*)rects,
                     (const int*)classids, image_h, image_w, (unsigned char*)full_masks, (unsigned char*)merged);
  DY_CHECK_LAUNCH();
  return DISYOLO_OK;
}

extern "C" size_t disyolo_paste_job_size(void) { return sizeof(disyolo_paste_job); }

// validates a HOST table of jobs and lays the jobs' blocks out: block0 = the first block of each job; returns the number of
// blocks of the launch, or a negative code
static int paste_job_plan_cap(disyolo_paste_job* jobs, int njobs, int cap) {
  DY_REQUIRE(jobs && njobs > 0, "paste_job_plan: null table or njobs <= 0");
  int64_t blocks = 0;
  for (int i = 0; i < njobs; ++i) {
    const disyolo_paste_job& j = jobs[i];
    DY_REQUIRE(j.n >= 0 && j.n <= cap, "paste job %d: n must be in 0..%d (got %d)", i, cap, j.n);
    DY_REQUIRE(j.ng >= 0, "paste job %d: ng < 0", i);
    DY_REQUIRE(j.image_h > 0 && j.image_w > 0 && (int64_t)j.image_h * j.image_w <= (1ll << 30), "paste job %d: bad image size", i);
    DY_REQUIRE(j.merged, "paste job %d: merged is NULL", i);
    DY_REQUIRE(j.n == 0 || (j.masks && j.rects && j.classids && j.counts), "paste job %d: null pointer with n > 0", i);
    DY_REQUIRE(j.ng == 0 || (j.gt && j.gt_class), "paste job %d: null pointer with ng > 0", i);
    jobs[i].block0 = (int32_t)blocks;
    blocks += ((int64_t)j.image_h * j.image_w + PB_CHUNK - 1) / PB_CHUNK;
    DY_REQUIRE(blocks < (1ll << 31), "paste jobs: too many pixels for one launch");
  }
  return (int)blocks;
}

extern "C" int disyolo_paste_job_plan(disyolo_paste_job* jobs, int njobs) { return paste_job_plan_cap(jobs, njobs, PB_MAXN); }

// ... for jobs of up to DISYOLO_MAX_DET detections (disyolo_mask_paste_iou_batch_x)
extern "C" int disyolo_paste_job_plan_x(disyolo_paste_job* jobs, int njobs) {
  return paste_job_plan_cap(jobs, njobs, PB_MAXN_X);
}

static int mask_paste_iou_batch_run(const disyolo_paste_job* jobs_host, const disyolo_paste_job* jobs, int njobs, int map_h,
                                    int map_w, int64_t* conf, void* stream, int cap);

extern "C" int disyolo_mask_paste_iou_batch(const disyolo_paste_job* jobs_host, const disyolo_paste_job* jobs, int njobs, int size,
                                            int64_t* conf, void* stream) {
  DY_REQUIRE(size > 0 || !(jobs_host && jobs && njobs > 0), "mask_paste_iou_batch: size must be > 0");
  return disyolo_mask_paste_iou_batch_hw(jobs_host, jobs, njobs, size, size, conf, stream);
}

extern "C" int disyolo_mask_paste_iou_batch_hw(const disyolo_paste_job* jobs_host, const disyolo_paste_job* jobs, int njobs,
                                               int map_h, int map_w, int64_t* conf, void* stream) {
  return mask_paste_iou_batch_run(jobs_host, jobs, njobs, map_h, map_w, conf, stream, PB_MAXN);
}

// ... with up to DISYOLO_MAX_DET detections per job (a table planned by disyolo_paste_job_plan_x): the same counts layout;
// a table whose jobs all hold <= 64 detections launches the one-word kernel of disyolo_mask_paste_iou_batch_hw
extern "C" int disyolo_mask_paste_iou_batch_x(const disyolo_paste_job* jobs_host, const disyolo_paste_job* jobs, int njobs,
                                              int map_h, int map_w, int64_t* conf, void* stream) {
  return mask_paste_iou_batch_run(jobs_host, jobs, njobs, map_h, map_w, conf, stream, PB_MAXN_X);
}

static int mask_paste_iou_batch_run(const disyolo_paste_job* jobs_host, const disyolo_paste_job* jobs, int njobs, int map_h,
                                    int map_w, int64_t* conf, void* stream, int cap) {
  DY_REQUIRE(jobs_host && jobs && njobs > 0, "mask_paste_iou_batch: null table or njobs <= 0");
  DY_REQUIRE(map_h > 0 && map_w > 0, "mask_paste_iou_batch: size must be > 0");
  // the host copy is what this call can check and size the grid from; it must be a planned table (disyolo_paste_job_plan)
  std::vector<disyolo_paste_job> plan(jobs_host, jobs_host + njobs);
  const int blocks = paste_job_plan_cap(plan.data(), njobs, cap);
  if (blocks < 0) return blocks;
  int nmax = 0;
  for (int i = 0; i < njobs; ++i) {
    nmax = plan[i].n > nmax ? plan[i].n : nmax;
    DY_REQUIRE(plan[i].block0 == jobs_host[i].block0, "mask_paste_iou_batch: job %d is not planned (disyolo_paste_job_plan)", i);
    DY_REQUIRE(!jobs_host[i].true_map || conf, "mask_paste_iou_batch: job %d has a true_map but conf is NULL", i);
  }
  DY_RECORD_OR_RUN([=](void* s) { return mask_paste_iou_batch_run(plan.data(), jobs, njobs, map_h, map_w, conf, s, cap); });
  hipLaunchKernelGGL(nmax > PB_MAXN ? mask_paste_iou_batch_kernel<PB_MAXN_X> : mask_paste_iou_batch_kernel<PB_MAXN>, dim3(blocks), dim3(PB_T), 0, (hipStream_t)stream, jobs, njobs, map_h, map_w,
                     (unsigned long long*)conf);
  DY_CHECK_LAUNCH();
  return DISYOLO_OK;
}

extern "C" int disyolo_letterbox(const uint8_t* rgb, int image_h, int image_w, float* out, int size, float* window_host,
                                 void* stream) {
  return disyolo_letterbox_hw(rgb, image_h, image_w, out, size, size, window_host, stream);
}

// the letter box of a net of net_h x net_w pixels: the width binds when net_w / image_w < net_h / image_h
extern "C" int disyolo_letterbox_hw(const uint8_t* rgb, int image_h, int image_w, float* out, int net_h, int net_w,
                                    float* window_host, void* stream) {
  DY_REQUIRE(rgb && out && image_h > 0 && image_w > 0 && net_h > 0 && net_w > 0, "letterbox: bad args");
  int new_h, new_w;
  if (((double)net_w / image_w) < ((double)net_h / image_h)) {   // Python float division
    new_h = (int)(((int64_t)image_h * net_w) / image_w);
    new_w = net_w;
  } else {
    new_w = (int)(((int64_t)image_w * net_h) / image_h);
    new_h = net_h;
  }
  DY_REQUIRE(new_h > 0 && new_w > 0 && new_h <= net_h && new_w <= net_w, "letterbox: degenerate image");
  const int top = (net_h - new_h) / 2, left = (net_w - new_w) / 2;
  if (window_host) {   // [top, left, bottom, right] normalised by (net_h, net_w), float32 of the float64 quotient like numpy
    window_host[0] = (float)((double)top / net_h);
    window_host[1] = (float)((double)left / net_w);
    window_host[2] = (float)((double)(new_h + top) / net_h);
    window_host[3] = (float)((double)(new_w + left) / net_w);
  }
  DY_RECORD_OR_RUN([=](void* s) { return disyolo_letterbox_hw(rgb, image_h, image_w, out, net_h, net_w, nullptr, s); });
  const int64_t total = (int64_t)net_h * net_w;
  int grid = (int)((total + 255) / 256);
  if (grid > 256 * 16) grid = 256 * 16;
  hipLaunchKernelGGL(letterbox_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, rgb, image_h, image_w, out, net_h,
                     net_w, new_h, new_w, top, left);
  DY_CHECK_LAUNCH();
  return DISYOLO_OK;
}

extern "C" int disyolo_confusion16(const uint8_t* true_map, const uint8_t* pred_map, int64_t n, int64_t* conf,
                                   void* stream) {
  DY_REQUIRE(true_map && pred_map && conf && n > 0, "confusion16: bad args");
  DY_RECORD_OR_RUN([=](void* s) { return disyolo_confusion16(true_map, pred_map, n, conf, s); });
  int grid = (int)((n + 255) / 256);
  if (grid > 1024) grid = 1024;
  hipLaunchKernelGGL(confusion16_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, true_map, pred_map, n,
                     (unsigned long long*)conf);
  DY_CHECK_LAUNCH();
  return DISYOLO_OK;
}

extern "C" int disyolo_confusion_n(const uint8_t* true_map, const uint8_t* pred_map, int64_t n, int nlabel, int64_t* conf,
                                   void* stream) {
  DY_REQUIRE(true_map && pred_map && conf && n > 0, "confusion_n: bad args");
  DY_REQUIRE(nlabel >= 2 && nlabel <= CONF_MAXL, "confusion_n: nlabel must be in 2..81 (got %d)", nlabel);
  DY_RECORD_OR_RUN([=](void* s) { return disyolo_confusion_n(true_map, pred_map, n, nlabel, conf, s); });
  int grid = (int)((n + 255) / 256);
  if (grid > 1024) grid = 1024;
  hipLaunchKernelGGL(confusion_n_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, true_map, pred_map, n, nlabel,
                     (unsigned long long*)conf);
  DY_CHECK_LAUNCH();
  return DISYOLO_OK;
}

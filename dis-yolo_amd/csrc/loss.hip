// Fused loss + gradient kernels: YOLO detection loss and the position-sensitive mask loss.
//
// Replace loss_yolo (yolo/yolo3_net_pos.py:631-747) and loss_mask / overlaps_graph /
// assemble_kmask_from_box (:750-860, 954-975) together with TF's autodiff of them.  The
// reference materialises [R,288,288,9] one-hot masks and a tiled copy of the score maps
// per image; here one thread owns one score-map pixel and walks the (<=10) RoIs.
//
// Gradients wrt head logits / score maps are written as bf16 rows padded to 32 channels
// (64 for the 49 score maps of a 7 x 7 grid; zeros beyond the real channels) so they feed
// the MFMA data/weight-gradient convs directly.  Scalar losses use per-block partials + a fixed-order final sum.
#include <array>
#include "common.h"
#include "runtime.h"

namespace {

__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }
// tf.nn.sigmoid_cross_entropy_with_logits: max(x,0) - x*z + log1p(exp(-|x|))
__device__ __forceinline__ float sigmoid_ce(float z, float x) {
  return fmaxf(x, 0.f) - x * z + log1pf(expf(-fabsf(x)));
}

constexpr int DL_LD = 32;  // padded channel count of the dlogits / dscore rows

struct YoloLossParams {
  const float* logits;  // [B,gh,gw,3,D]
  const float* labels;  // [B,gh,gw,3,D]
  const float* true_boxes;  // [B,G,5] xc,yc,w,h,cls (normalised)
  bf16* dlogits;        // [B,gh,gw,DL_LD]
  float* partial;       // [gridDim.y*gridDim.x][5]
  int B, gh, gw, C, G, H, W;   // grid gh x gw of a net of H x W pixels
  float aw[3], ah[3];
  float ignore_thresh, obj_scale, noobj_scale, class_scale, coord_scale;
  float inv_B;
};

// one thread = one (cell, anchor); blockIdx.y = image.  The three scales run as ONE launch (round 5: three dependent launches
// at the forward / backward boundary of the main lane were 44 us where the longest scale takes 24): block bx of scale s,
// whose grid is gx blocks wide -- the partial rows keep the layout of the three separate launches, so the sums are the same
// bit for bit.
struct YoloLoss3 {
  YoloLossParams p[3];
  int gx[3];
};
// TB >= G: the true boxes staged in LDS (64 up to max_boxes = 64, DISYOLO_MAX_BOXES = 256 beyond)
template <int TB>
__device__ __forceinline__ void yolo_loss_body(const YoloLossParams& p, const int bx, const int gx) {
  __shared__ float s_tb[TB * 4];
  __shared__ float s_red[4][5];
  const int b = blockIdx.y;
  for (int i = threadIdx.x; i < p.G * 4; i += 256) {
    const int gidx = i >> 2, k = i & 3;
    s_tb[i] = p.true_boxes[((size_t)b * p.G + gidx) * 5 + k];
  }
  __syncthreads();
  const int D = 5 + p.C;
  const int ncell = p.gh * p.gw;
  const int idx = bx * 256 + threadIdx.x;
  float l_obj = 0.f, l_noobj = 0.f, l_cls = 0.f, l_xy = 0.f, l_wh = 0.f;
  if (idx < ncell * 3) {
    const int a = idx % 3, cell = idx / 3;
    const int x = cell % p.gw, y = cell / p.gw;
    const size_t base = (((size_t)b * ncell + cell) * 3 + a) * D;
    const float* t = p.logits + base;
    const float* lab = p.labels + base;
    // grid_factor = [gw, gh], net_factor = [net_w, net_h] (:646, :709-718)
    const float gfx = (float)p.gw, gfy = (float)p.gh, netw = (float)p.W, neth = (float)p.H;
    const float sx = sigmoidf_(t[0]), sy = sigmoidf_(t[1]);
    // decoded normalised box (interpret_output, :493-506)
    const float bxc = ((float)x + sx) / gfx, byc = ((float)y + sy) / gfy;
    const float bw = expf(t[2]) * p.aw[a] / netw, bh = expf(t[3]) * p.ah[a] / neth;
    const float pminx = bxc - bw / 2.f, pmaxx = bxc + bw / 2.f, pminy = byc - bh / 2.f, pmaxy = byc + bh / 2.f;
    const float parea = bw * bh;
    float best = 0.f;  // iou is clipped to [0,1], so the max over >=1 boxes is >= 0
    for (int k = 0; k < p.G; ++k) {
      const float txc = s_tb[k * 4 + 0], tyc = s_tb[k * 4 + 1], tw = s_tb[k * 4 + 2], th = s_tb[k * 4 + 3];
      const float iw = fmaxf(fminf(pmaxx, txc + tw / 2.f) - fmaxf(pminx, txc - tw / 2.f), 0.f);
      const float ih = fmaxf(fminf(pmaxy, tyc + th / 2.f) - fmaxf(pminy, tyc - th / 2.f), 0.f);
      const float inter = iw * ih;
      const float uni = fmaxf(parea + tw * th - inter, 1e-10f);
      const float iou = fminf(fmaxf(inter / uni, 0.f), 1.f);
      best = fmaxf(best, iou);
    }
    const float ignore = best < p.ignore_thresh ? 1.f : 0.f;
    const float obj = lab[4];
    const float conf = t[4];
    const float ce = sigmoid_ce(obj, conf);
    l_obj = obj * ce * p.obj_scale;
    l_noobj = ignore * (1.f - obj) * ce * p.noobj_scale;
    const float sconf = sigmoidf_(conf);
    float d[8 + 8];  // up to 16 logits per anchor (C <= 11)
    const float dce = sconf - obj;
    d[4] = (obj * p.obj_scale + ignore * (1.f - obj) * p.noobj_scale) * dce * p.inv_B;
    // class: sparse softmax CE against argmax(label[5:]) (first max)
    int tc = 0;
    float lm = lab[5];
    for (int c = 1; c < p.C; ++c)
      if (lab[5 + c] > lm) {
        lm = lab[5 + c];
        tc = c;
      }
    float mx = t[5];
    for (int c = 1; c < p.C; ++c) mx = fmaxf(mx, t[5 + c]);
    float den = 0.f;
    for (int c = 0; c < p.C; ++c) den += expf(t[5 + c] - mx);
    const float lse = mx + logf(den);
    l_cls = obj * (lse - t[5 + tc]) * p.class_scale;
    for (int c = 0; c < p.C; ++c) {
      const float pr = expf(t[5 + c] - lse);
      d[5 + c] = obj * p.class_scale * (pr - (c == tc ? 1.f : 0.f)) * p.inv_B;
    }
    // coordinates (:706-726)
    const float tcx = lab[0] * gfx - (float)x, tcy = lab[1] * gfy - (float)y;
    const float ttw = fminf(fmaxf(logf(lab[2] * netw / p.aw[a]), -100.f), 100.f);
    const float tth = fminf(fmaxf(logf(lab[3] * neth / p.ah[a]), -100.f), 100.f);
    const float whs = 2.f - lab[2] * lab[3];
    const float whs2 = whs * whs * p.coord_scale;
    const float dx_ = obj * (sx - tcx), dy_ = obj * (sy - tcy);
    const float dw_ = obj * (t[2] - ttw), dh_ = obj * (t[3] - tth);
    l_xy = (dx_ * dx_ + dy_ * dy_) * whs2;
    l_wh = (dw_ * dw_ + dh_ * dh_) * whs2;
    d[0] = 2.f * obj * dx_ * whs2 * sx * (1.f - sx) * p.inv_B;
    d[1] = 2.f * obj * dy_ * whs2 * sy * (1.f - sy) * p.inv_B;
    d[2] = 2.f * obj * dw_ * whs2 * p.inv_B;
    d[3] = 2.f * obj * dh_ * whs2 * p.inv_B;
    bf16* o = p.dlogits + ((size_t)b * ncell + cell) * DL_LD + a * D;
    for (int k = 0; k < D; ++k) o[k] = (bf16)d[k];
    if (a == 2)
      for (int k = 3 * D; k < DL_LD; ++k) p.dlogits[((size_t)b * ncell + cell) * DL_LD + k] = (bf16)0.f;
  }
  l_obj = wave_sum(l_obj);
  l_noobj = wave_sum(l_noobj);
  l_cls = wave_sum(l_cls);
  l_xy = wave_sum(l_xy);
  l_wh = wave_sum(l_wh);
  if ((threadIdx.x & 63) == 0) {
    float* r = s_red[threadIdx.x >> 6];
    r[0] = l_obj; r[1] = l_noobj; r[2] = l_cls; r[3] = l_xy; r[4] = l_wh;
  }
  __syncthreads();
  if (threadIdx.x < 5) {
    const float v = s_red[0][threadIdx.x] + s_red[1][threadIdx.x] + s_red[2][threadIdx.x] + s_red[3][threadIdx.x];
    p.partial[((size_t)blockIdx.y * gx + bx) * 5 + threadIdx.x] = v;
  }
}
template <int TB>
__global__ __launch_bounds__(256) void yolo_loss_kernel(YoloLoss3 P) {
  int bx = blockIdx.x, s = 0;
  if (bx >= P.gx[0]) {
    bx -= P.gx[0];
    s = 1;
    if (bx >= P.gx[1]) {
      bx -= P.gx[1];
      s = 2;
    }
  }
  yolo_loss_body<TB>(P.p[s], bx, P.gx[s]);
}

// ---- class lists past the 32-channel rows: 3 (5 + C) <= ld <= 256, 1 <= C <= 80 ----
// The arithmetic of yolo_loss_body, organised for rows of up to 85 floats.  A block still owns 256 consecutive (cell, anchor)
// rows of one image and writes one partial row, so the partial layout and the final sum are the old ones.  Its rows are one
// contiguous span of 256 D floats in logits and in labels: the block walks it in four chunks of WL_ROWS rows, each copied
// into LDS by all threads with consecutive lanes on consecutive floats (a thread-per-row walk would put 4 D bytes between
// lanes).  Four adjacent lanes then share a row: each takes the classes c = q (mod 4) and the true boxes k = q (mod 4), and
// the four combine the maxima and sums through lane shuffles in a fixed order -- never the row in a per-thread array.  The
// gradients replace the logits in LDS and leave as bf16 rows of `ld` channels, a wave per row, lanes along the channels.
constexpr int WL_ROWS = 64;
constexpr int WL_MAXD = 85;

__device__ __forceinline__ float quad_max(float v) {
  v = fmaxf(v, __shfl_xor(v, 1, 64));
  return fmaxf(v, __shfl_xor(v, 2, 64));
}
__device__ __forceinline__ float quad_sum(float v) {   // (v0 + v1) + (v2 + v3) in every lane of the quad
  v += __shfl_xor(v, 1, 64);
  return v + __shfl_xor(v, 2, 64);
}

template <int TB>
__device__ __forceinline__ void yolo_loss_wide_body(const YoloLossParams& p, const int ld, const int bx, const int gx) {
  __shared__ float s_tb[TB * 4];
  __shared__ float s_red[4][5];
  __shared__ float s_t[WL_ROWS * WL_MAXD];   // logits of the chunk, then their gradients
  __shared__ float s_l[WL_ROWS * WL_MAXD];   // labels of the chunk
  const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  for (int i = tid; i < p.G * 4; i += 256) {
    const int gidx = i >> 2, k = i & 3;
    s_tb[i] = p.true_boxes[((size_t)b * p.G + gidx) * 5 + k];
  }
  const int D = 5 + p.C;
  const int ncell = p.gh * p.gw, nrow = ncell * 3;
  const float gfx = (float)p.gw, gfy = (float)p.gh, netw = (float)p.W, neth = (float)p.H;
  const int r = tid >> 2, q = tid & 3;
  float l_obj = 0.f, l_noobj = 0.f, l_cls = 0.f, l_xy = 0.f, l_wh = 0.f;
  for (int ch = 0; ch < 256 / WL_ROWS; ++ch) {
    const int row0 = bx * 256 + ch * WL_ROWS;          // (block-uniform)
    if (row0 >= nrow) break;
    const int nr = min(WL_ROWS, nrow - row0);
    const size_t base = ((size_t)b * nrow + row0) * D;
    __syncthreads();                                   // the previous chunk's rows are written out; s_tb is complete
    for (int e = tid; e < nr * D; e += 256) {
      s_t[e] = p.logits[base + e];
      s_l[e] = p.labels[base + e];
    }
    __syncthreads();
    if (r < nr) {                                      // (the four lanes of a quad agree)
      const int idx = row0 + r;
      const int a = idx % 3, cell = idx / 3;
      const int x = cell % p.gw, y = cell / p.gw;
      float* t = s_t + r * D;
      const float* lab = s_l + r * D;
      const float t0 = t[0], t1 = t[1], t2 = t[2], t3 = t[3], conf = t[4];
      const float sx = sigmoidf_(t0), sy = sigmoidf_(t1);
      const float bxc = ((float)x + sx) / gfx, byc = ((float)y + sy) / gfy;
      const float bw = expf(t2) * p.aw[a] / netw, bh = expf(t3) * p.ah[a] / neth;
      const float pminx = bxc - bw / 2.f, pmaxx = bxc + bw / 2.f, pminy = byc - bh / 2.f, pmaxy = byc + bh / 2.f;
      const float parea = bw * bh;
      float best = 0.f;
      for (int k = q; k < p.G; k += 4) {
        const float txc = s_tb[k * 4 + 0], tyc = s_tb[k * 4 + 1], tw = s_tb[k * 4 + 2], th = s_tb[k * 4 + 3];
        const float iw = fmaxf(fminf(pmaxx, txc + tw / 2.f) - fmaxf(pminx, txc - tw / 2.f), 0.f);
        const float ih = fmaxf(fminf(pmaxy, tyc + th / 2.f) - fmaxf(pminy, tyc - th / 2.f), 0.f);
        const float inter = iw * ih;
        const float uni = fmaxf(parea + tw * th - inter, 1e-10f);
        const float iou = fminf(fmaxf(inter / uni, 0.f), 1.f);
        best = fmaxf(best, iou);
      }
      best = quad_max(best);
      const float ignore = best < p.ignore_thresh ? 1.f : 0.f;
      const float obj = lab[4];
      const float ce = sigmoid_ce(obj, conf);
      const float sconf = sigmoidf_(conf);
      // class: sparse softmax CE against argmax(label[5:]) (first max): this lane's classes, then the quad's
      int tc = 0x7fffffff;
      float lm = -INFINITY, mx = -INFINITY;
      for (int c = q; c < p.C; c += 4) {
        const float lv = lab[5 + c];
        if (lv > lm || tc == 0x7fffffff) {
          lm = lv;
          tc = c;
        }
        mx = fmaxf(mx, t[5 + c]);
      }
#pragma unroll
      for (int o = 1; o <= 2; o <<= 1) {
        const float lm2 = __shfl_xor(lm, o, 64);
        const int tc2 = __shfl_xor(tc, o, 64);
        if (tc2 != 0x7fffffff && (tc == 0x7fffffff || lm2 > lm || (lm2 == lm && tc2 < tc))) {
          lm = lm2;
          tc = tc2;
        }
      }
      mx = quad_max(mx);
      float den = 0.f;
      for (int c = q; c < p.C; c += 4) den += expf(t[5 + c] - mx);
      den = quad_sum(den);
      const float lse = mx + logf(den);
      const float ttc = t[5 + tc];                     // read before any lane of the quad overwrites it
      const float tcx = lab[0] * gfx - (float)x, tcy = lab[1] * gfy - (float)y;
      const float ttw = fminf(fmaxf(logf(lab[2] * netw / p.aw[a]), -100.f), 100.f);
      const float tth = fminf(fmaxf(logf(lab[3] * neth / p.ah[a]), -100.f), 100.f);
      const float whs = 2.f - lab[2] * lab[3];
      const float whs2 = whs * whs * p.coord_scale;
      const float dx_ = obj * (sx - tcx), dy_ = obj * (sy - tcy);
      const float dw_ = obj * (t2 - ttw), dh_ = obj * (t3 - tth);
      for (int c = q; c < p.C; c += 4) {
        const float pr = expf(t[5 + c] - lse);
        t[5 + c] = obj * p.class_scale * (pr - (c == tc ? 1.f : 0.f)) * p.inv_B;
      }
      if (q == 0) {
        l_obj += obj * ce * p.obj_scale;
        l_noobj += ignore * (1.f - obj) * ce * p.noobj_scale;
        l_cls += obj * (lse - ttc) * p.class_scale;
        l_xy += (dx_ * dx_ + dy_ * dy_) * whs2;
        l_wh += (dw_ * dw_ + dh_ * dh_) * whs2;
        t[0] = 2.f * obj * dx_ * whs2 * sx * (1.f - sx) * p.inv_B;
        t[1] = 2.f * obj * dy_ * whs2 * sy * (1.f - sy) * p.inv_B;
        t[2] = 2.f * obj * dw_ * whs2 * p.inv_B;
        t[3] = 2.f * obj * dh_ * whs2 * p.inv_B;
        t[4] = (obj * p.obj_scale + ignore * (1.f - obj) * p.noobj_scale) * (sconf - obj) * p.inv_B;
      }
    }
    __syncthreads();
    for (int rr = wv; rr < nr; rr += 4) {
      const int idx = row0 + rr;
      const int a = idx % 3, cell = idx / 3;
      bf16* o = p.dlogits + ((size_t)b * ncell + cell) * ld;
      for (int k = lane; k < D; k += 64) o[a * D + k] = (bf16)s_t[rr * D + k];
      if (a == 2)
        for (int k = 3 * D + lane; k < ld; k += 64) o[k] = (bf16)0.f;
    }
  }
  l_obj = wave_sum(l_obj);
  l_noobj = wave_sum(l_noobj);
  l_cls = wave_sum(l_cls);
  l_xy = wave_sum(l_xy);
  l_wh = wave_sum(l_wh);
  if (lane == 0) {
    float* rd = s_red[wv];
    rd[0] = l_obj; rd[1] = l_noobj; rd[2] = l_cls; rd[3] = l_xy; rd[4] = l_wh;
  }
  __syncthreads();
  if (tid < 5) p.partial[((size_t)blockIdx.y * gx + bx) * 5 + tid] = s_red[0][tid] + s_red[1][tid] + s_red[2][tid] + s_red[3][tid];
}
template <int TB>
__global__ __launch_bounds__(256) void yolo_loss_wide_kernel(YoloLoss3 P, int ld) {
  int bx = blockIdx.x, s = 0;
  if (bx >= P.gx[0]) {
    bx -= P.gx[0];
    s = 1;
    if (bx >= P.gx[1]) {
      bx -= P.gx[1];
      s = 2;
    }
  }
  yolo_loss_wide_body<TB>(P.p[s], ld, bx, P.gx[s]);
}

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// losses[0..4] = obj, noobj, class, xy, wh summed over the three scales and averaged over
// the batch; [5] = conf, [6] = coord, [7] = conf + class + coord.  5 waves, one per term.
__global__ __launch_bounds__(320) void yolo_loss_final_kernel(const float* partial, int n, float inv_B, float* losses) {
  const int q = threadIdx.x >> 6, lane = threadIdx.x & 63;
  __shared__ double s[5];
  double acc = 0.0;
  for (int i = lane; i < n; i += 64) acc += (double)partial[(size_t)i * 5 + q];
  acc = wave_sum_d(acc);
  if (lane == 0) {
    s[q] = acc * inv_B;
    losses[q] = (float)s[q];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    losses[5] = (float)(s[0] + s[1]);
    losses[6] = (float)(s[3] + s[4]);
    losses[7] = (float)(s[0] + s[1] + s[2] + s[3] + s[4]);
  }
}

// ---- tf.random_shuffle of the proposal / GT-box order (yolo/yolo3_net_pos.py:781-782) ----
// A uniformly random permutation of 0..n-1 per image: each thread draws one counter-based
// 32-bit key (hash of seed, step, image, index), the rank of the key is its position.  The step
// count is read from device memory, so a recorded step reshuffles on every replay.
__device__ __forceinline__ unsigned hash32(unsigned x) {
  x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
  return x;
}
// T threads rank up to T keys: 64 for n <= 64, 256 beyond.  Key and rank of an index do not depend on T.
template <int T>
__global__ __launch_bounds__(T) void shuffle_perm_kernel(int* perm_a, int na, int* perm_b, int nb, unsigned seed,
                                                         const int64_t* step) {
  __shared__ unsigned keys[T];
  const int b = blockIdx.x, t = threadIdx.x;
  const unsigned st = step ? (unsigned)*step : 0u;
  for (int which = 0; which < 2; ++which) {
    const int n = which ? nb : na;
    int* out = (which ? perm_b : perm_a) + (size_t)b * n;
    if (t < n) keys[t] = hash32(hash32(seed + 0x9e3779b9u * st) ^ hash32((unsigned)(b * 2 + which) * 0x85ebca6bu + t));
    __syncthreads();
    if (t < n) {
      int rank = 0;
      for (int j = 0; j < n; ++j) rank += (keys[j] < keys[t]) || (keys[j] == keys[t] && j < t);
      out[rank] = t;
    }
    __syncthreads();
  }
}

// ---- mask-loss RoI selection (yolo/yolo3_net_pos.py:757-796, 842) ------------------
// An RoI row of a k x k grid holds roi_w(k) = 2 (k + 1) + 4 int32 words: gy0..gyk, gx0..gxk, gt_row, area, valid, 0
// (12 words at k = 3).  The grids of the reference's list k = 3, 5, 7 are separate template instances.
constexpr int ROI_MAX = 16;
constexpr int roi_w(int k) { return 2 * (k + 1) + 4; }
constexpr int dscore_ld(int k) { return (k * k + 31) / 32 * 32; }   // channel pitch of dscore: conv82's cout_pad
// bin edges of assemble_kmask_from_box (:804-813): [int(lo), rint(lo + j*sub) for j = 1..k-1, int(hi)], sub = (hi - lo)/k,
// f32 math (this file is compiled without contraction), rintf = round-half-to-even like tf.round
template <int K>
__device__ __forceinline__ void bin_edges(float lo, float hi, int e[K + 1]) {
  const float sub = (hi - lo) / (float)K;
  e[0] = (int)lo;
#pragma unroll
  for (int j = 1; j < K; ++j) e[j] = (int)rintf(lo + (float)j * sub);
  e[K] = (int)hi;
}
// One 64-thread block per image: the image's detections, ground-truth boxes and permutations are staged in
// LDS by all lanes, then lane 0 runs the (inherently sequential, order-defining) selection on them -- the
// single-thread version spent 40 us in dependent global loads.
template <int K>
__global__ __launch_bounds__(64) void mask_rois_kernel(const float* det_g, int max_det, const float* true_boxes_g, int G,
                                                       const int* perm_det_g, const int* perm_gt_g, int B, int Hm, int Wm,
                                                       int n_det, int n_gt, float iou_thr, int* rois, int* roi_count) {
  constexpr int RW = roi_w(K);
  __shared__ float s_det[64 * 6];
  __shared__ float s_tb[64 * 5];
  __shared__ int s_pd[64], s_pg[64];
  const int b = blockIdx.x;
  if (b >= B) return;
  for (int i = threadIdx.x; i < max_det * 6 && i < 64 * 6; i += 64) s_det[i] = det_g[(size_t)b * max_det * 6 + i];
  for (int i = threadIdx.x; i < G * 5 && i < 64 * 5; i += 64) s_tb[i] = true_boxes_g[(size_t)b * G * 5 + i];
  for (int i = threadIdx.x; i < max_det && i < 64; i += 64) s_pd[i] = perm_det_g ? perm_det_g[b * max_det + i] : i;
  for (int i = threadIdx.x; i < G && i < 64; i += 64) s_pg[i] = perm_gt_g ? perm_gt_g[b * G + i] : i;
  __syncthreads();
  if (threadIdx.x != 0) return;
  const float* det = s_det;            // image b's rows, staged
  const float* true_boxes = s_tb;
  const int* perm_det = s_pd;
  const int* perm_gt = s_pg;
  // trimmed lists (rows whose |coords| sum is non-zero), in row order
  int prow[64], grow[64];
  int np = 0, ng = 0;
  for (int r = 0; r < max_det && r < 64; ++r) {
    const float* d = det + ((size_t)r) * 6;
    if (fabsf(d[0]) + fabsf(d[1]) + fabsf(d[2]) + fabsf(d[3]) != 0.f) prow[np++] = r;
  }
  for (int r = 0; r < G && r < 64; ++r) {
    const float* t = true_boxes + ((size_t)r) * 5;
    if (fabsf(t[0]) + fabsf(t[1]) + fabsf(t[2]) + fabsf(t[3]) != 0.f) grow[ng++] = r;
  }
  // shuffled selection: first n_det proposals and first n_gt GT boxes in permuted order
  float rb[ROI_MAX][4];
  int nr = 0;
  for (int q = 0, taken = 0; q < max_det && taken < n_det; ++q) {
    const int j = perm_det[q];
    if (j < 0 || j >= np) continue;
    const float* d = det + ((size_t)prow[j]) * 6;
    rb[nr][0] = d[0]; rb[nr][1] = d[1]; rb[nr][2] = d[2]; rb[nr][3] = d[3];
    ++nr; ++taken;
  }
  for (int q = 0, taken = 0; q < G && taken < n_gt; ++q) {
    const int j = perm_gt[q];
    if (j < 0 || j >= ng) continue;
    const float* t = true_boxes + ((size_t)grow[j]) * 5;
    rb[nr][0] = t[1] - t[3] / 2.f; rb[nr][1] = t[0] - t[2] / 2.f;
    rb[nr][2] = t[1] + t[3] / 2.f; rb[nr][3] = t[0] + t[2] / 2.f;
    ++nr; ++taken;
  }
  int cnt = 0;
  int* out = rois + (size_t)b * ROI_MAX * RW;
  for (int r = 0; r < nr; ++r) {
    float best = -INFINITY;
    int arg = 0;
    for (int j = 0; j < ng; ++j) {
      const float* t = true_boxes + ((size_t)grow[j]) * 5;
      const float gy1 = t[1] - t[3] / 2.f, gx1 = t[0] - t[2] / 2.f, gy2 = t[1] + t[3] / 2.f, gx2 = t[0] + t[2] / 2.f;
      const float y1 = fmaxf(rb[r][0], gy1), x1 = fmaxf(rb[r][1], gx1);
      const float y2 = fminf(rb[r][2], gy2), x2 = fminf(rb[r][3], gx2);
      const float inter = fmaxf(x2 - x1, 0.f) * fmaxf(y2 - y1, 0.f);
      const float a1 = (rb[r][2] - rb[r][0]) * (rb[r][3] - rb[r][1]);
      const float a2 = (gy2 - gy1) * (gx2 - gx1);
      const float iou = inter / (a1 + a2 - inter);
      if (iou > best) {  // first maximum wins (tf.argmax); NaN never wins
        best = iou;
        arg = j;
      }
    }
    if (ng > 0 && best >= iou_thr) {
      // y-coordinates scale by the map's height, x-coordinates by its width (the reference's one `size` at Hm = Wm, :842)
      const float szy = (float)Hm, szx = (float)Wm;
      const float y1 = rintf(rb[r][0] * szy), x1 = rintf(rb[r][1] * szx);
      const float y2 = rintf(rb[r][2] * szy), x2 = rintf(rb[r][3] * szx);
      int gy[K + 1], gx[K + 1];
      bin_edges<K>(y1, y2, gy);
      bin_edges<K>(x1, x2, gx);
      int* o = out + cnt * RW;
      for (int k = 0; k <= K; ++k) {
        o[k] = gy[k];
        o[K + 1 + k] = gx[k];
      }
      o[2 * K + 2] = grow[arg];
      // mask_object pixel count (:848): sum over the k*k bins, clipped to the map
      int area = 0;
      for (int by = 0; by < K; ++by)
        for (int bx = 0; bx < K; ++bx) {
          const int hh = min(gy[by + 1], Hm) - max(gy[by], 0), ww = min(gx[bx + 1], Wm) - max(gx[bx], 0);
          if (hh > 0 && ww > 0) area += hh * ww;
        }
      o[2 * K + 3] = area;
      o[2 * K + 4] = 1;
      o[2 * K + 5] = 0;
      ++cnt;
    }
  }
  for (int r = cnt; r < ROI_MAX; ++r)
    for (int k = 0; k < RW; ++k) out[r * RW + k] = 0;
  roi_count[b] = cnt;
}

// The selection for up to MR_MAX = 256 detections and ground-truth boxes: the same rows as mask_rois_kernel, with the two
// parts that grow with the row count spread over the wave.  The trimmed row lists are built by ordered ballots, 64 rows a
// round, into LDS; lane 0 then runs the order-defining pick (first n_det / n_gt in permuted order, <= ROI_MAX rows) and
// leaves the RoI boxes in LDS; each RoI's IoU arg-max over the trimmed ground-truth rows is taken across the lanes -- lane l
// walks rows l, l + 64, ... in ascending order with the serial form's strict "iou > best" (NaN never wins), and the lanes
// combine by (greater IoU, then lower row), which is "the first maximum wins".  The IoU is the serial form's, operation by
// operation.  (Serial, G = 256 costs ~10 RoIs x 256 dependent IoUs on one lane of the chain that holds up the mask subnet's
// backward pass.)
constexpr int MR_MAX = 256;
template <int K>
__global__ __launch_bounds__(64) void mask_rois_wave_kernel(const float* det_g, int max_det, const float* true_boxes_g, int G,
                                                            const int* perm_det_g, const int* perm_gt_g, int B, int Hm, int Wm,
                                                            int n_det, int n_gt, float iou_thr, int* rois, int* roi_count) {
  constexpr int RW = roi_w(K);
  __shared__ float s_det[MR_MAX * 6];
  __shared__ float s_tb[MR_MAX * 5];
  __shared__ int s_pd[MR_MAX], s_pg[MR_MAX];
  __shared__ int s_prow[MR_MAX], s_grow[MR_MAX];
  __shared__ float s_rb[ROI_MAX][4];
  __shared__ int s_nr;
  const int b = blockIdx.x, lane = threadIdx.x;
  if (b >= B) return;
  if (max_det > MR_MAX) max_det = MR_MAX;      // (the entry point refuses more)
  if (G > MR_MAX) G = MR_MAX;
  for (int i = lane; i < max_det * 6; i += 64) s_det[i] = det_g[(size_t)b * max_det * 6 + i];
  for (int i = lane; i < G * 5; i += 64) s_tb[i] = true_boxes_g[(size_t)b * G * 5 + i];
  for (int i = lane; i < max_det; i += 64) s_pd[i] = perm_det_g ? perm_det_g[b * max_det + i] : i;
  for (int i = lane; i < G; i += 64) s_pg[i] = perm_gt_g ? perm_gt_g[b * G + i] : i;
  __syncthreads();
  // trimmed lists (rows whose |coords| sum is non-zero), in row order
  const unsigned long long below = (1ull << lane) - 1ull;
  int np = 0, ng = 0;
  for (int base = 0; base < max_det; base += 64) {
    const int r = base + lane;
    bool f = false;
    if (r < max_det) {
      const float* d = s_det + r * 6;
      f = fabsf(d[0]) + fabsf(d[1]) + fabsf(d[2]) + fabsf(d[3]) != 0.f;
    }
    const unsigned long long m = __ballot(f);
    if (f) s_prow[np + __popcll(m & below)] = r;
    np += __popcll(m);
  }
  for (int base = 0; base < G; base += 64) {
    const int r = base + lane;
    bool f = false;
    if (r < G) {
      const float* t = s_tb + r * 5;
      f = fabsf(t[0]) + fabsf(t[1]) + fabsf(t[2]) + fabsf(t[3]) != 0.f;
    }
    const unsigned long long m = __ballot(f);
    if (f) s_grow[ng + __popcll(m & below)] = r;
    ng += __popcll(m);
  }
  __syncthreads();
  // shuffled selection: first n_det proposals and first n_gt GT boxes in permuted order (sequential: it defines the order)
  if (lane == 0) {
    int nr = 0;
    for (int q = 0, taken = 0; q < max_det && taken < n_det && nr < ROI_MAX; ++q) {
      const int j = s_pd[q];
      if (j < 0 || j >= np) continue;
      const float* d = s_det + s_prow[j] * 6;
      s_rb[nr][0] = d[0]; s_rb[nr][1] = d[1]; s_rb[nr][2] = d[2]; s_rb[nr][3] = d[3];
      ++nr; ++taken;
    }
    for (int q = 0, taken = 0; q < G && taken < n_gt && nr < ROI_MAX; ++q) {
      const int j = s_pg[q];
      if (j < 0 || j >= ng) continue;
      const float* t = s_tb + s_grow[j] * 5;
      s_rb[nr][0] = t[1] - t[3] / 2.f; s_rb[nr][1] = t[0] - t[2] / 2.f;
      s_rb[nr][2] = t[1] + t[3] / 2.f; s_rb[nr][3] = t[0] + t[2] / 2.f;
      ++nr; ++taken;
    }
    s_nr = nr;
  }
  __syncthreads();
  const int nr = s_nr;
  int cnt = 0;
  int* out = rois + (size_t)b * ROI_MAX * RW;
  for (int r = 0; r < nr; ++r) {
    const float r0 = s_rb[r][0], r1 = s_rb[r][1], r2 = s_rb[r][2], r3 = s_rb[r][3];
    float best = -INFINITY;
    int arg = 0x7fffffff;
    for (int j = lane; j < ng; j += 64) {
      const float* t = s_tb + s_grow[j] * 5;
      const float gy1 = t[1] - t[3] / 2.f, gx1 = t[0] - t[2] / 2.f, gy2 = t[1] + t[3] / 2.f, gx2 = t[0] + t[2] / 2.f;
      const float y1 = fmaxf(r0, gy1), x1 = fmaxf(r1, gx1);
      const float y2 = fminf(r2, gy2), x2 = fminf(r3, gx2);
      const float inter = fmaxf(x2 - x1, 0.f) * fmaxf(y2 - y1, 0.f);
      const float a1 = (r2 - r0) * (r3 - r1);
      const float a2 = (gy2 - gy1) * (gx2 - gx1);
      const float iou = inter / (a1 + a2 - inter);
      if (iou > best) {  // this lane's first maximum; NaN never wins
        best = iou;
        arg = j;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float v2 = __shfl_xor(best, o, 64);
      const int a2 = __shfl_xor(arg, o, 64);
      if (v2 > best || (v2 == best && a2 < arg)) {
        best = v2;
        arg = a2;
      }
    }
    if (arg == 0x7fffffff) arg = 0;     // nothing won (every IoU NaN or -inf): the serial form's arg = 0, best = -inf
    if (ng > 0 && best >= iou_thr) {    // (wave-uniform)
      if (lane == 0) {
        // y-coordinates scale by the map's height, x-coordinates by its width (the reference's one `size` at Hm = Wm, :842)
        const float szy = (float)Hm, szx = (float)Wm;
        const float y1 = rintf(r0 * szy), x1 = rintf(r1 * szx);
        const float y2 = rintf(r2 * szy), x2 = rintf(r3 * szx);
        int gy[K + 1], gx[K + 1];
        bin_edges<K>(y1, y2, gy);
        bin_edges<K>(x1, x2, gx);
        int* o = out + cnt * RW;
        for (int k = 0; k <= K; ++k) {
          o[k] = gy[k];
          o[K + 1 + k] = gx[k];
        }
        o[2 * K + 2] = s_grow[arg];
        // mask_object pixel count (:848): sum over the k*k bins, clipped to the map
        int area = 0;
        for (int by = 0; by < K; ++by)
          for (int bx = 0; bx < K; ++bx) {
            const int hh = min(gy[by + 1], Hm) - max(gy[by], 0), ww = min(gx[bx + 1], Wm) - max(gx[bx], 0);
            if (hh > 0 && ww > 0) area += hh * ww;
          }
        o[2 * K + 3] = area;
        o[2 * K + 4] = 1;
        o[2 * K + 5] = 0;
      }
      ++cnt;
    }
  }
  for (int e = cnt * RW + lane; e < ROI_MAX * RW; e += 64) out[e] = 0;
  if (lane == 0) roi_count[b] = cnt;
}

// one thread = one score-map pixel; loops the image's positive RoIs.  score rows have k*k channels, dscore rows
// dscore_ld(k) (the pad channels are written as zeros); the k*k gradient accumulators stay in registers.  The GT masks
// are st x the score map's size (st = the mask subnet's stride: 1, 2, 4); the map is Hm x Wm.
template <int K>
__global__ __launch_bounds__(256) void psroi_loss_kernel(const float* score, const uint8_t* true_masks, int G,
                                                         const int* rois, const int* roi_count, int B, int Hm, int Wm,
                                                         int st, float mask_scale, bf16* dscore, float* partial) {
  constexpr int RW = roi_w(K), KK = K * K, LD = dscore_ld(K);
  __shared__ int s_roi[ROI_MAX * RW];
  __shared__ float s_red[4][ROI_MAX];
  const int b = blockIdx.y;
  const int cnt = roi_count[b];
  for (int i = threadIdx.x; i < ROI_MAX * RW; i += 256) s_roi[i] = rois[(size_t)b * ROI_MAX * RW + i];
  __syncthreads();
  const int npx = Hm * Wm;
  const int i = blockIdx.x * 256 + threadIdx.x;
  float g[KK];
#pragma unroll
  for (int k = 0; k < KK; ++k) g[k] = 0.f;
  float lsum[ROI_MAX];
#pragma unroll
  for (int r = 0; r < ROI_MAX; ++r) lsum[r] = 0.f;
  if (i < npx && cnt > 0) {
    const int y = i / Wm, x = i - y * Wm;
    const float* sc = score + ((size_t)b * npx + i) * KK;
    const int SH = st * Hm, SW = st * Wm;
    const float coef0 = mask_scale / ((float)B * (float)cnt);
#pragma unroll
    for (int r = 0; r < ROI_MAX; ++r) {
      if (r < cnt) {
        const int* o = s_roi + r * RW;
        if (y >= o[0] && y < o[K] && x >= o[K + 1] && x < o[2 * K + 1]) {
          int by = 0, bx = 0;
#pragma unroll
          for (int j = 1; j < K; ++j) {
            by += y >= o[j];
            bx += x >= o[K + 1 + j];
          }
          const int ch = by * K + bx;
          const float logit = sc[ch];
          // GT mask down-sampled by exact st-x legacy bilinear == [::st, ::st] (:773-775)
          const float gt = true_masks[(((size_t)b * G + o[2 * K + 2]) * SH + st * y) * SW + st * x] ? 1.f : 0.f;
          const float inv_area = 1.f / (float)o[2 * K + 3];
          lsum[r] = sigmoid_ce(gt, logit) * inv_area;
          const float dv = (sigmoidf_(logit) - gt) * inv_area * coef0;
#pragma unroll
          for (int k = 0; k < KK; ++k) g[k] += (k == ch) ? dv : 0.f;
        }
      }
    }
  }
  if (i < npx) {
    uint4* o = reinterpret_cast<uint4*>(dscore + ((size_t)b * npx + i) * LD);
#pragma unroll
    for (int c = 0; c < LD / 8; ++c) {
      float v[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] = c * 8 + k < KK ? g[c * 8 + k] : 0.f;
      o[c] = pack8(v);
    }
  }
#pragma unroll
  for (int r = 0; r < ROI_MAX; ++r) {
    const float s = wave_sum(lsum[r]);
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6][r] = s;
  }
  __syncthreads();
  if (threadIdx.x < ROI_MAX) {
    const int r = threadIdx.x;
    partial[((size_t)b * gridDim.x + blockIdx.x) * ROI_MAX + r] = s_red[0][r] + s_red[1][r] + s_red[2][r] + s_red[3][r];
  }
}

// per image: mask_scale * mean_r(sum_r);  an RoI whose area is 0 yields 0/0 = NaN like the
// reference.  One block per image: 16 RoIs x 16 partial-row lanes.
__global__ __launch_bounds__(256) void psroi_loss_image_kernel(const float* partial, const int* rois,
                                                               const int* roi_count, int nblk, int rw, float mask_scale,
                                                               float* img_loss) {
  __shared__ double sh[16][ROI_MAX];
  const int b = blockIdx.x, r = threadIdx.x % ROI_MAX, l = threadIdx.x / ROI_MAX;
  double acc = 0.0;
  for (int k = l; k < nblk; k += 16) acc += (double)partial[((size_t)b * nblk + k) * ROI_MAX + r];
  sh[l][r] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    const int cnt = roi_count[b];
    double img = 0.0;
    for (int q = 0; q < cnt; ++q) {
      double s = 0.0;
      for (int k = 0; k < 16; ++k) s += sh[k][q];
      if (rois[((size_t)b * ROI_MAX + q) * rw + rw - 3] == 0) s = NAN;   // the area word
      img += s;
    }
    img_loss[b] = cnt > 0 ? (float)((double)mask_scale * img / (double)cnt) : 0.f;
  }
}
__global__ void psroi_loss_final_kernel(const float* img_loss, int B, float* loss) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double tot = 0.0;
  for (int b = 0; b < B; ++b) tot += (double)img_loss[b];
  loss[0] = (float)(tot / (double)B);
}

// ---- the wide forms: up to ROI_CAP RoIs per image (disyolo_mask_rois_x / disyolo_psroi_loss_x) -------------------------
constexpr int ROI_CAP = DISYOLO_ROI_CAP;
static_assert(ROI_CAP == 512, "s_idx holds table rows as shorts; LDS of the wide kernels is sized for 512 rows");

// Ordered compaction over the NW waves of a block: the number of threads below this one whose flag is set, and the
// block's total.  s_w[NW] is scratch; the barrier in front keeps a call from overwriting the counts of the call before.
template <int NW>
__device__ __forceinline__ int block_rank(bool f, int* s_w, int& total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const unsigned long long m = __ballot(f);
  __syncthreads();
  if (lane == 0) s_w[w] = __popcll(m);
  __syncthreads();
  int before = 0, all = 0;
#pragma unroll
  for (int q = 0; q < NW; ++q) {
    const int c = s_w[q];
    before += q < w ? c : 0;
    all += c;
  }
  total = all;
  return before + __popcll(m & ((1ull << lane) - 1ull));
}

// The selection for n_det + n_gt <= roi_cap <= ROI_CAP: the rows mask_rois_kernel would write, one block of MRB_NW = 16 waves
// per image (with four waves the arg-max of 512 RoIs x 256 boxes was 128 rounds a wave and the call 167 us).  Wave 0 builds
// the trimmed detection list and wave 1 the trimmed box list by ordered ballots; the pick (the first n entries of a
// permutation that index a trimmed row) is an ordered compaction too, wave 0 over perm_det and wave 1 over perm_gt; every
// thread then fills the box of its RoI.  The IoU arg-max of RoI r runs on wave r % MRB_NW with the lanes over the trimmed
// boxes, by mask_rois_wave_kernel's lane rule and combine (the lower row wins a tie, NaN never wins) and the serial form's
// IoU, operation by operation.  The positives are compacted in RoI order by a block-wide ordered prefix, and the thread that
// owns an RoI writes its row.
constexpr int MRB_NW = 16, MRB_NT = MRB_NW * 64;
template <int K>
__global__ __launch_bounds__(MRB_NT) void mask_rois_block_kernel(const float* det_g, int max_det, const float* true_boxes_g,
                                                              int G, const int* perm_det_g, const int* perm_gt_g, int B,
                                                              int Hm, int Wm, int n_det, int n_gt, float iou_thr,
                                                              int roi_cap, int* rois, int* roi_count) {
  constexpr int RW = roi_w(K);
  __shared__ float s_det[MR_MAX * 6];
  __shared__ float s_tb[MR_MAX * 5];
  __shared__ int s_pd[MR_MAX], s_pg[MR_MAX];
  __shared__ int s_prow[MR_MAX], s_grow[MR_MAX];
  __shared__ int s_dpick[MR_MAX], s_gpick[MR_MAX];     // picked rows of s_det / s_tb, in pick order
  __shared__ float s_rb[ROI_CAP][4];
  __shared__ int s_arg[ROI_CAP];                       // assigned row of s_tb, -1 for a negative
  __shared__ int s_n[4];                               // np, ng, picked detections, picked boxes
  __shared__ int s_w[MRB_NW];
  const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  if (b >= B) return;
  if (max_det > MR_MAX) max_det = MR_MAX;      // (the entry point refuses more)
  if (G > MR_MAX) G = MR_MAX;
  if (n_det > MR_MAX) n_det = MR_MAX;          // a count above the row count takes every row
  if (n_gt > MR_MAX) n_gt = MR_MAX;
  for (int i = t; i < max_det * 6; i += MRB_NT) s_det[i] = det_g[(size_t)b * max_det * 6 + i];
  for (int i = t; i < G * 5; i += MRB_NT) s_tb[i] = true_boxes_g[(size_t)b * G * 5 + i];
  for (int i = t; i < max_det; i += MRB_NT) s_pd[i] = perm_det_g ? perm_det_g[b * max_det + i] : i;
  for (int i = t; i < G; i += MRB_NT) s_pg[i] = perm_gt_g ? perm_gt_g[b * G + i] : i;
  __syncthreads();
  const unsigned long long below = (1ull << lane) - 1ull;
  // trimmed lists (rows whose |coords| sum is non-zero), in row order: wave 0 the detections, wave 1 the boxes
  if (wave < 2) {
    const int n = wave ? G : max_det, pitch = wave ? 5 : 6;
    const float* src = wave ? s_tb : s_det;
    int* list = wave ? s_grow : s_prow;
    int cnt = 0;
    for (int base = 0; base < n; base += 64) {
      const int r = base + lane;
      bool f = false;
      if (r < n) {
        const float* d = src + r * pitch;
        f = fabsf(d[0]) + fabsf(d[1]) + fabsf(d[2]) + fabsf(d[3]) != 0.f;
      }
      const unsigned long long m = __ballot(f);
      if (f) list[cnt + __popcll(m & below)] = r;
      cnt += __popcll(m);
    }
    if (lane == 0) s_n[wave] = cnt;
  }
  __syncthreads();
  const int np = s_n[0], ng = s_n[1];
  // the pick: the first n_det / n_gt entries of the permutation that index a trimmed row, in permuted order
  if (wave < 2) {
    const int n = wave ? G : max_det, have = wave ? ng : np, want = wave ? n_gt : n_det;
    const int* perm = wave ? s_pg : s_pd;
    const int* list = wave ? s_grow : s_prow;
    int* pick = wave ? s_gpick : s_dpick;
    int taken = 0;
    for (int base = 0; base < n && taken < want; base += 64) {     // (wave-uniform)
      const int q = base + lane;
      const int j = q < n ? perm[q] : -1;
      const bool f = j >= 0 && j < have;
      const unsigned long long m = __ballot(f);
      const int pos = taken + __popcll(m & below);
      if (f && pos < want) pick[pos] = list[j];
      taken += __popcll(m);
    }
    if (lane == 0) s_n[2 + wave] = min(taken, want);
  }
  __syncthreads();
  const int nd = s_n[2], nr = nd + s_n[3];     // nr <= n_det + n_gt <= roi_cap
  for (int r = t; r < nr; r += MRB_NT) {
    if (r < nd) {
      const float* d = s_det + s_dpick[r] * 6;
      s_rb[r][0] = d[0]; s_rb[r][1] = d[1]; s_rb[r][2] = d[2]; s_rb[r][3] = d[3];
    } else {
      const float* g = s_tb + s_gpick[r - nd] * 5;
      s_rb[r][0] = g[1] - g[3] / 2.f; s_rb[r][1] = g[0] - g[2] / 2.f;
      s_rb[r][2] = g[1] + g[3] / 2.f; s_rb[r][3] = g[0] + g[2] / 2.f;
    }
  }
  __syncthreads();
  for (int r = wave; r < nr; r += MRB_NW) {
    const float r0 = s_rb[r][0], r1 = s_rb[r][1], r2 = s_rb[r][2], r3 = s_rb[r][3];
    float best = -INFINITY;
    int arg = 0x7fffffff;
    for (int j = lane; j < ng; j += 64) {
      const float* g = s_tb + s_grow[j] * 5;
      const float gy1 = g[1] - g[3] / 2.f, gx1 = g[0] - g[2] / 2.f, gy2 = g[1] + g[3] / 2.f, gx2 = g[0] + g[2] / 2.f;
      const float y1 = fmaxf(r0, gy1), x1 = fmaxf(r1, gx1);
      const float y2 = fminf(r2, gy2), x2 = fminf(r3, gx2);
      const float inter = fmaxf(x2 - x1, 0.f) * fmaxf(y2 - y1, 0.f);
      const float a1 = (r2 - r0) * (r3 - r1);
      const float a2 = (gy2 - gy1) * (gx2 - gx1);
      const float iou = inter / (a1 + a2 - inter);
      if (iou > best) {  // this lane's first maximum; NaN never wins
        best = iou;
        arg = j;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float v2 = __shfl_xor(best, o, 64);
      const int a2 = __shfl_xor(arg, o, 64);
      if (v2 > best || (v2 == best && a2 < arg)) {
        best = v2;
        arg = a2;
      }
    }
    if (arg == 0x7fffffff) arg = 0;     // nothing won (every IoU NaN or -inf): the serial form's arg = 0, best = -inf
    if (lane == 0) s_arg[r] = (ng > 0 && best >= iou_thr) ? s_grow[arg] : -1;
  }
  __syncthreads();
  int* out = rois + (size_t)b * roi_cap * RW;
  int cnt = 0;
  for (int base = 0; base < nr; base += MRB_NT) {       // (block-uniform)
    const int r = base + t;
    const bool f = r < nr && s_arg[r] >= 0;
    int total;
    const int row = cnt + block_rank<MRB_NW>(f, s_w, total);
    if (f) {
      // y-coordinates scale by the map's height, x-coordinates by its width (the reference's one `size` at Hm = Wm, :842)
      const float szy = (float)Hm, szx = (float)Wm;
      const float y1 = rintf(s_rb[r][0] * szy), x1 = rintf(s_rb[r][1] * szx);
      const float y2 = rintf(s_rb[r][2] * szy), x2 = rintf(s_rb[r][3] * szx);
      int gy[K + 1], gx[K + 1];
      bin_edges<K>(y1, y2, gy);
      bin_edges<K>(x1, x2, gx);
      int* o = out + row * RW;
      for (int k = 0; k <= K; ++k) {
        o[k] = gy[k];
        o[K + 1 + k] = gx[k];
      }
      o[2 * K + 2] = s_arg[r];
      // mask_object pixel count (:848): sum over the k*k bins, clipped to the map
      int area = 0;
      for (int by = 0; by < K; ++by)
        for (int bx = 0; bx < K; ++bx) {
          const int hh = min(gy[by + 1], Hm) - max(gy[by], 0), ww = min(gx[bx + 1], Wm) - max(gx[bx], 0);
          if (hh > 0 && ww > 0) area += hh * ww;
        }
      o[2 * K + 3] = area;
      o[2 * K + 4] = 1;
      o[2 * K + 5] = 0;
    }
    cnt += total;
  }
  for (int e = cnt * RW + t; e < roi_cap * RW; e += MRB_NT) out[e] = 0;
  if (t == 0) roi_count[b] = cnt;
}

// The mask loss and its gradient over a table of up to ROI_CAP rows.  One thread per score-map pixel, as in
// psroi_loss_kernel, but a pixel no longer tests every slot: the block culls the table to the rows that meet its pixel span
// (its row range, and its column range when it lies within one row of the map) by an ordered compaction, copies those rows
// to LDS in ascending RoI order, and every thread walks that list alone with psroi_loss_kernel's arithmetic.  A pixel so
// adds the terms of the RoIs that cover it in the narrow kernel's order: dscore has the same bits on a table both can take.
// The k*k gradient accumulators stay in registers.  Per RoI of the list the four waves' sums are combined in wave order,
// again as the narrow kernel does; the block writes one partial per RoI of the table, zeros for the culled ones.
template <int K>
__global__ __launch_bounds__(256) void psroi_loss_wide_kernel(const float* score, const uint8_t* true_masks, int G,
                                                              const int* rois, const int* roi_count, int roi_cap, int B,
                                                              int Hm, int Wm, int st, float mask_scale, bf16* dscore,
                                                              float* partial) {
  constexpr int RW = roi_w(K), KK = K * K, LD = dscore_ld(K);
  static_assert(RW % 4 == 0, "RoI rows are copied 16 bytes at a time");
  __shared__ int4 s_roi4[ROI_CAP * RW / 4];   // the culled rows, compacted
  __shared__ short s_idx[ROI_CAP];            // table row of each list entry
  __shared__ float s_red[4][ROI_CAP];         // per wave, per list entry
  __shared__ float s_out[ROI_CAP];            // per table row
  __shared__ int s_w[4];
  int* s_roi = reinterpret_cast<int*>(s_roi4);
  const int b = blockIdx.y, t = threadIdx.x;
  const int cnt = min(max(roi_count[b], 0), roi_cap);
  const int npx = Hm * Wm;
  const int i0 = blockIdx.x * 256, i1 = min(i0 + 255, npx - 1);
  const int ylo = i0 / Wm, yhi = i1 / Wm;
  const int xlo = ylo == yhi ? i0 - ylo * Wm : 0, xhi = ylo == yhi ? i1 - ylo * Wm : Wm - 1;
  const int* tab = rois + (size_t)b * roi_cap * RW;
  int nl = 0;
  for (int base = 0; base < cnt; base += 256) {      // (block-uniform)
    const int r = base + t;
    bool f = false;
    if (r < cnt) {
      const int* o = tab + r * RW;
      f = o[0] <= yhi && o[K] > ylo && o[K + 1] <= xhi && o[2 * K + 1] > xlo;
    }
    int total;
    const int e = nl + block_rank<4>(f, s_w, total);
    if (f) {
      const int4* src = reinterpret_cast<const int4*>(tab + r * RW);
#pragma unroll
      for (int q = 0; q < RW / 4; ++q) s_roi4[e * (RW / 4) + q] = src[q];
      s_idx[e] = (short)r;
    }
    nl += total;
  }
  for (int r = t; r < roi_cap; r += 256) s_out[r] = 0.f;
  __syncthreads();
  const int i = i0 + t;
  const bool live = i < npx && cnt > 0;
  const int y = i / Wm, x = i - y * Wm;
  const float* sc = score + ((size_t)b * npx + (live ? i : 0)) * KK;
  const int SH = st * Hm, SW = st * Wm;
  const float coef0 = mask_scale / ((float)B * (float)cnt);
  float g[KK];
#pragma unroll
  for (int k = 0; k < KK; ++k) g[k] = 0.f;
  for (int e = 0; e < nl; ++e) {
    const int* o = s_roi + e * RW;
    float term = 0.f;
    const bool in = live && y >= o[0] && y < o[K] && x >= o[K + 1] && x < o[2 * K + 1];
    if (in) {
      int by = 0, bx = 0;
#pragma unroll
      for (int j = 1; j < K; ++j) {
        by += y >= o[j];
        bx += x >= o[K + 1 + j];
      }
      const int ch = by * K + bx;
      const float logit = sc[ch];
      // GT mask down-sampled by exact st-x legacy bilinear == [::st, ::st] (:773-775)
      const float gt = true_masks[(((size_t)b * G + o[2 * K + 2]) * SH + st * y) * SW + st * x] ? 1.f : 0.f;
      const float inv_area = 1.f / (float)o[2 * K + 3];
      term = sigmoid_ce(gt, logit) * inv_area;
      const float dv = (sigmoidf_(logit) - gt) * inv_area * coef0;
#pragma unroll
      for (int k = 0; k < KK; ++k) g[k] += (k == ch) ? dv : 0.f;
    }
    float s = 0.f;
    if (__ballot(in) != 0ull) s = wave_sum(term);     // (wave-uniform)
    if ((t & 63) == 0) s_red[t >> 6][e] = s;
  }
  if (i < npx) {
    uint4* o = reinterpret_cast<uint4*>(dscore + ((size_t)b * npx + i) * LD);
#pragma unroll
    for (int c = 0; c < LD / 8; ++c) {
      float v[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] = c * 8 + k < KK ? g[c * 8 + k] : 0.f;
      o[c] = pack8(v);
    }
  }
  __syncthreads();
  for (int e = t; e < nl; e += 256) s_out[s_idx[e]] = s_red[0][e] + s_red[1][e] + s_red[2][e] + s_red[3][e];
  __syncthreads();
  float* prow = partial + ((size_t)b * gridDim.x + blockIdx.x) * roi_cap;
  for (int r = t; r < roi_cap; r += 256) prow[r] = s_out[r];
}

// per image, for the wide table: 64 RoIs x 16 partial-row slices a pass (psroi_loss_image_kernel's shape, 16 RoIs x 16
// slices, four times over).  Slice l sums blocks l, l + 16, ... of its RoI in f64, the 16 slice sums are added in slice
// order, an RoI whose area is 0 counts as NaN; the RoI sums are then added lane-strided in RoI order and
// combined by a fixed tree.  (One thread per RoI over all the blocks was 324 dependent loads a thread at 288^2: 450 us.)
__global__ __launch_bounds__(1024) void psroi_loss_image_wide_kernel(const float* partial, const int* rois,
                                                                     const int* roi_count, int roi_cap, int nblk, int rw,
                                                                     float mask_scale, float* img_loss) {
  __shared__ double sh[ROI_CAP];
  __shared__ double sh_part[16][64];
  const int b = blockIdx.x, t = threadIdx.x, q = t & 63, l = t >> 6;
  const int cnt = min(max(roi_count[b], 0), roi_cap);
  for (int base = 0; base < cnt; base += 64) {        // (block-uniform)
    const int r = base + q;
    double acc = 0.0;
    if (r < cnt) {
#pragma unroll 4
      for (int k = l; k < nblk; k += 16) acc += (double)partial[((size_t)b * nblk + k) * roi_cap + r];
    }
    sh_part[l][q] = acc;
    __syncthreads();
    if (l == 0 && r < cnt) {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < 16; ++k) s += sh_part[k][q];
      if (rois[((size_t)b * roi_cap + r) * rw + rw - 3] == 0) s = NAN;   // the area word
      sh[r] = s;
    }
    __syncthreads();
  }
  if (t < 64) {
    double img = 0.0;
    for (int r = t; r < cnt; r += 64) img += sh[r];
    img = wave_sum_d(img);
    if (t == 0) img_loss[b] = cnt > 0 ? (float)((double)mask_scale * img / (double)cnt) : 0.f;
  }
}

}  // namespace

extern "C" size_t disyolo_yolo_loss_workspace_hw(int B, int H, int W, int num_class) {
  if (B <= 0 || H <= 0 || W <= 0 || H % 32 || W % 32) return 0;
  const int h1 = H / 32, w1 = W / 32;
  size_t blocks = 0;
  for (int m = 1; m <= 4; m *= 2) blocks += (size_t)ceil_div((size_t)(m * h1) * (m * w1) * 3, 256) * B;
  return blocks * 5 * sizeof(float);
}

extern "C" size_t disyolo_yolo_loss_workspace(int B, int S, int num_class) {
  return disyolo_yolo_loss_workspace_hw(B, S, S, num_class);
}

// the launch both entry points share: ld = 0 is the 32-channel kernel of disyolo_yolo_loss, ld > 0 the wide one
static int yolo_loss_launch(const float* const logits[3], const float* const labels[3], const float* true_boxes,
                            int max_boxes, int B, int H, int W, int num_class, int ld, const float* anchors_host,
                            float ignore_thresh, const float scales[4], void* const dlogits[3], float* losses,
                            void* workspace, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const int ghs[3] = {H / 8, H / 16, H / 32}, gws[3] = {W / 8, W / 16, W / 32};
  float* part = (float*)workspace;
  int nblk[3];
  YoloLoss3 P;
  for (int s = 0; s < 3; ++s) {
    DY_REQUIRE(logits[s] && labels[s] && dlogits[s], "yolo_loss: null tensor for scale %d", s);
    YoloLossParams& p = P.p[s];
    p.logits = logits[s];
    p.labels = labels[s];
    p.true_boxes = true_boxes;
    p.dlogits = (bf16*)dlogits[s];
    p.partial = part;
    p.B = B; p.gh = ghs[s]; p.gw = gws[s]; p.C = num_class; p.G = max_boxes; p.H = H; p.W = W;
    for (int a = 0; a < 3; ++a) {
      p.aw[a] = anchors_host[(3 * s + a) * 2 + 0];
      p.ah[a] = anchors_host[(3 * s + a) * 2 + 1];
    }
    p.ignore_thresh = ignore_thresh;
    p.obj_scale = scales[0]; p.noobj_scale = scales[1]; p.class_scale = scales[2]; p.coord_scale = scales[3];
    p.inv_B = 1.f / (float)B;
    P.gx[s] = ceil_div(ghs[s] * gws[s] * 3, 256);
    nblk[s] = P.gx[s] * B;
    part += (size_t)nblk[s] * 5;
  }
  const bool tb256 = max_boxes > 64;      // (disyolo_yolo_loss_hw alone)
  if (ld)
    hipLaunchKernelGGL(tb256 ? yolo_loss_wide_kernel<DISYOLO_MAX_BOXES> : yolo_loss_wide_kernel<64>,
                       dim3(P.gx[0] + P.gx[1] + P.gx[2], B), dim3(256), 0, st, P, ld);
  else
    hipLaunchKernelGGL(tb256 ? yolo_loss_kernel<DISYOLO_MAX_BOXES> : yolo_loss_kernel<64>,
                       dim3(P.gx[0] + P.gx[1] + P.gx[2], B), dim3(256), 0, st, P);
  DY_CHECK_LAUNCH();
  hipLaunchKernelGGL(yolo_loss_final_kernel, dim3(1), dim3(320), 0, st, (const float*)workspace,
                     nblk[0] + nblk[1] + nblk[2], 1.f / (float)B, losses);
  DY_CHECK_LAUNCH();
  return DISYOLO_OK;
}

extern "C" int disyolo_yolo_loss(const float* const logits[3], const float* const labels[3], const float* true_boxes,
                                 int max_boxes, int B, int S, int num_class, const float* anchors_host,
                                 float ignore_thresh, const float scales[4], void* const dlogits[3], float* losses,
                                 void* workspace, size_t workspace_bytes, void* stream) {
  DY_REQUIRE(logits && labels && true_boxes && anchors_host && scales && dlogits && losses, "yolo_loss: null pointer");
  DY_REQUIRE(B > 0 && S > 0 && S % 32 == 0 && num_class > 0 && 3 * (5 + num_class) <= DL_LD && num_class <= 11,
             "yolo_loss: bad sizes");
  DY_REQUIRE(max_boxes > 0 && max_boxes <= 64, "yolo_loss: max_boxes must be in 1..64");
  if (!workspace || workspace_bytes < disyolo_yolo_loss_workspace(B, S, num_class)) {
    disyolo_set_error("yolo_loss: workspace too small");
    return DISYOLO_E_WORKSPACE;
  }
  {
    std::array<float, 18> anc;
    for (int i = 0; i < 18; ++i) anc[i] = anchors_host[i];
    std::array<float, 4> sc4 = {scales[0], scales[1], scales[2], scales[3]};
    std::array<const float*, 3> lg = {logits[0], logits[1], logits[2]}, lb = {labels[0], labels[1], labels[2]};
    std::array<void*, 3> dl = {dlogits[0], dlogits[1], dlogits[2]};
    DY_RECORD_OR_RUN([=](void* s) {
      return disyolo_yolo_loss(lg.data(), lb.data(), true_boxes, max_boxes, B, S, num_class, anc.data(), ignore_thresh,
                               sc4.data(), dl.data(), losses, workspace, workspace_bytes, s);
    });
  }
  return yolo_loss_launch(logits, labels, true_boxes, max_boxes, B, S, S, num_class, 0, anchors_host, ignore_thresh, scales,
                          dlogits, losses, workspace, stream);
}

extern "C" int disyolo_yolo_loss_wide(const float* const logits[3], const float* const labels[3], const float* true_boxes,
                                      int max_boxes, int B, int S, int num_class, int dlogits_ld,
                                      const float* anchors_host, float ignore_thresh, const float scales[4],
                                      void* const dlogits[3], float* losses, void* workspace, size_t workspace_bytes,
                                      void* stream) {
  DY_REQUIRE(logits && labels && true_boxes && anchors_host && scales && dlogits && losses,
             "yolo_loss_wide: null pointer");
  DY_REQUIRE(B > 0 && S > 0 && S % 32 == 0 && num_class >= 1 && num_class <= WL_MAXD - 5,
             "yolo_loss_wide: bad sizes (num_class must be in 1..80, got %d)", num_class);
  DY_REQUIRE(dlogits_ld % 32 == 0 && dlogits_ld >= 3 * (5 + num_class) && dlogits_ld <= 256,
             "yolo_loss_wide: bad sizes (dlogits_ld must be a multiple of 32 in [3 (5 + num_class), 256], got %d)",
             dlogits_ld);
  DY_REQUIRE(max_boxes > 0 && max_boxes <= 64, "yolo_loss_wide: max_boxes must be in 1..64");
  if (!workspace || workspace_bytes < disyolo_yolo_loss_workspace(B, S, num_class)) {
    disyolo_set_error("yolo_loss_wide: workspace too small");
    return DISYOLO_E_WORKSPACE;
  }
  {
    std::array<float, 18> anc;
    for (int i = 0; i < 18; ++i) anc[i] = anchors_host[i];
    std::array<float, 4> sc4 = {scales[0], scales[1], scales[2], scales[3]};
    std::array<const float*, 3> lg = {logits[0], logits[1], logits[2]}, lb = {labels[0], labels[1], labels[2]};
    std::array<void*, 3> dl = {dlogits[0], dlogits[1], dlogits[2]};
    DY_RECORD_OR_RUN([=](void* s) {
      return disyolo_yolo_loss_wide(lg.data(), lb.data(), true_boxes, max_boxes, B, S, num_class, dlogits_ld, anc.data(),
                                    ignore_thresh, sc4.data(), dl.data(), losses, workspace, workspace_bytes, s);
    });
  }
  return yolo_loss_launch(logits, labels, true_boxes, max_boxes, B, S, S, num_class, dlogits_ld, anchors_host, ignore_thresh,
                          scales, dlogits, losses, workspace, stream);
}

extern "C" int disyolo_yolo_loss_hw(const float* const logits[3], const float* const labels[3], const float* true_boxes,
                                    int max_boxes, int B, int H, int W, int num_class, int dlogits_ld,
                                    const float* anchors_host, float ignore_thresh, const float scales[4],
                                    void* const dlogits[3], float* losses, void* workspace, size_t workspace_bytes,
                                    void* stream) {
  DY_REQUIRE(logits && labels && true_boxes && anchors_host && scales && dlogits && losses, "yolo_loss_hw: null pointer");
  DY_REQUIRE(B > 0 && H > 0 && W > 0 && H % 32 == 0 && W % 32 == 0, "yolo_loss_hw: bad sizes (H = %d, W = %d)", H, W);
  if (dlogits_ld == 0) {
    DY_REQUIRE(num_class > 0 && 3 * (5 + num_class) <= DL_LD && num_class <= 11,
               "yolo_loss_hw: bad sizes (dlogits_ld = 0 takes at most 5 classes, got %d)", num_class);
  } else {
    DY_REQUIRE(num_class >= 1 && num_class <= WL_MAXD - 5, "yolo_loss_hw: bad sizes (num_class must be in 1..80, got %d)",
               num_class);
    DY_REQUIRE(dlogits_ld % 32 == 0 && dlogits_ld >= 3 * (5 + num_class) && dlogits_ld <= 256,
               "yolo_loss_hw: bad sizes (dlogits_ld must be 0 or a multiple of 32 in [3 (5 + num_class), 256], got %d)",
               dlogits_ld);
  }
  DY_REQUIRE(max_boxes > 0 && max_boxes <= DISYOLO_MAX_BOXES, "yolo_loss_hw: max_boxes must be in 1..%d (got %d)",
             DISYOLO_MAX_BOXES, max_boxes);
  if (!workspace || workspace_bytes < disyolo_yolo_loss_workspace_hw(B, H, W, num_class)) {
    disyolo_set_error("yolo_loss_hw: workspace too small");
    return DISYOLO_E_WORKSPACE;
  }
  {
    std::array<float, 18> anc;
    for (int i = 0; i < 18; ++i) anc[i] = anchors_host[i];
    std::array<float, 4> sc4 = {scales[0], scales[1], scales[2], scales[3]};
    std::array<const float*, 3> lg = {logits[0], logits[1], logits[2]}, lb = {labels[0], labels[1], labels[2]};
    std::array<void*, 3> dl = {dlogits[0], dlogits[1], dlogits[2]};
    DY_RECORD_OR_RUN([=](void* s) {
      return disyolo_yolo_loss_hw(lg.data(), lb.data(), true_boxes, max_boxes, B, H, W, num_class, dlogits_ld, anc.data(),
                                  ignore_thresh, sc4.data(), dl.data(), losses, workspace, workspace_bytes, s);
    });
  }
  return yolo_loss_launch(logits, labels, true_boxes, max_boxes, B, H, W, num_class, dlogits_ld, anchors_host, ignore_thresh,
                          scales, dlogits, losses, workspace, stream);
}

extern "C" int disyolo_shuffle_perm(int32_t* perm_det, int n_det, int32_t* perm_gt, int n_gt, int B, uint32_t seed,
                                    const int64_t* step_counter, void* stream) {
  DY_REQUIRE(perm_det && perm_gt && B > 0, "shuffle_perm: bad args");
  DY_REQUIRE(n_det > 0 && n_det <= 256 && n_gt > 0 && n_gt <= 256, "shuffle_perm: n_det and n_gt must be in 1..256 (got %d, %d)",
             n_det, n_gt);
  DY_RECORD_OR_RUN([=](void* s) { return disyolo_shuffle_perm(perm_det, n_det, perm_gt, n_gt, B, seed, step_counter, s); });
  if (n_det <= 64 && n_gt <= 64)
    hipLaunchKernelGGL(shuffle_perm_kernel<64>, dim3(B), dim3(64), 0, (hipStream_t)stream, perm_det, n_det, perm_gt, n_gt,
                       seed, step_counter);
  else
    hipLaunchKernelGGL(shuffle_perm_kernel<256>, dim3(B), dim3(256), 0, (hipStream_t)stream, perm_det, n_det, perm_gt, n_gt,
                       seed, step_counter);
  DY_CHECK_LAUNCH();
  return DISYOLO_OK;
}

// the grids of the reference's list (yolo/yolo3_net_pos.py:808-823): "k = 3" stays in every refusal's text
static bool kmap_supported(int k) { return k == 3 || k == 5 || k == 7; }

extern "C" int disyolo_mask_rois_k(const float* detections, int max_det, const float* true_boxes, int G,
                                   const int32_t* perm_det, const int32_t* perm_gt, int B, int map_size, int k, int n_det,
                                   int n_gt, float iou_thresh, int32_t* rois, int32_t* roi_count, void* stream) {
  return disyolo_mask_rois_hw(detections, max_det, true_boxes, G, perm_det, perm_gt, B, map_size, map_size, k, n_det, n_gt,
                              iou_thresh, rois, roi_count, stream);
}

extern "C" int disyolo_mask_rois_hw(const float* detections, int max_det, const float* true_boxes, int G,
                                    const int32_t* perm_det, const int32_t* perm_gt, int B, int map_h, int map_w, int k,
                                    int n_det, int n_gt, float iou_thresh, int32_t* rois, int32_t* roi_count,
                                    void* stream) {
  DY_REQUIRE(detections && true_boxes && rois && roi_count, "mask_rois: null pointer");
  DY_REQUIRE(kmap_supported(k), "mask_rois: k must be one of k = 3, 5, 7 (got %d)", k);
  DY_REQUIRE(B > 0 && map_h > 0 && map_w > 0, "mask_rois: bad sizes");
  DY_REQUIRE(max_det > 0 && max_det <= DISYOLO_MAX_DET && G > 0 && G <= DISYOLO_MAX_BOXES,
             "mask_rois: bad sizes (max_det must be in 1..%d and G in 1..%d, got %d and %d)", DISYOLO_MAX_DET,
             DISYOLO_MAX_BOXES, max_det, G);
  DY_REQUIRE(n_det >= 0 && n_gt >= 0 && n_det + n_gt <= ROI_MAX, "mask_rois: n_det + n_gt > %d", ROI_MAX);
  DY_RECORD_OR_RUN([=](void* s) {
    return disyolo_mask_rois_hw(detections, max_det, true_boxes, G, perm_det, perm_gt, B, map_h, map_w, k, n_det, n_gt,
                                iou_thresh, rois, roi_count, s);
  });
  auto kern = k == 3 ? mask_rois_kernel<3> : k == 5 ? mask_rois_kernel<5> : mask_rois_kernel<7>;
  if (max_det > 64 || G > 64) kern = k == 3 ? mask_rois_wave_kernel<3> : k == 5 ? mask_rois_wave_kernel<5> : mask_rois_wave_kernel<7>;
  hipLaunchKernelGGL(kern, dim3(B), dim3(64), 0, (hipStream_t)stream, detections, max_det, true_boxes, G, perm_det,
                     perm_gt, B, map_h, map_w, n_det, n_gt, iou_thresh, rois, roi_count);
  DY_CHECK_LAUNCH();
  return DISYOLO_OK;
}

extern "C" int disyolo_mask_rois(const float* detections, int max_det, const float* true_boxes, int G,
                                 const int32_t* perm_det, const int32_t* perm_gt, int B, int map_size, int n_det,
                                 int n_gt, float iou_thresh, int32_t* rois, int32_t* roi_count, void* stream) {
  return disyolo_mask_rois_k(detections, max_det, true_boxes, G, perm_det, perm_gt, B, map_size, 3, n_det, n_gt,
                             iou_thresh, rois, roi_count, stream);
}

extern "C" size_t disyolo_psroi_loss_workspace_hw(int B, int map_h, int map_w) {
  if (B <= 0 || map_h <= 0 || map_w <= 0) return 0;
  return ((size_t)B * ceil_div((size_t)map_h * map_w, 256) * ROI_MAX + B) * sizeof(float);
}

extern "C" size_t disyolo_psroi_loss_workspace(int B, int map_size) {
  return disyolo_psroi_loss_workspace_hw(B, map_size, map_size);
}

extern "C" int disyolo_psroi_loss(const float* score, const uint8_t* true_masks, int G, const int32_t* rois,
                                  const int32_t* roi_count, int B, int map_size, int k, float mask_scale, void* dscore,
                                  float* loss, void* workspace, size_t workspace_bytes, void* stream) {
  return disyolo_psroi_loss_s(score, true_masks, G, rois, roi_count, B, map_size, 2, k, mask_scale, dscore, loss,
                              workspace, workspace_bytes, stream);
}

extern "C" int disyolo_psroi_loss_s(const float* score, const uint8_t* true_masks, int G, const int32_t* rois,
                                    const int32_t* roi_count, int B, int map_size, int mask_stride, int k,
                                    float mask_scale, void* dscore, float* loss, void* workspace,
                                    size_t workspace_bytes, void* stream) {
  return disyolo_psroi_loss_hw(score, true_masks, G, rois, roi_count, B, map_size, map_size, mask_stride, k, mask_scale,
                               dscore, loss, workspace, workspace_bytes, stream);
}

extern "C" int disyolo_psroi_loss_hw(const float* score, const uint8_t* true_masks, int G, const int32_t* rois,
                                     const int32_t* roi_count, int B, int map_h, int map_w, int mask_stride, int k,
                                     float mask_scale, void* dscore, float* loss, void* workspace,
                                     size_t workspace_bytes, void* stream) {
  DY_REQUIRE(score && true_masks && rois && roi_count && dscore && loss, "psroi_loss: null pointer");
  DY_REQUIRE(B > 0 && map_h > 0 && map_w > 0 && (int64_t)map_h * map_w <= (1ll << 30) && G > 0, "psroi_loss: bad sizes");
  DY_REQUIRE(kmap_supported(k), "psroi_loss: k must be one of k = 3, 5, 7 (got %d)", k);
  DY_REQUIRE(mask_stride == 1 || mask_stride == 2 || mask_stride == 4,
             "psroi_loss: mask_stride must be one of 1, 2, 4 (got %d)", mask_stride);
  if (!workspace || workspace_bytes < disyolo_psroi_loss_workspace_hw(B, map_h, map_w)) {
    disyolo_set_error("psroi_loss: workspace too small");
    return DISYOLO_E_WORKSPACE;
  }
  DY_RECORD_OR_RUN([=](void* s) {
    return disyolo_psroi_loss_hw(score, true_masks, G, rois, roi_count, B, map_h, map_w, mask_stride, k, mask_scale, dscore,
                                 loss, workspace, workspace_bytes, s);
  });
  hipStream_t st = (hipStream_t)stream;
  const int nblk = ceil_div((size_t)map_h * map_w, 256);
  auto kern = k == 3 ? psroi_loss_kernel<3> : k == 5 ? psroi_loss_kernel<5> : psroi_loss_kernel<7>;
  hipLaunchKernelGGL(kern, dim3(nblk, B), dim3(256), 0, st, score, true_masks, G, rois, roi_count, B, map_h, map_w,
                     mask_stride, mask_scale, (bf16*)dscore, (float*)workspace);
  DY_CHECK_LAUNCH();
  float* img_loss = (float*)workspace + (size_t)B * nblk * ROI_MAX;
  hipLaunchKernelGGL(psroi_loss_image_kernel, dim3(B), dim3(256), 0, st, (const float*)workspace, rois, roi_count,
                     nblk, roi_w(k), mask_scale, img_loss);
  DY_CHECK_LAUNCH();
  hipLaunchKernelGGL(psroi_loss_final_kernel, dim3(1), dim3(64), 0, st, (const float*)img_loss, B, loss);
  DY_CHECK_LAUNCH();
  return DISYOLO_OK;
}

// ---- up to DISYOLO_ROI_CAP RoIs per image ----
extern "C" int disyolo_mask_rois_x(const float* detections, int max_det, const float* true_boxes, int G,
                                   const int32_t* perm_det, const int32_t* perm_gt, int B, int map_h, int map_w, int k,
                                   int n_det, int n_gt, float iou_thresh, int roi_cap, int32_t* rois, int32_t* roi_count,
                                   void* stream) {
  DY_REQUIRE(detections && true_boxes && rois && roi_count, "mask_rois_x: null pointer");
  DY_REQUIRE(kmap_supported(k), "mask_rois_x: k must be one of k = 3, 5, 7 (got %d)", k);
  DY_REQUIRE(B > 0 && map_h > 0 && map_w > 0, "mask_rois_x: bad sizes");
  DY_REQUIRE(max_det > 0 && max_det <= DISYOLO_MAX_DET && G > 0 && G <= DISYOLO_MAX_BOXES,
             "mask_rois_x: bad sizes (max_det must be in 1..%d and G in 1..%d, got %d and %d)", DISYOLO_MAX_DET,
             DISYOLO_MAX_BOXES, max_det, G);
  DY_REQUIRE(roi_cap > 0 && roi_cap <= ROI_CAP, "mask_rois_x: roi_cap must be in 1..%d (got %d)", ROI_CAP, roi_cap);
  DY_REQUIRE(n_det >= 0 && n_gt >= 0 && n_det <= ROI_CAP && n_gt <= ROI_CAP && n_det + n_gt <= roi_cap,
             "mask_rois_x: n_det + n_gt > roi_cap (got %d + %d, roi_cap %d)", n_det, n_gt, roi_cap);
  DY_RECORD_OR_RUN([=](void* s) {
    return disyolo_mask_rois_x(detections, max_det, true_boxes, G, perm_det, perm_gt, B, map_h, map_w, k, n_det, n_gt,
                               iou_thresh, roi_cap, rois, roi_count, s);
  });
  auto kern = k == 3 ? mask_rois_block_kernel<3> : k == 5 ? mask_rois_block_kernel<5> : mask_rois_block_kernel<7>;
  hipLaunchKernelGGL(kern, dim3(B), dim3(MRB_NT), 0, (hipStream_t)stream, detections, max_det, true_boxes, G, perm_det,
                     perm_gt, B, map_h, map_w, n_det, n_gt, iou_thresh, roi_cap, rois, roi_count);
  DY_CHECK_LAUNCH();
  return DISYOLO_OK;
}

extern "C" size_t disyolo_psroi_loss_workspace_x(int B, int map_h, int map_w, int roi_cap) {
  if (B <= 0 || map_h <= 0 || map_w <= 0 || roi_cap <= 0 || roi_cap > ROI_CAP) return 0;
  return ((size_t)B * ceil_div((size_t)map_h * map_w, 256) * roi_cap + B) * sizeof(float);
}

extern "C" int disyolo_psroi_loss_x(const float* score, const uint8_t* true_masks, int G, const int32_t* rois,
                                    const int32_t* roi_count, int roi_cap, int B, int map_h, int map_w, int mask_stride,
                                    int k, float mask_scale, void* dscore, float* loss, void* workspace,
                                    size_t workspace_bytes, void* stream) {
  DY_REQUIRE(score && true_masks && rois && roi_count && dscore && loss, "psroi_loss_x: null pointer");
  DY_REQUIRE(B > 0 && map_h > 0 && map_w > 0 && (int64_t)map_h * map_w <= (1ll << 30) && G > 0, "psroi_loss_x: bad sizes");
  DY_REQUIRE(roi_cap > 0 && roi_cap <= ROI_CAP, "psroi_loss_x: roi_cap must be in 1..%d (got %d)", ROI_CAP, roi_cap);
  DY_REQUIRE(kmap_supported(k), "psroi_loss_x: k must be one of k = 3, 5, 7 (got %d)", k);
  DY_REQUIRE(mask_stride == 1 || mask_stride == 2 || mask_stride == 4,
             "psroi_loss_x: mask_stride must be one of 1, 2, 4 (got %d)", mask_stride);
  if (!workspace || workspace_bytes < disyolo_psroi_loss_workspace_x(B, map_h, map_w, roi_cap)) {
    disyolo_set_error("psroi_loss_x: workspace too small");
    return DISYOLO_E_WORKSPACE;
  }
  DY_RECORD_OR_RUN([=](void* s) {
    return disyolo_psroi_loss_x(score, true_masks, G, rois, roi_count, roi_cap, B, map_h, map_w, mask_stride, k, mask_scale,
                                dscore, loss, workspace, workspace_bytes, s);
  });
  hipStream_t st = (hipStream_t)stream;
  const int nblk = ceil_div((size_t)map_h * map_w, 256);
  auto kern = k == 3 ? psroi_loss_wide_kernel<3> : k == 5 ? psroi_loss_wide_kernel<5> : psroi_loss_wide_kernel<7>;
  hipLaunchKernelGGL(kern, dim3(nblk, B), dim3(256), 0, st, score, true_masks, G, rois, roi_count, roi_cap, B, map_h, map_w,
                     mask_stride, mask_scale, (bf16*)dscore, (float*)workspace);
  DY_CHECK_LAUNCH();
  float* img_loss = (float*)workspace + (size_t)B * nblk * roi_cap;
  hipLaunchKernelGGL(psroi_loss_image_wide_kernel, dim3(B), dim3(1024), 0, st, (const float*)workspace, rois, roi_count,
                     roi_cap, nblk, roi_w(k), mask_scale, img_loss);
  DY_CHECK_LAUNCH();
  hipLaunchKernelGGL(psroi_loss_final_kernel, dim3(1), dim3(64), 0, st, (const float*)img_loss, B, loss);
  DY_CHECK_LAUNCH();
  return DISYOLO_OK;
}

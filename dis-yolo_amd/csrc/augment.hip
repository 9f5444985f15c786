// Training-data pipeline kernels (reference: utils/train_data.py:44-276, 321-531).
// The reference prepares every batch synchronously on the host (cv2 + scikit-image, :145) -- at the
// step rates of this path that is three orders of magnitude short, so the pixel work runs here:
//   polygon_mask   skimage.draw.polygon + the out/in/vertex rules of load_mask (:321-338)
//   place_image    cv2.resize(INTER_LINEAR, uint8) -> shift/crop/pad 127 -> flip (:466-494, 392-397)
//   place_mask     cv2.resize(INTER_LINEAR, float32) -> shift/crop/pad 0 -> flip -> np.around -> bool (:418-444)
//   salt_pepper / change_light / motion_blur3     the photometric augmentations (:496-531)
//   to_float       uint8 -> float32 / 255 (:411-413)
// Host code (train_data.py) only draws the random decisions and transforms the handful of boxes.
// scikit-image's rasteriser is pinned by golden vectors (tests/golden/polygon.json); cv2 and pyblur are not
// installable here: their arithmetic is restated from the libraries' documented behaviour -- unpinned.
#include <climits>

#include "common.h"
#include "runtime.h"

namespace {

// scikit-image's point_in_polygon (measure/_pnpoly): 0 outside, non-zero inside / on a vertex / on an edge.
// Coordinates are doubles like there (the annotation lists are integers).
__device__ __forceinline__ int point_in_polygon(const float* xp, const float* yp, int n, double x, double y) {
  const double eps = 1e-12;
  double x0 = (double)xp[n - 1] - x, y0 = (double)yp[n - 1] - y;
  unsigned l = 0, r = 0;
  for (int i = 0; i < n; ++i) {
    const double x1 = (double)xp[i] - x, y1 = (double)yp[i] - y;
    if (x1 > -eps && x1 < eps && y1 > -eps && y1 < eps) return 2;
    if (((y0 > 0) != (y1 > 0)) && (__ddiv_rn(x0 * y1 - x1 * y0, y1 - y0) > 0)) ++r;
    if (((y0 < 0) != (y1 < 0)) && (__ddiv_rn(x0 * y1 - x1 * y0, y1 - y0) < 0)) ++l;
    x0 = x1;
    y0 = y1;
  }
  if ((r & 1) != (l & 1)) return 3;
  return (r & 1) ? 1 : 0;
}

// one instance = npoly polygons drawn in order: 'out' polygons set their pixels, 'in' polygons clear them
// (holes), and every polygon finally sets its own vertex pixels (utils/train_data.py:325-336)
__global__ __launch_bounds__(256) void polygon_mask_kernel(const float* px, const float* py, const int* start,
                                                           const int* type_out, int npoly, int H, int W,
                                                           unsigned char* mask) {
  const int64_t total = (int64_t)H * W;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int r = (int)(i / W), c = (int)(i - (int64_t)r * W);
    unsigned char v = 0;
    for (int k = 0; k < npoly; ++k) {
      const int a = start[k], n = start[k + 1] - a;
      if (n <= 0) continue;
      // bounding box of skimage's _polygon: rows [max(0,min), ceil(max)], same for columns
      float ymin = py[a], ymax = py[a], xmin = px[a], xmax = px[a];
      for (int j = 1; j < n; ++j) {
        ymin = fminf(ymin, py[a + j]); ymax = fmaxf(ymax, py[a + j]);
        xmin = fminf(xmin, px[a + j]); xmax = fmaxf(xmax, px[a + j]);
      }
      if (r >= (int)fmaxf(0.f, ymin) && r <= (int)ceilf(ymax) && c >= (int)fmaxf(0.f, xmin) && c <= (int)ceilf(xmax) &&
          point_in_polygon(px + a, py + a, n, (double)c, (double)r))
        v = type_out[k] ? 1 : 0;
      for (int j = 0; j < n; ++j)
        if ((int)py[a + j] == r && (int)px[a + j] == c) v = 1;
    }
    mask[i] = v;
  }
}

struct Taps {
  int s0, s1;
  float a;
};
// cv2.resize INTER_LINEAR source taps of destination index d (dn destination / sn source samples)
__device__ __forceinline__ Taps taps(int d, int dn, int sn) {
  float f = (float)(((double)d + 0.5) * ((double)sn / (double)dn) - 0.5);
  int s = (int)floorf(f);
  float a = __fsub_rn(f, (float)s);
  if (s < 0) { a = 0.f; s = 0; }
  if (s >= sn - 1) { a = 0.f; s = sn - 1; }
  return Taps{s, min(s + 1, sn - 1), a};
}

// destination pixel (y, x) of the SH x SW training image (net_h x net_w) -> position in the resized image, or outside (pad):
// the resized image (new_w x new_h) is placed with its corner at (dx, dy) (negative = cropped), then flipped
__device__ __forceinline__ bool locate(int y, int x, int SH, int SW, int new_w, int new_h, int dx, int dy, int flip, int* ry,
                                       int* rx) {
  if (flip == 2) x = SW - 1 - x;    // horizontal flip: image[:, ::-1]
  if (flip == 3) y = SH - 1 - y;    // vertical flip
  *ry = y - dy;
  *rx = x - dx;
  return *ry >= 0 && *ry < new_h && *rx >= 0 && *rx < new_w;
}

// uint8 image: OpenCV's 8-bit bilinear path works in fixed point -- coefficients rounded to 11 bits,
// horizontal pass in int, vertical pass (b0*S0 + b1*S1 + 2^21) >> 22
__device__ __forceinline__ void place_image_px(const unsigned char* src, int H, int W, unsigned char* dst, int SH, int SW, int new_w,
                                               int new_h, int dx, int dy, int flip, int64_t i) {
  const int y = (int)(i / SW), x = (int)(i - (int64_t)y * SW);
  int ry, rx;
  unsigned char v[3] = {127, 127, 127};
  if (locate(y, x, SH, SW, new_w, new_h, dx, dy, flip, &ry, &rx)) {
    const Taps tx = taps(rx, new_w, W), ty = taps(ry, new_h, H);
    const int ax1 = (int)rintf(tx.a * 2048.f), ax0 = 2048 - ax1;
    const int ay1 = (int)rintf(ty.a * 2048.f), ay0 = 2048 - ay1;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int h0 = src[((size_t)ty.s0 * W + tx.s0) * 3 + c] * ax0 + src[((size_t)ty.s0 * W + tx.s1) * 3 + c] * ax1;
      const int h1 = src[((size_t)ty.s1 * W + tx.s0) * 3 + c] * ax0 + src[((size_t)ty.s1 * W + tx.s1) * 3 + c] * ax1;
      const int r = (h0 * ay0 + h1 * ay1 + (1 << 21)) >> 22;
      v[c] = (unsigned char)min(max(r, 0), 255);
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) dst[i * 3 + c] = v[c];
}
__global__ __launch_bounds__(256) void place_image_kernel(const unsigned char* src, int H, int W, unsigned char* dst, int SH, int SW,
                                                          int new_w, int new_h, int dx, int dy, int flip) {
  const int64_t total = (int64_t)SH * SW;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x)
    place_image_px(src, H, W, dst, SH, SW, new_w, new_h, dx, dy, flip, i);
}

// float mask (0/1 bytes in, treated as float32): float bilinear path, pad 0, np.around (half to even) -> bool
__device__ __forceinline__ void place_mask_px(const unsigned char* src, int H, int W, unsigned char* dst, int SH, int SW, int new_w,
                                              int new_h, int dx, int dy, int flip, int64_t i) {
  const int y = (int)(i / SW), x = (int)(i - (int64_t)y * SW);
  int ry, rx;
  float v = 0.f;
  if (locate(y, x, SH, SW, new_w, new_h, dx, dy, flip, &ry, &rx)) {
    const Taps tx = taps(rx, new_w, W), ty = taps(ry, new_h, H);
    const float bx = __fsub_rn(1.f, tx.a), by = __fsub_rn(1.f, ty.a);
    const float h0 = __fadd_rn(__fmul_rn((float)src[(size_t)ty.s0 * W + tx.s0], bx), __fmul_rn((float)src[(size_t)ty.s0 * W + tx.s1], tx.a));
    const float h1 = __fadd_rn(__fmul_rn((float)src[(size_t)ty.s1 * W + tx.s0], bx), __fmul_rn((float)src[(size_t)ty.s1 * W + tx.s1], tx.a));
    v = __fadd_rn(__fmul_rn(h0, by), __fmul_rn(h1, ty.a));
  }
  dst[i] = rintf(v) != 0.f ? 1 : 0;
}
__global__ __launch_bounds__(256) void place_mask_kernel(const unsigned char* src, int H, int W, unsigned char* dst, int SH, int SW,
                                                         int new_w, int new_h, int dx, int dy, int flip) {
  const int64_t total = (int64_t)SH * SW;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x)
    place_mask_px(src, H, W, dst, SH, SW, new_w, new_h, dx, dy, flip, i);
}

// a whole batch's placements in ONE launch (round 6: the loader's ~25 per-image / per-instance launches were its GPU time):
// blockIdx.y = job; the per-pixel arithmetic is the single-job kernels' own
__global__ __launch_bounds__(256) void place_batch_kernel(const disyolo_place_job* jobs, int SH, int SW) {
  const disyolo_place_job j = jobs[blockIdx.y];
  const int64_t total = (int64_t)SH * SW;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    if (j.is_mask)
      place_mask_px(j.src, j.image_h, j.image_w, j.dst, SH, SW, j.new_w, j.new_h, j.dx, j.dy, j.flip, i);
    else
      place_image_px(j.src, j.image_h, j.image_w, j.dst, SH, SW, j.new_w, j.new_h, j.dx, j.dy, j.flip, i);
  }
}

// add_salt_pepper_noise (:511-525): im[rows, cols, :] = 1 for the salt coordinates, then 0 for the pepper ones
__global__ void salt_pepper_kernel(unsigned char* img, int SH, int SW, const int* rows, const int* cols, int nsalt, int npepper) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nsalt + npepper) return;
  const unsigned char v = i < nsalt ? 1 : 0;
  if ((unsigned)rows[i] >= (unsigned)SH || (unsigned)cols[i] >= (unsigned)SW) return;   // (a coordinate outside the image)
  unsigned char* p = img + ((size_t)rows[i] * SW + cols[i]) * 3;
  p[0] = v; p[1] = v; p[2] = v;
}

// change_light (:527-535): RGB -> HLS (8-bit: H/2, 255 L, 255 S), L *= coeff (float64, clipped at 255, truncated
// to uint8), HLS -> RGB.  Formulas of OpenCV's colour-conversion documentation, float32, rounded to nearest.
__device__ __forceinline__ unsigned char sat8(float v) { return (unsigned char)min(max((int)rintf(v), 0), 255); }
__global__ __launch_bounds__(256) void change_light_kernel(unsigned char* img, int64_t npix, double coeff) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += (int64_t)gridDim.x * blockDim.x) {
    const float r = img[i * 3] * (1.f / 255.f), g = img[i * 3 + 1] * (1.f / 255.f), b = img[i * 3 + 2] * (1.f / 255.f);
    const float vmax = fmaxf(r, fmaxf(g, b)), vmin = fminf(r, fminf(g, b));
    const float diff = vmax - vmin, sum = vmax + vmin;
    float h = 0.f, s = 0.f;
    const float l = sum * 0.5f;
    if (diff > 1.1920929e-07f) {
      s = l < 0.5f ? diff / sum : diff / (2.f - sum);
      const float d60 = 60.f / diff;
      if (vmax == r) h = (g - b) * d60;
      else if (vmax == g) h = (b - r) * d60 + 120.f;
      else h = (r - g) * d60 + 240.f;
      if (h < 0.f) h += 360.f;
    }
    const unsigned char H8 = sat8(h * 0.5f), S8 = sat8(s * 255.f);
    double L = (double)sat8(l * 255.f) * coeff;
    if (L > 255.0) L = 255.0;
    const unsigned char L8 = (unsigned char)L;           // np.array(..., dtype=np.uint8): truncation
    // back: HLS -> RGB
    const float hh = (float)H8 * 2.f, ll = (float)L8 * (1.f / 255.f), ss = (float)S8 * (1.f / 255.f);
    float ro, go, bo;
    if (ss == 0.f) {
      ro = go = bo = ll;
    } else {
      const float p2 = ll <= 0.5f ? ll * (1.f + ss) : ll + ss - ll * ss;
      const float p1 = 2.f * ll - p2;
      float hq = hh * (1.f / 60.f);
      if (hq < 0.f) do hq += 6.f; while (hq < 0.f);
      else if (hq >= 6.f) do hq -= 6.f; while (hq >= 6.f);
      const int sector = (int)floorf(hq);
      const float f = hq - (float)sector;
      const float tab[4] = {p2, p1, p1 + (p2 - p1) * (1.f - f), p1 + (p2 - p1) * f};
      const int idx[6][3] = {{1, 3, 0}, {1, 0, 2}, {3, 0, 1}, {0, 2, 1}, {0, 1, 3}, {2, 1, 0}};   // (b, g, r) per sector
      bo = tab[idx[sector][0]]; go = tab[idx[sector][1]]; ro = tab[idx[sector][2]];
    }
    img[i * 3] = sat8(ro * 255.f); img[i * 3 + 1] = sat8(go * 255.f); img[i * 3 + 2] = sat8(bo * 255.f);
  }
}

// linearmotion_blur3C (:466-494) with lineLength 3: a 3x3 line kernel through the centre (angle 0 / 45 / 90 / 135,
// "full" = three taps, "right" / "left" = the centre and one neighbour), normalised; pixels outside the image count as
// 255 (pyblur's LinearMotionBlur: scipy.signal.convolve2d(img, kernel, mode='same', fillvalue=255.0)), result truncated
// to uint8
__global__ __launch_bounds__(256) void motion_blur3_kernel(const unsigned char* src, unsigned char* dst, int SH, int SW, int dyA,
                                                           int dxA, int use_a, int use_b) {
  const int64_t total = (int64_t)SH * SW;
  const float wgt = 1.f / (float)(1 + use_a + use_b);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int y = (int)(i / SW), x = (int)(i - (int64_t)y * SW);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      // taps in the (flipped) kernel's row-major order: the "b" end first when it lies above / left of the centre
      float acc = 0.f;
      const int ya = y + dyA, xa = x + dxA, yb = y - dyA, xb = x - dxA;
      const float va = (ya >= 0 && ya < SH && xa >= 0 && xa < SW) ? (float)src[((size_t)ya * SW + xa) * 3 + c] : 255.f;
      const float vb = (yb >= 0 && yb < SH && xb >= 0 && xb < SW) ? (float)src[((size_t)yb * SW + xb) * 3 + c] : 255.f;
      if (use_a) acc += va * wgt;
      acc += (float)src[i * 3 + c] * wgt;
      if (use_b) acc += vb * wgt;
      dst[i * 3 + c] = (unsigned char)min(max((int)acc, 0), 255);
    }
  }
}

__global__ __launch_bounds__(256) void to_float_kernel(const unsigned char* src, float* dst, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    dst[i] = __fdiv_rn((float)src[i], 255.f);           // image.astype(float32) / 255.0 stays float32 in numpy
}

// ---- window training: a batch image is a net-size window of its record at scale 1 ---------------------------
// the visible part of a job's instance: crop n window n image, in image coordinates (empty when x2 <= x1 or y2 <= y1)
struct WinRect {
  int x1, y1, x2, y2;
};
__device__ __forceinline__ WinRect window_rect(const disyolo_window_job& j, int net_h, int net_w) {
  WinRect r;
  r.x1 = max(max(j.crop_x, j.x0), 0);
  r.y1 = max(max(j.crop_y, j.y0), 0);
  r.x2 = min(min(j.crop_x + j.crop_w, j.x0 + net_w), j.image_w);
  r.y2 = min(min(j.crop_y + j.crop_h, j.y0 + net_h), j.image_h);
  return r;
}
constexpr int WIN_ROWS = 16;       // rows of a job's visible rect per block: a crack's crop as tall as the window takes net_h / 16 blocks

__global__ void window_vis_init_kernel(int* vis, int njobs) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= njobs) return;
  vis[5 * i] = 0; vis[5 * i + 1] = INT_MAX; vis[5 * i + 2] = INT_MAX; vis[5 * i + 3] = 0; vis[5 * i + 4] = 0;
}
__global__ void window_vis_finish_kernel(int* vis, int njobs) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= njobs) return;
  if (vis[5 * i] == 0) vis[5 * i + 1] = vis[5 * i + 2] = 0;      // nothing visible: the box is zeros
}

// blockIdx.y = job, blockIdx.x = a group of WIN_ROWS rows of its visible rect.  Only bytes inside the rect are read, as aligned
// 4-byte words where a whole word lies inside the row's segment.  Integer wave reductions, then one set of integer atomics
// per block: sums, minima and maxima of integers do not depend on the order.
__global__ __launch_bounds__(256) void window_visible_kernel(const disyolo_window_job* jobs, int net_h, int net_w, int* vis) {
  const disyolo_window_job j = jobs[blockIdx.y];
  const WinRect r = window_rect(j, net_h, net_w);
  const int ya = r.y1 + (int)blockIdx.x * WIN_ROWS, yb = min(ya + WIN_ROWS, r.y2);
  if (r.x2 <= r.x1 || ya >= yb) return;                          // (the same for every thread of the block)
  const int width = r.x2 - r.x1, nslot = (width + 3) / 4 + 1;
  int cnt = 0, xmin = INT_MAX, xmax = -1, ymin = INT_MAX, ymax = -1;
  for (int i = threadIdx.x; i < (yb - ya) * nslot; i += blockDim.x) {
    const int y = ya + i / nslot, k = i % nslot;
    const unsigned char* lo = j.src + (size_t)(y - j.crop_y) * j.crop_w + (r.x1 - j.crop_x);
    const uintptr_t a_lo = (uintptr_t)lo, a_hi = a_lo + width, wa = (a_lo & ~(uintptr_t)3) + 4 * (uintptr_t)k;
    if (wa >= a_hi) continue;
    unsigned word = 0;                                           // the word's bytes inside [lo, hi), others 0
    if (wa >= a_lo && wa + 4 <= a_hi) {
      word = *reinterpret_cast<const unsigned*>(wa);
    } else {
#pragma unroll
      for (int t = 0; t < 4; ++t)
        if (wa + t >= a_lo && wa + t < a_hi) word |= (unsigned)*reinterpret_cast<const unsigned char*>(wa + t) << (8 * t);
    }
    if (word == 0) continue;
#pragma unroll
    for (int t = 0; t < 4; ++t)
      if ((word >> (8 * t)) & 0xffu) {
        const int x = r.x1 + (int)((int64_t)(wa + t) - (int64_t)a_lo) - j.x0;   // window coordinates
        ++cnt;
        xmin = min(xmin, x); xmax = max(xmax, x);
        ymin = min(ymin, y - j.y0); ymax = max(ymax, y - j.y0);
      }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    cnt += __shfl_xor(cnt, o, 64);
    xmin = min(xmin, __shfl_xor(xmin, o, 64)); ymin = min(ymin, __shfl_xor(ymin, o, 64));
    xmax = max(xmax, __shfl_xor(xmax, o, 64)); ymax = max(ymax, __shfl_xor(ymax, o, 64));
  }
  __shared__ int part[4][5];
  const int wave = threadIdx.x / DY_WAVE;
  if (threadIdx.x % DY_WAVE == 0) {
    part[wave][0] = cnt; part[wave][1] = xmin; part[wave][2] = ymin; part[wave][3] = xmax; part[wave][4] = ymax;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w) {
      cnt += part[w][0];
      xmin = min(xmin, part[w][1]); ymin = min(ymin, part[w][2]);
      xmax = max(xmax, part[w][3]); ymax = max(ymax, part[w][4]);
    }
    if (cnt > 0) {
      int* v = vis + 5 * (size_t)blockIdx.y;
      atomicAdd(v, cnt);
      atomicMin(v + 1, xmin); atomicMin(v + 2, ymin);
      atomicMax(v + 3, xmax + 1); atomicMax(v + 4, ymax + 1);
    }
  }
}

// blockIdx.y = which array: the four target arrays <- 0, rows <- -1; 16-byte stores between the unaligned ends
struct WinClear {
  unsigned* p[5];
  int64_t n[5];
};
__global__ __launch_bounds__(256) void window_clear_kernel(WinClear c) {
  unsigned* p = c.p[blockIdx.y];
  const int64_t n = c.n[blockIdx.y];
  const unsigned v = blockIdx.y == 4 ? 0xffffffffu : 0u;
  int64_t head = (int64_t)((16 - ((uintptr_t)p & 15)) & 15) / 4;
  if (head > n) head = n;
  const int64_t quads = (n - head) / 4, tail = head + 4 * quads;
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
  uint4* q = reinterpret_cast<uint4*>(p + head);
  for (int64_t i = tid; i < quads; i += step) q[i] = make_uint4(v, v, v, v);
  if (tid < head) p[tid] = v;
  if (tid < n - tail) p[tail + tid] = v;
}

// ONE lane per image walks the image's jobs in order: the order defines the rows of true_boxes and which box keeps a
// (cell, anchor) that two boxes fall into.  f32 arithmetic operation by operation as synth.assign_target_entries and
// defect_train._fill do it in numpy (this file is compiled without contraction).
__global__ void window_targets_kernel(const disyolo_window_job* jobs, int njobs, const int* vis, const float* anchors, int B, int G,
                                      int C, int net_h, int net_w, int min_visible, float* true_boxes, float* yolo3, float* yolo2,
                                      float* yolo1, int* rows) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  float ahw[9][2], a_area[9];
  for (int k = 0; k < 9; ++k) {
    ahw[k][0] = __fmul_rn(anchors[2 * k], 0.5f);
    ahw[k][1] = __fmul_rn(anchors[2 * k + 1], 0.5f);
    a_area[k] = __fmul_rn(__fmul_rn(ahw[k][0], ahw[k][1]), 4.f);
  }
  const float fw = (float)net_w, fh = (float)net_h;
  int r = 0;
  for (int i = 0; i < njobs; ++i) {
    if (jobs[i].b != b) continue;
    const int flip = jobs[i].flip, cls = jobs[i].cls;
    const int* v = vis + 5 * (size_t)i;
    // the loader's clamp of each coordinate to [0, net - 1] (sx = sy = 1, dx = dy = 0)
    const int x1 = max(min(v[1], net_w - 1), 0), y1 = max(min(v[2], net_h - 1), 0);
    const int x2 = max(min(v[3], net_w - 1), 0), y2 = max(min(v[4], net_h - 1), 0);
    if (v[0] < min_visible || x2 - x1 <= 0 || y2 - y1 <= 0 || r >= G) {
      rows[i] = -1;
      continue;
    }
    rows[i] = r;
    const float xc = __fmul_rn((float)(x1 + x2), 0.5f), yc = __fmul_rn((float)(y1 + y2), 0.5f);    // integers or halves: exact
    const float w = (float)(x2 - x1), h = (float)(y2 - y1);
    const float xcf = flip == 2 ? __fsub_rn((float)(net_w - 1), xc) : xc, ycf = flip == 3 ? __fsub_rn((float)(net_h - 1), yc) : yc;
    const float out[4] = {__fdiv_rn(xcf, fw), __fdiv_rn(ycf, fh), __fdiv_rn(w, fw), __fdiv_rn(h, fh)};
    float* tb = true_boxes + ((size_t)b * G + r) * 5;
    tb[0] = out[0]; tb[1] = out[1]; tb[2] = out[2]; tb[3] = out[3]; tb[4] = (float)cls;
    ++r;
    // best of the nine anchors, boxes centred at the origin
    const float hw = __fmul_rn(w, 0.5f), hh = __fmul_rn(h, 0.5f);
    const float area = __fmul_rn(__fmul_rn(hw, hh), 4.f);
    float best = 0.f;
    int idx = 0;
    for (int k = 0; k < 9; ++k) {
      const float iw = fmaxf(__fmul_rn(2.f, fminf(hw, ahw[k][0])), 0.f), ih = fmaxf(__fmul_rn(2.f, fminf(hh, ahw[k][1])), 0.f);
      const float ia = __fmul_rn(iw, ih);
      const float iou = __fdiv_rn(ia, __fsub_rn(__fadd_rn(area, a_area[k]), ia));
      if (k == 0 || iou > best) { best = iou; idx = k; }         // the first maximum, like argmax
    }
    if (!(best > 0.f)) continue;                                 // the box row stays, no cell
    const int s = idx / 3, a = idx - 3 * s, d = 8 << s;
    const int gh = net_h / d, gw = net_w / d;
    // int(xc * gw / net_w): gw / net_w = 1 / d and xc is a multiple of 1/2, so the quotient is exact in any precision
    int xi = min((x1 + x2) / (2 * d), gw - 1), yi = min((y1 + y2) / (2 * d), gh - 1);
    if (flip == 2) xi = gw - 1 - xi;
    if (flip == 3) yi = gh - 1 - yi;
    float* grid = s == 0 ? yolo3 : (s == 1 ? yolo2 : yolo1);
    float* cell = grid + ((((size_t)b * gh + yi) * gw + xi) * 3 + a) * (size_t)(5 + C);
    if (cell[4] != 0.f) continue;                                // an occupied (cell, anchor) keeps its first box
    cell[0] = out[0]; cell[1] = out[1]; cell[2] = out[2]; cell[3] = out[3]; cell[4] = 1.f;
    if (cls >= 0 && cls < C) cell[5 + cls] = 1.f;
  }
}

// blockIdx.y = job, blockIdx.x = a group of WIN_ROWS rows of its visible rect; one thread per aligned 4-byte word of the
// destination row: a word that lies inside the row's segment and whose four source bytes are aligned too moves as one word
// (byte-swapped for the horizontal flip), everything else byte by byte
__global__ __launch_bounds__(256) void window_place_masks_kernel(const disyolo_window_job* jobs, const int* rows,
                                                                 unsigned char* true_masks, int G, int net_h, int net_w) {
  const int row = rows[blockIdx.y];
  if (row < 0 || row >= G) return;
  const disyolo_window_job j = jobs[blockIdx.y];
  const WinRect r = window_rect(j, net_h, net_w);
  const int ya = r.y1 + (int)blockIdx.x * WIN_ROWS, yb = min(ya + WIN_ROWS, r.y2);
  if (r.x2 <= r.x1 || ya >= yb || j.b < 0) return;
  unsigned char* plane = true_masks + ((size_t)j.b * G + row) * net_h * net_w;
  const int wx1 = r.x1 - j.x0, wx2 = r.x2 - j.x0;                // window columns [wx1, wx2)
  const int dlo = j.flip == 2 ? net_w - wx2 : wx1, dhi = j.flip == 2 ? net_w - wx1 : wx2;
  const int nslot = (dhi - dlo + 3) / 4 + 1;
  for (int i = threadIdx.x; i < (yb - ya) * nslot; i += blockDim.x) {
    const int y = ya + i / nslot, k = i % nslot;
    const int wy = y - j.y0;
    unsigned char* drow = plane + (size_t)(j.flip == 3 ? net_h - 1 - wy : wy) * net_w;
    // source byte of window column wx: srow[wx - wx1]
    const unsigned char* srow = j.src + (size_t)(y - j.crop_y) * j.crop_w + (r.x1 - j.crop_x);
    const uintptr_t d_lo = (uintptr_t)(drow + dlo), d_hi = (uintptr_t)(drow + dhi), wa = (d_lo & ~(uintptr_t)3) + 4 * (uintptr_t)k;
    if (wa >= d_hi) continue;
    const int c0 = dlo + (int)((int64_t)wa - (int64_t)d_lo);     // destination column of the word's first byte
    if (wa >= d_lo && wa + 4 <= d_hi) {
      const unsigned char* s4 = j.flip == 2 ? srow + (net_w - 1 - (c0 + 3) - wx1) : srow + (c0 - wx1);
      if (((uintptr_t)s4 & 3) == 0) {
        const unsigned word = *reinterpret_cast<const unsigned*>(s4);
        *reinterpret_cast<unsigned*>(wa) = j.flip == 2 ? __builtin_bswap32(word) : word;
        continue;
      }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int c = c0 + t;
      if (c >= dlo && c < dhi) drow[c] = srow[(j.flip == 2 ? net_w - 1 - c : c) - wx1];
    }
  }
}

int grid_for(int64_t n) {
  int64_t g = (n + 255) / 256;
  if (g > 256 * 16) g = 256 * 16;
  return (int)(g < 1 ? 1 : g);
}

}  // namespace

extern "C" int disyolo_polygon_mask(const float* px, const float* py, const int32_t* poly_start, const int32_t* poly_is_out,
                                    int npoly, int image_h, int image_w, uint8_t* mask, void* stream) {
  DY_REQUIRE(px && py && poly_start && poly_is_out && mask && npoly >= 0 && image_h > 0 && image_w > 0, "polygon_mask: bad args");
  DY_RECORD_OR_RUN([=](void* s) { return disyolo_polygon_mask(px, py, poly_start, poly_is_out, npoly, image_h, image_w, mask, s); });
  hipLaunchKernelGGL(polygon_mask_kernel, dim3(grid_for((int64_t)image_h * image_w)), dim3(256), 0, (hipStream_t)stream, px, py,
                     poly_start, poly_is_out, npoly, image_h, image_w, mask);
  DY_CHECK_LAUNCH();
  return DISYOLO_OK;
}

extern "C" int disyolo_aug_place(const uint8_t* src, int is_mask, int image_h, int image_w, uint8_t* dst, int size, int new_w,
                                 int new_h, int dx, int dy, int flip, void* stream) {
  return disyolo_aug_place_hw(src, is_mask, image_h, image_w, dst, size, size, new_w, new_h, dx, dy, flip, stream);
}

extern "C" int disyolo_aug_place_hw(const uint8_t* src, int is_mask, int image_h, int image_w, uint8_t* dst, int net_h, int net_w,
                                    int new_w, int new_h, int dx, int dy, int flip, void* stream) {
  DY_REQUIRE(src && dst && image_h > 0 && image_w > 0 && net_h > 0 && net_w > 0 && new_w > 0 && new_h > 0 && flip >= 1 && flip <= 3,
             "aug_place: bad args");
  DY_RECORD_OR_RUN([=](void* s) {
    return disyolo_aug_place_hw(src, is_mask, image_h, image_w, dst, net_h, net_w, new_w, new_h, dx, dy, flip, s);
  });
  const int g = grid_for((int64_t)net_h * net_w);
  if (is_mask)
    hipLaunchKernelGGL(place_mask_kernel, dim3(g), dim3(256), 0, (hipStream_t)stream, src, image_h, image_w, dst, net_h, net_w, new_w, new_h, dx, dy, flip);
  else
    hipLaunchKernelGGL(place_image_kernel, dim3(g), dim3(256), 0, (hipStream_t)stream, src, image_h, image_w, dst, net_h, net_w, new_w, new_h, dx, dy, flip);
  DY_CHECK_LAUNCH();
  return DISYOLO_OK;
}

extern "C" int disyolo_aug_place_batch(const disyolo_place_job* jobs, int njobs, int size, void* stream) {
  return disyolo_aug_place_batch_hw(jobs, njobs, size, size, stream);
}

extern "C" int disyolo_aug_place_batch_hw(const disyolo_place_job* jobs, int njobs, int net_h, int net_w, void* stream) {
  DY_REQUIRE(jobs && njobs > 0 && njobs <= 65535 && net_h > 0 && net_w > 0, "aug_place_batch: bad args");
  DY_RECORD_OR_RUN([=](void* s) { return disyolo_aug_place_batch_hw(jobs, njobs, net_h, net_w, s); });
  int gx = grid_for((int64_t)net_h * net_w);
  if (gx > 512) gx = 512;     // (grid-stride: the jobs of a batch fill the chip between them)
  hipLaunchKernelGGL(place_batch_kernel, dim3(gx, njobs), dim3(256), 0, (hipStream_t)stream, jobs, net_h, net_w);
  DY_CHECK_LAUNCH();
  return DISYOLO_OK;
}

extern "C" int disyolo_aug_salt_pepper(uint8_t* image, int size, const int32_t* rows, const int32_t* cols, int nsalt, int npepper,
                                       void* stream) {
  return disyolo_aug_salt_pepper_hw(image, size, size, rows, cols, nsalt, npepper, stream);
}

extern "C" int disyolo_aug_salt_pepper_hw(uint8_t* image, int net_h, int net_w, const int32_t* rows, const int32_t* cols, int nsalt,
                                          int npepper, void* stream) {
  DY_REQUIRE(image && rows && cols && net_h > 0 && net_w > 0 && nsalt >= 0 && npepper >= 0, "aug_salt_pepper: bad args");
  DY_RECORD_OR_RUN([=](void* s) { return disyolo_aug_salt_pepper_hw(image, net_h, net_w, rows, cols, nsalt, npepper, s); });
  const int n = nsalt + npepper;
  if (n == 0) return DISYOLO_OK;
  // two launches keep the reference's order: all salt writes, then all pepper writes
  if (nsalt) hipLaunchKernelGGL(salt_pepper_kernel, dim3((nsalt + 255) / 256), dim3(256), 0, (hipStream_t)stream, image, net_h, net_w, rows, cols, nsalt, 0);
  if (npepper) hipLaunchKernelGGL(salt_pepper_kernel, dim3((npepper + 255) / 256), dim3(256), 0, (hipStream_t)stream, image, net_h, net_w, rows + nsalt, cols + nsalt, 0, npepper);
  DY_CHECK_LAUNCH();
  return DISYOLO_OK;
}

extern "C" int disyolo_aug_change_light(uint8_t* image, int size, double coeff, void* stream) {
  return disyolo_aug_change_light_hw(image, size, size, coeff, stream);
}

extern "C" int disyolo_aug_change_light_hw(uint8_t* image, int net_h, int net_w, double coeff, void* stream) {
  DY_REQUIRE(image && net_h > 0 && net_w > 0 && coeff >= 0.0, "aug_change_light: bad args");
  DY_RECORD_OR_RUN([=](void* s) { return disyolo_aug_change_light_hw(image, net_h, net_w, coeff, s); });
  hipLaunchKernelGGL(change_light_kernel, dim3(grid_for((int64_t)net_h * net_w)), dim3(256), 0, (hipStream_t)stream, image, (int64_t)net_h * net_w, coeff);
  DY_CHECK_LAUNCH();
  return DISYOLO_OK;
}

extern "C" int disyolo_aug_motion_blur3(const uint8_t* src, uint8_t* dst, int size, int angle, int line_type, void* stream) {
  return disyolo_aug_motion_blur3_hw(src, dst, size, size, angle, line_type, stream);
}

extern "C" int disyolo_aug_motion_blur3_hw(const uint8_t* src, uint8_t* dst, int net_h, int net_w, int angle, int line_type,
                                           void* stream) {
  DY_REQUIRE(src && dst && src != dst && net_h > 0 && net_w > 0 && (angle == 0 || angle == 45 || angle == 90 || angle == 135) && line_type >= 0 && line_type <= 2,
             "aug_motion_blur3: bad args (angle 0/45/90/135, line_type 0 full / 1 right / 2 left)");
  DY_RECORD_OR_RUN([=](void* s) { return disyolo_aug_motion_blur3_hw(src, dst, net_h, net_w, angle, line_type, s); });
  // the "right" end of the 3x3 line in kernel coordinates (row down): pyblur's LineDictionary anchors
  // {0: [1,0,1,2], 45: [2,0,0,2], 90: [0,1,2,1], 135: [0,0,2,2]} = (row0, col0, row1, col1); 'right' keeps the SECOND
  // anchor (the first is replaced by the centre), 'left' the first: 0: +x, 45: up-right, 90: DOWN, 135: DOWN-right.
  // (Restated from pyblur 0.2.x, which is not installable here: unpinned.  pyblur also mutates the shared anchor list in
  // place, so after one 'right' and one 'left' call an angle degenerates to the identity for the rest of the process: not
  // reproduced.)
  const int dxA = angle == 0 ? 1 : (angle == 45 ? 1 : (angle == 90 ? 0 : 1));
  const int dyA = angle == 0 ? 0 : (angle == 45 ? -1 : 1);
  const int use_a = line_type != 2, use_b = line_type != 1;
  // a convolution flips the kernel: the tap at kernel offset (+dy,+dx) reads the pixel at (-dy,-dx)
  hipLaunchKernelGGL(motion_blur3_kernel, dim3(grid_for((int64_t)net_h * net_w)), dim3(256), 0, (hipStream_t)stream, src, dst, net_h,
                     net_w, -dyA, -dxA, use_a, use_b);
  DY_CHECK_LAUNCH();
  return DISYOLO_OK;
}

extern "C" size_t disyolo_window_job_size(void) { return sizeof(disyolo_window_job); }

extern "C" int disyolo_window_visible(const disyolo_window_job* jobs, int njobs, int net_h, int net_w, int32_t* vis, void* stream) {
  DY_REQUIRE(njobs >= 0 && njobs <= 65535 && net_h > 0 && net_w > 0, "window_visible: bad args (0 <= njobs <= 65535, net_h, net_w > 0)");
  DY_REQUIRE(njobs == 0 || (jobs && vis), "window_visible: null jobs / vis");
  DY_RECORD_OR_RUN([=](void* s) { return disyolo_window_visible(jobs, njobs, net_h, net_w, vis, s); });
  if (njobs == 0) return DISYOLO_OK;
  const int gj = (njobs + 255) / 256;
  hipLaunchKernelGGL(window_vis_init_kernel, dim3(gj), dim3(256), 0, (hipStream_t)stream, vis, njobs);
  hipLaunchKernelGGL(window_visible_kernel, dim3((net_h + WIN_ROWS - 1) / WIN_ROWS, njobs), dim3(256), 0, (hipStream_t)stream, jobs,
                     net_h, net_w, vis);
  hipLaunchKernelGGL(window_vis_finish_kernel, dim3(gj), dim3(256), 0, (hipStream_t)stream, vis, njobs);
  DY_CHECK_LAUNCH();
  return DISYOLO_OK;
}

extern "C" int disyolo_window_targets(const disyolo_window_job* jobs, int njobs, const int32_t* vis, const float* anchors, int B, int G,
                                      int C, int net_h, int net_w, int min_visible, float* true_boxes, float* yolo3, float* yolo2,
                                      float* yolo1, int32_t* rows, void* stream) {
  DY_REQUIRE(njobs >= 0 && njobs <= 65535 && B > 0, "window_targets: bad args (0 <= njobs <= 65535, B > 0)");
  DY_REQUIRE(G >= 1 && G <= DISYOLO_MAX_BOXES, "window_targets: G = %d, need 1 .. %d", G, DISYOLO_MAX_BOXES);
  DY_REQUIRE(C >= 1 && C <= 80, "window_targets: C = %d, need 1 .. 80", C);
  DY_REQUIRE(net_h > 0 && net_w > 0 && net_h % 32 == 0 && net_w % 32 == 0,
             "window_targets: the net's sides must be positive multiples of 32 (got %d x %d)", net_h, net_w);
  DY_REQUIRE(min_visible >= 1, "window_targets: min_visible = %d, need >= 1", min_visible);
  DY_REQUIRE(anchors && true_boxes && yolo3 && yolo2 && yolo1, "window_targets: null anchors / outputs");
  DY_REQUIRE(njobs == 0 || (jobs && vis && rows), "window_targets: null jobs / vis / rows");
  DY_RECORD_OR_RUN([=](void* s) {
    return disyolo_window_targets(jobs, njobs, vis, anchors, B, G, C, net_h, net_w, min_visible, true_boxes, yolo3, yolo2, yolo1, rows, s);
  });
  WinClear c;
  float* out[4] = {true_boxes, yolo3, yolo2, yolo1};
  int64_t biggest = 0;
  for (int k = 0; k < 4; ++k) {
    const int d = 4 << k;                                        // (k = 1, 2, 3: the grids at net / 8, 16, 32)
    c.p[k] = reinterpret_cast<unsigned*>(out[k]);
    c.n[k] = k == 0 ? (int64_t)B * G * 5 : (int64_t)B * (net_h / d) * (net_w / d) * 3 * (5 + C);
    if (c.n[k] > biggest) biggest = c.n[k];
  }
  c.p[4] = reinterpret_cast<unsigned*>(rows);
  c.n[4] = njobs;
  hipLaunchKernelGGL(window_clear_kernel, dim3(grid_for(biggest / 4 + 8), 5), dim3(256), 0, (hipStream_t)stream, c);
  if (njobs > 0)
    hipLaunchKernelGGL(window_targets_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, jobs, njobs, (const int*)vis,
                       anchors, B, G, C, net_h, net_w, min_visible, true_boxes, yolo3, yolo2, yolo1, (int*)rows);
  DY_CHECK_LAUNCH();
  return DISYOLO_OK;
}

extern "C" int disyolo_window_place_masks(const disyolo_window_job* jobs, int njobs, const int32_t* rows, uint8_t* true_masks, int G,
                                          int net_h, int net_w, void* stream) {
  DY_REQUIRE(njobs >= 0 && njobs <= 65535 && net_h > 0 && net_w > 0, "window_place_masks: bad args (0 <= njobs <= 65535, net_h, net_w > 0)");
  DY_REQUIRE(G >= 1 && G <= DISYOLO_MAX_BOXES, "window_place_masks: G = %d, need 1 .. %d", G, DISYOLO_MAX_BOXES);
  DY_REQUIRE(njobs == 0 || (jobs && rows && true_masks), "window_place_masks: null jobs / rows / true_masks");
  DY_RECORD_OR_RUN([=](void* s) { return disyolo_window_place_masks(jobs, njobs, rows, true_masks, G, net_h, net_w, s); });
  if (njobs == 0) return DISYOLO_OK;
  hipLaunchKernelGGL(window_place_masks_kernel, dim3((net_h + WIN_ROWS - 1) / WIN_ROWS, njobs), dim3(256), 0, (hipStream_t)stream, jobs,
                     (const int*)rows, true_masks, G, net_h, net_w);
  DY_CHECK_LAUNCH();
  return DISYOLO_OK;
}

extern "C" int disyolo_aug_to_float(const uint8_t* image, float* out, int64_t n, void* stream) {
  DY_REQUIRE(image && out && n > 0, "aug_to_float: bad args");
  DY_RECORD_OR_RUN([=](void* s) { return disyolo_aug_to_float(image, out, n, s); });
  hipLaunchKernelGGL(to_float_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, image, out, n);
  DY_CHECK_LAUNCH();
  return DISYOLO_OK;
}

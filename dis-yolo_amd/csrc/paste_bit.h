// THE tap arithmetic and the > 0.5 decision of the mask paste (calculate_test_map.py:237-262), shared by every kernel that
// pastes -- mask_paste_kernel and mask_paste_iou_batch_kernel of detect.hip, tile_paste_bits_kernel of tiles.hip -- so they
// cannot drift.  cv2.resize(INTER_LINEAR) semantics: pixel centres aligned, border taps clamped with weight 0, horizontal
// then vertical pass, every product and sum rounded to f32 separately.  A file that includes this is compiled with
// -ffp-contract=off (csrc/Makefile).
#pragma once
#include <hip/hip_runtime.h>

// the bit of pixel (y, x) for one detection, m = its mask (rows of `size` floats: the map's width), r = its rect row
// (cy1,cx1,cy2,cx2, y1,x1,y2,x2)
static __device__ __forceinline__ unsigned char paste_bit(const float* m, int size, const int* r, int y, int x) {
  const int cy1 = r[0], cx1 = r[1], cy2 = r[2], cx2 = r[3], y1 = r[4], x1 = r[5], y2 = r[6], x2 = r[7];
  const int sh = cy2 - cy1, sw = cx2 - cx1, dh = y2 - y1, dw = x2 - x1;
  if (!(sh > 0 && sw > 0 && dh > 0 && dw > 0 && y >= y1 && y < y2 && x >= x1 && x < x2)) return 0;
  float fx = (float)(((double)(x - x1) + 0.5) * ((double)sw / (double)dw) - 0.5);
  float fy = (float)(((double)(y - y1) + 0.5) * ((double)sh / (double)dh) - 0.5);
  int sx = (int)floorf(fx), sy = (int)floorf(fy);
  float ax = __fsub_rn(fx, (float)sx), ay = __fsub_rn(fy, (float)sy);
  if (sx < 0) { ax = 0.f; sx = 0; }
  if (sx >= sw - 1) { ax = 0.f; sx = sw - 1; }
  if (sy < 0) { ay = 0.f; sy = 0; }
  if (sy >= sh - 1) { ay = 0.f; sy = sh - 1; }
  const int sx1 = min(sx + 1, sw - 1), sy1 = min(sy + 1, sh - 1);
  const float* row0 = m + (size_t)(cy1 + sy) * size + cx1;
  const float* row1 = m + (size_t)(cy1 + sy1) * size + cx1;
  const float bx = __fsub_rn(1.f, ax), by = __fsub_rn(1.f, ay);
  const float h0 = __fadd_rn(__fmul_rn(row0[sx], bx), __fmul_rn(row0[sx1], ax));
  const float h1 = __fadd_rn(__fmul_rn(row1[sx], bx), __fmul_rn(row1[sx1], ax));
  const float v = __fadd_rn(__fmul_rn(h0, by), __fmul_rn(h1, ay));
  return v > 0.5f ? 1 : 0;
}

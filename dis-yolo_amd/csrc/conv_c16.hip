// Convolutions whose sources have 16 * odd channels (C0 or C1 = 16, 48, ...): the m = 1 mask subnet's conv83 (act1 +
// upsampled 16-channel act82), conv84 (3x3 over 16 channels) and the data gradients whose source is a 16-channel layer
// gradient (conv82, conv83).  The implicit-GEMM kernels gather K in slices of 32 channels; these shapes take this direct
// kernel instead, reached through disyolo_conv2d_fwd with the same descriptor semantics: optional fused 2x nearest
// upsample + concat of x1, scale / shift / LEAKY, residual after the activation, bf16 or f32 output, STATS (per-channel
// sum / sum of squares of the raw f32 accumulators, one row per 64-pixel block).  No in-launch batch norm, in_div 1 only.
//
// One block = 64 output pixels x every output channel; lane = pixel, wave w = output channels 16 w ... in steps of 64.
// The inputs are read as 8-channel (16-byte) vectors, the weights are wave-uniform loads.  f32 accumulation in the order
// tap, channel -- deterministic.
#include "common.h"
#include "runtime.h"

namespace {

constexpr int C16_BM = 64;
constexpr int C16_NJ = 16;      // output channels per lane and pass

struct C16Params {
  const bf16* x0;
  const bf16* x1;
  const bf16* w;
  const float* scale;
  const float* shift;
  const bf16* residual;
  void* y;
  float* stats;
  int B, H, W, C0, C1, Cin, Ho, Wo, Cout, ks, stride, pad_t, pad_l, flags, M, K;
  float alpha;
};

__global__ __launch_bounds__(256) void conv_c16_kernel(C16Params p) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int m = blockIdx.x * C16_BM + lane;
  const bool valid = m < p.M;
  int b = 0, yo = 0, xo = 0;
  if (valid) {
    b = m / (p.Ho * p.Wo);
    const int r = m - b * p.Ho * p.Wo;
    yo = r / p.Wo;
    xo = r - yo * p.Wo;
  }
  const int H1 = p.H >> 1, W1 = p.W >> 1;
  for (int n0 = wave * C16_NJ; n0 < p.Cout; n0 += 4 * C16_NJ) {
    float acc[C16_NJ];
#pragma unroll
    for (int j = 0; j < C16_NJ; ++j) acc[j] = 0.f;
    if (valid) {
      for (int kh = 0; kh < p.ks; ++kh) {
        const int yi = yo * p.stride - p.pad_t + kh;
        if (yi < 0 || yi >= p.H) continue;
        for (int kw = 0; kw < p.ks; ++kw) {
          const int xi = xo * p.stride - p.pad_l + kw;
          if (xi < 0 || xi >= p.W) continue;
          const int kbase = (kh * p.ks + kw) * p.Cin;
          for (int ci = 0; ci < p.Cin; ci += 8) {
            const uint4* src = ci < p.C0
                ? reinterpret_cast<const uint4*>(p.x0 + (((size_t)b * p.H + yi) * p.W + xi) * p.C0 + ci)
                : reinterpret_cast<const uint4*>(p.x1 + (((size_t)b * H1 + (yi >> 1)) * W1 + (xi >> 1)) * p.C1 + (ci - p.C0));
            float xf[8];
            unpack8(*src, xf);
#pragma unroll
            for (int j = 0; j < C16_NJ; ++j) {
              const int n = min(n0 + j, p.Cout - 1);      // (rows past Cout are computed on a valid row and dropped)
              float wf[8];
              unpack8(*reinterpret_cast<const uint4*>(p.w + (size_t)n * p.K + kbase + ci), wf);
#pragma unroll
              for (int t = 0; t < 8; ++t) acc[j] = fmaf(xf[t], wf[t], acc[j]);
            }
          }
        }
      }
    }
    if (p.flags & DISYOLO_CONV_STATS) {
      // per-channel partial sums of this block's 64 pixels (invalid pixels hold zeros): fixed shuffle tree
#pragma unroll
      for (int j = 0; j < C16_NJ; ++j) {
        float s = acc[j], s2 = acc[j] * acc[j];
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
          s += __shfl_xor(s, o, 64);
          s2 += __shfl_xor(s2, o, 64);
        }
        const int n = n0 + j;
        if (lane == 0 && n < p.Cout) {
          p.stats[((size_t)blockIdx.x * p.Cout + n) * 2 + 0] = s;
          p.stats[((size_t)blockIdx.x * p.Cout + n) * 2 + 1] = s2;
        }
      }
    }
    if (!valid) continue;
#pragma unroll
    for (int j = 0; j < C16_NJ; ++j) {
      const int n = n0 + j;
      if (n >= p.Cout) break;
      float v = acc[j];
      if (p.scale) v *= p.scale[n];
      if (p.shift) v += p.shift[n];
      if (p.flags & DISYOLO_CONV_LEAKY) v = fmaxf(p.alpha * v, v);
      const size_t o = (size_t)m * p.Cout + n;
      if (p.residual) v += bf2f(p.residual[o]);
      if (p.flags & DISYOLO_CONV_OUT_F32)
        reinterpret_cast<float*>(p.y)[o] = v;
      else
        reinterpret_cast<bf16*>(p.y)[o] = (bf16)v;
    }
  }
}

}  // namespace

// 1 when the descriptor has a source of 16 * odd channels (this kernel's shapes)
int conv_c16_shape(const disyolo_conv_desc* d) { return (d->C0 % 32) != 0 || (d->C1 % 32) != 0; }

int conv_c16_stats_rows(const disyolo_conv_desc* d) {
  return (int)(((int64_t)d->B * d->Ho * d->Wo + C16_BM - 1) / C16_BM);
}

// called by disyolo_conv2d_fwd after validate(): C0, C1 multiples of 16, ksize 1 / 3, the sizes checked
int conv_c16_launch(const disyolo_conv_desc* d, void* stream) {
  DY_REQUIRE(d->in_div == 1, "conv: 16-channel sources need in_div 1 (got %d)", d->in_div);
  DY_REQUIRE(!(d->flags & (DISYOLO_CONV_BN_BWD_STATS | DISYOLO_CONV_BN_FUSED | DISYOLO_CONV_BN_BWD_FUSED)),
             "conv: 16-channel sources run a kernel without the in-launch batch-norm epilogues");
  DY_REQUIRE(d->Cout % 8 == 0 || (d->flags & DISYOLO_CONV_OUT_F32), "conv: 16-channel sources need Cout %% 8 == 0 (bf16 y)");
  C16Params p;
  p.x0 = (const bf16*)d->x0;
  p.x1 = (const bf16*)d->x1;
  p.w = (const bf16*)d->w;
  p.scale = d->scale;
  p.shift = d->shift;
  p.residual = (const bf16*)d->residual;
  p.y = d->y;
  p.stats = d->stats;
  p.B = d->B; p.H = d->H; p.W = d->W; p.C0 = d->C0; p.C1 = d->C1; p.Cin = d->C0 + d->C1;
  p.Ho = d->Ho; p.Wo = d->Wo; p.Cout = d->Cout;
  p.ks = d->ksize; p.stride = d->stride; p.pad_t = d->pad_t; p.pad_l = d->pad_l;
  p.flags = d->flags; p.alpha = d->alpha;
  p.M = d->B * d->Ho * d->Wo;
  p.K = d->ksize * d->ksize * p.Cin;
  hipLaunchKernelGGL(conv_c16_kernel, dim3(conv_c16_stats_rows(d)), dim3(256), 0, (hipStream_t)stream, p);
  DY_CHECK_LAUNCH();
  return DISYOLO_OK;
}

// Weight gradient of the implicit-GEMM convolution on gfx950.
//
//   dw[(kh,kw,ci)][co] = sum_m xcol[m][(kh,kw,ci)] * dy[m][co]       (f32, HWIO order)
//
// i.e. TF autodiff of tf.nn.conv2d wrt its filter (train_yolo3_mask.py:55 minimize()).
// GEMM view: rows = K index, cols = Cout, reduction over the M = B*Ho*Wo output pixels.
// Both operands live in memory with the *reduction* index (pixel) as the slow dimension
// (NHWC), so the LDS tiles are [pixel][k] / [pixel][co] images read back with the gfx950
// transposing load ds_read_b64_tr_b16 straight into v_mfma_f32_16x16x32_bf16 fragments.
// The pixel range is split over the grid (K tile fastest, XCD-aware order); each split writes an f32 slab and a second
// kernel adds the slabs in a fixed order (deterministic, no float atomics).
#include "common.h"
#include "runtime.h"

namespace {

struct WgradParams {
  const bf16* x0;
  const bf16* x1;
  const bf16* dy;
  float* out;  // slabs [splits][K][Cout]
  int B, H, W, C0, C1, Cin;
  int Ho, Wo, Cout, ldy;
  int ks, stride, pad_t, pad_l;
  int M, K;
  int steps_per_split, steps;
  int tilesK, tilesN;
  unsigned bytes0, bytes1, bytesy;
};

typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
typedef int i32x4 __attribute__((ext_vector_type(4)));
constexpr unsigned OOB = 0x80000000u;

// 32-byte-unit swizzle inside one LDS row of `units` units: the two 16-lane groups of a
// 32-lane half of ds_read_b64_tr_b16 (rows 8g..8g+3 and 8g+8..) land on disjoint banks
__device__ __forceinline__ int swz_u(int row, int u, int units) {
  const int h = (row & 3) | (((row >> 3) & 1) << 2);
  return u ^ (h & (units - 1));
}
// LDS-DMA through a buffer descriptor: out-of-range lanes write zeros (see conv_igemm.hip)
__device__ __forceinline__ void dma16(unsigned voff, i32x4 srd, unsigned lds_dst) {
  asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tbuffer_load_dwordx4 %0, %1, 0 offen lds"
               :
               : "v"(voff), "s"(srd), "s"(lds_dst)
               : "memory");
}
__device__ __forceinline__ i32x4 make_srd(const void* base, unsigned bytes) {
  i32x4 r;
  r[0] = __builtin_amdgcn_readfirstlane((int)(unsigned)(size_t)base);
  r[1] = __builtin_amdgcn_readfirstlane((int)((size_t)base >> 32)) & 0xffff;
  r[2] = __builtin_amdgcn_readfirstlane((int)bytes);
  r[3] = 0x00020000;
  return r;
}
__device__ uint4 g_zero16;
__device__ __forceinline__ void dma16_flat(const void* gsrc, unsigned lds_dst) {
  asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" : : "v"(gsrc), "s"(lds_dst) : "memory");
}
template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// Block = 128 K-rows x BN channels, 4 waves (2x2).  Per reduction step the block stages a
// [32 pixels][128 k] image of the gathered input and a [32 pixels][BN] image of dy with LDS-DMA
// (ST stages, counted vmcnt, one barrier per step) and multiplies them with transposed LDS reads.
template <int BN, int ST>
__global__ __launch_bounds__(256) void conv_wgrad_kernel(WgradParams p) {
  constexpr int BM = 128;
  constexpr int WM = 2, WN = 2, NW = 4;
  constexpr int WTM = BM / WM, WTN = BN / WN;
  constexpr int MI = WTM / 16, NI = WTN / 16;
  constexpr int XCH = BM / 8, YCH = BN / 8;  // 16-byte chunks per pixel row
  constexpr int XP = BM * 2, YP = BN * 2;    // row pitch in bytes
  constexpr int SLAB = 1024 * NW;
  constexpr int X_BYTES = 32 * XP;                                      // 8 KiB
  constexpr int Y_BYTES = (32 * YP + SLAB - 1) / SLAB * SLAB;
  constexpr int XI = X_BYTES / SLAB, YI = Y_BYTES / SLAB;
  constexpr int LPT = XI + YI;
  constexpr int STB = X_BYTES + Y_BYTES;
  constexpr int PRE = ST - 1;
  static_assert(WTN % 16 == 0, "BN must be a multiple of 32");

  extern __shared__ __attribute__((aligned(16))) char smem[];
  const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smem;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave % WN;
  // XCD-aware block order (blocks b and b+8 share an XCD and its L2): every XCD gets a contiguous
  // run of work items with the K tile fastest, so the blocks that read the same dy tile (same
  // channel tile and pixel split, all K tiles) sit on one L2 instead of filling all eight
  int lin;
  {
    const int nblk = gridDim.x, bid = blockIdx.x;
    const int q = nblk >> 3, r = nblk & 7, xcd = bid & 7, loc = bid >> 3;
    lin = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + loc;
  }
  const int bkt = lin % p.tilesK, brest = lin / p.tilesK;
  const int bnt = brest % p.tilesN, bsplit = brest / p.tilesN;
  const int kt0 = bkt * BM;  // first K index of this block
  const int n0 = bnt * BN;
  const int step0 = bsplit * p.steps_per_split;
  int step1 = step0 + p.steps_per_split;
  if (step1 > p.steps) step1 = p.steps;
  const int nsteps = step1 - step0;

  const i32x4 srd0 = make_srd(p.x0, p.bytes0);
  const i32x4 srd1 = make_srd(p.x1 ? (const void*)p.x1 : (const void*)p.x0, p.x1 ? p.bytes1 : 0u);
  const i32x4 srdy = make_srd(p.dy, p.bytesy);

  // ---- X gather: DMA j of this wave fills rows (j*NW+wave)*4 .. +3 of the step's image; the
  //      lane's (tap, channel) is fixed for the block, its pixel advances by 32 per step
  int x_kh[XI], x_kw[XI], x_ci[XI], x_b[XI], x_yo[XI], x_xo[XI];
  bool x_kok[XI], x_second[XI];
#pragma unroll
  for (int j = 0; j < XI; ++j) {
    const int chunk = (j * NW + wave) * 64 + lane;
    const int row = chunk / XCH, pc = chunk % XCH;
    const int lc = swz_u(row, pc >> 1, XCH / 2) * 2 + (pc & 1);
    const int kk = kt0 + lc * 8;
    x_kok[j] = kk < p.K;
    const int kq = x_kok[j] ? kk : 0;
    const int tap = kq / p.Cin;
    int ci = kq - tap * p.Cin;
    x_second[j] = ci >= p.C0;
    x_ci[j] = x_second[j] ? ci - p.C0 : ci;
    x_kh[j] = tap / p.ks;
    x_kw[j] = tap - x_kh[j] * p.ks;
    const int m = step0 * 32 + row;
    const int hw = p.Ho * p.Wo;
    const int b = m / hw;
    const int rem = m - b * hw;
    x_b[j] = b;
    x_yo[j] = rem / p.Wo;
    x_xo[j] = rem - x_yo[j] * p.Wo;
  }
  // ---- dy: plain rows of ldy channels
  unsigned y_off[YI];
  int y_m[YI];
  bool y_nok[YI];
#pragma unroll
  for (int j = 0; j < YI; ++j) {
    const int chunk = (j * NW + wave) * 64 + lane;
    const int row = chunk / YCH, pc = chunk % YCH;
    const int lc = swz_u(row, pc >> 1, YCH / 2) * 2 + (pc & 1);
    const int n = n0 + lc * 8;
    y_nok[j] = (row < 32) && (n < p.ldy);
    y_m[j] = step0 * 32 + row;
    y_off[j] = ((unsigned)y_m[j] * (unsigned)p.ldy + (unsigned)n) * 2u;
  }

  const bool mixed = (p.C1 > 0) && ((p.C0 & (BM - 1)) != 0);
  const bool blk_second = (p.C1 > 0) && (kt0 >= p.C0);
  auto issue_tile = [&](int stage) {
    const unsigned sbase = lds0 + stage * STB + wave * 1024;
#pragma unroll
    for (int j = 0; j < XI; ++j) {
      const int iy = x_yo[j] * p.stride - p.pad_t + x_kh[j];
      const int ix = x_xo[j] * p.stride - p.pad_l + x_kw[j];
      const bool ok = x_kok[j] && (x_b[j] < p.B) && ((unsigned)iy < (unsigned)p.H) && ((unsigned)ix < (unsigned)p.W);
      unsigned off;
      if (!x_second[j]) {
        off = (unsigned)(((x_b[j] * p.H + iy) * p.W + ix) * p.C0 + x_ci[j]) * 2u;
      } else {
        const int H1 = p.H >> 1, W1 = p.W >> 1;
        off = (unsigned)(((x_b[j] * H1 + (iy >> 1)) * W1 + (ix >> 1)) * p.C1 + x_ci[j]) * 2u;
      }
      if (!mixed) {
        // the block's 128 K rows come from one source: one descriptor per block
        if (blk_second) dma16(ok ? off : OOB, srd1, sbase + j * SLAB);
        else dma16(ok ? off : OOB, srd0, sbase + j * SLAB);
      } else {
        // concat boundary inside the block's K range (C0 not a multiple of 128): per-lane
        // flat addresses, zeros from a 16-byte zero page
        const void* src = ok ? (const void*)((const char*)(x_second[j] ? p.x1 : p.x0) + off) : (const void*)&g_zero16;
        dma16_flat(src, sbase + j * SLAB);
      }
      // advance this lane's pixel by 32
      x_xo[j] += 32;
      while (x_xo[j] >= p.Wo) {
        x_xo[j] -= p.Wo;
        if (++x_yo[j] == p.Ho) {
          x_yo[j] = 0;
          ++x_b[j];
        }
      }
    }
#pragma unroll
    for (int j = 0; j < YI; ++j) {
      dma16((y_nok[j] && y_m[j] < p.M) ? y_off[j] : OOB, srdy, sbase + X_BYTES + j * SLAB);
      y_m[j] += 32;
      y_off[j] += 32u * (unsigned)p.ldy * 2u;
    }
  };

  f32x4 acc[MI][NI];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

#pragma unroll
  for (int s = 0; s < PRE; ++s)
    if (s < nsteps) issue_tile(s);

  // transposed-read addressing (cdna guide T10): inside a 16-lane group, lane 4q+p supplies
  // the address of row q, columns 4p..4p+3 of a 4x16 block and receives column (lane&15).
  const int g = lane >> 4, li = lane & 15, q = li >> 2, pc = li & 3;
  for (int st = 0; st < nsteps; ++st) {
    if (PRE >= 1 && st + PRE - 1 < nsteps)
      wait_vmcnt<LPT*(PRE >= 1 ? PRE - 1 : 0)>();
    else
      wait_vmcnt<0>();
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (st + PRE < nsteps) issue_tile((st + PRE) % ST);
    const char* sX = smem + (st % ST) * STB;
    const char* sY = sX + X_BYTES;
    bf16x8 af[MI], bfr[NI];
    typedef short s16x8 __attribute__((ext_vector_type(8)));
    const int r0 = 8 * g + q, r1 = r0 + 4;
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      const int u = (wm * WTM + i * 16) >> 4;
      const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
          (lds_s16x4*)(sX + r0 * XP + swz_u(r0, u, XCH / 2) * 32 + pc * 8));
      const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
          (lds_s16x4*)(sX + r1 * XP + swz_u(r1, u, XCH / 2) * 32 + pc * 8));
      const s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
      af[i] = __builtin_bit_cast(bf16x8, v);
    }
#pragma unroll
    for (int j = 0; j < NI; ++j) {
      const int u = (wn * WTN + j * 16) >> 4;
      const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
          (lds_s16x4*)(sY + r0 * YP + swz_u(r0, u, YCH / 2) * 32 + pc * 8));
      const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
          (lds_s16x4*)(sY + r1 * YP + swz_u(r1, u, YCH / 2) * 32 + pc * 8));
      const s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
      bfr[j] = __builtin_bit_cast(bf16x8, v);
    }
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int j = 0; j < NI; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
  }

  // D: row (K index) = 4*(lane>>4) + r, col (co) = lane&15.  Each wave stages its WTM x WTN f32
  // tile in LDS (row pitch + 16 B) and writes it out 16 B per lane, WTN*4 contiguous bytes per K
  // row, instead of 64-byte pieces of four rows per store.
  float* slab = p.out + (size_t)bsplit * p.K * p.Cout;
  __syncthreads();   // every wave is done with the operand stages
  constexpr int ROWP = WTN * 4 + 16;
  constexpr int HALF = MI / 2 * 16;                     // rows staged per round (two rounds)
  if constexpr (NW * HALF * ROWP <= ST * STB) {
    if ((p.Cout & 3) == 0) {
      char* sw = smem + wave * (HALF * ROWP);
      constexpr int CPR4 = WTN / 4, CH = HALF * CPR4;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
#pragma unroll
        for (int i2 = 0; i2 < MI / 2; ++i2)
#pragma unroll
          for (int j = 0; j < NI; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r)
              *reinterpret_cast<float*>(sw + (i2 * 16 + g * 4 + r) * ROWP + (j * 16 + li) * 4) = acc[h * (MI / 2) + i2][j][r];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
        for (int it = 0; it < (CH + 63) / 64; ++it) {
          const int idx = it * 64 + lane;
          const int row = idx / CPR4, ch = idx % CPR4;
          const int kk = kt0 + wm * WTM + h * HALF + row, n = n0 + wn * WTN + ch * 4;
          if (idx < CH && kk < p.K && n < p.Cout)
            *reinterpret_cast<float4*>(slab + (size_t)kk * p.Cout + n) =
                *reinterpret_cast<const float4*>(sw + row * ROWP + ch * 16);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
      }
      return;
    }
  }
#pragma unroll
  for (int i = 0; i < MI; ++i) {
#pragma unroll
    for (int j = 0; j < NI; ++j) {
      const int n = n0 + wn * WTN + j * 16 + li;
      if (n >= p.Cout) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int kk = kt0 + wm * WTM + i * 16 + g * 4 + r;
        if (kk < p.K) slab[(size_t)kk * p.Cout + n] = acc[i][j][r];
      }
    }
  }
}


// ---------------------------------------------------------------------------------------------
// 3x3 stride-1 weight gradient with all nine filter taps fed from ONE staged copy of the input.
//
// Pixels are numbered in a padded frame, Q = b*(H+1)*P + (y+1)*P + (x+1) with P = W+1: every image
// row is followed by one pad pixel (it is the right pad of that row and the left pad of the next),
// every image is preceded by one pad row (the bottom pad of the image before).  In that numbering
// the input pixel of tap (kh,kw) for output pixel Q is Q + (kh-1)*P + (kw-1) -- one uniform shift,
// pads included -- so
//     dw[kh][kw][ci][co] = sum_Q X''(Q + shift(kh,kw))[ci] * dY'(Q)[co]
// where X'' / dY' are the input / output-gradient in frame numbering, zero on pad pixels (those
// lanes of the LDS-DMA are out of range of the buffer descriptor: the hardware writes zeros).
//
// A block owns 32 input channels x CO_T output channels x 9 taps (accumulators: 9*32*CO_T f32 in
// registers, 144 or 72 per lane) and a range of 64-pixel chunks of Q.  Per chunk it stages 64 x 32
// input values ONCE into a ring of R chunks (the nine taps read it at nine row shifts) and 64 x CO_T
// gradient values into a 3-stage pipeline: 20 KiB staged per 4.7 MFLOP (236 FLOP/B; the im2col kernel
// above: 64).  Both images are [pixel][channel]; fragments come out of ds_read_b64_tr_b16.  The k
// order inside an MFMA is permuted (lane group g holds pixels 4g..4g+3 and 16+4g..16+4g+3) -- the
// same permutation for both operands, so the sum is unchanged -- which makes the second transposed
// read of a fragment the first one + 16 rows: one address computation per fragment half.
// XOR swizzles on 32-byte units (applied on the DMA source side and on the read) keep every
// transposed read conflict-free: input ring (64-byte rows) unit ^ ((row>>2)&1) at ANY row alignment,
// gradient stages unit ^ (row&7) (256-byte rows) resp. unit ^ ((row>>1)&3) (128-byte rows).
struct Wg3Params {
  const bf16* x;
  const bf16* dy;
  float* out;  // slabs [splits][9*Cin][Cout]
  int B, H, W, Cin, Cout, ldy;
  int Ho, Wo;               // output map (= H, W at stride 1; H/2, W/2 at stride 2)
  int P, Hp, frame, kbias;  // P = W+1, Hp = H+1, frame = Hp*P, kbias*frame >= the prologue's reach below Q = 0
  int a64, r64;             // 64 = a64*P + r64
  int chunks, chunks_per_split;
  int tilesCi, tilesCo, tiles;
  int leadA, leadB;
  unsigned bytesx, bytesy;
  int debug;  // ablation bits the kernel still tests; the host always passes 0 (1: no epilogue stores, 2: no main loop, 4: no DMA in the loop)
};

struct PixState {
  int b, yy, xx;
};
__device__ __forceinline__ void pix_init(PixState& s, int Q, const Wg3Params& p) {
  const int Qn = Q + p.kbias * p.frame;
  const int bb = Qn / p.frame;
  const int rem = Qn - bb * p.frame;
  s.b = bb - p.kbias;
  s.yy = rem / p.P;
  s.xx = rem - s.yy * p.P;
}
__device__ __forceinline__ void pix_advance64(PixState& s, const Wg3Params& p) {
  s.xx += p.r64;
  s.yy += p.a64;
  if (s.xx >= p.P) {
    s.xx -= p.P;
    ++s.yy;
  }
  while (s.yy >= p.Hp) {
    s.yy -= p.Hp;
    ++s.b;
  }
}
// element index of the real pixel behind a frame position, or -1 on a pad / outside the batch
__device__ __forceinline__ int pix_index(const PixState& s, const Wg3Params& p) {
  const bool ok = ((unsigned)s.b < (unsigned)p.B) && (s.yy >= 1) && (s.xx >= 1);
  return ok ? (s.b * p.H + s.yy - 1) * p.W + s.xx - 1 : -1;
}

// stride 2 (pad 0 before, 1 after: even H, W): the frame is the OUTPUT map with the pad column / row at the END of a row /
// image, P = Wo+1, Hp = Ho+1; a frame position is output pixel (yy, xx) and, in parity class (py, px) of the input,
// input pixel (2yy+py, 2xx+px)
__device__ __forceinline__ int pix_index_s2_in(const PixState& s, const Wg3Params& p) {     // class (0, 0)
  const bool ok = ((unsigned)s.b < (unsigned)p.B) && (s.yy < p.Ho) && (s.xx < p.Wo);
  return ok ? (s.b * p.H + 2 * s.yy) * p.W + 2 * s.xx : -1;
}
__device__ __forceinline__ int pix_index_s2_out(const PixState& s, const Wg3Params& p) {
  const bool ok = ((unsigned)s.b < (unsigned)p.B) && (s.yy < p.Ho) && (s.xx < p.Wo);
  return ok ? (s.b * p.Ho + s.yy) * p.Wo + s.xx : -1;
}

// LDS-DMA with an immediate byte offset added to the per-lane source offset (still range-checked).
// The hardware adds the instruction offset to the LDS address as well (LDS address = M0 base +
// instruction offset + 16 * lane), so it is taken off the base again.
template <int IMM>
__device__ __forceinline__ void dma16_imm(unsigned voff, i32x4 srd, unsigned lds_dst) {
  asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tbuffer_load_dwordx4 %0, %1, 0 offen offset:%3 lds"
               :
               : "v"(voff), "s"(srd), "s"(lds_dst - (unsigned)IMM), "n"(IMM)
               : "memory");
}

// NW = 4: one wave per SIMD, every wave all nine taps.  NW = 8: two waves per SIMD -- waves 0-3 take taps 0-4,
// waves 4-7 taps 5-8 of the same (input fragment, channel half): half the accumulators per wave, no reduction
// between the groups, and two instruction streams per SIMD to interleave (the one-wave loop is issue-bound).
//
// S2 = 1: the stride-2 layers (conv2 / 5 / 10 / 27 / 44).  Tap (kh, kw) reads input pixel (2yo+kh, 2xo+kw): ONE of the four
// parity classes of the input, (kh&1, kw&1), at a uniform shift of (kh>>1) rows + (kw>>1) pixels in the output-map frame
// -- so the input is staged as FOUR rings, one per class (every input pixel still crosses into LDS exactly once), and a tap
// is a (ring, row shift) pair: taps (0,0) (0,2) (2,0) (2,2) read class 0, (0,1) (2,1) class 1, (1,0) (1,2) class 2, (1,1) class 3.
template <int CO_T, int R, int ST, int NW, int S2 = 0>
__global__ __launch_bounds__(NW * 64) void conv_wgrad3x3_kernel(Wg3Params p) {
  constexpr int NJ = CO_T / 32;      // 16-channel gradient fragments per wave (the wave owns CO_T/2 channels)
  constexpr int YD = CO_T / 32;      // 32-channel sub-tiles of a gradient stage
  constexpr int YDW = YD * 4 / NW;   // gradient DMAs per wave per chunk
  constexpr int TPW = NW == 8 ? 5 : 9;   // taps per wave (the second group of 8 waves uses 4 of its 5 slots)
  constexpr int YST = YD * 4096;     // bytes per gradient stage: YD sub-tiles of [64 pixels][32 channels]
  constexpr int XRING = R * 4096;
  constexpr int XALLOC = XRING + 1024;   // + a copy of the ring's first 16 rows behind its end (see below)
  constexpr int NR = S2 ? 4 : 1;         // input rings
  constexpr int XTOT = NR * XALLOC;
  constexpr int PRE = ST - 1;
  constexpr int LPT0 = NR + YDW, LPT1 = YDW;   // DMAs per chunk of the waves that stage the input / that do not
  static_assert(!S2 || NW == 4, "stride 2: the four-wave form only");
  static_assert((R & (R - 1)) == 0 && ST >= 2, "ring");

  extern __shared__ __attribute__((aligned(16))) char smem[];
  const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smem;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wq = wave & 3, tg = wave >> 2;  // position in the 4-wave group, tap group
  const int u = wq & 1, ch = wq >> 1;       // input-channel fragment, output-channel half
  const int tap0 = tg * 5, ntaps = NW == 8 ? (tg ? 4 : 5) : 9;
  int lin;
  {
    const int nblk = gridDim.x, bid = blockIdx.x;
    const int q8 = nblk >> 3, r8 = nblk & 7, xcd = bid & 7, loc = bid >> 3;
    lin = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + loc;
  }
  const int tile = lin % p.tiles, bsplit = lin / p.tiles;
  const int ci0 = (tile % p.tilesCi) * 32, co0 = (tile / p.tilesCi) * CO_T;
  const int c0 = bsplit * p.chunks_per_split;
  int c1 = c0 + p.chunks_per_split;
  if (c1 > p.chunks) c1 = p.chunks;
  const int nsteps = c1 - c0;

  const i32x4 srdx = make_srd(p.x, p.bytesx);
  const i32x4 srdy = make_srd(p.dy, p.bytesy);

  // ---- DMA lanes.  Every image in LDS is [64 pixels][32 channels] (64-byte rows); one DMA of wave w
  // fills rows 16w..16w+15, lane -> row 16w + lane/4, 16-byte piece lane%4.  The gradient stage is
  // YD such images (channels 32j..32j+31): the lane's pixel is the same in all of them, so ONE pixel
  // walk serves the YD gradient DMAs (the sub-tile is the instruction's immediate offset) and one more
  // the input DMA.
  const int drow = wq * 16 + (lane >> 2), dpc = lane & 3;
  const int dlu = (dpc >> 1) ^ ((drow >> 2) & 1);
  const unsigned x_const = (unsigned)(ci0 + dlu * 16 + (dpc & 1) * 8) * 2u;
  const int y_n = co0 + (NW == 8 ? tg * 32 : 0) + dlu * 16 + (dpc & 1) * 8;   // 8 waves: group tg stages sub-tiles tg and tg + 2
  const unsigned y_const = (unsigned)y_n * 2u;
  PixState xs, ys;
  pix_init(xs, (c0 - p.leadB) * 64 + drow, p);
  pix_init(ys, c0 * 64 + drow, p);
  const unsigned xrow_bytes = (unsigned)p.Cin * 2u, yrow_bytes = (unsigned)p.ldy * 2u;
  auto issue_x = [&](int c) {   // stages chunk c of the input (this wave's quarter), advances the lane's pixel
    const unsigned slot = (unsigned)(c & (R - 1));
    if constexpr (S2) {
      const int pix = pix_index_s2_in(xs, p);
#pragma unroll
      for (int cls = 0; cls < 4; ++cls) {
        const unsigned voff = pix >= 0 ? (unsigned)(pix + (cls >> 1) * p.W + (cls & 1)) * xrow_bytes + x_const : OOB;
        if (wave == 0 && slot == 0) dma16(voff, srdx, lds0 + cls * XALLOC + XRING);
        dma16(voff, srdx, lds0 + cls * XALLOC + slot * 4096u + wq * 1024u);
      }
    } else {
      const int pix = pix_index(xs, p);
      const unsigned voff = pix >= 0 ? (unsigned)pix * xrow_bytes + x_const : OOB;
      // rows 0..15 of the ring are also kept behind its end: a fragment's second transposed read is the
      // first + 16 rows, which then never needs the wrap-around mask
      if (tg == 0) {
        if (wave == 0 && slot == 0) dma16(voff, srdx, lds0 + XRING);
        dma16(voff, srdx, lds0 + slot * 4096u + wq * 1024u);
      }
    }
    pix_advance64(xs, p);
  };
  auto issue_y = [&](int stage) {
    const int pix = S2 ? pix_index_s2_out(ys, p) : pix_index(ys, p);
    const unsigned voff = pix >= 0 ? (unsigned)pix * yrow_bytes + y_const : OOB;
    const unsigned dst = lds0 + XTOT + stage * YST + (NW == 8 ? tg * 4096u : 0u) + wq * 1024u;
    dma16_imm<0>((y_n < p.ldy) ? voff : OOB, srdy, dst);
    if constexpr (NW == 4) {
      dma16_imm<64>((y_n + 32 < p.ldy) ? voff : OOB, srdy, dst + 4096u);
      if constexpr (YD == 4) {
        dma16_imm<128>((y_n + 64 < p.ldy) ? voff : OOB, srdy, dst + 8192u);
        dma16_imm<192>((y_n + 96 < p.ldy) ? voff : OOB, srdy, dst + 12288u);
      }
    } else if constexpr (YD == 4) {
      dma16_imm<128>((y_n + 64 < p.ldy) ? voff : OOB, srdy, dst + 8192u);
    }
    pix_advance64(ys, p);
  };

  // ---- fragment read addresses
  const int g = lane >> 4, li = lane & 15, q = li >> 2, pc = li & 3;
  int E[TPW], EC[TPW];      // byte address of the tap's fragment inside its ring at chunk 0; the ring
#pragma unroll
  for (int i = 0; i < TPW; ++i) {
    const int tap = tap0 + i;
    const int kh = tap / 3, kw = tap % 3;
    const int rowc = (S2 ? (kh >> 1) * p.P + (kw >> 1) : (kh - 1) * p.P + (kw - 1)) + 4 * g + q;
    E[i] = rowc * 64 + ((u ^ ((rowc >> 2) & 1)) * 32) + pc * 8;
    EC[i] = S2 ? ((kh & 1) * 2 + (kw & 1)) * XALLOC : 0;
  }
  int Fy[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int f = ch * NJ + j, row = 4 * g + q;
    Fy[j] = XTOT + (f >> 1) * 4096 + row * 64 + (((f & 1) ^ ((row >> 2) & 1)) * 32) + pc * 8;
  }

  f32x4 acc[TPW][NJ];
#pragma unroll
  for (int i = 0; i < TPW; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // prologue: the input chunks behind and ahead of the first step, then PRE pipelined chunks
  for (int c = c0 - p.leadB; c < c0 + p.leadA; ++c) issue_x(c);
#pragma unroll
  for (int s = 0; s < PRE; ++s) {
    issue_x(c0 + p.leadA + s);
    issue_y(s);
  }

  typedef short s16x8 __attribute__((ext_vector_type(8)));
  for (int t = 0; t < ((p.debug & 2) ? 1 : nsteps); ++t) {
    // (wave 0's occasional extra DMA only makes this wait for more than it needs)
    if (t + PRE - 1 >= nsteps)
      wait_vmcnt<0>();
    else if (tg == 0)
      wait_vmcnt<LPT0*(PRE - 1)>();
    else
      wait_vmcnt<LPT1*(PRE - 1)>();
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (t + PRE < nsteps && !(p.debug & 4)) {
      issue_x(c0 + t + PRE + p.leadA);
      issue_y((t + PRE) % ST);
    }
    const int T = (c0 + t) * 4096;
    const char* sY = smem + (t % ST) * YST;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 bfr[NJ];
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const char* a = sY + Fy[j] + ks * 2048;
        const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)a);
        const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(a + 1024));
        const s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        bfr[j] = __builtin_bit_cast(bf16x8, v);
      }
#pragma unroll
      for (int i = 0; i < TPW; ++i) {
        if (NW == 8 && i >= ntaps) continue;       // (wave-uniform: the last slot of the second tap group is unused)
        const char* a = smem + EC[i] + ((E[i] + T + ks * 2048) & (XRING - 1));
        const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)a);
        const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(a + 1024));
        const s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        const bf16x8 af = __builtin_bit_cast(bf16x8, v);
#pragma unroll
        for (int j = 0; j < NJ; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bfr[j], acc[i][j], 0, 0, 0);
      }
    }
  }

  // ---- epilogue: per tap the wave's 16 x (CO_T/2) f32 tile goes through LDS and leaves as whole rows
  float* slab = p.out + (size_t)bsplit * 9 * p.Cin * p.Cout;
  wait_vmcnt<0>();
  __syncthreads();
  constexpr int WTN = CO_T / 2;
  constexpr int ROWP = WTN * 4 + 16;
  constexpr int CPR4 = WTN / 4;
  char* sw = smem + wave * (16 * ROWP);
#pragma unroll
  for (int i = 0; i < TPW; ++i) {
    if (NW == 8 && i >= ntaps) continue;
    const int tap = tap0 + i;
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) *reinterpret_cast<float*>(sw + (g * 4 + r) * ROWP + (j * 16 + li) * 4) = acc[i][j][r];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
    for (int it = 0; it < (16 * CPR4) / 64; ++it) {
      const int idx = it * 64 + lane;
      const int row = idx / CPR4, c4 = idx % CPR4;
      const int kk = tap * p.Cin + ci0 + u * 16 + row, n = co0 + ch * WTN + c4 * 4;
      if (n < p.Cout && !(p.debug & 1))
        *reinterpret_cast<float4*>(slab + (size_t)kk * p.Cout + n) = *reinterpret_cast<const float4*>(sw + row * ROWP + c4 * 16);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
}

// out[i] = sum_k slabs[k][i] in a fixed order.  256 threads = 64 outputs x 4 split lanes
// (lane g sums k = g, g+4, ... with four loads in flight), combined through LDS: short
// dependent chains even for hundreds of splits of a small matrix.
__global__ __launch_bounds__(256) void slab_reduce_kernel(const float* slabs, float* out, int64_t n, int splits) {
  __shared__ float sh[4][64];
  const int o = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int64_t i = (int64_t)blockIdx.x * 64 + o;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  if (i < n) {
    int k = g;
    for (; k + 12 < splits; k += 16) {
      a0 += slabs[(size_t)k * n + i];
      a1 += slabs[(size_t)(k + 4) * n + i];
      a2 += slabs[(size_t)(k + 8) * n + i];
      a3 += slabs[(size_t)(k + 12) * n + i];
    }
    for (; k < splits; k += 4) a0 += slabs[(size_t)k * n + i];
  }
  sh[g][o] = (a0 + a1) + (a2 + a3);
  __syncthreads();
  if (g == 0 && i < n) out[i] = (sh[0][o] + sh[1][o]) + (sh[2][o] + sh[3][o]);
}

// first layer (Cin = 3): dw[27][Cout] by direct accumulation; each block reduces a pixel
// range for all 27*Cout outputs (thread = one (k, co) pair), partials summed afterwards.
__global__ __launch_bounds__(1024) void conv_first_wgrad_kernel(const float* img, const bf16* dy, float* slabs, int B,
                                                                int H, int W, int Cout, int px_per_block) {
  const int M = B * H * W;
  const int o = threadIdx.x;
  const int nout = 27 * Cout;
  if (o >= nout) return;
  const int k = o / Cout, co = o - k * Cout;
  const int tap = k / 3, ci = k - tap * 3;
  const int kh = tap / 3, kw = tap - kh * 3;
  const int m0 = blockIdx.x * px_per_block;
  int m1 = m0 + px_per_block;
  if (m1 > M) m1 = M;
  float acc = 0.f;
  for (int m = m0; m < m1; ++m) {
    const int b = m / (H * W);
    const int rem = m - b * H * W;
    const int y = rem / W, x = rem - y * W;
    const int iy = y + kh - 1, ix = x + kw - 1;
    if ((unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W)
      acc += img[((size_t)(b * H + iy) * W + ix) * 3 + ci] * (float)dy[(size_t)m * Cout + co];
  }
  slabs[(size_t)blockIdx.x * nout + o] = acc;
}

// ---------------------------------------------------------------------------------------------
// First layer (Cin = 3, Cout = 32) on the matrix cores, taps as the M axis: dw[27][32] = sum over pixels of
// x(pixel + tap)[c] * dy(pixel)[n] is a [32 x P] x [P x 32] product with the PIXELS as the reduction axis -- 27 of the 32
// rows real, against 27 of 72 (K = 9 taps x 8 padded channels, 128-row tiles) in the im2col form this replaces.
// Unit of work: 128 pixels of one image row.  Its gradient tile [128][32] comes in by LDS-DMA exactly like a chunk of the
// tap-fused kernel (two [64 pixels][32 channels] images, same swizzle, same transposed reads, same k permutation: lane
// group g holds pixels 4g..4g+3 and 16+4g..16+4g+3 of a 32-pixel group).  The image rows y-1..y+1 are loaded as f32,
// rounded to bf16 and written to LDS as 27 rows, one per (kh, kw, c): row (kh, kw, c)[j] = x(y+kh-1, x0+j+kw-1)[c] -- the
// three kw copies make every A fragment two aligned 8-byte reads (row pitch 272 B: conflict-free).  Wave w multiplies
// pixel group w of the unit: 4 MFMAs per 4 + 4 LDS reads.  Two LDS stages, the next unit's DMA and image loads in flight
// under the current unit's MFMAs; a block sums its four waves and writes one [27][32] slab.
constexpr int F1_ROWB = 272;
constexpr int F1_IMGB = 27 * F1_ROWB + 80;     // 7424: the gradient tile behind it stays 1 KiB-aligned
constexpr int F1_STB = F1_IMGB + 8192;

__global__ __launch_bounds__(512) void conv_first_wgrad_mfma_kernel(const float* img, const bf16* dy, float* slabs, int B,
                                                                   int H, int W, int units_x, int nunits, unsigned bytesy) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smem;
  // two independent 4-wave groups per block, each walking its own units through its own two stages (twice the bytes in
  // flight per CU for the same number of slabs; the block's barriers serve both)
  const int grp = __builtin_amdgcn_readfirstlane(threadIdx.x >> 8);
  const int tid = threadIdx.x & 255, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const unsigned gbase = (unsigned)grp * 2u * F1_STB;
  const int g = lane >> 4, li = lane & 15, q = li >> 2, pc = li & 3;
  const i32x4 srdy = make_srd(dy, bytesy);
  // gradient DMA: row 16*wave + lane/4 of each 64-pixel image, 16-byte piece lane%4 (source-side swizzle)
  const int drow = wave * 16 + (lane >> 2), dpc = lane & 3;
  const unsigned y_const = (unsigned)((((dpc >> 1) ^ ((drow >> 2) & 1)) * 16 + (dpc & 1) * 8) * 2);
  // image loads: element e = tid (+256) of the 390 floats [x0-1, x0+128] x 3 channels of a row
  int e_x[2], e_c[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int e = tid + h * 256;
    e_x[h] = e / 3;
    e_c[h] = e - e_x[h] * 3;
  }
  float iv[3][2];
  auto unit_of = [&](int u, int& b, int& y, int& x0) {
    const int xb = u % units_x, r = u / units_x;
    y = r % H;
    b = r / H;
    x0 = xb * 128;
  };
  auto issue_dy = [&](int stage, int b, int y, int x0) {
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      const int x = x0 + s2 * 64 + drow;
      const unsigned voff = x < W ? (unsigned)((b * H + y) * W + x) * 64u + y_const : OOB;
      dma16(voff, srdy, lds0 + gbase + stage * F1_STB + F1_IMGB + s2 * 4096 + wave * 1024);
    }
  };
  auto load_img = [&](int b, int y, int x0) {
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
      const int yy = y + kh - 1;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int x = x0 - 1 + e_x[h];
        const bool ok = (tid + h * 256 < 390) && ((unsigned)yy < (unsigned)H) && ((unsigned)x < (unsigned)W);
        iv[kh][h] = ok ? img[((size_t)(b * H + yy) * W + x) * 3 + e_c[h]] : 0.f;
      }
    }
  };
  auto write_img = [&](int stage) {
    char* base = smem + gbase + stage * F1_STB;
#pragma unroll
    for (int kh = 0; kh < 3; ++kh)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        if (tid + h * 256 >= 390) continue;
        const bf16 v = (bf16)iv[kh][h];
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
          const int j = e_x[h] - kw;
          if ((unsigned)j < 128u) *reinterpret_cast<bf16*>(base + ((kh * 3 + kw) * 3 + e_c[h]) * F1_ROWB + j * 2) = v;
        }
      }
  };
  f32x4 acc[2][2];
#pragma unroll
  for (int f = 0; f < 2; ++f)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[f][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int a_off = li * F1_ROWB + (32 * wave + 4 * g) * 2;             // row li (fragment 0); fragment 1 = row 16 + li
  const bool a1_ok = 16 + li < 27;
  const int brow = 4 * g + q;
  int Fy[2];
#pragma unroll
  for (int j = 0; j < 2; ++j)
    Fy[j] = F1_IMGB + (wave >> 1) * 4096 + (wave & 1) * 2048 + brow * 64 + ((j ^ ((brow >> 2) & 1)) * 32) + pc * 8;

  int u = blockIdx.x * 2 + grp;
  const int ustep = gridDim.x * 2;
  int stage = 0;
  if (u < nunits) {
    int b, y, x0;
    unit_of(u, b, y, x0);
    issue_dy(0, b, y, x0);
    load_img(b, y, x0);
    write_img(0);
  }
  wait_vmcnt<0>();
  __syncthreads();
  typedef short s16x8 __attribute__((ext_vector_type(8)));
  // (both groups run the same number of rounds: the barriers are the block's)
  const int rounds = (nunits - (int)blockIdx.x * 2 + ustep - 1) / ustep;
  for (int it = 0; it < rounds; ++it, u += ustep) {
    const int un = u + ustep;
    const bool more = un < nunits;
    if (more) {
      int b, y, x0;
      unit_of(un, b, y, x0);
      issue_dy(stage ^ 1, b, y, x0);
      load_img(b, y, x0);
    }
    const char* sb = smem + gbase + stage * F1_STB;
    if (u < nunits) {
    bf16x8 af[2], bfr[2];
    {
      const uint2 lo = *reinterpret_cast<const uint2*>(sb + a_off), hi = *reinterpret_cast<const uint2*>(sb + a_off + 32);
      const uint4 v = {lo.x, lo.y, hi.x, hi.y};
      af[0] = __builtin_bit_cast(bf16x8, v);
      uint4 w = {0u, 0u, 0u, 0u};
      if (a1_ok) {
        const uint2 lo1 = *reinterpret_cast<const uint2*>(sb + a_off + 16 * F1_ROWB);
        const uint2 hi1 = *reinterpret_cast<const uint2*>(sb + a_off + 16 * F1_ROWB + 32);
        w = uint4{lo1.x, lo1.y, hi1.x, hi1.y};
      }
      af[1] = __builtin_bit_cast(bf16x8, w);
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const char* a = sb + Fy[j];
      const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)a);
      const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(a + 1024));
      const s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
      bfr[j] = __builtin_bit_cast(bf16x8, v);
    }
#pragma unroll
    for (int f = 0; f < 2; ++f)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[f][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[f], bfr[j], acc[f][j], 0, 0, 0);
    }
    if (more) write_img(stage ^ 1);
    wait_vmcnt<0>();
    __syncthreads();
    stage ^= 1;
  }
  // ---- the eight waves' [32][32] sums -> one slab [27][32] per block
  float* red = reinterpret_cast<float*>(smem);             // [8][32][32]
  __syncthreads();
#pragma unroll
  for (int f = 0; f < 2; ++f)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) red[((grp * 4 + wave) * 32 + 16 * f + 4 * g + r) * 32 + 16 * j + li] = acc[f][j][r];
  __syncthreads();
  float* slab = slabs + (size_t)blockIdx.x * 27 * 32;
  for (int o = threadIdx.x; o < 27 * 32; o += 512)
    slab[o] = ((red[o] + red[1024 + o]) + (red[2048 + o] + red[3072 + o])) + ((red[4096 + o] + red[5120 + o]) + (red[6144 + o] + red[7168 + o]));
}

void plan(const disyolo_conv_desc* d, int* bn, int* splits, int* steps_per_split, int* steps) {
  const int M = d->B * d->Ho * d->Wo;
  const int K = d->ksize * d->ksize * (d->C0 + d->C1);
  *bn = d->Cout > 64 ? 128 : (d->Cout > 32 ? 64 : 32);
  const int tiles = ceil_div(K, 128) * ceil_div(d->Cout, *bn);
  *steps = ceil_div(M, 32);
  const int target = 256, min_steps = 16;
  int s = target / tiles;  // fill the 256 CUs about twice; a full grid needs no pixel split
  if (s < 1) s = 1;
  const int max_s = ceil_div(*steps, min_steps);
  if (s > max_s) s = max_s;
  if (s < 1) s = 1;
  *steps_per_split = ceil_div(*steps, s);
  *splits = ceil_div(*steps, *steps_per_split);
}


constexpr int WG3_ST = 3;     // pipeline stages of the gradient image (prefetch depth WG3_ST - 1)
struct Plan3 {
  int co_t, R, splits, cps, chunks, tilesCi, tilesCo, leadA, leadB, s2;
  size_t lds;
};
// tap-fused kernel: 3x3, SAME pads, no fused concat, 32 | Cin, 4 | Cout; stride 1, or stride 2 on even maps (pad 0 before,
// 1 after) where four rings of 8 chunks fit (output rows up to 319 pixels)
bool plan3(const disyolo_conv_desc* d, int opts, Plan3* q) {
  // blocks aimed at per launch.  192, not one per CU: in the step these kernels run on the side lane beside the main
  // lane's data-gradient convs, and a grid that leaves a quarter of the CUs free costs the weight gradient less than it gives
  // the critical chain (interleaved A/B, ms per step at 256 / 192 / 160: stage 1 4.181 / 4.162 / 4.162, stage 2 9.849 / 9.807 /
  // 9.846, 832^2 4.312 / 4.297 / 4.286; 384 and 512: +4 %)
  const int target = 192;
  if (opts & DISYOLO_WGRAD_IM2COL) return false;
  if (d->ksize != 3 || d->C1 != 0 || d->in_div != 1 || d->C0 % 32 || d->Cout % 4 || d->Cout < 32) return false;
  q->s2 = 0;
  if (d->stride == 2) {
    if (d->pad_t != 0 || d->pad_l != 0 || (d->H & 1) || (d->W & 1) || d->Ho * 2 != d->H || d->Wo * 2 != d->W) return false;
    q->s2 = 1;
  } else if (d->stride != 1 || d->pad_t != 1 || d->pad_l != 1 || d->Ho != d->H || d->Wo != d->W) {
    return false;
  }
  const int P = d->Wo + 1, Hp = d->Ho + 1;
  q->co_t = d->Cout > 64 ? 128 : 64;
  // A layer whose 128-channel tiles would need exactly two pixel splits gets 64-channel tiles and no split
  // instead: same block count, the gradient is stored once, no partial sums to write and re-read.
  if (q->co_t == 128) {
    const int t128 = (d->C0 / 32) * ceil_div(d->Cout, 128);
    if ((target + t128 / 2) / t128 == 2) q->co_t = 64;
  }
  q->leadB = q->s2 ? 0 : ceil_div(P + 1, 64);
  q->leadA = 1 + P / 64;
  if (q->s2) q->co_t = 64;                // (four rings: 132 KiB of input, 24 KiB of gradient stages)
  const int need = (WG3_ST - 1) + q->leadA + q->leadB + 1;
  q->R = need <= 8 ? 8 : (need <= 16 ? 16 : 32);
  for (;;) {
    q->lds = (size_t)(q->s2 ? 4 : 1) * ((size_t)q->R * 4096 + 1024) + (size_t)WG3_ST * 64 * (size_t)q->co_t * 2;
    if (need <= 32 && q->lds <= 160 * 1024) break;
    if (q->co_t == 128) { q->co_t = 64; continue; }
    return false;
  }
  q->chunks = ceil_div((int64_t)d->B * Hp * P, 64);
  q->tilesCi = d->C0 / 32;
  q->tilesCo = ceil_div(d->Cout, q->co_t);
  const int tiles = q->tilesCi * q->tilesCo;
  int s = (target + tiles / 2) / tiles;
  const int max_s = q->chunks / 4 > 1 ? q->chunks / 4 : 1;
  if (s > max_s) s = max_s;
  if (s < 1) s = 1;
  q->cps = ceil_div(q->chunks, s);
  q->splits = ceil_div(q->chunks, q->cps);
  return true;
}
template <int CO_T, int R>
int launch3(const Wg3Params& p, const Plan3& q, hipStream_t s) {
  static bool attr_done = false;
  auto fn = conv_wgrad3x3_kernel<CO_T, R, WG3_ST, 4>;
  if (!attr_done) {
    if (hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess) {
      (void)hipGetLastError();
    }
    attr_done = true;
  }
  hipLaunchKernelGGL(fn, dim3(q.tilesCi * q.tilesCo * q.splits), dim3(256), q.lds, s, p);
  return 0;
}
int launch3_s2(const Wg3Params& p, const Plan3& q, hipStream_t s) {
  static bool attr_done = false;
  auto fn = conv_wgrad3x3_kernel<64, 8, WG3_ST, 4, 1>;
  if (!attr_done) {
    if (hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess) (void)hipGetLastError();
    attr_done = true;
  }
  hipLaunchKernelGGL(fn, dim3(q.tilesCi * q.tilesCo * q.splits), dim3(256), q.lds, s, p);
  return 0;
}

}  // namespace

extern "C" size_t disyolo_conv2d_wgrad_workspace(const disyolo_conv_desc* d, int opts) {
  if (!d) return 0;
  int bn, splits, sps, steps;
  plan(d, &bn, &splits, &sps, &steps);
  Plan3 q;
  if (plan3(d, opts, &q)) splits = q.splits;
  const size_t K = (size_t)d->ksize * d->ksize * (d->C0 + d->C1);
  return (size_t)splits * K * d->Cout * sizeof(float);
}

extern "C" int disyolo_conv2d_wgrad_plan(const disyolo_conv_desc* d, int opts, int* kind, int* tile_n, int* ring, int* splits) {
  if (!d || !kind || !tile_n || !ring || !splits) return DISYOLO_E_ARG;
  Plan3 q;
  if (plan3(d, opts, &q)) {
    *kind = 1; *tile_n = q.co_t; *ring = q.R; *splits = q.splits;
    return DISYOLO_OK;
  }
  int bn, sp, sps, steps;
  plan(d, &bn, &sp, &sps, &steps);
  *kind = 0; *tile_n = bn; *ring = 0; *splits = sp;
  return DISYOLO_OK;
}

// NOTE: the descriptor's `tile` field belongs to conv2d_fwd (a tuner pins forward / data-gradient tiles per GEMM shape
// in it) and is NOT read here: round 2 overloaded its bits as weight-gradient timing switches, so a layer whose forward
// shape had been tuned to a tile code with bit 9 set silently lost its slab reduction -- its weights trained on stale
// gradients (the stage-2 NaN of VERDICT r2).  The switches are the explicit `opts` argument now.
extern "C" int disyolo_conv2d_wgrad(const disyolo_conv_desc* d, const void* dy, int dy_ld, float* dw, void* workspace,
                                    size_t workspace_bytes, int opts, void* stream) {
  DY_REQUIRE(d && dy && dw, "wgrad: null pointer");
  DY_REQUIRE(d->ksize == 1 || d->ksize == 3, "wgrad: ksize");
  DY_REQUIRE(d->C0 > 0 && d->C0 % 8 == 0 && d->C1 % 8 == 0, "wgrad: channels must be multiples of 8");
  DY_REQUIRE(d->C1 == 0 || (d->ksize == 1 && d->stride == 1 && d->x1), "wgrad: bad fused-concat layer");
  DY_REQUIRE(dy_ld >= d->Cout && dy_ld % 8 == 0, "wgrad: dy_ld must be >= Cout and a multiple of 8");
  DY_REQUIRE(d->in_div == 1, "wgrad: in_div must be 1");
  DY_REQUIRE((int64_t)d->B * d->H * d->W * d->C0 * 2 < (1LL << 31) && (int64_t)d->B * d->Ho * d->Wo * dy_ld * 2 < (1LL << 31),
             "wgrad: a source tensor exceeds the 2 GiB the 32-bit gather offsets address");
  DY_REQUIRE((opts & ~(DISYOLO_WGRAD_IM2COL | DISYOLO_WGRAD_PARTIAL_ONLY | DISYOLO_WGRAD_REDUCE_ONLY | DISYOLO_WGRAD_STAGES_MASK)) == 0,
             "wgrad: unknown opts bits");
  if (!workspace || workspace_bytes < disyolo_conv2d_wgrad_workspace(d, opts)) {
    disyolo_set_error("wgrad: workspace too small");
    return DISYOLO_E_WORKSPACE;
  }
  {
    const disyolo_conv_desc c = *d;
    DY_RECORD_OR_RUN([=](void* s) { return disyolo_conv2d_wgrad(&c, dy, dy_ld, dw, workspace, workspace_bytes, opts, s); });
  }
  Plan3 q3;
  if (plan3(d, opts, &q3)) {
    Wg3Params p;
    p.x = (const bf16*)d->x0;
    p.dy = (const bf16*)dy;
    p.B = d->B; p.H = d->H; p.W = d->W; p.Cin = d->C0; p.Cout = d->Cout; p.ldy = dy_ld;
    p.Ho = d->Ho; p.Wo = d->Wo;
    p.P = d->Wo + 1; p.Hp = d->Ho + 1; p.frame = p.Hp * p.P;
    p.kbias = q3.s2 ? 0 : ceil_div((q3.leadB + 1) * 64, p.frame);
    p.a64 = 64 / p.P; p.r64 = 64 % p.P;
    p.chunks = q3.chunks; p.chunks_per_split = q3.cps;
    p.tilesCi = q3.tilesCi; p.tilesCo = q3.tilesCo; p.tiles = q3.tilesCi * q3.tilesCo;
    p.leadA = q3.leadA; p.leadB = q3.leadB;
    p.bytesx = (unsigned)((size_t)d->B * d->H * d->W * d->C0 * 2);
    p.bytesy = (unsigned)((size_t)d->B * d->Ho * d->Wo * dy_ld * 2);
    p.out = q3.splits == 1 ? dw : (float*)workspace;
    p.debug = 0;
    hipStream_t s = (hipStream_t)stream;
    if (opts & DISYOLO_WGRAD_REDUCE_ONLY) goto reduce3;
    if (q3.s2) {
      launch3_s2(p, q3, s);
    } else if (q3.co_t == 128) {
      if (q3.R == 8) launch3<128, 8>(p, q3, s);
      else if (q3.R == 16) launch3<128, 16>(p, q3, s);
      else launch3<128, 32>(p, q3, s);
    } else {
      if (q3.R == 8) launch3<64, 8>(p, q3, s);
      else if (q3.R == 16) launch3<64, 16>(p, q3, s);
      else launch3<64, 32>(p, q3, s);
    }
    DY_CHECK_LAUNCH();
  reduce3:
    if (q3.splits > 1 && !(opts & DISYOLO_WGRAD_PARTIAL_ONLY)) {
      const int64_t n = (int64_t)9 * p.Cin * p.Cout;
      hipLaunchKernelGGL(slab_reduce_kernel, dim3(ceil_div(n, 64)), dim3(256), 0, s, (const float*)workspace, dw, n,
                         q3.splits);
      DY_CHECK_LAUNCH();
    }
    return DISYOLO_OK;
  }
  WgradParams p;
  p.x0 = (const bf16*)d->x0;
  p.x1 = (const bf16*)d->x1;
  p.dy = (const bf16*)dy;
  p.B = d->B; p.H = d->H; p.W = d->W; p.C0 = d->C0; p.C1 = d->C1; p.Cin = d->C0 + d->C1;
  p.Ho = d->Ho; p.Wo = d->Wo; p.Cout = d->Cout; p.ldy = dy_ld;
  p.ks = d->ksize; p.stride = d->stride; p.pad_t = d->pad_t; p.pad_l = d->pad_l;
  p.M = d->B * d->Ho * d->Wo;
  p.K = d->ksize * d->ksize * p.Cin;
  p.bytes0 = (unsigned)((size_t)d->B * d->H * d->W * d->C0 * 2);
  p.bytes1 = (unsigned)((size_t)d->B * (d->H / 2) * (d->W / 2) * d->C1 * 2);
  p.bytesy = (unsigned)((size_t)p.M * dy_ld * 2);
  int bn, splits;
  plan(d, &bn, &splits, &p.steps_per_split, &p.steps);
  p.out = splits == 1 ? dw : (float*)workspace;
  hipStream_t s = (hipStream_t)stream;
  p.tilesK = ceil_div(p.K, 128);
  p.tilesN = ceil_div(p.Cout, bn);
  dim3 grid(p.tilesK * p.tilesN * splits);
  // pipeline depth: opts bits 4-5 (1..3 -> 2..4 stages) override the default (tuning)
  const int sto = (opts & DISYOLO_WGRAD_STAGES_MASK) >> 4;
  const int st = sto ? sto + 1 : 3;
  if (opts & DISYOLO_WGRAD_REDUCE_ONLY) goto reduce1;
#define DY_WG(BNV, YB)                                                                                   \
  if (st == 2) hipLaunchKernelGGL((conv_wgrad_kernel<BNV, 2>), grid, dim3(256), 2 * (8192 + YB), s, p);      \
  else if (st == 3) hipLaunchKernelGGL((conv_wgrad_kernel<BNV, 3>), grid, dim3(256), 3 * (8192 + YB), s, p); \
  else hipLaunchKernelGGL((conv_wgrad_kernel<BNV, 4>), grid, dim3(256), 4 * (8192 + YB), s, p);
  if (bn == 128) { DY_WG(128, 8192) }
  else if (bn == 64) { DY_WG(64, 4096) }
  else { DY_WG(32, 4096) }
#undef DY_WG
  DY_CHECK_LAUNCH();
reduce1:
  if (splits > 1 && !(opts & DISYOLO_WGRAD_PARTIAL_ONLY)) {
    const int64_t n = (int64_t)p.K * p.Cout;
    hipLaunchKernelGGL(slab_reduce_kernel, dim3(ceil_div(n, 64)), dim3(256), 0, s, (const float*)workspace, dw, n,
                       splits);
    DY_CHECK_LAUNCH();
  }
  return DISYOLO_OK;
}

static int first_wgrad_blocks(int B, int H, int W) {
  const int64_t pairs = ((int64_t)B * H * ceil_div(W, 128) + 1) / 2;     // a block walks two units at a time
  return (int)(pairs < 512 ? pairs : 512);         // two resident blocks per CU
}

extern "C" size_t disyolo_conv_first_wgrad_workspace(int B, int H, int W, int Cout) {
  const int64_t M = (int64_t)B * H * W;
  const int blocks = ceil_div(M, 1024);
  const size_t direct = (size_t)blocks * 27 * Cout * sizeof(float);
  const size_t mfma = (size_t)first_wgrad_blocks(B, H, W) * 27 * 32 * sizeof(float);
  return direct > mfma ? direct : mfma;
}

extern "C" int disyolo_conv_first_wgrad(const float* images, const void* dy, float* dw, int B, int H, int W, int Cout,
                                        void* workspace, size_t workspace_bytes, void* stream) {
  DY_REQUIRE(images && dy && dw && B > 0 && H > 0 && W > 0 && Cout > 0 && 27 * Cout <= 1024, "first_wgrad: bad args");
  if (!workspace || workspace_bytes < disyolo_conv_first_wgrad_workspace(B, H, W, Cout)) {
    disyolo_set_error("first_wgrad: workspace too small");
    return DISYOLO_E_WORKSPACE;
  }
  DY_RECORD_OR_RUN([=](void* s) { return disyolo_conv_first_wgrad(images, dy, dw, B, H, W, Cout, workspace, workspace_bytes, s); });
  const int64_t M = (int64_t)B * H * W;
  hipStream_t s = (hipStream_t)stream;
  const int64_t n = 27 * Cout;
  if (Cout == 32 && M * 64 < (1LL << 31)) {
    // the matrix-core form (the layer as the reference builds it: 32 filters, yolo/yolo3_net_pos.py:159)
    const int units_x = ceil_div(W, 128);
    const int nunits = B * H * units_x;
    const int blocks = first_wgrad_blocks(B, H, W);
    hipLaunchKernelGGL(conv_first_wgrad_mfma_kernel, dim3(blocks), dim3(512), 4 * F1_STB, s, images, (const bf16*)dy,
                       (float*)workspace, B, H, W, units_x, nunits, (unsigned)(M * 64));
    DY_CHECK_LAUNCH();
    hipLaunchKernelGGL(slab_reduce_kernel, dim3(ceil_div(n, 64)), dim3(256), 0, s, (const float*)workspace, dw, n, blocks);
    DY_CHECK_LAUNCH();
    return DISYOLO_OK;
  }
  const int blocks = ceil_div(M, 1024);
  hipLaunchKernelGGL(conv_first_wgrad_kernel, dim3(blocks), dim3(1024), 0, s, images, (const bf16*)dy,
                     (float*)workspace, B, H, W, Cout, 1024);
  DY_CHECK_LAUNCH();
  hipLaunchKernelGGL(slab_reduce_kernel, dim3(ceil_div(n, 64)), dim3(256), 0, s, (const float*)workspace, dw, n,
                     blocks);
  DY_CHECK_LAUNCH();
  return DISYOLO_OK;
}

// Instance measurement: length, width and area of every merged instance (dis-yolo_amd/measure.py).
//
// The reference has no counterpart; the definition these kernels are held to is tests/measure_ref.py.  They read the [G,8]
// groups table and the byte arena exactly as disyolo_tile_compose leaves them (tiles.hip): group g's mask is its crop,
// bh x bw bytes, row-major with pitch bw, at arena + 16 * off16; a non-zero byte is foreground; the bytes between two crops
// belong to nobody and are never read as pixels.  Every output lies in the same layout, one element per pixel, and the
// elements between two crops are never written.
//   measure_colg     thread per column: g = the distance within the column to the nearest zero (rows -1 and bh are zeros)
//   measure_rowd2    D2(y, x) = min over x' of (x - x')^2 + g(y, x')^2, searched outwards from x: the exact squared Euclidean
//                    distance to the background in int32, no float in it
//   measure_thin     one sub-step of Zhang-Suen thinning for all groups, from one byte buffer into the other
//   measure_counts   the exact per-group counts (integer atomics) and per-block float64 partials of the sum of sqrt(D2)
//   measure_sumsqrt  the partials of a group summed in block order: no float atomic, the same bits on every run
// A block owns ME_CHUNK consecutive pixels of a crop (the groups table's block0 column, found by binary search, as
// tile_compose_kernel does), a thread ME_PX of them ME_T apart: the lanes of a wave touch neighbouring bytes.
#include "measure_common.h"

namespace {

constexpr int ME_STAGE_BW = 1024;           // rows of g up to this width are staged in LDS by the row pass
constexpr int ME_STAGE = ME_CHUNK + 2 * ME_STAGE_BW;

// ---- distance: column pass ------------------------------------------------------------------------------------------------
// grid (G, column blocks of the widest crop): a thread walks its column down and up again; consecutive lanes are on
// consecutive bytes of the mask and consecutive halfwords of g in every step.  g <= (bh + 1) / 2 fits 16 bits.
__global__ __launch_bounds__(ME_T) void measure_colg_kernel(const int* groups, const unsigned char* arena, unsigned short* colg) {
  const int* g = groups + (size_t)blockIdx.x * 8;
  const int bh = g[4] - g[2], bw = g[5] - g[3];
  const int x = blockIdx.y * ME_T + threadIdx.x;
  if (x >= bw) return;
  const size_t off = (size_t)g[7] * 16;
  const unsigned char* m = arena + off + x;
  unsigned short* o = colg + off + x;
  int d = 0;
  for (int y = 0; y < bh; ++y) {
    d = m[(size_t)y * bw] ? d + 1 : 0;
    o[(size_t)y * bw] = (unsigned short)d;
  }
  d = 0;
  for (int y = bh - 1; y >= 0; --y) {
    d = m[(size_t)y * bw] ? d + 1 : 0;
    if (d < (int)o[(size_t)y * bw]) o[(size_t)y * bw] = (unsigned short)d;
  }
}

// ---- distance: row pass ---------------------------------------------------------------------------------------------------
// A candidate at distance dx along the row costs at least dx^2, so the search ends when dx^2 reaches the best so far: a crack
// costs a handful of steps per pixel, a blob its half-width.  Column -1 and column bw hold g = 0 and end every search that
// reaches them, so nothing beyond them is read.  The rows the chunk touches are staged in LDS when the crop is at most
// ME_STAGE_BW wide (ME_CHUNK pixels then touch at most ME_CHUNK / bw + 2 rows: at most ME_STAGE elements); a wider crop's
// chunk lies in one or two rows and is searched through the cache.
__global__ __launch_bounds__(ME_T) void measure_rowd2_kernel(const int* groups, int G, const unsigned char* arena,
                                                             const unsigned short* colg, int* d2) {
  __shared__ unsigned short rows[ME_STAGE];
  const Crop c = crop_of_block(groups, G);
  const int bw = c.bw;
  const int pend = min(c.p0 + ME_CHUNK, c.area);
  const int y0 = c.p0 / bw, y1 = (pend - 1) / bw;                     // (the block has at least one pixel: p0 < area)
  const unsigned short* gg = colg + c.off;
  const bool staged = bw <= ME_STAGE_BW;                              // (block-uniform)
  if (staged) {
    const int n = (y1 - y0 + 1) * bw;
    for (int i = threadIdx.x; i < n; i += ME_T) rows[i] = gg[(size_t)y0 * bw + i];
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < ME_PX; ++k) {
    const int p = c.p0 + k * ME_T + threadIdx.x;
    if (p >= c.area) break;
    int best = 0;
    if (arena[c.off + p]) {
      const int y = p / bw, x = p - y * bw;
      if (staged) {
        const unsigned short* r = rows + (y - y0) * bw;
        const int g0 = r[x];
        best = g0 * g0;
        for (int dx = 1; dx * dx < best; ++dx) {
          const int gl = x - dx >= 0 ? (int)r[x - dx] : 0, gr = x + dx < bw ? (int)r[x + dx] : 0;
          best = min(best, dx * dx + min(gl * gl, gr * gr));
        }
      } else {
        const unsigned short* r = gg + (size_t)y * bw;
        const int g0 = r[x];
        best = g0 * g0;
        for (int dx = 1; dx * dx < best; ++dx) {
          const int gl = x - dx >= 0 ? (int)r[x - dx] : 0, gr = x + dx < bw ? (int)r[x + dx] : 0;
          best = min(best, dx * dx + min(gl * gl, gr * gr));
        }
      }
    }
    d2[c.off + p] = best;
  }
}

// ---- thinning -------------------------------------------------------------------------------------------------------------
// One sub-step for every group: a pixel's 3x3 neighbourhood comes from `src` (the state at the sub-step's start), its new state
// goes to `dst`; every pixel of a live group is written, so both buffers always hold a whole state and block borders inside a
// crop need no care.  flags rows: row[g] != 0 <=> iteration deleted something in group g.  A group whose previous iteration
// deleted nothing is finished: its blocks return at once, its row stays 0 for every later iteration, and the buffer the second
// sub-step writes keeps its skeleton.  No block waits for another: the flags are read only by later launches.
__global__ __launch_bounds__(ME_T) void measure_thin_kernel(const int* groups, int G, const unsigned char* src, unsigned char* dst,
                                                            const int* prev_flags, int* flags, int* iters, int iteration,
                                                            int step) {
  const Crop c = crop_of_block(groups, G);
  if (prev_flags[c.g] == 0) return;                                   // (block-uniform)
  if (step == 1 && c.p0 == 0 && threadIdx.x == 0) iters[c.g] = iteration + 1;
  const unsigned char* s = src + c.off;
  const int bh = c.bh, bw = c.bw;
  int deleted = 0;
#pragma unroll
  for (int k = 0; k < ME_PX; ++k) {
    const int p = c.p0 + k * ME_T + threadIdx.x;
    if (p >= c.area) break;
    int keep = s[p] != 0;
    if (keep) {
      const int y = p / bw, x = p - y * bw;
      const bool n = y > 0, so = y + 1 < bh, w = x > 0, e = x + 1 < bw;
      const unsigned char* r = s + p;
      const int P2 = n && r[-bw], P3 = n && e && r[1 - bw], P4 = e && r[1], P5 = so && e && r[bw + 1];
      const int P6 = so && r[bw], P7 = so && w && r[bw - 1], P8 = w && r[-1], P9 = n && w && r[-bw - 1];
      const int B = P2 + P3 + P4 + P5 + P6 + P7 + P8 + P9;
      const int A = (!P2 && P3) + (!P3 && P4) + (!P4 && P5) + (!P5 && P6) + (!P6 && P7) + (!P7 && P8) + (!P8 && P9) + (!P9 && P2);
      const bool c1 = step == 1 ? !(P2 && P4 && P6) && !(P4 && P6 && P8) : !(P2 && P4 && P8) && !(P2 && P6 && P8);
      if (B >= 2 && B <= 6 && A == 1 && c1) keep = 0, deleted = 1;
    }
    dst[c.off + p] = (unsigned char)keep;
  }
  if (__ballot(deleted) != 0ull && (threadIdx.x & 63) == 0) atomicOr(&flags[c.g], 1);
}

// ---- counts ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double wave_sum_d(double v) {              // (a butterfly: every lane gets the same bits)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// counts[g] = {area, skel_px, n_orth, n_diag, n_end, max_d2, max_d2_skel, 0}.  A pair of skeleton pixels is counted at its
// upper (or, in a row, left) pixel, so every pair is counted once whichever blocks its pixels lie in.  The wave reduces its
// lanes' values, the block its waves' through LDS, and one integer atomic per block and quantity goes to the table.  The sum of
// sqrt(D2) takes no atomic: lanes add their pixels in k order, the butterfly and the four waves are added in a fixed order,
// and the block's partial goes to partials[blockIdx.x].
__global__ __launch_bounds__(ME_T) void measure_counts_kernel(const int* groups, int G, const unsigned char* arena,
                                                              const unsigned char* skel, const int* d2,
                                                              unsigned long long* counts, double* partials) {
  __shared__ long long part[ME_T / 64][8];
  __shared__ double dpart[ME_T / 64];
  const Crop c = crop_of_block(groups, G);
  const unsigned char* s = skel + c.off;
  const int bh = c.bh, bw = c.bw;
  int area = 0, sk = 0, orth = 0, diag = 0, nend = 0, mx = 0, mxs = 0;
  double ssq = 0.0;
#pragma unroll
  for (int k = 0; k < ME_PX; ++k) {
    const int p = c.p0 + k * ME_T + threadIdx.x;
    if (p >= c.area) break;
    const int d = d2[c.off + p];
    if (arena[c.off + p]) ++area, mx = max(mx, d);
    if (s[p]) {
      const int y = p / bw, x = p - y * bw;
      const bool n = y > 0, so = y + 1 < bh, w = x > 0, e = x + 1 < bw;
      const unsigned char* r = s + p;
      const int N = n && r[-bw], NE = n && e && r[1 - bw], E = e && r[1], SE = so && e && r[bw + 1];
      const int S = so && r[bw], SW = so && w && r[bw - 1], W = w && r[-1], NW = n && w && r[-bw - 1];
      ++sk;
      orth += E + S;
      diag += (SE && !E && !S) + (SW && !W && !S);
      const int nb = N + NE + E + SE + S + SW + W + NW;
      nend += nb == 1 ? 1 : nb == 0 ? 2 : 0;
      mxs = max(mxs, d);
      ssq += sqrt((double)d);
    }
  }
  const int wv = threadIdx.x >> 6;
  const long long v[5] = {wave_sum_ll(area), wave_sum_ll(sk), wave_sum_ll(orth), wave_sum_ll(diag), wave_sum_ll(nend)};
  mx = wave_max_i(mx), mxs = wave_max_i(mxs);
  ssq = wave_sum_d(ssq);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int q = 0; q < 5; ++q) part[wv][q] = v[q];
    part[wv][5] = mx, part[wv][6] = mxs;
    dpart[wv] = ssq;
  }
  __syncthreads();
  if (threadIdx.x < 7) {
    const int q = threadIdx.x;
    long long t = part[0][q];
#pragma unroll
    for (int i = 1; i < ME_T / 64; ++i) t = q < 5 ? t + part[i][q] : max(t, part[i][q]);
    if (t) {
      if (q < 5) atomicAdd(&counts[(size_t)c.g * 8 + q], (unsigned long long)t);
      else atomicMax(&counts[(size_t)c.g * 8 + q], (unsigned long long)t);
    }
  }
  if (threadIdx.x == 0) partials[blockIdx.x] = ((dpart[0] + dpart[1]) + dpart[2]) + dpart[3];
}

// one wave per group: lane l adds the partials of the group's blocks l, l + 64, ... in that order, then the butterfly
__global__ __launch_bounds__(64) void measure_sumsqrt_kernel(const int* groups, int G, int blocks, const double* partials,
                                                             double* sum_sqrt) {
  const int g = blockIdx.x;
  const int b0 = groups[(size_t)g * 8 + 6], b1 = g + 1 < G ? groups[(size_t)(g + 1) * 8 + 6] : blocks;
  double t = 0.0;
  for (int b = b0 + (int)threadIdx.x; b < b1; b += 64) t += partials[b];
  t = wave_sum_d(t);
  if (threadIdx.x == 0) sum_sqrt[g] = t;
}

}  // namespace

static int measure_d2_run(const int32_t* groups, int G, int blocks, int max_bw, const uint8_t* arena, uint16_t* colg, int32_t* d2,
                          void* stream) {
  DY_RECORD_OR_RUN([=](void* s) { return measure_d2_run(groups, G, blocks, max_bw, arena, colg, d2, s); });
  hipLaunchKernelGGL(measure_colg_kernel, dim3(G, (max_bw + ME_T - 1) / ME_T), dim3(ME_T), 0, (hipStream_t)stream,
                     (const int*)groups, (const unsigned char*)arena, (unsigned short*)colg);
  DY_CHECK_LAUNCH();
  hipLaunchKernelGGL(measure_rowd2_kernel, dim3(blocks), dim3(ME_T), 0, (hipStream_t)stream, (const int*)groups, G,
                     (const unsigned char*)arena, (const unsigned short*)colg, (int*)d2);
  DY_CHECK_LAUNCH();
  return DISYOLO_OK;
}

extern "C" int disyolo_measure_d2(const int32_t* groups_host, const int32_t* groups, int G, const uint8_t* arena,
                                  int64_t arena_bytes, uint16_t* colg, int32_t* d2, void* stream) {
  DY_REQUIRE(G <= 0 || (groups_host && groups && arena && colg && d2), "measure_d2: null pointer");
  int max_bw = 0;
  ME_TABLES("measure_d2", &max_bw);
  return measure_d2_run(groups, G, (int)blocks, max_bw, arena, colg, d2, stream);
}

static int measure_thin_run(const int32_t* groups, int G, int blocks, const uint8_t* arena, uint8_t* skel, uint8_t* tmp,
                            int32_t* flags, int32_t* iters, int it0, int chunk, void* stream) {
  DY_RECORD_OR_RUN([=](void* s) { return measure_thin_run(groups, G, blocks, arena, skel, tmp, flags, iters, it0, chunk, s); });
  hipStream_t st = (hipStream_t)stream;
  const size_t row = (size_t)G * sizeof(int32_t);
  hipError_t e;
  if (it0 == 0) {
    e = hipMemsetAsync(flags, 1, row, st);                            // row 0: "the iteration before the first" left every group live
    if (e == hipSuccess) e = hipMemsetAsync(iters, 0, row, st);
  } else {
    e = hipMemcpyAsync(flags, flags + (size_t)chunk * G, row, hipMemcpyDeviceToDevice, st);      // the last call's last row
  }
  if (e == hipSuccess) e = hipMemsetAsync(flags + G, 0, row * chunk, st);
  if (e != hipSuccess) {
    disyolo_set_error("measure_thin: preparing the flags failed: %s", hipGetErrorString(e));
    return DISYOLO_E_HIP;
  }
  for (int i = 0; i < chunk; ++i) {
    const int* prev = (const int*)flags + (size_t)i * G;
    int* cur = (int*)flags + (size_t)(i + 1) * G;
    // the very first sub-step reads the masks themselves (any non-zero byte is foreground); the arena is never written
    const unsigned char* src = (it0 + i == 0) ? (const unsigned char*)arena : (const unsigned char*)skel;
    hipLaunchKernelGGL(measure_thin_kernel, dim3(blocks), dim3(ME_T), 0, st, (const int*)groups, G, src, (unsigned char*)tmp, prev,
                       cur, (int*)iters, it0 + i, 1);
    DY_CHECK_LAUNCH();
    hipLaunchKernelGGL(measure_thin_kernel, dim3(blocks), dim3(ME_T), 0, st, (const int*)groups, G, (const unsigned char*)tmp,
                       (unsigned char*)skel, prev, cur, (int*)iters, it0 + i, 2);
    DY_CHECK_LAUNCH();
  }
  return DISYOLO_OK;
}

extern "C" int disyolo_measure_thin(const int32_t* groups_host, const int32_t* groups, int G, const uint8_t* arena,
                                    int64_t arena_bytes, uint8_t* skel, uint8_t* tmp, int32_t* flags, int32_t* iters, int it0,
                                    int chunk, void* stream) {
  DY_REQUIRE(G <= 0 || (groups_host && groups && arena && skel && tmp && flags && iters), "measure_thin: null pointer");
  DY_REQUIRE(it0 >= 0 && chunk >= 1 && chunk <= 1024 && it0 <= (1 << 30), "measure_thin: need it0 >= 0 and 1 <= chunk <= 1024 (got %d, %d)",
             it0, chunk);
  ME_TABLES("measure_thin", nullptr);
  return measure_thin_run(groups, G, (int)blocks, arena, skel, tmp, flags, iters, it0, chunk, stream);
}

static int measure_counts_run(const int32_t* groups, int G, int blocks, const uint8_t* arena, const uint8_t* skel, const int32_t* d2,
                              int64_t* counts, double* partials, double* sum_sqrt, void* stream) {
  DY_RECORD_OR_RUN([=](void* s) { return measure_counts_run(groups, G, blocks, arena, skel, d2, counts, partials, sum_sqrt, s); });
  if (hipMemsetAsync(counts, 0, (size_t)G * 8 * sizeof(int64_t), (hipStream_t)stream) != hipSuccess) {
    disyolo_set_error("measure_counts: hipMemsetAsync failed");
    return DISYOLO_E_HIP;
  }
  if (blocks) {
    hipLaunchKernelGGL(measure_counts_kernel, dim3(blocks), dim3(ME_T), 0, (hipStream_t)stream, (const int*)groups, G,
                       (const unsigned char*)arena, (const unsigned char*)skel, (const int*)d2, (unsigned long long*)counts,
                       partials);
    DY_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(measure_sumsqrt_kernel, dim3(G), dim3(64), 0, (hipStream_t)stream, (const int*)groups, G, blocks,
                     (const double*)partials, sum_sqrt);
  DY_CHECK_LAUNCH();
  return DISYOLO_OK;
}

extern "C" int disyolo_measure_counts(const int32_t* groups_host, const int32_t* groups, int G, const uint8_t* arena,
                                      int64_t arena_bytes, const uint8_t* skel, const int32_t* d2, int64_t* counts,
                                      double* partials, int64_t partials_len, double* sum_sqrt, void* stream) {
  DY_REQUIRE(G <= 0 || (groups_host && groups && arena && skel && d2 && counts && partials && sum_sqrt),
             "measure_counts: null pointer");
  ME_ARGS("measure_counts");
  ME_PLAN("measure_counts", nullptr);
  DY_REQUIRE(partials_len >= blocks, "measure_counts: %lld partials for %lld blocks", (long long)partials_len, (long long)blocks);
  // (groups without a pixel still get their zero row and their zero sum)
  return measure_counts_run(groups, G, (int)blocks, arena, skel, d2, counts, partials, sum_sqrt, stream);
}

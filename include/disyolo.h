/*
 * disyolo.h -- C ABI of the MI355X (gfx950) kernel library for the DIS-YOLO hot path.
 *
 * The reference (ZHANGKEON/DIS-YOLO) has no FFI/plugin interface: its hot path is a
 * TensorFlow-1.x graph (yolo/yolo3_net_pos.py) driven through tf.Session.run.  Each
 * entry point below replaces the TF op call sites named in its comment (file:line in
 * the reference checkout).  A maintainer binds them with ctypes.
 *
 * Conventions
 *   - extern "C", plain pointers + sizes; no torch / C++ types.
 *   - every pointer is a DEVICE pointer unless stated; `stream` is a hipStream_t
 *     passed as void*.  Calls are stream-ordered, never synchronise, never allocate
 *     (graph-capture safe); scratch comes from caller-provided workspaces.
 *   - return 0 on success, a negative DISYOLO_E_* code otherwise.  Nothing throws or
 *     exits.  disyolo_last_error() returns a static message for the calling thread.
 *   - activations are NHWC bf16; logits / score maps / losses / statistics are f32;
 *     master weights are f32 HWIO [k,k,Cin,Cout] (the reference checkpoint layout,
 *     yolo/yolo3_net_pos.py:112,118); the MFMA kernels read a packed bf16 copy made
 *     by disyolo_pack_weights.
 */
#ifndef DISYOLO_H
#define DISYOLO_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DISYOLO_OK 0
#define DISYOLO_E_ARG (-1)      /* invalid argument / unsupported shape */
#define DISYOLO_E_WORKSPACE (-2) /* workspace too small */
#define DISYOLO_E_HIP (-3)      /* a HIP runtime call failed */

#define DISYOLO_GRAD_LD 32      /* channel pitch of the head-logit / score-map gradients */
#define DISYOLO_ROI_MAX 16      /* RoI slots per image in the mask-loss RoI table       */
#define DISYOLO_ROI_W 12        /* int32 words per RoI: gy0..3, gx0..3, gt_row, area, valid, 0 */
/* int32 words per RoI of a k x k position-sensitive grid (k = 3, 5, 7): gy0..gyk, gx0..gxk, gt_row, area, valid, 0;
 * DISYOLO_ROI_W_K(3) == DISYOLO_ROI_W */
#define DISYOLO_ROI_W_K(k) (2 * ((k) + 1) + 4)

int disyolo_version(void);
const char* disyolo_last_error(void);

/* ---- convolution (replaces tf.nn.conv2d + bias_add + folded batch_normalization +
 *      leaky_relu + residual add + resize_nearest_neighbor/concat feeding a 1x1 conv:
 *      yolo/yolo3_net_pos.py:125-129,142-145,150,290-291,325-326,386-387,401-402) ---- */
enum {
  DISYOLO_CONV_LEAKY = 1,       /* y = max(alpha*y, y) after scale/shift            */
  DISYOLO_CONV_OUT_F32 = 2,     /* y is f32 (head logits / score maps), else bf16    */
  DISYOLO_CONV_STATS = 4,       /* also emit per-channel (sum, sum of squares) of the
                                   raw accumulators into `stats` (training BN, :90)  */
  DISYOLO_CONV_BN_BWD_STATS = 8,/* y is the (now final) gradient wrt the OUTPUT of a batch-
                                   normalised layer: also emit that layer's batch-norm
                                   backward sums, per channel over this block's pixels,
                                   (sum g, sum g*xhat) with g = y*act'(bn_x*bn_scale+bn_shift),
                                   xhat = (bn_x-bn_mean)*bn_rstd, from the bf16 values
                                   stored to y, into `bn_partials` -- the column reduction
                                   disyolo_bn_act_bwd would otherwise start with.  Only the
                                   3x3 patch kernels have this epilogue (tile ids 16-18, 24,
                                   25: disyolo_conv2d_bn_bwd_stats_ok tells), bf16 y,
                                   Cout % 8 == 0 (TF autodiff of :68-107)                */
  DISYOLO_CONV_BN_FUSED = 16,   /* with DISYOLO_CONV_STATS: training-mode batch norm INSIDE the launch
                                   (tf.nn.moments + batch_normalization + the moving-average assigns +
                                   leaky_relu, :90-107, in the conv's epilogue).  The blocks that share a
                                   channel tile exchange their statistics rows through `stats` within the
                                   launch (write-through stores, an arrival counter in `cluster_sync`,
                                   every block sums the rows in the same fixed order), then write BOTH
                                   y = the conv output (bf16, what the backward pass keeps) and y_act =
                                   leaky(y*scale + shift) computed from the bf16-rounded y -- bit for bit
                                   what disyolo_bn_finalize + disyolo_bn_act_fwd produce from y (up to the
                                   f64 summation order of the statistics rows) -- and one block per channel
                                   tile writes bn_out_* and updates the moving statistics.  Needs every
                                   block of the launch resident at once: disyolo_conv2d_bn_fused_ok tells;
                                   never run two such launches concurrently on one device (each waits for
                                   its own blocks: with both half-resident neither completes; the wait is
                                   bounded and reports through disyolo_cluster_sync_error)             */
  DISYOLO_CONV_BN_BWD_FUSED = 32,/* with the bn_* fields of DISYOLO_CONV_BN_BWD_STATS: the whole batch-norm
                                   backward of the target layer inside the data-gradient conv that makes its
                                   output gradient final: the sums are exchanged within the launch like the
                                   forward statistics, then y receives dx of the TARGET's conv output
                                   (scale*(g - mean(g) - xhat*mean(g*xhat))) instead of the gradient wrt its
                                   activation, and one block per channel tile writes bn_dgamma / bn_dbeta.
                                   disyolo_conv2d_bn_fused_ok tells; same residency rule                */
};

typedef struct disyolo_conv_desc {
  int32_t B, H, W;        /* source-0 spatial size                                   */
  int32_t C0, C1;         /* channels of source 0 / source 1 (C1 = 0: single source) */
  int32_t Ho, Wo, Cout;   /* output size                                              */
  int32_t ksize, stride;  /* 1 or 3; 1 or 2                                           */
  int32_t pad_t, pad_l;   /* TF 'SAME' leading pads (asymmetric for k=3,s=2)          */
  int32_t in_div;         /* 1 = forward gather.  s>1 = transposed gather for the
                             data-gradient of a stride-s conv: a tap contributes only
                             where (yo*stride + kh - pad_t) is divisible by in_div    */
  int32_t flags;          /* DISYOLO_CONV_*                                           */
  float alpha;            /* leaky slope                                              */
  int32_t tile;           /* 0 = the launcher's heuristic; else a tile code a caller-side
                             tuner pins (what YOLONet.autotune does): low byte = id
                             (1-12 GEMM block tiles 64x64 ... 256x128, 13-15 the same
                             with two K groups per block, 16/17 the 3x3 stride-1 patch
                             kernel with 8/4 waves, 18 = 16 with 32 instead of 64 output
                             channels per block, 20 = the persistent streaming form of
                             the patch kernel for 3x3 stride-1 layers with exactly 32
                             input channels, 21 = the streaming 1x1 kernel (stride 1,
                             Cout <= 64, C0 + C1 <= 192); an id that does not cover the shape
                             falls back), bit 8 = force K depth 32, bit 9 = the tile's
                             alternative pipeline depth                              */
  const void* x0;         /* bf16 [B,H,W,C0]                                          */
  const void* x1;         /* bf16 [B,H/2,W/2,C1]: nearest-upsampled x2 and concatenated
                             after x0 along channels (1x1 convs only), or NULL        */
  const void* w;          /* bf16 packed [Cout][ksize*ksize*(C0+C1)], k = (kh,kw,ci) */
  const float* scale;     /* [Cout] or NULL (=1)                                      */
  const float* shift;     /* [Cout] or NULL (=0)  (folded BN beta / conv bias)        */
  const void* residual;   /* bf16 [B,Ho,Wo,Cout] added after the activation, or NULL  */
  void* y;                /* bf16 or f32 [B,Ho,Wo,Cout]                               */
  float* stats;           /* f32 [disyolo_conv2d_stats_rows][Cout][2] or NULL         */
  /* DISYOLO_CONV_BN_BWD_STATS only (else ignored): */
  const void* bn_x;       /* bf16 [B,Ho,Wo,Cout]: the conv output the target layer normalised */
  const float* bn_scale;  /* [Cout] gamma*rstd                                         */
  const float* bn_shift;  /* [Cout] beta - mean*gamma*rstd                             */
  const float* bn_mean;   /* [Cout] batch mean                                         */
  const float* bn_rstd;   /* [Cout] 1/sqrt(var+eps)                                    */
  float* bn_partials;     /* f32 [disyolo_conv2d_stats_rows][Cout][2]                  */
  float bn_alpha;         /* the target layer's leaky slope                            */
  /* DISYOLO_CONV_BN_FUSED / DISYOLO_CONV_BN_BWD_FUSED only (else ignored): */
  float bn_decay, bn_eps; /* moving-average decay (0.997), variance epsilon            */
  void* y_act;            /* bf16 [B,Ho,Wo,Cout]: the activation (BN_FUSED)            */
  const float* bn_gamma;  /* [Cout]                                                    */
  const float* bn_beta;   /* [Cout]                                                    */
  float* bn_moving_mean;  /* [Cout] updated in place (or NULL)                         */
  float* bn_moving_var;   /* [Cout] updated in place (or NULL)                         */
  float* bn_out_scale;    /* [Cout] gamma*rstd              } what the backward pass   */
  float* bn_out_shift;    /* [Cout] beta - mean*gamma*rstd  } of this layer reads      */
  float* bn_out_mean;     /* [Cout] batch mean                                         */
  float* bn_out_rstd;     /* [Cout] 1/sqrt(var + eps)                                  */
  float* bn_dgamma;       /* [Cout] (BN_BWD_FUSED)                                     */
  float* bn_dbeta;        /* [Cout] (BN_BWD_FUSED)                                     */
  uint32_t* cluster_sync; /* disyolo_cluster_sync_words(Cout) words, zeroed ONCE by the caller
                             (the launches leave it zero); one buffer per layer and direction  */
} disyolo_conv_desc;

/* Host-side (no device work): the contour extraction of the dataset pre-processing, cv2.findContours(img,
 * cv2.RETR_TREE, cv2.CHAIN_APPROX_NONE) of pre_process.py:78-86 -- Suzuki-Abe border following, OpenCV's point
 * order and contour numbering (cv2 not available in the build environment: parity unpinned).  binary: h x w bytes,
 * non-zero = foreground.  points_xy int32 [n_points][2] (x, y); contour_start int32 [n_contours + 1]; hierarchy
 * int32 [n_contours][4] = next, previous, first child, parent.  Too-small buffers: DISYOLO_E_WORKSPACE with the
 * needed sizes in *n_contours / *n_points (call once with max 0 to size them). */
int disyolo_find_contours(const uint8_t* binary, int h, int w, int32_t* points_xy, int64_t max_points,
                          int32_t* contour_start, int32_t* hierarchy, int max_contours, int* n_contours,
                          int64_t* n_points);
/* sizeof(disyolo_conv_desc) as this library was built: a binding checks its mirror against it */
size_t disyolo_conv_desc_size(void);
/* 1 when a call with this descriptor runs a kernel that can emit DISYOLO_CONV_BN_BWD_STATS: the patch kernels and (round 6)
 * the GEMM tiles that carry that epilogue (1x1: 64x64, 64x128, 128x64, 96x128, 128x128; 1x1 and 3x3: 192x128), in_div 1 */
int disyolo_conv2d_bn_bwd_stats_ok(const disyolo_conv_desc* d);
/* 1 when a call with this descriptor (shape and tile as given) can run batch norm inside the launch -- the backward form
 * when DISYOLO_CONV_BN_BWD_FUSED is set in its flags, the forward form otherwise (DISYOLO_CONV_BN_FUSED need not be set):
 * a kernel that has the epilogue, bf16 y, Cout % 8 == 0, and a grid that is resident at once on this device (blocks <=
 * occupancy x compute units, queried from the runtime) with statistics rows few enough to be summed by every block */
int disyolo_conv2d_bn_fused_ok(const disyolo_conv_desc* d);
/* words of a `cluster_sync` buffer for a layer with Cout channels (any tile); the last word is the error word */
int disyolo_cluster_sync_words(int Cout);
/* 0, or the code a bounded in-launch wait left in the buffer's error word (device memory is read with a blocking copy:
 * call it at a synchronisation point, e.g. when the losses are fetched) */
int disyolo_cluster_sync_error(const uint32_t* cluster_sync, int Cout);
/* rows of the `stats` partial buffer a call with this descriptor writes */
int disyolo_conv2d_stats_rows(const disyolo_conv_desc* d);
int disyolo_conv2d_fwd(const disyolo_conv_desc* d, void* stream);
/* tile configuration the launcher picks for this descriptor: returns its id (> 0) and the
 * block tile (pixels x channels), K depth and pipeline stages -- the template arguments of the
 * conv_igemm_kernel instance that will run (ids 16/17: the conv_halo_kernel patch, 64
 * channels, 32-channel slices, 2 stages); bench.py attributes time per instance with it */
int disyolo_conv2d_tile(const disyolo_conv_desc* d, int* bm, int* bn, int* bk, int* stages);

/* first layer (Cin=3, k=3, s=1; yolo/yolo3_net_pos.py:159): f32 NHWC image in, exact f32
 * FMA with the f32 HWIO weights, folded BN + leaky, bf16 out. */
int disyolo_conv_first_fwd(const float* images, const float* w_hwio, const float* scale,
                           const float* shift, void* y_bf16, int B, int H, int W, int Cout,
                           float alpha, void* stream);

/* conv1 + conv2 in one launch when both run in inference mode (locked / inference net): act2 = leaky(bn2(conv3x3 stride 2
 * (leaky(bn1(conv3x3(images)))))), conv_bn 'convolutional1' + 'convolutional2', yolo/yolo3_net_pos.py:159-167 -- conv1's output (one consumer, the largest tensor of the
 * network) is never written.  images f32 NHWC [B,H,W,3]; w1 f32 HWIO [3,3,3,32]; w2 bf16 packed [64][9*32] (pack_weights);
 * folded BN scale / shift per layer; y bf16 [B,H/2,W/2,64].  conv1 runs on the bf16 matrix cores with hi/lo-split operands
 * (relative error 2^-16 per product against exact f32, before the rounding to bf16).  disyolo_conv12_fused_ok: 1 when the
 * sizes are covered (H/2 a multiple of 8, W/2 of 16). */
int disyolo_conv12_fused_ok(int B, int H, int W);
int disyolo_conv12_fused_fwd(const float* images, const float* w1_hwio, const float* scale1, const float* shift1,
                             const void* w2_packed, const float* scale2, const float* shift2, void* y_bf16, int B, int H,
                             int W, float alpha, void* stream);

/* The two HBM-bound [1x1 -> 32] -> [3x3 32 -> 64] chains of the half-resolution maps in one launch each, batch norms in
 * inference mode (folded scale / shift, leaky alpha); the 32- and 64-channel intermediates stay on chip:
 *   post 0  (C0 = 64, C1 = 0): y bf16 [B,H,W,64] = leaky(bnB(conv3x3(leaky(bnA(conv1x1(x0)))))) + x0 -- the first residual
 *           block (conv_bn 'convolutional3' + res_conv_bn 'convolutional4'), yolo/yolo3_net_pos.py:169-176;
 *   post 1  (C0 = 64, C1 = 32): y f32 [B,H,W,9] = conv1x1(leaky(bnB(conv3x3(leaky(bnA(conv1x1([x0, up2(x1)]))))))) + biasC -- the
 *           mask head (conv_bn 'convolutional80', 'convolutional81', conv 'convolutional82'), yolo/yolo3_net_pos.py:404-412; x1 bf16 [B,H/2,W/2,32] is read at (y/2, x/2);
 *   post 2, 3: the same mask head with NOUT = 25, 49 score maps (K_MAP = 5, 7): y f32 [B,H,W,NOUT].
 * x0 bf16 NHWC; wA packed [32][C0+C1], wB packed [64][9*32], wC packed [NOUT][64] (pack_weights; NOUT = 9 for post 1).
 * _ok: 1 when covered (those shapes, H a multiple of 8, W of 16, the largest tensor under 2^31 bytes). */
int disyolo_block32_fused_ok(int B, int H, int W, int C0, int C1, int post);
int disyolo_block32_fused_fwd(const void* x0, const void* x1, int C0, int C1, const void* wA, const float* scaleA,
                              const float* shiftA, const void* wB, const float* scaleB, const float* shiftB, int post,
                              const void* wC, const float* biasC, void* y, int B, int H, int W, float alpha, void* stream);

/* A residual block of the quarter-resolution maps in one launch, batch norms in inference mode: y bf16 [B,H,W,128] =
 * leaky(bnB(conv3x3(leaky(bnA(conv1x1(x)))))) + x with x bf16 [B,H,W,128], wA packed [64][128], wB packed [128][9*64]
 * (conv_bn + res_conv_bn, yolo/yolo3_net_pos.py:184-201, conv6+7 and conv8+9); the 64-channel intermediate stays in LDS.  _ok: C0 == 128, H a
 * multiple of 8, W of 16. */
int disyolo_block64_fused_ok(int B, int H, int W, int C0);
int disyolo_block64_fused_fwd(const void* x, const void* wA, const float* scaleA, const float* shiftA, const void* wB,
                              const float* scaleB, const float* shiftB, void* y, int B, int H, int W, int C0, float alpha,
                              void* stream);

/* Data gradient of a 3x3 stride-2 SAME conv over an even-sized input (TF autodiff of tf.nn.conv2d wrt its input,
 * train_yolo3_mask.py:55; conv2 / conv5 of the network, yolo/yolo3_net_pos.py:167,192) as one 2x2-tap conv over dy with a
 * depth-to-space store: dx bf16 [B, 2 Hdy, 2 Wdy, C] (+= residual when given) from dy bf16 [B, Hdy, Wdy, Cdy] and wq =
 * disyolo_pack_quad(w) (bf16 [4 C][9 Cdy], rebuilt from the f32 HWIO master [3][3][C][Cdy] whenever it changes).
 * The generic path (disyolo_conv2d_fwd with in_div = 2) gives the same values; this one is for the shallow layers
 * (C <= 64), where the generic tiles are bound by their fixed cost.  _ok: Cdy % 64 == 0, C in {32, 64}. */
int disyolo_pack_quad(const float* w_hwio, void* wq, int C, int Cdy, void* stream);
int disyolo_dgrad_s2_quad_ok(int B, int Hdy, int Wdy, int Cdy, int C);
int disyolo_dgrad_s2_quad(const void* dy, const void* wq, void* dx, const void* residual, int B, int Hdy, int Wdy, int Cdy,
                          int C, void* stream);

/* weight gradient (TF autodiff of tf.nn.conv2d wrt filters; train_yolo3_mask.py:55):
 * dw[kh,kw,ci,co] (f32 HWIO, overwritten) = sum_m xcol[m,(kh,kw,ci)] * dy[m,co].
 * Uses d->x0/x1 (the layer input, same gather as forward) and `dy` bf16 [B*Ho*Wo, dy_ld]
 * (dy_ld >= Cout, multiple of 8; columns >= Cout are ignored).
 * workspace: disyolo_conv2d_wgrad_workspace(d, opts) bytes.
 * The descriptor's `tile` field is NOT read (it pins the forward / data-gradient tile of the same GEMM shape);
 * `opts` = 0 for the product path, or DISYOLO_WGRAD_* bits for tuning and per-kernel timing. */
enum {
  DISYOLO_WGRAD_IM2COL = 1,       /* force the im2col kernel where the tap-fused 3x3 kernel would run   */
  DISYOLO_WGRAD_PARTIAL_ONLY = 2, /* launch only the partial-sum kernel (dw is NOT written if it splits) */
  DISYOLO_WGRAD_REDUCE_ONLY = 4,  /* launch only the slab reduction (workspace must hold the slabs)      */
  DISYOLO_WGRAD_STAGES_MASK = 0x30 /* im2col kernel pipeline depth: (n << 4), n = 1..3 -> 2..4 stages    */
};
/* ---- Workspaces.  Every entry point with a `workspace` / `workspace_bytes` pair keeps one contract; `need` is the answer
 * of its size query (disyolo_*_workspace*), or the size its comment states where it has no query:
 *   1. with workspace_bytes == need the call succeeds;
 *   2. it writes nothing outside [workspace, workspace + need);
 *   3. its outputs do not depend on what the workspace held before the call;
 *   4. with need - 1 bytes it returns DISYOLO_E_WORKSPACE before any launch.
 * Workspace contents are undefined on entry and on return: a caller may hand the same buffer to the next call on the same
 * stream, and must not read it.  tests/test_gpu_workspace.py holds every entry point to rules 1-3 (exact size between guard
 * bands, poisoned contents), tests/test_workspace.py to rule 4. */
size_t disyolo_conv2d_wgrad_workspace(const disyolo_conv_desc* d, int opts);
int disyolo_conv2d_wgrad(const disyolo_conv_desc* d, const void* dy, int dy_ld, float* dw,
                         void* workspace, size_t workspace_bytes, int opts, void* stream);
/* same for the first layer (f32 image input, Cin = 3): dw f32 [3,3,3,Cout] */
/* ---- fp8 (OCP e4m3) forward path of the inference-mode layers (BASELINE.json configs[4]; the reference
 * is f32: yolo/yolo3_net_pos.py:132-146 conv_bn with lock=True) ----
 * y = leaky(acc * escale[c] + eshift[c]) [+ residual_fp8 * residual_scale], acc = sum of e4m3 products in
 * f32 (v_mfma_f32_16x16x32_fp8_fp8).  desc: x0 = e4m3 NHWC input, geometry / alpha / LEAKY flag as for
 * conv2d_fwd (w, scale, shift, residual, y of the descriptor are ignored); w_fp8 = e4m3 [Cout][k*k*Cin]
 * (pack_weights_fp8); escale = s_in * s_w * folded-BN scale, eshift = folded-BN shift (f32 [Cout]).
 * Outputs: y_fp8 = e4m3 of y / out_scale and/or y_bf16 = bf16 of y (either may be NULL).
 * Cin a power of two >= 32, Cout a multiple of 16, no fused concat. */
int disyolo_conv2d_fp8_fwd(const disyolo_conv_desc* d, const void* w_fp8, const float* escale,
                           const float* eshift, const void* residual_fp8, float residual_scale,
                           void* y_fp8, float out_scale, void* y_bf16, void* stream);
/* first layer (f32 image, exact f32 FMA, folded BN + leaky) with the output stored as e4m3 of y / out_scale */
int disyolo_conv_first_fwd_fp8(const float* images, const float* w_hwio, const float* scale, const float* shift,
                               void* y_fp8, float out_scale, int B, int H, int W, int Cout, float alpha,
                               void* stream);
/* e4m3 of x / scale (x bf16, or f32 when x_is_f32; n % 8 == 0, saturating at +-448); back to f32 * scale */
int disyolo_quant_fp8(const void* x, int x_is_f32, void* y_fp8, int64_t n, float scale, void* stream);
int disyolo_dequant_fp8(const void* x_fp8, float* y, int64_t n, float scale, void* stream);
/* HWIO f32 weights -> e4m3 [Cout][k*k*Cin] of w / scale */
int disyolo_pack_weights_fp8(const float* w_hwio, void* w_fp8, int ksize, int Cin, int Cout,
                             float scale, void* stream);

/* which kernel the launcher picks for this descriptor: kind 0 = im2col kernel (tile_n = channel tile),
 * 1 = tap-fused 3x3 kernel, stride 1 or 2 (tile_n = channel tile, ring = input ring slots); splits = pixel splits
 * (f32 slabs summed by slab_reduce when > 1).  opts: DISYOLO_WGRAD_* as passed to disyolo_conv2d_wgrad. */
int disyolo_conv2d_wgrad_plan(const disyolo_conv_desc* d, int opts, int* kind, int* tile_n, int* ring, int* splits);
/* weight gradient of the first layer (yolo/yolo3_net_pos.py:159: 3 -> 32 filters, 3x3, stride 1): images f32 [B,H,W,3], dy bf16
 * [B,H,W,Cout], dw f32 [3][3][3][Cout].  Cout == 32 runs on the matrix cores with the 27 (tap, channel) pairs as the M axis (the image
 * is rounded to bf16 on its way into LDS); other Cout (27 * Cout <= 1024) by direct f32 accumulation. */
size_t disyolo_conv_first_wgrad_workspace(int B, int H, int W, int Cout);
int disyolo_conv_first_wgrad(const float* images, const void* dy, float* dw, int B, int H, int W,
                             int Cout, void* workspace, size_t workspace_bytes, void* stream);

/* first-layer helpers for the MFMA weight gradient: images f32 [pixels,3] -> bf16 [pixels,8]
 * (zero padded channels), and a pitched f32 copy used to drop the padded rows of its result */
int disyolo_image_pad8(const float* images, void* out_bf16, int64_t pixels, void* stream);
int disyolo_copy2d_f32(const float* src, float* dst, int rows, int cols, int src_ld, int dst_ld,
                       void* stream);

/* f32 HWIO master -> packed bf16 operands.  w_fwd [Cout][k*k*Cin] (may be NULL); w_dgrad
 * (may be NULL) [Cin][k*k*cout_pad] with taps flipped and zero columns for co >= Cout, i.e.
 * the forward operand of the data-gradient conv over a dy padded to cout_pad channels. */
int disyolo_pack_weights(const float* w_hwio, void* w_fwd, void* w_dgrad, int ksize, int Cin,
                         int Cout, int cout_pad, void* stream);

/* the same for many layers in ONE launch (re-pack after every optimizer step): the caller
 * builds a table with pack_table_build (host memory, pack_table_bytes(njobs) bytes), copies it
 * to the device once, and calls pack_all each step */
typedef struct disyolo_pack_job {
  const float* w_hwio;
  void* w_fwd;
  void* w_dgrad;      /* or NULL */
  int32_t ksize, Cin, Cout, cout_pad;
} disyolo_pack_job;
size_t disyolo_pack_table_bytes(int njobs);
int disyolo_pack_table_build(const disyolo_pack_job* jobs, int njobs, void* host_table, int* total_blocks);
int disyolo_pack_all(const void* device_table, int njobs, int total_blocks, void* stream);

/* ---- batch normalisation (yolo/yolo3_net_pos.py:71-107) ---- */
/* stats partials -> batch mean / population variance; scale = gamma*rsqrt(var+eps),
 * shift = beta - mean*scale; moving <- decay*moving + (1-decay)*batch (:93-96). */
int disyolo_bn_finalize(const float* stats, int rows, int C, int64_t count, const float* gamma,
                        const float* beta, float* moving_mean, float* moving_var, float decay,
                        float eps, float* scale, float* shift, float* mean, float* rstd,
                        void* stream);
/* SyncBN building blocks (data-parallel option; the reference is single-GPU): the phases of
 * bn_finalize / bn_act_bwd as separate calls, so that a caller can add the per-channel f64 sums [C][2] up over
 * the ranks (one small all-reduce) between them.  Forward: conv partials -> bn_partial_sums -> (all-reduce) ->
 * bn_finalize_sums(count = elements per channel over ALL ranks).  Backward: bn_bwd_reduce -> (all-reduce of a
 * copy) -> bn_bwd_apply_sums: dgamma/dbeta stay this rank's sums (the gradient exchange adds the ranks up), dx
 * uses the global ones.  With one rank and no all-reduce the results equal bn_finalize / bn_act_bwd. */
int disyolo_bn_partial_sums(const float* partials, int rows, int C, double* sums, void* stream);
int disyolo_bn_finalize_sums(const double* sums, int C, int64_t count, const float* gamma, const float* beta,
                             float* moving_mean, float* moving_var, float decay, float eps, float* scale,
                             float* shift, float* mean, float* rstd, void* stream);
int disyolo_bn_bwd_reduce_rows(int64_t rows, int C);   /* workspace of bn_bwd_reduce: rows x C x 2 floats */
int disyolo_bn_bwd_reduce(const void* dy, const void* x, const float* scale, const float* shift,
                          const float* mean, const float* rstd, int64_t rows, int C, float alpha, double* sums,
                          void* workspace, size_t workspace_bytes, void* stream);
/* workspace of bn_bwd_apply_sums: 2 x C floats */
int disyolo_bn_bwd_apply_sums(const void* dy, const void* x, const float* scale, const float* shift,
                              const float* mean, const float* rstd, const double* local_sums,
                              const double* global_sums, int64_t count, void* dx, float* dgamma, float* dbeta,
                              int64_t rows, int C, float alpha, void* shortcut_grad, int shortcut_accumulate,
                              void* workspace, size_t workspace_bytes, void* stream);
/* (sum, sum of squares) partials of a materialised bf16 [rows,C] conv output, in the layout
 * bn_finalize consumes: stats f32 [disyolo_colstats_rows(rows,C)][C][2] */
int disyolo_colstats_rows(int64_t rows, int C);
int disyolo_colstats(const void* x, float* stats, int64_t rows, int C, void* stream);
/* locked / inference BN folded to scale/shift from the moving statistics (:81,:101) */
int disyolo_bn_fold(const float* gamma, const float* beta, const float* moving_mean,
                    const float* moving_var, float eps, float* scale, float* shift, int C,
                    void* stream);
/* y = leaky(x*scale + shift) [+ residual], bf16 [rows,C] */
int disyolo_bn_act_fwd(const void* x, const float* scale, const float* shift, const void* residual,
                       void* y, int64_t rows, int C, float alpha, void* stream);
/* backward of y = leaky(gamma*xhat + beta), training statistics.  dy, x bf16 [rows,C];
 * writes dx bf16 and dgamma/dbeta f32.  workspace: disyolo_bn_act_bwd_workspace bytes.
 * shortcut_grad (bf16 [rows,C] or NULL): the gradient buffer of the layer a residual shortcut comes from
 * (res_conv_bn, :148-151): it receives dy (shortcut_accumulate = 0) or dy + itself (1) in the same pass that
 * reads dy for dx -- what disyolo_add_bf16(dy, shortcut_grad) would do in a launch of its own. */
size_t disyolo_bn_act_bwd_workspace(int64_t rows, int C);
int disyolo_bn_act_bwd(const void* dy, const void* x, const float* scale, const float* shift,
                       const float* mean, const float* rstd, void* dx, float* dgamma, float* dbeta,
                       int64_t rows, int C, float alpha, void* shortcut_grad, int shortcut_accumulate,
                       void* workspace, size_t workspace_bytes, void* stream);
/* the same when the per-channel sums (sum g, sum g*xhat) over disjoint row sets are already in
 * `partials` f32 [part_rows][C][2]: written by the data-gradient conv that produced dy, with
 * DISYOLO_CONV_BN_BWD_STATS (part_rows = disyolo_conv2d_stats_rows of that conv). */
size_t disyolo_bn_act_bwd_partials_workspace(int C);
int disyolo_bn_act_bwd_partials(const void* dy, const void* x, const float* scale, const float* shift,
                                const float* mean, const float* rstd, void* dx, float* dgamma,
                                float* dbeta, int64_t rows, int C, float alpha, const float* partials,
                                int part_rows, void* shortcut_grad, int shortcut_accumulate, void* workspace,
                                size_t workspace_bytes, void* stream);
/* backward of a LOCKED layer (conv_bn / res_conv_bn with lock=True, yolo/yolo3_net_pos.py:76-81,134-136,148-151): the
 * layer normalises with its moving statistics even in training, so with scale = gamma*rsqrt(moving_var+eps),
 * shift = beta - moving_mean*scale (disyolo_bn_fold) and z = x*scale + shift its backward has no batch-statistics
 * terms and no parameter gradients:  dx = bf16(scale_c * (dy * (z > 0 ? 1 : alpha))), f32 math on bf16 [rows,C]
 * operands.  x is the layer's conv output (the pre-activation decides the branch, not the stored activation, which
 * for a residual layer has the shortcut folded in).  shortcut_grad / shortcut_accumulate as in disyolo_bn_act_bwd.
 * dx == dy (in place) is allowed; shortcut_grad must alias none of dy, x, dx.  No workspace; C % 8 == 0. */
int disyolo_bn_frozen_bwd(const void* dy, const void* x, const float* scale, const float* shift, void* dx,
                          int64_t rows, int C, float alpha, void* shortcut_grad, int shortcut_accumulate,
                          void* stream);

/* ---- small data-movement ops of the backward pass ---- */
/* dst[b,y,x,c] = sum of the 2x2 block of src (gradient of resize_nearest_neighbor x2),
 * reading channels [c_off, c_off+C) of a src row of src_C channels; bf16. */
int disyolo_upsample2x_bwd(const void* src, void* dst, int B, int Hs, int Ws, int src_C, int c_off,
                           int C, int accumulate, void* stream);
/* column sums of a bf16 [rows,C] matrix -> f32 out[0:out_C] (bias gradient; out_C <= C) */
size_t disyolo_colsum_workspace(int64_t rows, int C);
int disyolo_colsum(const void* x, float* out, int64_t rows, int C, int out_C, void* workspace,
                   size_t workspace_bytes, void* stream);

/* ---- detection decode + filter (interpret_output / filter_detections,
 *      yolo/yolo3_net_pos.py:465-628,940-952) ---- */
/* logits: three f32 tensors [B,g,g,3,5+C] in the reference's scale order (S/8, S/16, S/32
 * grids).  anchors: host pointer to 18 floats (w,h)x9 in pixels.  Writes detections f32
 * [B,max_det,6] rows (y1,x1,y2,x2,classid,score), score-descending, zero padded, and
 * det_count int32 [B].  workspace: disyolo_detect_workspace bytes; it starts with the decode results
 * boxes float4 [B][NC], scores f32 [B][NC], classes i32 [B][NC] (NC candidates per image).
 * 1 <= num_class <= 80, max_det <= 64.  Up to 16 classes a block per (image, class) compacts its own
 * candidate list; above 16 one pass per image buckets the candidates by class and the greedy NMS runs
 * per class segment, so work and workspace do not grow with B*num_class*NC. */
size_t disyolo_detect_workspace(int B, int S, int num_class);
int disyolo_detect(const float* logits3, const float* logits2, const float* logits1, int B, int S,
                   int num_class, const float* anchors_host, const float* clip_window,
                   float obj_thresh, float nms_thresh, int max_det, float* detections,
                   int32_t* det_count, void* workspace, size_t workspace_bytes, void* stream);
/* the same filter on a net of H x W pixels (both positive multiples of 32): head grids (H/8, W/8),
 * (H/16, W/16), (H/32, W/32), logits [B,gh,gw,3,5+C], candidates in scale, y, x, anchor order; box x and w
 * are normalised by gw / W, y and h by gh / H.  disyolo_detect is its H = W = S call. */
size_t disyolo_detect_workspace_hw(int B, int H, int W, int num_class);
int disyolo_detect_hw(const float* logits3, const float* logits2, const float* logits1, int B, int H, int W,
                      int num_class, const float* anchors_host, const float* clip_window,
                      float obj_thresh, float nms_thresh, int max_det, float* detections,
                      int32_t* det_count, void* workspace, size_t workspace_bytes, void* stream);
/* ... with the choice of which candidates with score > obj_thresh (on the clipped boxes, :558) survive:
 *   DISYOLO_NMS_PER_CLASS  Method 1 (:564-592), what disyolo_detect / disyolo_detect_hw run: greedy NMS per arg-max class,
 *                          then the max_det best survivors;
 *   DISYOLO_NMS_AGNOSTIC   Method 2 (:594-605): ONE greedy NMS over all of an image's candidates whatever their class --
 *                          visited by descending score, ties to the lower candidate index, dropped iff the IoU with an
 *                          already kept one is > nms_thresh, at most max_det kept;
 *   DISYOLO_NMS_NONE       nms=False (:518, 585): the max_det highest scores, ties to the lower candidate index.
 * Any other nms_mode: DISYOLO_E_ARG.  Same outputs, same workspace (disyolo_detect_workspace_hw) in every mode.  The two
 * image-wide modes run one block per image; its candidate list sits in registers up to disyolo_detect_list_capacity()
 * candidates above the threshold (a whole 576 x 576 image) and in the workspace beyond -- the same result either way. */
#define DISYOLO_NMS_PER_CLASS 0
#define DISYOLO_NMS_AGNOSTIC 1
#define DISYOLO_NMS_NONE 2
int disyolo_detect_list_capacity(void);
int disyolo_detect_nms_hw(const float* logits3, const float* logits2, const float* logits1, int B, int H, int W,
                          int num_class, const float* anchors_host, const float* clip_window,
                          float obj_thresh, float nms_thresh, int max_det, int nms_mode, float* detections,
                          int32_t* det_count, void* workspace, size_t workspace_bytes, void* stream);
/* Per-net limits: a net takes up to DISYOLO_MAX_BOXES ground-truth boxes and writes up to DISYOLO_MAX_DET detections per
 * image.  The entry points above keep their limit of 64; the _x forms below (and disyolo_yolo_loss_hw, disyolo_mask_rois_hw,
 * disyolo_shuffle_perm, widened in place) take the whole range, and compute the same bits where both forms take a size. */
#define DISYOLO_MAX_BOXES 256
#define DISYOLO_MAX_DET 256
/* disyolo_detect_nms_hw for 1 <= max_det <= DISYOLO_MAX_DET, every nms_mode: the same rows, zero padding and det_count
 * (score descending, ties to the lower candidate index).  The workspace is disyolo_detect_workspace_x's, which grows with
 * max_det above 64 (the kept lists per (image, class)); 0 for sizes the filter refuses.  Up to 16 classes the survivors merge
 * by rank in LDS while num_class * max_det <= 512 and by the k-way merge of the longer class lists beyond -- also at
 * max_det <= 64, where disyolo_detect_nms_hw refuses num_class <= 16 with num_class * max_det > 512. */
size_t disyolo_detect_workspace_x(int B, int H, int W, int num_class, int max_det);
int disyolo_detect_x(const float* logits3, const float* logits2, const float* logits1, int B, int H, int W,
                     int num_class, const float* anchors_host, const float* clip_window,
                     float obj_thresh, float nms_thresh, int max_det, int nms_mode, float* detections,
                     int32_t* det_count, void* workspace, size_t workspace_bytes, void* stream);

/* ---- YOLO loss + gradient (loss_yolo, yolo/yolo3_net_pos.py:631-747) ---- */
/* labels: f32 [B,g,g,3,5+C] per scale (yolo3, yolo2, yolo1); true_boxes f32 [B,20,5].
 * dlogits: bf16 [B,g,g,32] per scale = d(loss)/d(logits) (already divided by B), rows padded
 * with zeros from 3*(5+C) to 32 channels (DISYOLO_GRAD_LD) so they feed the MFMA convs.
 * losses f32[8]: obj, noobj, class, xy, wh, (conf, coord, yolo_total). */
size_t disyolo_yolo_loss_workspace(int B, int S, int num_class);
int disyolo_yolo_loss(const float* const logits[3], const float* const labels[3],
                      const float* true_boxes, int max_boxes, int B, int S, int num_class,
                      const float* anchors_host, float ignore_thresh, const float scales[4],
                      void* const dlogits[3], float* losses, void* workspace,
                      size_t workspace_bytes, void* stream);
/* the same loss for class lists whose rows do not fit 32 channels: 1 <= num_class <= 80, dlogits bf16
 * [B,g,g,dlogits_ld] per scale with dlogits_ld a multiple of 32, 3*(5+num_class) <= dlogits_ld <= 256 (the
 * head conv's padded channel count); channels [3*(5+num_class), dlogits_ld) are written as zeros.  Same
 * loss terms, losses[8] and workspace (disyolo_yolo_loss_workspace) as disyolo_yolo_loss; one launch for the
 * three scales plus the fixed-order final sum, the same bits in every run. */
int disyolo_yolo_loss_wide(const float* const logits[3], const float* const labels[3],
                           const float* true_boxes, int max_boxes, int B, int S, int num_class,
                           int dlogits_ld, const float* anchors_host, float ignore_thresh,
                           const float scales[4], void* const dlogits[3], float* losses,
                           void* workspace, size_t workspace_bytes, void* stream);
/* both losses on a net of H x W pixels (positive multiples of 32): labels, logits and dlogits
 * [B,gh,gw,...] per scale with (gh, gw) = (H/8, W/8), (H/16, W/16), (H/32, W/32); grid_factor = [gw, gh],
 * net_factor = [W, H] as in the reference (:646, :709-718).  dlogits_ld = 0 runs the 32-channel kernel of
 * disyolo_yolo_loss, any other value the wide one; those two are the H = W = S calls of this one, with max_boxes <= 64.
 * This one takes 1 <= max_boxes <= DISYOLO_MAX_BOXES: above 64 an instance of the same kernel that stages 256 true boxes
 * runs -- the same arithmetic, partial layout and summation order. */
size_t disyolo_yolo_loss_workspace_hw(int B, int H, int W, int num_class);
int disyolo_yolo_loss_hw(const float* const logits[3], const float* const labels[3],
                         const float* true_boxes, int max_boxes, int B, int H, int W, int num_class,
                         int dlogits_ld, const float* anchors_host, float ignore_thresh,
                         const float scales[4], void* const dlogits[3], float* losses,
                         void* workspace, size_t workspace_bytes, void* stream);

/* ---- position-sensitive RoI assembly (yolo/yolo3_net_pos.py:750-938) ---- */
/* RoI selection for the mask loss (:757-796): detections [B,max_det,6], true_boxes [B,G,5],
 * perm_det int32 [B,max_det] / perm_gt int32 [B,G] replace tf.random_shuffle (:781-782).
 * Writes rois int32 [B,DISYOLO_ROI_MAX,DISYOLO_ROI_W_K(k)] (positive RoIs first: the k+1 bin edges
 * per axis on the S/2 grid after tf.round, assigned GT row, pixel area) and roi_count [B].
 * k = 3, 5 or 7; disyolo_mask_rois is the k = 3 case (rows of DISYOLO_ROI_W words). */
int disyolo_mask_rois_k(const float* detections, int max_det, const float* true_boxes, int G,
                        const int32_t* perm_det, const int32_t* perm_gt, int B, int map_size, int k,
                        int n_det, int n_gt, float iou_thresh, int32_t* rois, int32_t* roi_count,
                        void* stream);
int disyolo_mask_rois(const float* detections, int max_det, const float* true_boxes, int G,
                      const int32_t* perm_det, const int32_t* perm_gt, int B, int map_size,
                      int n_det, int n_gt, float iou_thresh, int32_t* rois, int32_t* roi_count,
                      void* stream);
/* RoI selection on a score map of map_h x map_w: y-coordinates are scaled by map_h, x-coordinates by map_w,
 * each through tf.round; bin edges per axis; the area is the pixel count clipped to the map.
 * disyolo_mask_rois_k is its map_h = map_w call.  max_det <= DISYOLO_MAX_DET, G <= DISYOLO_MAX_BOXES: with either above 64
 * a wave builds the trimmed row lists with ordered ballots and takes each RoI's IoU arg-max across its lanes (first maximum
 * wins, NaN never wins); up to 64 the single-lane form runs as before.  The same rows either way. */
int disyolo_mask_rois_hw(const float* detections, int max_det, const float* true_boxes, int G,
                         const int32_t* perm_det, const int32_t* perm_gt, int B, int map_h, int map_w, int k,
                         int n_det, int n_gt, float iou_thresh, int32_t* rois, int32_t* roi_count,
                         void* stream);
/* tf.random_shuffle replacement (:781-782): uniformly random permutations perm_det int32
 * [B,n_det], perm_gt int32 [B,n_gt] from a counter-based hash of (seed, *step_counter, image);
 * step_counter (device int64, may be NULL) makes every replay of a recorded step reshuffle.  n_det, n_gt <= 256; the keys and
 * the rank rule do not depend on which of the two block sizes (64 threads up to n = 64, 256 beyond) ranks them. */
int disyolo_shuffle_perm(int32_t* perm_det, int n_det, int32_t* perm_gt, int n_gt, int B, uint32_t seed,
                         const int64_t* step_counter, void* stream);
/* masked BCE over assembled logits + gradient wrt the score maps (:799-858).
 * k = 3, 5 or 7; score f32 [B,Sm,Sm,k*k]; rois from disyolo_mask_rois_k with the same k;
 * true_masks uint8 [B,G,2Sm,2Sm]; dscore bf16 [B,Sm,Sm,P] with P = round_up(k*k, 32) (32 for
 * k = 3, 5; 64 for k = 7: conv82's padded output pitch), channels k*k..P-1 written as zeros;
 * loss f32[1] = mask_scale * mean_b(mean_r(sum BCE / area)). */
size_t disyolo_psroi_loss_workspace(int B, int map_size);
int disyolo_psroi_loss(const float* score, const uint8_t* true_masks, int G, const int32_t* rois,
                       const int32_t* roi_count, int B, int map_size, int k, float mask_scale,
                       void* dscore, float* loss, void* workspace, size_t workspace_bytes,
                       void* stream);
/* disyolo_psroi_loss at any mask subnet stride: true_masks uint8 [B,G,s*Sm,s*Sm] sampled at
 * [::s, ::s] (TF's legacy bilinear resize at an exact integer factor; identity at s = 1).
 * mask_stride s = 1, 2 or 4 (score maps at S, S/2, S/4); disyolo_psroi_loss is its s = 2 case. */
int disyolo_psroi_loss_s(const float* score, const uint8_t* true_masks, int G, const int32_t* rois,
                         const int32_t* roi_count, int B, int map_size, int mask_stride, int k,
                         float mask_scale, void* dscore, float* loss, void* workspace,
                         size_t workspace_bytes, void* stream);
/* disyolo_psroi_loss_s on a score map of map_h x map_w: score f32 [B,map_h,map_w,k*k], true_masks uint8
 * [B,G,s*map_h,s*map_w], dscore bf16 [B,map_h,map_w,P]; rois from disyolo_mask_rois_hw with the same map. */
size_t disyolo_psroi_loss_workspace_hw(int B, int map_h, int map_w);
int disyolo_psroi_loss_hw(const float* score, const uint8_t* true_masks, int G, const int32_t* rois,
                          const int32_t* roi_count, int B, int map_h, int map_w, int mask_stride, int k,
                          float mask_scale, void* dscore, float* loss, void* workspace,
                          size_t workspace_bytes, void* stream);
/* The mask loss on more than DISYOLO_ROI_MAX RoIs per image (the reference's `[:7]` and `[:3]`, :783, as two counts of the
 * net).  The entry points above keep their table of DISYOLO_ROI_MAX rows; the _x forms take a table of roi_cap rows,
 * n_det + n_gt <= roi_cap <= DISYOLO_ROI_CAP, with the same row layout: positives first in RoI order, rows from
 * roi_count[b] on zero.  A count above the number of non-zero rows takes them all.  On a table both forms can take, the
 * selection writes the same rows and the loss the same dscore bits.
 * disyolo_mask_rois_x: rois int32 [B,roi_cap,DISYOLO_ROI_W_K(k)]; one block of sixteen waves per image (ordered compaction
 * for the trimmed lists, the pick and the positives; the IoU arg-max of an RoI across a wave's lanes).
 * disyolo_psroi_loss_x: every block culls the table to the rows that meet its 256 pixels and walks those alone, in RoI
 * order; its workspace holds one f32 partial per (block, table row). */
#define DISYOLO_ROI_CAP 512
int disyolo_mask_rois_x(const float* detections, int max_det, const float* true_boxes, int G,
                        const int32_t* perm_det, const int32_t* perm_gt, int B, int map_h, int map_w, int k,
                        int n_det, int n_gt, float iou_thresh, int roi_cap, int32_t* rois, int32_t* roi_count,
                        void* stream);
size_t disyolo_psroi_loss_workspace_x(int B, int map_h, int map_w, int roi_cap);
int disyolo_psroi_loss_x(const float* score, const uint8_t* true_masks, int G, const int32_t* rois,
                         const int32_t* roi_count, int roi_cap, int B, int map_h, int map_w, int mask_stride, int k,
                         float mask_scale, void* dscore, float* loss, void* workspace,
                         size_t workspace_bytes, void* stream);
/* inference assembly (val_test, :862-938): masks f32 [B,max_det,Sm,Sm] = sigmoid(selected
 * channel) inside the box, 0.5 outside; keep int32 [B,max_det] = 1 for rows with h>0 and w>0.
 * k = 3, 5 or 7; score f32 [B,Sm,Sm,k*k]. */
int disyolo_psroi_assemble(const float* score, const float* detections, int B, int max_det,
                           int map_size, int k, float* masks, int32_t* keep, void* stream);
/* the assembly on a score map of map_h x map_w: masks f32 [B,max_det,map_h,map_w]; y scaled by map_h, x by map_w */
int disyolo_psroi_assemble_hw(const float* score, const float* detections, int B, int max_det,
                              int map_h, int map_w, int k, float* masks, int32_t* keep, void* stream);

/* evaluate()'s per-image mask post-processing (calculate_test_map.py:237-262), the caller side
 * of `evaluation`: for each of the image's n detections the crop [cy1:cy2, cx1:cx2] of its
 * size x size f32 mask (disyolo_psroi_assemble output) is resized to (y2-y1) x (x2-x1) with
 * cv2.resize(INTER_LINEAR) semantics, thresholded (> 0.5) and pasted at [y1:y2, x1:x2] of an
 * image_h x image_w mask.  rects: int32 [n][8] = cy1,cx1,cy2,cx2, y1,x1,y2,x2 (host side:
 * np.around(box*size) and correct_yolo_boxes, :121-138,244-251); a detection with an empty crop
 * or destination contributes nothing.  full_masks uint8 [n][image_h][image_w] or NULL; merged
 * uint8 [image_h][image_w] = class id + 1 of the LAST detection covering the pixel (:258-266). */
int disyolo_mask_paste(const float* masks, int n, int size, const int32_t* rects,
                       const int32_t* classids, int image_h, int image_w, uint8_t* full_masks,
                       uint8_t* merged, void* stream);
/* the paste from masks of map_h x map_w (disyolo_psroi_assemble_hw output): the crop rows are cy1,cy2 on map_h
 * and cx1,cx2 on map_w.  disyolo_mask_paste is its map_h = map_w call. */
int disyolo_mask_paste_hw(const float* masks, int n, int map_h, int map_w, const int32_t* rects,
                          const int32_t* classids, int image_h, int image_w, uint8_t* full_masks,
                          uint8_t* merged, void* stream);
/* the same paste for a whole batch of images in ONE launch, with the counts the mask AP and the mIoU need instead of the
 * full-resolution masks (which are never written).  One job per image:
 *   masks / rects / classids / image_h / image_w / merged: as in disyolo_mask_paste, n <= 64 rows; a row whose rect is all zero
 *     (not kept, empty crop or destination) contributes nothing, and so does a row whose crop leaves the size x size mask;
 *   gt uint8 [ng][image_h][image_w] (0 / 1) with gt_class int32 [ng]: the image's ground-truth instances, ng >= 0, no upper bound;
 *   true_map uint8 [image_h][image_w] or NULL: when given, the 4x4 confusion counts of (true_map, merged) are added to `conf`
 *     (int64 [16], disyolo_confusion16's layout and rule: values >= 4 are ignored) in the same pass;
 *   counts int32 [n][1 + ng], ZEROED BY THE CALLER: column 0 receives the detection's pasted pixel count, column 1 + g its
 *     intersection with instance g when gt_class[g] == classids[k]; other pairs stay zero.
 * Integer adds only: the values are the same in every run.  An image has at most 2^30 pixels.
 * The table exists twice: a HOST copy, which disyolo_paste_job_plan checks and completes (block0 = the job's first block in the
 * launch; it returns the number of blocks or a negative code), and the same bytes on the DEVICE (`jobs`), uploaded by the caller
 * after planning -- with the rects and class ids in the same copy if it likes.  The launch checks the host copy again (it never
 * reads device memory on the host) and fails with an error code, before any launch, on n > 64, a NULL table, njobs <= 0,
 * size <= 0, an unplanned table, or a true_map without conf. */
typedef struct disyolo_paste_job {
  const float* masks;        /* f32 [n][size][size] */
  const int32_t* rects;      /* [n][8] */
  const int32_t* classids;   /* [n] */
  const uint8_t* gt;         /* [ng][image_h][image_w], NULL when ng == 0 */
  const int32_t* gt_class;   /* [ng] */
  uint8_t* merged;           /* out [image_h][image_w] */
  const uint8_t* true_map;   /* [image_h][image_w] or NULL */
  int32_t* counts;           /* out [n][1 + ng] */
  int32_t n, ng, image_h, image_w;
  int32_t block0, reserved;  /* block0: written by disyolo_paste_job_plan */
} disyolo_paste_job;
/* sizeof(disyolo_paste_job) as this library was built (88): a binding checks its mirror against it */
size_t disyolo_paste_job_size(void);
int disyolo_paste_job_plan(disyolo_paste_job* jobs_host, int njobs);
int disyolo_mask_paste_iou_batch(const disyolo_paste_job* jobs_host, const disyolo_paste_job* jobs, int njobs, int size,
                                 int64_t* conf, void* stream);
/* the batched paste from masks of map_h x map_w; disyolo_mask_paste_iou_batch is its map_h = map_w call */
int disyolo_mask_paste_iou_batch_hw(const disyolo_paste_job* jobs_host, const disyolo_paste_job* jobs, int njobs, int map_h,
                                    int map_w, int64_t* conf, void* stream);
/* both for jobs of up to DISYOLO_MAX_DET rows (n <= 256): a pixel keeps one 64-bit cover word per 64 detections and walks the
 * words in order, so the last covering detection still owns the merged pixel across a word boundary; counts has the same
 * layout.  A table must be planned by the _x plan to be launched by the _x launch. */
int disyolo_paste_job_plan_x(disyolo_paste_job* jobs_host, int njobs);
int disyolo_mask_paste_iou_batch_x(const disyolo_paste_job* jobs_host, const disyolo_paste_job* jobs, int njobs, int map_h,
                                   int map_w, int64_t* conf, void* stream);
/* image_read of the test / validation drivers (calculate_test_map.py:149-176; utils/val_data.py:36-63):
 * rgb uint8 [image_h, image_w, 3] (device) -> out f32 [size, size, 3] (device): aspect-preserving
 * bilinear resize (cv2.resize INTER_LINEAR on the float32 image) centred in the letter box, padding
 * 127, / 255.  window_host (host, may be NULL) receives the clip window [top, left, bottom, right]. */
int disyolo_letterbox(const uint8_t* rgb, int image_h, int image_w, float* out, int size,
                      float* window_host, void* stream);
/* the letter box of a net of net_h x net_w pixels: out f32 [net_h, net_w, 3]; the width binds when
 * net_w / image_w < net_h / image_h; the window is normalised by (net_h, net_w).  disyolo_letterbox is its
 * net_h = net_w call. */
int disyolo_letterbox_hw(const uint8_t* rgb, int image_h, int image_w, float* out, int net_h, int net_w,
                         float* window_host, void* stream);
/* ---- tiled detection: an image larger than the net (csrc/tiles.hip, dis-yolo_amd/tiles.py; defined by tests/tiles_ref.py) ----
 * origins int32 [T, 2] = (y0, x0) of the tiles, row-major (tiles.plan_tiles); a tile is net_h x net_w pixels, net_w % 32 == 0.
 * Tables the kernels follow indices through are passed twice, like disyolo_paste_job tables: the `_host` copy is what the call
 * checks before any launch, the device copy (the same bytes, uploaded by the caller on `stream`) is what the kernel reads.
 *
 * tile_gather: rgb uint8 [image_h, image_w, 3] (device) -> out f32 [t1 - t0, net_h, net_w, 3] (device), tiles t0 .. t1 - 1 in
 * one launch: a pixel inside the image is (float)((double)v / 255.0) -- bit for bit disyolo_letterbox at scale 1 --, a pixel
 * outside it 127 through the same division, and a tile index >= T a whole pad tile (it fills the last batch of an image). */
int disyolo_tile_gather(const uint8_t* rgb, int image_h, int image_w, const int32_t* origins, int T, int t0, int t1, float* out,
                        int net_h, int net_w, void* stream);
/* masks f32 [n, map_h, map_w], rects int32 [n, 8] (disyolo_mask_paste's, the tile as the image) -> planes uint32
 * [n, net_h, net_w / 32]: bit i of word j of a row = the paste's bit at column 32 j + i.  A crop rect outside the map gives an
 * empty plane.  n = 0 is allowed. */
int disyolo_tile_paste_bits(const float* masks, int n, int map_h, int map_w, const int32_t* rects, int net_h, int net_w,
                            uint32_t* planes, void* stream);
/* pairs int32 [P, 2] = instance numbers (a, b) < N, inst_tile int32 [N] = each instance's tile < T -> counts int32 [P, 3] =
 * |A n R|, |B n R|, |A n B|, R = the two tiles' windows n the image.  Integer sums: order-independent. */
int disyolo_tile_seam_counts(const int32_t* pairs_host, const int32_t* pairs, int P, const int32_t* inst_tile_host,
                             const int32_t* inst_tile, int N, const int32_t* origins_host, const int32_t* origins, int T,
                             int image_h, int image_w, const uint32_t* planes, int net_h, int net_w, int32_t* counts,
                             void* stream);
/* groups int32 [G, 8] = {m0, m1, y1, x1, y2, x2, block0, off16} in rank order: members[m0 .. m1) int32 are the group's instances,
 * the box is in image pixels, block0 = the sum of disyolo_tile_compose_blocks(box area) over the groups before it, off16 * 16 the
 * group's offset in `arena` (room for the area rounded up to 16 bytes).  Writes the OR of the members cropped to the box as bytes
 * 0 / 1, row-major, and owner int32 [image_h, image_w] = 0 or 1 + the index of the LAST covering group (zeroed here, then
 * integer atomicMax: disyolo_mask_paste's rule, order-independent). */
int disyolo_tile_compose_blocks(int64_t area);
int disyolo_tile_compose(const int32_t* groups_host, const int32_t* groups, int G, const int32_t* members_host,
                         const int32_t* members, int M, const int32_t* inst_tile_host, const int32_t* inst_tile, int N,
                         const int32_t* origins_host, const int32_t* origins, int T, const uint32_t* planes, int net_h, int net_w,
                         int image_h, int image_w, uint8_t* arena, int64_t arena_bytes, int32_t* owner, void* stream);
/* tiled evaluation: pixel counts of merged groups against ground truth kept as cropped bit planes (evaluate.MAP.collect_tiled;
 * defined by tests/tiles_eval_ref.py).  groups int32 [G, 8] and arena (arena_bytes) are what disyolo_tile_compose took and
 * wrote: group g's mask is bytes 0 / 1, row-major over its box, at arena + 16 * off16 (only columns 2 .. 5 and 7 are read; the
 * padding behind a group's area is never counted).  gt int32 [ng, 8] = {y1, x1, y2, x2, classid, pitch, off, area}: instance
 * j's plane is cropped to its box, pitch >= ceil((x2 - x1) / 32) words per row from word `off` of gt_bits (gt_words words);
 * bit i of word k of row r is pixel (y1 + r, x1 + 32 k + i), bits past the box's last column are zero; classid and area are
 * the caller's.  pairs int32 [P, 3] = {g, j, block0}: j >= 0 asks for |mask_g n gt_j|, j = -1 for the group's own pixel count;
 * block0 = the sum of disyolo_tile_group_counts_blocks(area of the pair's rectangle) over the pairs before it, the rectangle
 * being the group's box (j = -1) or box n gt box; an empty rectangle takes one block, a large one at most 1024, which stride
 * over its 2048-pixel chunks.  counts int32 [P] is zeroed here, then
 * integer atomicAdd of per-block popcounts: order-independent.  P = 0 or G = 0 launches nothing. */
int disyolo_tile_group_counts_blocks(int64_t area);
int disyolo_tile_group_counts(const int32_t* groups_host, const int32_t* groups, int G, const uint8_t* arena, int64_t arena_bytes,
                              const int32_t* gt_host, const int32_t* gt, int ng, const uint32_t* gt_bits, int64_t gt_words,
                              const int32_t* pairs_host, const int32_t* pairs, int P, int image_h, int image_w, int32_t* counts,
                              void* stream);
/* ---- instance measurement: length, width and area of merged instances (csrc/measure.hip, dis-yolo_amd/measure.py; defined by
 * tests/measure_ref.py) ----
 * groups int32 [G, 8] and arena (arena_bytes) are what disyolo_tile_compose took and wrote: group g's mask is its crop, bh x bw
 * bytes, row-major, at arena + 16 * off16; a non-zero byte is foreground (columns 2 .. 7 are read).  Every entry point checks
 * the host copy before any launch: box sides in 0 .. 32767, block0 = the sum of disyolo_tile_compose_blocks(box area) over the
 * groups before, crops inside arena_bytes in table order without overlap; otherwise DISYOLO_E_ARG.  Outputs lie in the arena's
 * layout, one element per pixel (buffers of arena_bytes elements); the elements between two crops are never read and never
 * written.  None allocates or synchronises.  G = 0 launches nothing.
 *
 * measure_d2: d2 int32 = the exact squared Euclidean distance of a foreground pixel to the nearest background pixel, a
 * one-pixel ring around the crop counting as background; 0 on background.  colg uint16 is scratch (column distances). */
int disyolo_measure_d2(const int32_t* groups_host, const int32_t* groups, int G, const uint8_t* arena, int64_t arena_bytes,
                       uint16_t* colg, int32_t* d2, void* stream);
/* `chunk` iterations of Zhang-Suen thinning (two launches each) for all groups, numbered it0 .. it0 + chunk - 1; the caller
 * starts with it0 = 0 and continues with it0 += chunk while a word of the last flags row is non-zero.  skel and tmp are byte
 * buffers; after every call skel holds each group's state (bytes 0 / 1), and once a group's iteration deleted nothing its blocks
 * return at once and skel keeps its skeleton, whatever iteration it stopped at.  flags int32 [(chunk + 1) G]: row 1 + i, word g
 * is non-zero when iteration it0 + i deleted a pixel of group g (vector atomic or); row 0 is the last row of the call before
 * (it0 = 0: all live).  iters int32 [G]: the iterations each group ran, counting the one that deleted nothing (zeroed at
 * it0 = 0).  The arena is only read.  The result does not depend on `chunk`. */
int disyolo_measure_thin(const int32_t* groups_host, const int32_t* groups, int G, const uint8_t* arena, int64_t arena_bytes,
                         uint8_t* skel, uint8_t* tmp, int32_t* flags, int32_t* iters, int it0, int chunk, void* stream);
/* counts int64 [G, 8] = {area, skel_px, n_orth, n_diag, n_end, max_d2, max_d2_skel, 0} (zeroed here, then integer atomics: exact
 * and order-independent); sum_sqrt f64 [G] = the sum over the skeleton of sqrt(d2), through partials f64 [partials_len >= the
 * plan's block count]: per-block sums in a fixed order, added per group in block order -- no float atomic, the same bits on
 * every run. */
int disyolo_measure_counts(const int32_t* groups_host, const int32_t* groups, int G, const uint8_t* arena, int64_t arena_bytes,
                           const uint8_t* skel, const int32_t* d2, int64_t* counts, double* partials, int64_t partials_len,
                           double* sum_sqrt, void* stream);
/* ---- the graph of a skeleton: links, branches, rows per branch, spur pruning (csrc/skeleton.hip, measure.skeleton_graph;
 * defined by tests/skeleton_ref.py; integers only) ----
 * The groups table, its check on the host copy before any launch, the layout of every per-pixel buffer (arena_bytes elements,
 * the elements between two crops never read and never written) and G = 0 are as for disyolo_measure_*.  Neighbours are numbered
 * N, NE, E, SE, S, SW, W, NW = bits 0 .. 7.  None allocates or synchronises; no block waits for another.
 *
 * classify: links uint8 = the link bits of every pixel of src (a non-zero byte is a skeleton pixel): adjacent in a row or a
 * column, or diagonal with neither pixel completing the 2x2 square set; 0 off the skeleton.  When skel != src, skel gets the
 * 0 / 1 state of src as well (the copy a pruning starts from); skel == src writes links only. */
int disyolo_skeleton_classify(const int32_t* groups_host, const int32_t* groups, int G, int64_t arena_bytes, const uint8_t* src,
                              uint8_t* skel, uint8_t* links, void* stream);
/* labels int32: on a pixel of degree <= 2 the smallest index y bw + x of its branch (the component under links between two
 * such pixels), -1 on every other pixel of the crop.  Three launches: init, merge (union-find, the larger root hung under the
 * smaller by an atomic min: the result does not depend on the order of arrival), flatten. */
int disyolo_skeleton_label(const int32_t* groups_host, const int32_t* groups, int G, int64_t arena_bytes, const uint8_t* skel,
                           const uint8_t* links, int32_t* labels, void* stream);
/* rows int64 [capacity, 12], in any order: {group, root, px, n_orth, n_diag, n_end, n_attach, sum_q8, max_d2, min_d2, spur, 0}
 * of every branch, spur from M2 = twice min_branch_px (0 .. 65534).  ctrl int32 [1 + G]: word 0 = the number of branches, which
 * counts beyond `capacity` while nothing is written there (the caller repeats the call with more rows); word 1 + g is non-zero
 * when group g has a spur.  junctions int64 [G, 4] = {junction_px, jj_orth, jj_diag, n_branches}.  rowid int32 per pixel is
 * scratch (a root's row number).  ctrl and junctions are zeroed here; integer atomics only: exact and order-independent. */
int disyolo_skeleton_rows(const int32_t* groups_host, const int32_t* groups, int G, int64_t arena_bytes, const uint8_t* links,
                          const int32_t* labels, const int32_t* d2, int32_t* rowid, int64_t* rows, int64_t capacity, int M2,
                          int32_t* ctrl, int64_t* junctions, void* stream);
/* zeroes the bytes of skel whose branch's row has its spur bit set (labels, rowid, rows as disyolo_skeleton_rows left them, with
 * a capacity that held every row) */
int disyolo_skeleton_prune(const int32_t* groups_host, const int32_t* groups, int G, int64_t arena_bytes, const int32_t* labels,
                           const int32_t* rowid, const int64_t* rows, int64_t capacity, uint8_t* skel, void* stream);
/* ---- the traced skeleton graph: nodes, ordered branches, edges, profiles (csrc/trace.hip, measure.skeleton_trace; defined by
 * tests/trace_ref.py; integers only) ----
 * They go on from what disyolo_skeleton_* left of the final skeleton: links, labels, rowid, rows; d2 is disyolo_measure_d2's.  The
 * groups table, its check on the host copy before any launch, the layout of the per-pixel buffers and G = 0 are as above; the
 * arena must hold fewer than 2^31 elements (positions are int32).  None allocates or synchronises; no block waits for another, and
 * apart from the union-find none reads what another block writes in the same launch.
 *
 * nodes: node_labels int32 = on a pixel of degree >= 3 the smallest index y bw + x of its node (the component under the links
 * between two such pixels), -1 on every other pixel of the crop.  nodes int64 [capacity, 8], in any order: {group, root, px,
 * sum_y, sum_x, max_d2, n_attach, 0}; ctrl int32 [1] = the number of nodes (zeroed here; it counts beyond `capacity` while nothing
 * is written there).  noderow int32 per pixel is scratch.  Five launches: init, merge, flatten, alloc, accumulate. */
int disyolo_trace_nodes(const int32_t* groups_host, const int32_t* groups, int G, int64_t arena_bytes, const uint8_t* links,
                        const int32_t* d2, int32_t* node_labels, int32_t* noderow, int64_t* nodes, int64_t capacity, int32_t* ctrl,
                        void* stream);
/* rank, rank_diag int32: on a pixel of degree <= 2 the steps from its branch's start and how many of them were diagonal links, -1
 * on every other pixel of the crop.  The start of a path is its end pixel with the smaller index, the start of a loop its root,
 * walked first to the linked neighbour with the smaller index.  The pixels of branches are compacted into ents int32
 * [capacity, 12], in any order (count int32 [1] = how many; zeroed here): {position in the arena, index in the crop, root, the two
 * in-branch neighbours and the two junction neighbours as arena positions or -1, flags, row number, group, d2, crop width}.  Then
 * list ranking by pointer jumping over the doubled states (entry, direction) between the two halves of nxt int32 [4 capacity] and
 * val int64 [4 capacity]: one launch per round, `rounds` >= log2 of the longest branch's pixel count.  3 + rounds launches. */
int disyolo_trace_rank(const int32_t* groups_host, const int32_t* groups, int G, int64_t arena_bytes, const uint8_t* links,
                       const int32_t* labels, const int32_t* d2, const int32_t* rowid, const int64_t* rows, int64_t rows_capacity,
                       int32_t* ents, int64_t capacity, int rounds, int32_t* nxt, int64_t* val, int32_t* count, int32_t* rank,
                       int32_t* rank_diag, void* stream);
/* edges int64 [edges_capacity, 12], row r = the branch of row r of disyolo_skeleton_rows: {group, root, end0_kind, end0_id,
 * end1_kind, end1_id, attach0_px, attach1_px, end0_px, end1_px, inner_diag, last_rank}.  End 0 is at rank 0, end 1 at the last rank.
 * kind 1: a node, id = its root, attach = the junction pixel linked to; kind 0: a free end, id = the end pixel, attach = -1; kind
 * 2: a loop, id = the root.  Every slot has one writer.  One launch over the list. */
int disyolo_trace_edges(const int32_t* groups_host, const int32_t* groups, int G, int64_t arena_bytes, const int32_t* ents,
                        const int32_t* count, int64_t capacity, const int32_t* rank, const int32_t* rank_diag,
                        const int32_t* node_labels, int64_t* edges, int64_t edges_capacity, void* stream);
/* profile int32 [capacity, 4]: every list entry writes {y, x, d2, rank_diag} at offsets[row] + rank (offsets int32 [n_rows]).
 * tprofile int32 [tprofile_len, 5] = {y, x, d2, cum_orth, cum_diag}, the trunk profiles by the host's plan: seg int32 [n_rows, 4] =
 * {first entry or -1, reversed, cum_orth and cum_diag at its first entry} per branch row, attach int32 [n_attach, 6] = {arena
 * position, entry, y, x, cum_orth, cum_diag} per junction pixel between two branches.  trunkrows int64 [G, 8] = {px, sum_q8,
 * max_d2, the position, y and x of its first occurrence, the last entry's cum_orth and cum_diag} of the entries tstart[g] ..
 * tstart[g + 1] (tstart int32 [G + 1]).  Two launches; entries outside the buffers are dropped, not written. */
int disyolo_trace_gather(const int32_t* groups_host, const int32_t* groups, int G, int64_t arena_bytes, const int32_t* ents,
                         const int32_t* count, int64_t capacity, const int32_t* rank, const int32_t* rank_diag, const int32_t* d2,
                         const int32_t* offsets, int64_t n_rows, int32_t* profile, const int32_t* seg, const int64_t* edges,
                         const int32_t* attach, int64_t n_attach, int32_t* tprofile, int64_t tprofile_len, const int32_t* tstart,
                         int64_t* trunkrows, void* stream);
/* ---- the shape of an instance: moment sums, tight box and bit quads; 8-connected parts; extents along K directions
 * (csrc/shape.hip, measure.instance_shapes; defined by tests/shape_ref.py; integers only) ----
 * groups, arena (arena_bytes), the check on the host copy before any launch, the layout of the per-pixel buffers (arena_bytes
 * elements, the elements between two crops never read and never written) and G = 0 are as for disyolo_measure_*; a non-zero byte
 * is foreground, everything outside a crop background.  None allocates or synchronises; no block waits for another; integer
 * atomics only: exact and order-independent.
 *
 * sums int64 [G, 16] = {n, Sy, Sx, Syy, Sxx, Sxy, ymin, ymax, xmin, xmax, Q1, Q2, Q3, Q4, QD, 0}, initialised here (a group
 * without foreground keeps ymin, ymax, xmin, xmax = bh, -1, bw, -1): the sums over the foreground of a pixel's crop coordinates
 * and their products, the tight box (inclusive), and the bit quads over the (bh + 1)(bw + 1) 2x2 windows of the crop padded by a
 * ring of background -- the windows with one / three / four pixels set, QD two on a diagonal, Q2 two otherwise.  With sides
 * <= 32767 every sum fits int64.  Two launches: the rows, then one over the arena in which a block walks 8 consecutive chunks of
 * the plan and issues one atomic per group among them and column (for the box only where it changes the row). */
int disyolo_shape_sums(const int32_t* groups_host, const int32_t* groups, int G, const uint8_t* arena, int64_t arena_bytes,
                       int64_t* sums, void* stream);
/* labels int32: on a foreground pixel the smallest index y bw + x of its 8-connected part, -1 on every other pixel of the crop.
 * parts int64 [G, 2] = {n_parts, largest_part_px} (zeroed here).  px int32 per pixel is scratch (a root's pixel count).  Five
 * launches: init (a pixel starts at the first pixel of its row run within its wave's 64 pixels), merge (union-find as
 * disyolo_skeleton_label, with path halving: the result does not depend on the order of arrival), flatten, count, roots. */
int disyolo_shape_parts(const int32_t* groups_host, const int32_t* groups, int G, const uint8_t* arena, int64_t arena_bytes,
                        int32_t* labels, int32_t* px, int64_t* parts, void* stream);
/* pminmax int32 [G, K, 2] = the minimum and maximum over the foreground of c_k x + s_k y for the K directions dirs int32 [K, 2] =
 * {c_k, s_k} (a unit vector in 2^-14; the table is made on the host, no kernel evaluates a cosine); (INT32_MAX, INT32_MIN) for a
 * group without foreground.  dirs_host is checked before any launch: K even in 2 .. 360 and |c|, |s| <= 16384 (the projection
 * then fits int32), otherwise DISYOLO_E_ARG.  Two launches: the rows, then one over the arena in which only boundary pixels
 * (foreground with a background 4-neighbour, which hold the same extrema) are projected and a block issues at most 2 K atomics,
 * none where the row already holds a value as good. */
int disyolo_shape_extents(const int32_t* groups_host, const int32_t* groups, int G, const uint8_t* arena, int64_t arena_bytes,
                          const int32_t* dirs_host, const int32_t* dirs, int K, int32_t* pminmax, void* stream);
/* ---- outlines of the crops of an arena (csrc/outline.hip; the definition is tests/outline_ref.py) --------------------------------
 * A boundary edge is (p, s): a foreground pixel and a side 0 = N, 1 = E, 2 = S, 3 = W whose neighbour across it is background
 * (outside the crop is background); its successor is the diagonal pixel ahead with side s - 1 if that pixel is foreground, else the
 * pixel ahead with side s, else p with side s + 1.  The cycles of the successor are the borders.  All three calls take the groups
 * table as disyolo_measure_d2 does and return DISYOLO_E_ARG for a bad table, a null pointer, 4 * arena_bytes >= 2^31 (an edge's key
 * in the arena is 4 (off + p) + s) or a capacity of 2^30 or more; they launch nothing for G = 0 or a plan without a block.
 *
 * disyolo_outline_edges: the list.  first int32 and sides uint8 in the arena's layout = a pixel's first list entry (-1 without one)
 * and the mask of its boundary sides; per entry (capacity of them, = the sum of the shapes' edges) ekey int32 = its key, nxt int32 =
 * its successor's entry, flag uint8 = 1: its predecessor belongs to another pixel | 2: to another side, aterm int32 = its term of the
 * shoelace sum.  work int64 [>= 10 * capacity].  ctrl int32 [4] (zeroed here) = the entries listed, the rows taken, bit 0: the list
 * overflowed | bit 1: the rows did, 0: the host reads it with the rows, nothing faults, and every later kernel returns at once when
 * a bit is set. */
int disyolo_outline_edges(const int32_t* groups_host, const int32_t* groups, int G, const uint8_t* arena, int64_t arena_bytes,
                          int32_t* first, uint8_t* sides, int32_t* ekey, int32_t* nxt, uint8_t* flag, int32_t* aterm,
                          int64_t capacity, int64_t* work, int64_t work_elems, int32_t* ctrl, void* stream);
/* the loops, after disyolo_outline_edges on the same buffers; part_labels = disyolo_shape_parts' labels of the arena.  rounds
 * launches of min-propagation give every entry its loop's smallest key, the cycle is cut in front of that edge, and rounds launches
 * of list ranking give the sums from an entry to the end: 2^rounds must reach the longest loop's edges.  rows int64
 * [rows_capacity, 12], one per loop in the order the key edges arrived (an atomic counter, ctrl[1]) = instance, key = 4 p + s in its
 * crop, n_edges, n_points, n_corners, area2 (> 0: an outer border), part, west = the key of the loop through the E side of the first
 * foreground pixel west of an outer loop's key pixel (-1: none), the smallest key of an E side, the runs of one owner (0: one pixel),
 * the run the chain starts with, 0.  eidx int32 [capacity, 3] = per entry its loop's row, its index among the loop's points and
 * among its corners. */
int disyolo_outline_loops(const int32_t* groups_host, const int32_t* groups, int G, const uint8_t* arena, int64_t arena_bytes,
                          const int32_t* part_labels, const int32_t* first, const uint8_t* sides, const int32_t* ekey,
                          const int32_t* nxt, const uint8_t* flag, const int32_t* aterm, int64_t capacity, int rounds, int64_t* work,
                          int64_t work_elems, int32_t* eidx, int64_t* rows, int64_t rows_capacity, int32_t* ctrl, void* stream);
/* the points and corners, after disyolo_outline_loops: plan int32 [rows_capacity, 8] per row of rows = where its points begin, where
 * its corners begin, rows columns 10 and 9, its crop's width, first arena element, x1, y1.  points int32 [n_points, 2] = (x, y) of the
 * pixel chain (cv2's CHAIN_APPROX_NONE border: the run of the start edge, then the others in reverse), corners int32 [n_corners, 2]
 * = the ring of turning corners on the corner grid, both in the image.  One writer per element; a place outside the buffers is
 * skipped. */
int disyolo_outline_gather(const int32_t* groups_host, const int32_t* groups, int G, int64_t arena_bytes, const int32_t* ekey,
                           const uint8_t* flag, const int32_t* eidx, int64_t capacity, const int32_t* ctrl, const int32_t* plan,
                           int64_t rows_capacity, int32_t* points, int64_t n_points, int32_t* corners, int64_t n_corners, void* stream);
/* semantic-segmentation accuracy of evaluate (calculate_test_map.py:303-346): adds the 4x4 pixel
 * confusion counts of two uint8 class maps (0 = background, 1..3 = classes; other values are
 * ignored) to conf int64 [16], conf[true*4 + pred]; the caller zeroes conf before the first image
 * and forms IoU_c = n_cc / (row_c + column_c - n_cc) at the end. */
int disyolo_confusion16(const uint8_t* true_map, const uint8_t* pred_map, int64_t n, int64_t* conf,
                        void* stream);
/* the same counts for nlabel labels (0 = background, 1..nlabel-1 = classes; 2 <= nlabel <= 81): adds to
 * conf int64 [nlabel*nlabel], conf[true*nlabel + pred]; values >= nlabel are ignored.  Integer adds only;
 * nlabel = 4 gives disyolo_confusion16's numbers. */
int disyolo_confusion_n(const uint8_t* true_map, const uint8_t* pred_map, int64_t n, int nlabel,
                        int64_t* conf, void* stream);

/* ---- optimizer (tf.train.AdamOptimizer.minimize, train_yolo3_mask.py:55) ---- */
/* TF-form Adam on a flat f32 arena; elements [0, n_decay) also receive the gradient of the
 * l2 regulariser (grad += l2*w; yolo/yolo3_net_pos.py:38).  step t >= 1. */
int disyolo_adam_step(float* w, const float* grad, float* m, float* v, int64_t n, int64_t n_decay,
                      float lr, float beta1, float beta2, float eps, float l2, int64_t t,
                      float grad_scale, void* stream);
/* same with the step count kept in device memory: uses t = *step_counter + 1 and then
 * increments the counter (nothing about the step lives on the host: replayable) */
int disyolo_adam_step_dev(float* w, const float* grad, float* m, float* v, int64_t n,
                          int64_t n_decay, float lr, float beta1, float beta2, float eps, float l2,
                          int64_t* step_counter, float grad_scale, void* stream);
/* same, with the learning rate read from device memory too (lr_dev f32[1]: a recorded step follows
 * the schedule of train_yolo3_mask.py:130-141 by rewriting one float), and -- when reg_loss_out is
 * not NULL -- the value of the l2 term of total_loss (yolo/yolo3_net_pos.py:38,61),
 * 0.5*l2*sum(w[0:n_decay]^2) of the weights BEFORE the update, produced by the same sweep
 * (workspace: disyolo_adam_fused_workspace(n) bytes; deterministic fixed-order partial sums) */
size_t disyolo_adam_fused_workspace(int64_t n);
int disyolo_adam_step_fused(float* w, const float* grad, float* m, float* v, int64_t n,
                            int64_t n_decay, const float* lr_dev, float beta1, float beta2, float eps,
                            float l2, int64_t* step_counter, float grad_scale, float* reg_loss_out,
                            void* workspace, size_t workspace_bytes, void* stream);
/* The same update as sweeps over slices of the variables + one finish (train_yolo3_mask.py:55 is one
 * op over all variables; the slices only choose WHEN each part of it runs): a recorded step sweeps a
 * slice as soon as its gradients are final, beside the rest of the backward pass.  Every sweep uses
 * t = *step_counter + 1 and writes disyolo_adam_sweep_parts(n) l2 partial sums to `parts` (NULL: none;
 * n_decay = how many leading elements of THIS slice are regularised); the finish sums the nparts
 * partials of all sweeps in order into reg_loss_out (NULL: skip) and increments the counter. */
int disyolo_adam_sweep_parts(int64_t n);
int disyolo_adam_sweep(float* w, const float* grad, float* m, float* v, int64_t n, int64_t n_decay,
                       const float* lr_dev, float beta1, float beta2, float eps, float l2,
                       const int64_t* step_counter, float grad_scale, float* parts, void* stream);
int disyolo_adam_finish(int64_t* step_counter, const float* parts, int nparts, float l2,
                        float* reg_loss_out, void* stream);
/* the finish that also files the step's total loss (get_total_loss, yolo/yolo3_net_pos.py:61: the four YOLO terms
 * [losses8[7]] + the mask term + the l2 term) into ring[t % ring_len], t = the counter before its increment.  The
 * reference fetches total_loss with every sess.run (train_yolo3_mask.py:216) and only accumulates it (:218); a host that
 * reads the ring every ring_len steps or less gets the same values without joining the device once per step.
 * reg_loss_in: the l2 term when this finish sums none (reg_loss_out NULL); NULL = 0. */
int disyolo_adam_finish_record(int64_t* step_counter, const float* parts, int nparts, float l2, float* reg_loss_out,
                               const float* losses8, const float* mask_loss, const float* reg_loss_in, float* ring,
                               int ring_len, void* stream);
/* 0.5*l2*sum(w[0:n]^2) -> out f32[1] (only needed when the loss value is logged) */
size_t disyolo_l2_workspace(int64_t n);
int disyolo_l2_loss(const float* w, int64_t n, float l2, float* out, void* workspace,
                    size_t workspace_bytes, void* stream);

/* dst (+)= src over n bf16 elements (n % 8 == 0): gradient accumulation at the residual
 * shortcuts (yolo/yolo3_net_pos.py:150) */
int disyolo_add_bf16(const void* src, void* dst, int64_t n, int accumulate, void* stream);

/* ---- training-data pipeline (utils/train_data.py:44-276, 321-531): the pixel work of defect_train.get() ----
 * polygon_mask: one annotated instance = npoly polygons (vertices px/py f32, polygon k = [poly_start[k],
 * poly_start[k+1]), poly_is_out[k] = 1 'out' / 0 'in' = hole) -> uint8 mask [image_h, image_w]:
 * skimage.draw.polygon per polygon in order, holes cleared, vertex pixels set (load_mask, :321-338). */
int disyolo_polygon_mask(const float* px, const float* py, const int32_t* poly_start,
                         const int32_t* poly_is_out, int npoly, int image_h, int image_w, uint8_t* mask,
                         void* stream);
/* apply_random_scale_and_crop + flip (:392-397, 428-434, 446-464): src resized to new_w x new_h (cv2
 * INTER_LINEAR), placed with its corner at (dx, dy) of the size x size frame (negative = cropped),
 * flip 1 none / 2 horizontal / 3 vertical.  is_mask = 0: src uint8 RGB [H,W,3], pad 127, dst uint8
 * [size,size,3]; is_mask = 1: src uint8 0/1 [H,W] resized as float32, pad 0, np.around, dst uint8 0/1. */
int disyolo_aug_place(const uint8_t* src, int is_mask, int image_h, int image_w, uint8_t* dst, int size,
                      int new_w, int new_h, int dx, int dy, int flip, void* stream);
/* a whole batch's placements in one launch (round 6).  jobs: DEVICE array of njobs entries; per-pixel arithmetic = disyolo_aug_place's
 * (image: OpenCV's 8-bit fixed-point bilinear path, pad 127; mask: float bilinear, pad 0, half-to-even rounding to 0 / 1).
 * Replaces nothing in the reference (its loader is host code, utils/train_data.py:376-444); it replaces ~25 launches per batch here. */
typedef struct disyolo_place_job {
  const uint8_t* src;      /* image [image_h, image_w, 3] or mask [image_h, image_w], uint8 */
  uint8_t* dst;            /* [size, size, 3] or [size, size] */
  int32_t is_mask, image_h, image_w, new_w, new_h, dx, dy, flip;
} disyolo_place_job;
int disyolo_aug_place_batch(const disyolo_place_job* jobs, int njobs, int size, void* stream);
/* add_salt_pepper_noise (:511-525): pixels (rows[i], cols[i]) <- 1 for i < nsalt, then <- 0 for the next npepper */
int disyolo_aug_salt_pepper(uint8_t* image, int size, const int32_t* rows, const int32_t* cols, int nsalt,
                            int npepper, void* stream);
/* change_light (:527-535): L of HLS scaled by coeff, clipped */
int disyolo_aug_change_light(uint8_t* image, int size, double coeff, void* stream);
/* linearmotion_blur3C (:466-494), line length 3: angle 0/45/90/135, line_type 0 full / 1 right / 2 left */
int disyolo_aug_motion_blur3(const uint8_t* src, uint8_t* dst, int size, int angle, int line_type, void* stream);
/* the five kernels above on a frame of net_h x net_w (the loader of a rectangular net: dst [net_h, net_w, 3] or
 * [net_h, net_w], flips about the frame's own width / height, salt-and-pepper rows < net_h and cols < net_w -- a coordinate
 * outside the frame is skipped); each entry point above is the net_h = net_w = size call of its _hw form */
int disyolo_aug_place_hw(const uint8_t* src, int is_mask, int image_h, int image_w, uint8_t* dst, int net_h, int net_w,
                         int new_w, int new_h, int dx, int dy, int flip, void* stream);
int disyolo_aug_place_batch_hw(const disyolo_place_job* jobs, int njobs, int net_h, int net_w, void* stream);
int disyolo_aug_salt_pepper_hw(uint8_t* image, int net_h, int net_w, const int32_t* rows, const int32_t* cols, int nsalt,
                               int npepper, void* stream);
int disyolo_aug_change_light_hw(uint8_t* image, int net_h, int net_w, double coeff, void* stream);
int disyolo_aug_motion_blur3_hw(const uint8_t* src, uint8_t* dst, int net_h, int net_w, int angle, int line_type,
                                void* stream);
/* image.astype(float32) / 255.0 (:411-413) */
int disyolo_aug_to_float(const uint8_t* image, float* out, int64_t n, void* stream);

/* ---- window training (defect_train(placement="window"); nothing in the reference: its loader always
 * fits the whole record into the net) ----
 * A batch image is a net_h x net_w window of its record at scale 1 with its origin (x0, y0) in image pixels.  A window cuts
 * instances, so boxes and target grids come from the VISIBLE pixels, on the device.  One job per (batch image, candidate
 * instance), the jobs of an image adjacent and in record order.  src: the instance's 0 / 1 byte mask cropped to
 * [crop_y, crop_y + crop_h) x [crop_x, crop_x + crop_w) of the image (row stride crop_w); the visible part of the instance is
 * crop n window n image.  b: batch index, cls: class index, flip: 1 none / 2 horizontal / 3 vertical.
 * jobs is a DEVICE array in the three calls below; njobs = 0 is allowed (window_targets then only zeroes its outputs). */
typedef struct disyolo_window_job {
  const uint8_t* src;
  int32_t crop_h, crop_w, crop_x, crop_y, x0, y0, image_h, image_w, b, cls, flip, reserved;
} disyolo_window_job;
size_t disyolo_window_job_size(void);
/* vis int32 [njobs, 5] <- per job (count, x1, y1, x2, y2): the number of set pixels of the visible part and their tight box
 * in window coordinates, unflipped, x2 / y2 one past the last; all zeros when nothing is visible.  vis is initialised by the
 * call; integer reductions only, so the result does not depend on the order the blocks run in. */
int disyolo_window_visible(const disyolo_window_job* jobs, int njobs, int net_h, int net_w, int32_t* vis, void* stream);
/* Target assignment of utils/train_data.py:136-178, 187-226, 250-257 on the device.  Zeroes true_boxes f32 [B, G, 5] and the
 * grids yolo3 / yolo2 / yolo1 f32 [B, net_h / d, net_w / d, 3, 5 + C] (d = 8, 16, 32), then walks each image's jobs in order:
 * a job is kept when its count >= min_visible, its box clamped to [0, net - 1] has w > 0 and h > 0, and fewer than G jobs of
 * its image were kept before it.  A kept job takes the next row r of true_boxes ((xc, yc, w, h) / (net_w, net_h, net_w,
 * net_h), class), its best-IoU anchor of the nine (f32, the first maximum; a maximum <= 0 writes no cell) and the cell its
 * centre falls in unless an earlier job holds that (cell, anchor); centres and cells are reflected for flip 2 / 3.
 * rows int32 [njobs] <- r, or -1 for a dropped job.  anchors f32 [9, 2] (device).  1 <= G <= DISYOLO_MAX_BOXES, 1 <= C <= 80,
 * net_h and net_w multiples of 32, min_visible >= 1. */
int disyolo_window_targets(const disyolo_window_job* jobs, int njobs, const int32_t* vis, const float* anchors, int B, int G,
                           int C, int net_h, int net_w, int min_visible, float* true_boxes, float* yolo3, float* yolo2,
                           float* yolo1, int32_t* rows, void* stream);
/* true_masks uint8 [B, G, net_h, net_w]: every job with rows[job] >= 0 copies its visible bytes into plane [b, rows[job]],
 * flipped; the caller zeroes true_masks first. */
int disyolo_window_place_masks(const disyolo_window_job* jobs, int njobs, const int32_t* rows, uint8_t* true_masks, int G,
                               int net_h, int net_w, void* stream);

/* ---- host helper of the checkpoint reader / writer (dis-yolo_amd/checkpoint.py; train_yolo3_mask.py:58,
 * 221-226 Saver.save / calculate_test_map.py:184-185 Saver.restore): CRC-32C (Castagnoli) of n bytes,
 * continuing from `crc` (0 to start) -- TensorFlow tensor bundles store it masked per tensor and per
 * index block.  Runs on the host; no device work. */
uint32_t disyolo_crc32c(const void* data, size_t n, uint32_t crc);

/* ---- command lists: the native step executor ----
 * Between cmdlist_begin and cmdlist_end every launch entry point above, called from the
 * recording thread, appends itself to the list (arguments captured by value; device buffers
 * and workspaces must outlive the list) instead of launching.  cmdlist_run replays commands
 * [first,last) on `stream` in one call -- the replacement for tf.Session.run's executor on
 * this path (train_yolo3_mask.py:216), and capturable into a hipGraph. */
void* disyolo_cmdlist_create(void);
void disyolo_cmdlist_destroy(void* list);
int disyolo_cmdlist_begin(void* list);
int disyolo_cmdlist_end(void);
int disyolo_cmdlist_size(void* list);
/* packets a replay puts on `lane`: what = 0 launches, 1 event records, 2 event waits (an event packet costs its stream ~3 us) */
int disyolo_cmdlist_count(void* list, int what, int lane);
/* out = { kind, lane, from, to } of command `index` (0 <= index < cmdlist_size), as the list holds them.  Read-only, no
 * device work: a caller can rebuild the partial order a replay's edges define (tests/lane_order.py does).
 *   kind 0 launch      on `lane`
 *   kind 1 sync        lane `to` waits for everything lane `from` has recorded so far
 *   kind 2 mark        a point of lane `from`
 *   kind 3 wait        lane `to` waits for the mark at list index `from`
 *   kind 4 mark_slot   a point of lane `from`, under slot `to`
 *   kind 5 wait_slot   lane `to` waits for the last mark of slot `from`
 * (`lane` is 0 for every kind but 0.)  A null list, null out or an index out of range: DISYOLO_E_ARG. */
int disyolo_cmdlist_describe(void* list, int index, int32_t out[4]);
/* four lanes: 0 = the stream passed to cmdlist_run, 1..3 = side streams owned by the list (3 = the gradient exchange).
 * set_lane selects the lane of the launches recorded next; sync(from,to) makes lane `to` wait
 * for what lane `from` has recorded so far.  Both are no-ops outside a recording.  Every
 * cmdlist_run range forks the side lane after the caller's stream and joins it at the end. */
int disyolo_cmdlist_set_lane(int lane);
int disyolo_cmdlist_sync(int from_lane, int to_lane);
/* finer edge: mark(lane) remembers this point of `lane` (returns the mark's id, -1 outside a recording);
 * wait(mark, lane) makes `lane` wait for that point only -- not for what the marked lane recorded later */
int disyolo_cmdlist_mark(int lane);
int disyolo_cmdlist_wait(int mark, int lane);
/* named marks that outlive a replay: wait_slot waits for the point the slot was LAST marked at -- earlier in this replay
 * or in the previous replay of the list (no wait on the first).  Lets a step's side-lane tail overlap the next step's
 * main-lane start with per-tensor dependencies (YOLONet.build_program(overlap_tail=True)).  slot 0..15. */
int disyolo_cmdlist_mark_slot(int lane, int slot);
int disyolo_cmdlist_wait_slot(int slot, int lane);
int disyolo_cmdlist_run(void* list, int first, int last, void* stream);
/* same with explicit fork/join control (flags bit 0 = fork at the start, bit 1 = join at the
 * end) for a step replayed in several ranges, and the side lane's hipStream_t so a caller can
 * order other work (an RCCL all-reduce) after the side lane only */
int disyolo_cmdlist_run_ex(void* list, int first, int last, void* stream, int flags);
void* disyolo_cmdlist_side_stream(void* list);
void* disyolo_cmdlist_lane_stream(void* list, int lane);   /* lane 1..3 (side_stream = lane 1) */
/* the side lanes are streams of one process-wide pool, created when a list first uses them; lanes_reserve(mask) (bit i =
 * lane i) creates them NOW on the current device -- before torch.distributed's NCCL backend (whose stream pool takes
 * the hardware queues: a lane created afterwards may share the caller's stream's queue, 2.5x the step time) */
int disyolo_lanes_reserve(int mask);
/* how the side lanes of the current device were chosen, one text line per lane that exists (priority, probed or not,
 * candidates tried, whether the fallback was taken, the probe's times): bench.py puts it into its line so that a run that
 * fell back to an unmeasured stream can be told from one that did not */
int disyolo_lanes_report(char* buf, int size);

/* ---- data-parallel gradient exchange as COMMANDS of the step (csrc/comm.hip) ----
 * The reference trains on one GPU (yolo/config.py:18; the op being distributed is train_yolo3_mask.py:55-56,
 * AdamOptimizer.minimize(total_loss)): every loss term is a per-image sum averaged over the batch
 * (yolo/yolo3_net_pos.py:692-726,858), so N ranks with equal local batches exchange ONE thing per step -- the sum of
 * their gradients.  These entry points put that exchange on RCCL (xGMI) without leaving the command list: inside a
 * recording a collective is a command of the current lane like any launch.
 * comm_load: dlopen RCCL (path NULL = default search; the host binding passes the copy the process already maps);
 *   no link-time dependency.  comm_unique_id (rank 0) -> 128 opaque bytes, exchanged by the host out of band ->
 *   comm_init on every rank (a collective; the current HIP device is the rank's GPU) -> an opaque communicator.
 * dtype: 0 = f32, 1 = bf16, 2 = f64.  Every rank must issue the same collectives in the same order. */
int disyolo_comm_load(const char* rccl_path, int* version);
int disyolo_comm_unique_id(void* id128);
int disyolo_comm_init(const void* id128, int rank, int nranks, void** comm);
int disyolo_comm_destroy(void* comm);
int disyolo_comm_allreduce_sum(void* comm, void* buf, int64_t count, int dtype, void* stream);
int disyolo_comm_reduce_scatter_sum(void* comm, const void* send, void* recv, int64_t recvcount, int dtype, void* stream);
int disyolo_comm_all_gather(void* comm, const void* send, void* recv, int64_t sendcount, int dtype, void* stream);
/* wire-format conversions of a gradient bucket (bf16 on the links, round to nearest even): any n > 0 */
int disyolo_cast_f32_bf16(const void* src_f32, void* dst_bf16, int64_t n, void* stream);
int disyolo_cast_bf16_f32(const void* src_bf16, void* dst_f32, int64_t n, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DISYOLO_H */

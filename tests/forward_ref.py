"""Float64 references of the forward pass and the element-wise checkers that hold the kernels to them.

Test infrastructure (imported by tests/test_gpu_forward.py and tests/test_forward_ref.py), the forward counterpart of
tests/backward_ref.py, whose helpers (f64, bf16_round, layer_input, check_bounded, the conv padding) it reuses.  Plain torch
float64 on whatever device its inputs live on; nothing calls this project's kernels.  NHWC activations, HWIO weights.

A layer's reference is built from the kernels' own tensors one step upstream (its input activation(s) as the layer reads
them, its bf16 weights, its residual source, and -- where a check is about the epilogue -- its own scale / shift), never
from the reference's own earlier results.  Each output element gets a bound:
  * U_BF16 * |want| per bf16 rounding (one unit roundoff, 2^-8);
  * C_ACC * twin for the f32 accumulation, twin = the same f64 conv on |operands|;
  * C_SPLIT * twin for the split-bf16 products of conv1 inside the conv1+conv2 launch (2^-16 per product);
  * C_EPI * (|conv*scale| + |shift| + |residual|) for the f32 epilogue (scale, shift, leaky, residual add);
  * leaky is 1-Lipschitz, so a pre-activation bound carries through it unchanged: where the f64 pre-activation is within
    its bound of 0, either leaky side is inside the bound (such elements are counted as "ambiguous").
Batch statistics are one-pass in the kernels: f32 partial sums of x and x^2 (from the f32 accumulators, or from the bf16
raw output for conv1), added in double, var = E[x^2] - mean^2.  ``stats_bounds`` derives their error from e (each x's
own error), sum|x| and E[x^2]; the reference moments are two-pass f64 over the unrounded f64 conv.
"""
import numpy as np
import torch
import torch.nn.functional as F

import disyolo_oracle as O
from backward_ref import F64, ALPHA, f64, bf16_round, layer_input, check_bounded, upsample2, _pads, _tap  # noqa: F401

BN_DECAY = float(torch.tensor(O.BN_DECAY, dtype=torch.float32))     # the kernels take the decay as an f32
BN_EPS = O.BN_EPS

# bounds of the teacher-forced checks (tests/test_gpu_forward.py, Part A).  Measured on an MI355X over the configurations of
# that module, planted channels included (worst err/bound ratio of the tensors the term governs in brackets).  The bf16
# terms are one unit roundoff per rounding and cannot shrink: outputs reach 0.996 of them.
U_BF16 = 2.0 ** -8          # one bf16 rounding (round to nearest-even): u * |value|  [act, raw 0.996; fused launches 0.51]
C_ACC = 2.0 ** -20          # f32 accumulation of a conv: C_ACC * twin  [f32 outputs of the linear layers 0.16]
# the e4m3 convs (conv10-52) on the block-scaled fp8 MFMA: the dot products of that instruction are not accumulated as
# exactly as an f32 chain -- with C_ACC their codes miss the midpoint test by 3x and more, so they get a term of their own
C_ACC8 = 2.0 ** -14         # e4m3 conv accumulation: C_ACC8 * twin  [distance of an accepted adjacent code from its midpoint 0.25]
C_SPLIT = 2.0 ** -16        # conv1 on split-bf16 operands inside conv1+conv2: per product (the rounding of the split)
C_EPI = 2.0 ** -22          # f32 epilogue: C_EPI * (|conv*scale| + |shift| + |residual|)  (inside the act ratios)
C_SUM = 2.0 ** -21          # f32 partial sums of the statistics: C_SUM * sum|x| (sum x) and C_SUM * sum x^2 (sum x^2)
                            # [mean 0.053, rstd 0.11 with the planted |mean|/std = 64 channels]
C_COEF = 2.0 ** -21         # f32 finalize arithmetic (scale, shift, rstd, moving averages), relative  [mm / mv 0.23, escale 0.19, scale 0.11]
# the relative rstd error a planted channel with |mean|/std of 16 or 64 must stay below: half a bf16 ulp of xhat
RSTD_LIMIT = 2.0 ** -9


def leaky(x, alpha=ALPHA):
    return torch.maximum(alpha * x, x)


# ------------------------------------------------------------------------------------------------ convolution references
def conv_ref(x: torch.Tensor, w: torch.Tensor, stride: int, twin: bool = True):
    """the TF-SAME convolution of x [B,H,W,C] with w [k,k,C,Cout] in float64, and (``twin``) the same on |x|, |w|"""
    x, w = f64(x), f64(w)
    B, H, W, C = x.shape
    k, cout = w.shape[0], w.shape[3]
    Ho, Wo, pt, pb, pl, pr = _pads((H, W), k, stride)
    xp = F.pad(x, (0, 0, pl, pr, pt, pb))
    out = torch.zeros(B * Ho * Wo, cout, dtype=F64, device=x.device)
    tw = torch.zeros_like(out) if twin else None
    for ky, kx, sy, sx in _tap(k, stride, Ho, Wo):
        a = xp[:, sy, sx, :].reshape(-1, C)
        out += a @ w[ky, kx]
        if twin:
            tw += a.abs() @ w[ky, kx].abs()
    out = out.view(B, Ho, Wo, cout)
    return (out, tw.view(B, Ho, Wo, cout)) if twin else out


def moments(y: torch.Tensor):
    """two-pass batch moments over N, H, W with population variance (tf.nn.moments)"""
    y = f64(y).reshape(-1, y.shape[-1])
    mean = y.mean(0)
    return mean, ((y - mean) ** 2).mean(0)


def bn_fold_ref(gamma, beta, mm, mv, eps=BN_EPS):
    sc = f64(gamma) / torch.sqrt(f64(mv) + eps)
    return sc, f64(beta) - f64(mm) * sc


# ------------------------------------------------------------------------------------------------ one conv stage
def stage_ref(x, w, stride, scale=None, shift=None, res=None, x_err=None, split=False, act=True, c_acc=None):
    """one conv + epilogue in float64 as a kernel computes it: z = conv(x, w)*scale + shift, y = leaky(z) + res (act) or
    z + shift (a linear layer: ``scale`` None).  Returns dict(y, z, bz): bz bounds |z_kernel - z| before the output is
    rounded -- the f32 accumulation, split-bf16 products, the f32 epilogue, and an input error ``x_err`` carried through
    the conv to first order.  Since leaky is 1-Lipschitz bz also bounds the error of y.  ``c_acc``: the accumulation
    constant (C_ACC unless given)."""
    c, tw = conv_ref(x, w, stride)
    e = ((C_ACC if c_acc is None else c_acc) + (C_SPLIT if split else 0.0)) * tw
    if x_err is not None:
        e = e + conv_ref(x_err, f64(w).abs(), stride, twin=False)
    sc = f64(scale) if scale is not None else torch.ones(c.shape[-1], dtype=F64, device=c.device)
    sh = f64(shift) if shift is not None else torch.zeros_like(sc)
    cs = c * sc
    z = cs + sh
    bz = e * sc.abs() + C_EPI * (cs.abs() + sh.abs())
    if not act:
        return dict(y=z, z=z, bz=bz)
    y = leaky(z)
    if res is not None:
        r = f64(res)
        y = y + r
        bz = bz + C_EPI * r.abs()
    return dict(y=y, z=z, bz=bz)


def rounded_mid(s):
    """the bf16 intermediate of a fused launch: the reference rounds its own f64 value; the kernel rounds a value within
    bz of it, so the two differ by at most bz + 2u|y| (two roundings of nearby values)"""
    return bf16_round(s["y"]), s["bz"] + 2 * U_BF16 * s["y"].abs()


def bf16_bound(s):
    """bound of a stored bf16 output of stage_ref: one rounding + the pre-rounding error"""
    return U_BF16 * s["y"].abs() + s["bz"]


def ambiguous(s):
    """elements whose f64 pre-activation is within its bound of 0 (either leaky side is acceptable)"""
    return int((s["z"].abs() <= s["bz"]).sum())


# ------------------------------------------------------------------------------------------------ batch statistics
def stats_bounds(y, e, M=None):
    """bounds of the kernels' one-pass statistics of y (the f64 conv, [.., C]) whose elements carry errors e:
      S1 = sum x  : dS1 <= sum e + C_SUM * sum|x|
      S2 = sum x^2: dS2 <= sum(2|x| e + e^2) + C_SUM * sum x^2
      mean = S1/M : dmean <= dS1/M + 2^-24 |mean|                          (the f32 result)
      var = S2/M - mean^2: dvar <= dS2/M + 2|mean| dS1/M + (dS1/M)^2 + C_COEF * (E[x^2] + var)
    so var's error grows with E[x^2] = var + mean^2: the (mean/std)^2 of a channel.  Returns (mean, var, bmean, bvar)."""
    C = y.shape[-1]
    y, e = f64(y).reshape(-1, C), f64(e).reshape(-1, C)
    M = M or y.shape[0]
    mean, var = moments(y)
    ax = y.abs()
    d1 = (e.sum(0) + C_SUM * ax.sum(0)) / M
    ex2 = (y * y).sum(0) / M
    d2 = (2 * ax * e + e * e).sum(0) / M + C_SUM * ex2
    bmean = d1 + 2.0 ** -24 * mean.abs()
    bvar = d2 + 2 * mean.abs() * d1 + d1 * d1 + C_COEF * (ex2 + var)
    return mean, var, bmean, bvar


def rstd_ref(var, bvar, eps=BN_EPS):
    """1/sqrt(var + eps) and its bound: half the relative error of var + eps, plus the f32 arithmetic"""
    r = 1.0 / torch.sqrt(var + eps)
    return r, r * (0.5 * bvar / (var + eps) + C_COEF)


def moving_ref(old, batch, b_batch, decay=BN_DECAY):
    """decay*old + (1 - decay)*batch in f64 (decay the f32 value the kernels use) and its bound"""
    old = f64(old)
    want = old * decay + batch * (1.0 - decay)
    return want, (1.0 - decay) * b_batch + C_COEF * ((old * decay).abs() + (batch * (1.0 - decay)).abs())


def coeffs_from(gamma, beta, mean, rstd):
    """scale / shift from a kernel's own mean / rstd, f64, and the bound of their f32 evaluation (a few ulps)"""
    g, b, m, r = f64(gamma), f64(beta), f64(mean), f64(rstd)
    sc = g * r
    sh = b - m * sc
    return sc, sh, C_COEF * sc.abs(), C_COEF * (b.abs() + 2 * (m * sc).abs())


def fold_bounds(gamma, beta, mm, mv):
    """bn_fold in f64 and its bound in f32 ulps (mv + eps, sqrt, divide; beta - mm*scale)"""
    sc, sh = bn_fold_ref(gamma, beta, mm, mv)
    return sc, sh, C_COEF * sc.abs(), C_COEF * (f64(beta).abs() + 2 * (f64(mm) * sc).abs())


# ------------------------------------------------------------------------------------------------ e4m3
E4M3_MAX = 448.0


def rne_e4m3(v: torch.Tensor) -> torch.Tensor:
    """OCP e4m3 (saturating at +-448, round to nearest-even, subnormals down to 2^-9) of an f64 tensor, as f64"""
    v = f64(v)
    a = v.abs().clamp(max=E4M3_MAX)
    e = torch.floor(torch.log2(torch.where(a > 0, a, torch.ones_like(a)))).clamp(min=-6)
    ulp = torch.exp2(e - 3)
    q = (torch.round(a / ulp) * ulp).clamp(max=E4M3_MAX)
    return torch.copysign(q, v)


_E4M3_LUT = {}


def decode_e4m3(codes: torch.Tensor) -> torch.Tensor:
    """uint8 codes (OCP e4m3) -> f64 values (NaN for the NaN codes)"""
    dev = codes.device
    if dev not in _E4M3_LUT:
        lut = torch.arange(256, dtype=torch.int32).to(torch.uint8).view(torch.float8_e4m3fn).float().double()
        _E4M3_LUT[dev] = lut.to(dev)
    return _E4M3_LUT[dev][codes.long()]


def check_e4m3(got_codes, want, bound, s_out: float, what: str, fails=None):
    """every code must be RNE_e4m3(want / s_out); where want / s_out lies within its bound of a rounding midpoint the
    adjacent code is accepted too.  ``bound`` bounds |want_kernel - want| before the division (the kernel multiplies by
    1/s_out in f32: two more f32 roundings).  Returns (mismatches, other codes accepted, the worst accepted one's distance
    from its midpoint over the bound)."""
    v = f64(want) / s_out
    b = f64(bound) / s_out + 2.0 ** -22 * v.abs()
    got = decode_e4m3(got_codes.reshape(v.shape))
    q, lo, hi = rne_e4m3(v), rne_e4m3(v - b), rne_e4m3(v + b)
    ok = (got == q) | ((got >= lo) & (got <= hi))          # (NaN compares false: never accepted)
    other = ok & (got != q)
    adj = int(other.sum())
    bad = int((~ok).sum())
    # how close an accepted other code came to its limit: distance of v from the midpoint between it and q, over the bound
    worst = float(((v - (got + q) / 2).abs() / b)[other].max()) if adj else 0.0
    if bad:
        i = int((~ok).flatten().nonzero()[0])
        msg = "%s: %d of %d e4m3 codes differ from RNE(want / s_out); first at flat %d: got %r want %r (v %r, bound %.3g)" % (
            what, bad, ok.numel(), i, float(got.flatten()[i]), float(q.flatten()[i]), float(v.flatten()[i]), float(b.flatten()[i]))
        if fails is None:
            raise AssertionError(msg)
        fails.append(msg)
    return bad, adj, worst


def fp8_weights(w8: torch.Tensor, k: int, cin: int, cout: int) -> torch.Tensor:
    """the packed e4m3 weights [Cout][k*k*Cin] (HWIO order within a row) as HWIO f64 values (units of s_w)"""
    return decode_e4m3(w8).view(cout, k, k, cin).permute(1, 2, 3, 0)


def layer_input_of(layer, by_idx, sl=slice(None), images=None):
    """what layer convolves, float64, for the images ``sl``: the f32 image (layer 1), src.act, or cat(src.act, up2(src_up.act))"""
    return layer_input(layer, by_idx, image_bf16=None if images is None else images[sl], act_of=lambda m: m.act[sl])


# ------------------------------------------------------------------------------------------------ mask assembly
def val_test_k(detections, mask_pos, k):
    """O.val_test (yolo/yolo3_net_pos.py:862-938) with a k x k grid (the oracle's own assembles k = 3)"""
    det_box, det_mask = [], []
    size = mask_pos.shape[1]
    for i in range(mask_pos.shape[0]):
        prop = detections[i].astype(np.float32)
        pb = np.round(prop[:, :4] * np.float32(size))
        keep = np.where(((pb[:, 2] - pb[:, 0]) > 0) & ((pb[:, 3] - pb[:, 1]) > 0))[0]
        prop, pb = prop[keep], pb[keep]
        if prop.size > 0:
            det_mask.append(torch.stack([torch.sigmoid(O.assemble_logits(mask_pos[i], b, k)[0]) for b in pb]).float().numpy())
        else:
            det_mask.append(np.float32(0.0))
        det_box.append(prop)
    return det_box, det_mask

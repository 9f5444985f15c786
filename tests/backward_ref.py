"""Float64 references of the training step's backward pass and the element-wise checkers that hold the kernels to them.

Test infrastructure (imported by tests/test_gpu_backward.py and tests/test_backward_ref.py).  Everything here is plain torch
float64 on whatever device its inputs live on; nothing calls this project's kernels.  Tensors are NHWC, weights HWIO, as in
the net and the oracle.

Two kinds of check:
  * bounded (``check_bounded``): |got - want| <= bound element by element, the bound built from the operation's rounding
    (bf16 storage, f32 accumulation measured against the "absolute twin": the same computation on |inputs|);
  * exact (``check_exact_f32`` / ``check_exact_bf16``): on integer operands every f32 partial sum is an integer below 2^24, so
    any summation order gives the exact sum -- an f32 output must equal it, a bf16 output must equal it rounded once to
    nearest-even.
"""
import math

import pytest
import torch
import torch.nn.functional as F

import disyolo_oracle as O

F64 = torch.float64
ALPHA = O.ALPHA
EXACT_LIMIT = 2.0 ** 24

# bounds of the teacher-forced checks (tests/test_gpu_backward.py, Part A); "twin" = the same f64 computation on |operands|.
# Measured on an MI355X over the four configurations of that module (worst err/bound ratio in brackets): the f32 sums are
# held to about 4x their worst; the bf16 terms are one unit roundoff (2^-8) per rounding and cannot shrink.
C_DW = 2.0 ** -18                                       # dW: C_DW * twin  [0.26]
C_DBIAS = 2.0 ** -22                                    # dbias: C_DBIAS * sum|dx|  [0.24]
C_G_REL, C_G_ACC, C_G_TWIN = 2.0 ** -8, 2.0 ** -8, 2.0 ** -20  # output gradient g: rel*|want| + acc*sum|c| + twin*twin  [0.98]
C_DX_REL, C_DX_FIRST = 2.0 ** -8, 2.0 ** -8             # dx: rel*|want| + first*(first-order term of bn_bounds)  [0.50]
# dgamma, dbeta: sqrt*sqrt(sum term^2) + abs*sum|term|.  Where the reference reads the kernel's own stored g (plain and
# partial-sums forms) only the f32 summation differs  [0.13]; the in-launch form never stores its g, so the reference's g
# differs from it by independent bf16 roundings, which the sqrt term carries  [0.77]
C_SUM_SQRT_OWN, C_SUM_ABS_OWN = 2.0 ** -16, 2.0 ** -23
C_SUM_SQRT, C_SUM_ABS = 2.0 ** -7, 2.0 ** -14


@pytest.fixture
def tuned_tables():
    """a test that loads a tile table (net.autotune(cache=...) fills lib.TUNED) clears it afterwards"""
    from disyolo_amd import lib as L
    yield
    L.TUNED.clear()


def f64(t: torch.Tensor) -> torch.Tensor:
    return t.detach().to(F64)


def bf16_round(t: torch.Tensor) -> torch.Tensor:
    """round to bf16 (nearest-even) and back, in t's dtype"""
    return t.to(torch.bfloat16).to(t.dtype)


# ------------------------------------------------------------------------------------------------ convolution references
def _pads(x_hw, k, s):
    Ho, pt, pb = O.same_pads(x_hw[0], k, s)
    Wo, pl, pr = O.same_pads(x_hw[1], k, s)
    return Ho, Wo, pt, pb, pl, pr


def _tap(k, s, Ho, Wo):
    for ky in range(k):
        for kx in range(k):
            yield ky, kx, slice(ky, ky + s * (Ho - 1) + 1, s), slice(kx, kx + s * (Wo - 1) + 1, s)


def wgrad_ref(x: torch.Tensor, dy: torch.Tensor, k: int, stride: int) -> torch.Tensor:
    """dW [k,k,C,Cout] of the TF-SAME convolution of x [B,H,W,C] whose output gradient is dy [B,Ho,Wo,Cout]"""
    x, dy = f64(x), f64(dy)
    B, H, W, C = x.shape
    Ho, Wo, pt, pb, pl, pr = _pads((H, W), k, stride)
    assert dy.shape[:3] == (B, Ho, Wo), (dy.shape, (B, Ho, Wo))
    xp = F.pad(x, (0, 0, pl, pr, pt, pb))
    d = dy.reshape(-1, dy.shape[-1])
    out = torch.empty(k, k, C, dy.shape[-1], dtype=F64, device=x.device)
    for ky, kx, sy, sx in _tap(k, stride, Ho, Wo):
        out[ky, kx] = xp[:, sy, sx, :].reshape(-1, C).t() @ d
    return out


def dgrad_ref(dy: torch.Tensor, w: torch.Tensor, stride: int, H: int, W: int) -> torch.Tensor:
    """gradient [B,H,W,C] wrt the input of the TF-SAME convolution with weights w [k,k,C,Cout], from dy [B,Ho,Wo,Cout]
    (the transposed convolution)"""
    dy, w = f64(dy), f64(w)
    k, C = w.shape[0], w.shape[2]
    B = dy.shape[0]
    Ho, Wo, pt, pb, pl, pr = _pads((H, W), k, stride)
    assert dy.shape[1:] == (Ho, Wo, w.shape[3]), (dy.shape, (Ho, Wo, w.shape[3]))
    out = torch.zeros(B, H + pt + pb, W + pl + pr, C, dtype=F64, device=dy.device)
    d = dy.reshape(-1, dy.shape[-1])
    for ky, kx, sy, sx in _tap(k, stride, Ho, Wo):
        out[:, sy, sx, :] += (d @ w[ky, kx].t()).view(B, Ho, Wo, C)
    return out[:, pt:pt + H, pl:pl + W, :]


def upsample2(x: torch.Tensor) -> torch.Tensor:
    return O.upsample2(x)


def upsample2_bwd(t: torch.Tensor) -> torch.Tensor:
    """gradient of the nearest 2x upsampling: the sum of each 2x2 block"""
    B, H, W, C = t.shape
    return t.view(B, H // 2, 2, W // 2, 2, C).sum(dim=(2, 4))


def concat_input(a: torch.Tensor, up: torch.Tensor) -> torch.Tensor:
    """what a concat layer convolves: its direct source, then its src_up source upsampled 2x"""
    return torch.cat([f64(a), upsample2(f64(up))], dim=-1)


# ------------------------------------------------------------------------------------------------ batch norm + leaky backward
def bn_act_bwd_ref(g, raw, scale, shift, mean, rstd, gamma, alpha=ALPHA):
    """closed-form backward of leaky(batch_norm(raw)) in float64 from the kernel's own statistics.

    g' = g * (z > 0 ? 1 : alpha), z = raw*scale + shift, xhat = (raw - mean)*rstd;
    dbeta = sum g', dgamma = sum g'*xhat, dx = gamma*rstd*(g' - dbeta/M - xhat*dgamma/M).
    ``amb`` marks elements whose z is within rounding of 0 (either slope is right); ``dx_alt`` is dx with the other slope
    there."""
    g, raw = f64(g), f64(raw)
    C = raw.shape[-1]
    g, raw = g.reshape(-1, C), raw.reshape(-1, C)
    scale, shift, mean, rstd, gamma = (f64(t) for t in (scale, shift, mean, rstd, gamma))
    M = raw.shape[0]
    z = raw * scale + shift
    amb = z.abs() <= 2.0 ** -20 * ((raw * scale).abs() + shift.abs())
    slope = torch.where(z > 0, torch.ones_like(z), torch.full_like(z, alpha))
    gp = g * slope
    xh = (raw - mean) * rstd
    dbeta = gp.sum(0)
    dgamma = (gp * xh).sum(0)
    k = gamma * rstd
    dx = k * (gp - dbeta / M - xh * dgamma / M)
    other = torch.where(z > 0, torch.full_like(z, alpha), torch.ones_like(z))
    dx_alt = k * (g * other - dbeta / M - xh * dgamma / M)
    return dict(dx=dx, dgamma=dgamma, dbeta=dbeta, gp=gp, xh=xh, amb=amb, dx_alt=dx_alt, g=g, M=M, k=k, slope=slope,
                amb_gap=torch.where(amb, (1.0 - alpha) * g.abs(), torch.zeros_like(g)))


# ------------------------------------------------------------------------------------------------ bounds
# (module constants: tests/test_gpu_backward.py holds the values; these helpers take them as arguments)
def bn_bounds(r, c_rel, c_first, c_sum_sqrt, c_sum_abs, g_err=None):
    """bounds of dx / dgamma / dbeta around the reference ``r`` of bn_act_bwd_ref.
    dx: c_rel*|want| + c_first*|gamma|*rstd*(|g'| + (|dbeta| + |xhat|*|dgamma|)/M), and when the reference's g is its
    own rather than the kernel's (the in-launch form never stores its g) that g's error bound e carried through the same
    linear map: |gamma|*rstd*(s*e + sum(s*e)/M + |xhat|*sum(s*e*|xhat|)/M), s = the leaky slope -- the mean terms spread
    the rounding of a few large g' over the whole channel.  dgamma / dbeta: c_sum_sqrt*sqrt(sum term^2) + c_sum_abs*sum|term|
    (+ the ambiguous slopes' share)."""
    k = r["k"].abs()
    first = k * (r["gp"].abs() + (r["dbeta"].abs() + r["xh"].abs() * r["dgamma"].abs()) / r["M"])
    bdx = c_rel * r["dx"].abs() + c_first * first
    tg, tb = r["gp"] * r["xh"], r["gp"]
    amb_g = (r["amb_gap"] * r["xh"].abs()).sum(0)
    amb_b = r["amb_gap"].sum(0)
    if g_err is not None:
        e = g_err.reshape(r["gp"].shape) * r["slope"]
        xa = r["xh"].abs()
        bdx = bdx + k * (e + e.sum(0) / r["M"] + xa * (e * xa).sum(0) / r["M"])
    bdg = c_sum_sqrt * (tg * tg).sum(0).sqrt() + c_sum_abs * tg.abs().sum(0) + amb_g
    bdb = c_sum_sqrt * (tb * tb).sum(0).sqrt() + c_sum_abs * tb.abs().sum(0) + amb_b
    return bdx, bdg, bdb


# ------------------------------------------------------------------------------------------------ checkers
def _where(idx, shape):
    out = []
    for n in reversed(shape):
        out.append(idx % n)
        idx //= n
    return tuple(reversed(out))


def check_bounded(got, want, bound, what: str, alt=None, fails=None) -> float:
    """every element: |got - want| <= bound (or |got - alt| <= bound where ``alt`` is given and not NaN).  Returns the
    worst err/bound ratio; a violation raises AssertionError naming the worst element and the count of violations (or,
    with a ``fails`` list, appends that message to it)"""
    g = f64(got).reshape(want.shape)
    err = (g - want).abs()
    if alt is not None:
        ea = (g - alt).abs()
        err = torch.where(torch.isnan(ea), err, torch.minimum(err, ea))
    err = torch.where(torch.isnan(g), torch.full_like(err, math.inf), err)
    bound = bound.expand_as(err) if bound.shape != err.shape else bound
    ratio = torch.where(bound > 0, err / torch.where(bound > 0, bound, torch.ones_like(bound)),
                        torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    if not worst <= 1.0:
        bad = int((ratio > 1.0).sum())
        i = int(ratio.flatten().argmax())
        at = _where(i, tuple(ratio.shape))
        msg = ("%s: %d of %d elements out of bounds; worst at %s: got %.9g want %.9g bound %.3g (ratio %.3g)"
               % (what, bad, ratio.numel(), at, float(g.flatten()[i]), float(want.flatten()[i]), float(bound.flatten()[i]), worst))
        if fails is None:
            raise AssertionError(msg)
        fails.append(msg)
    return worst


def _assert_integral(exact, what):
    assert bool((exact == exact.round()).all()), what + ": reference is not integral (operands not integers?)"
    assert float(exact.abs().max()) < EXACT_LIMIT, what + ": reference reaches 2^24, f32 sums would round"


def check_exact_f32(got, exact, what: str) -> None:
    """an f32 output from integer operands: bit-equal to the exact f64 sum"""
    _assert_integral(exact, what)
    g = got.detach().reshape(exact.shape)
    assert g.dtype == torch.float32, what
    want = exact.to(torch.float32)
    ne = g != want
    if bool(ne.any()):
        i = int(ne.flatten().nonzero()[0])
        raise AssertionError("%s: %d of %d elements differ; first at %s: got %r want %r" % (
            what, int(ne.sum()), ne.numel(), _where(i, tuple(ne.shape)), float(g.flatten()[i]), float(want.flatten()[i])))


def rne_bf16(exact: torch.Tensor) -> torch.Tensor:
    """an integral f64 tensor below 2^24 rounded ONCE to bf16, nearest-even (the f32 step is exact there)"""
    return exact.to(torch.float32).to(torch.bfloat16)


def check_exact_bf16(got, exact, what: str) -> None:
    """a bf16 output from integer operands: bit-equal to the exact sum rounded once to nearest-even"""
    _assert_integral(exact, what)
    g = got.detach().reshape(exact.shape)
    assert g.dtype == torch.bfloat16, what
    want = rne_bf16(exact)
    ne = g.view(torch.int16) != want.view(torch.int16)
    if bool(ne.any()):
        i = int(ne.flatten().nonzero()[0])
        raise AssertionError("%s: %d of %d elements differ; first at %s: got %r want %r (exact %r)" % (
            what, int(ne.sum()), ne.numel(), _where(i, tuple(ne.shape)), float(g.flatten()[i]), float(want.flatten()[i]),
            float(exact.flatten()[i])))


# ------------------------------------------------------------------------------------------------ the net's graph
def consumers(layers, idx):
    """(layer, how) for every layer that reads layer idx's output: "direct" (as src), "up" (as src_up, upsampled 2x and
    concatenated after src), "add" (as a residual shortcut)"""
    out = []
    for m in layers:
        if m.src == idx:
            out.append((m, "direct"))
        if m.src_up == idx:
            out.append((m, "up"))
        if m.shortcut == idx:
            out.append((m, "add"))
    return out


def output_grad_ref(layer, by_idx, weights_bf16, dx_of, grad_of):
    """float64 gradient wrt layer's output from its consumers, teacher-forced: each consumer's output gradient as the
    kernels left it (``dx_of(m)`` [B,Ho,Wo,cout]; ``grad_of(m)`` = the residual layer's materialised output gradient) and
    its bf16-rounded weights (``weights_bf16(m)``).

    Returns (want, acc, twin): acc = sum over contributions of |contribution| (for the "up" path, of every pre-upsample
    element: the step stores them in bf16 one by one), twin = the same computation on |dx| and |w|."""
    want = acc = twin = None
    for m, how in consumers(by_idx.values(), layer.idx):
        if how == "add":
            c = f64(grad_of(m))
            ca, ct = c.abs(), c.abs()
        else:
            w = f64(weights_bf16(m))
            lo = 0 if how == "direct" else by_idx[m.src].cout
            w = w[:, :, lo:lo + layer.cout, :]
            d = dx_of(m)
            c = dgrad_ref(d, w, m.stride, m.H, m.W)
            ca = c.abs()
            ct = dgrad_ref(f64(d).abs(), w.abs(), m.stride, m.H, m.W)
            if how == "up":
                c, ca, ct = upsample2_bwd(c), upsample2_bwd(ca), upsample2_bwd(ct)
        want = c if want is None else want + c
        acc = ca if acc is None else acc + ca
        twin = ct if twin is None else twin + ct
    return want, acc, twin


def grad_bound(want, acc, twin, c_rel, c_acc, c_twin):
    """bound of an output gradient the step stores in bf16 (one rounding per contribution) from f32 sums"""
    return c_rel * want.abs() + c_acc * acc + c_twin * twin


def layer_input(layer, by_idx, image_bf16=None, act_of=None):
    """what layer convolves, float64: the bf16-rounded image (layer 1), src.act, or cat(src.act, upsample2(src_up.act))"""
    act_of = act_of or (lambda m: m.act)
    if layer.src == 0:
        return f64(image_bf16)
    x = f64(act_of(by_idx[layer.src]))
    if layer.src_up is not None:
        x = concat_input(x, act_of(by_idx[layer.src_up]))
    return x

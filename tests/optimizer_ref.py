"""Float64 references of the optimizer tail (Adam sweeps, their finish, the l2 term, the re-pack of the bf16 operands),
the bounds the kernels are held to, and the inputs the tests share.

Test infrastructure (imported by tests/test_gpu_optimizer.py and tests/test_optimizer_ref.py), the optimizer counterpart
of tests/forward_ref.py / tests/backward_ref.py.  Plain numpy / torch on the CPU; nothing here calls this project's kernels.

The kernels take beta1, beta2, epsilon, l2, the gradient scale and the learning rate as f32, so the references use those
f32 values (``f32v``) in float64: 1 - beta is then exact in f32 too and does not enter the count.

Bounds, by counting f32 roundings (u = 2^-24 is one rounding to nearest); none is taken from a kernel's output:
  * g' = g*grad_scale + l2*w (on [0, n_decay)): two products and a sum, each within u of its result:
    |err g'| <= u*(|g*gs| + |l2*w| + |g'|) = u*(2|g'| + c), c = |g*gs| + |l2*w| - |g'| >= 0 (0 unless the two terms cancel);
  * m' = b1*m + (1-b1)*g': two products and a sum on top of err g': within u*(2|b1*m| + 4|(1-b1)g'| + 2|m'|) without
    cancellation, inside  2^-21 * (|b1*m| + |(1-b1)*g'|)  = ``bound_m``;
  * v' = b2*v + (1-b2)*g'^2: g'^2 carries 2*(2u) of g' and one product, then two products and a sum: 8u = 2^-21
    relative to v' (all terms are non-negative) = ``bound_v``;
  * w' = w - lr_t*m'/(sqrt(v') + eps): one rounding of the result (2^-23 * |w'| allows two), and the step itself through
    the 8u of m', half the 8u of v', the f32 lr_t, the square root, the sum, the product and a division that may be
    approximate: 2^-20 * |w' - w| = ``bound_w``.
Where g*gs and l2*w cancel, the error of g' is no longer small relative to g', and the m' and v' bounds grow by exactly what
that lets through (``cancellation`` below): (1-b1)*u*c on m' and (1-b2)*(2u*|g'|*c + u^2*(2|g'| + c)^2) on v'.  It shows
only from zero moments (a handful of elements in a million); without cancellation both terms are 0 and the bounds are the
ones above.  The w' bound needs no such term: the step of such an element is tiny against 2^-23*|w'|.
  * an l2 sum accumulated per thread in f32: every square is one rounding, a thread adds T of them, the wave and block
    reduction adds 8 more levels: (T + 10)*u relative to the float64 sum (all terms are non-negative, so the relative
    bound holds whatever the order, and for the sum of the per-block partials as for each of them);
    T = ceil(n / (blocks*256)).  At the 4099 elements of test_fused_adam_matches_the_plain_sweep that is 15u = 9e-7 plus
    the finish: inside that test's 2e-6;
  * the finish adds the f32 partials in double and rounds once, 0.5*l2 is exact in f32: 2^-23 relative to the float64
    sum of the f32 partials times 0.5*l2 allows that rounding twice.
"""
import functools
import math

import numpy as np
import torch

import disyolo_oracle as O
from test_gpu_conv import pack_ref

U = 2.0 ** -24


def f32v(x) -> float:
    """the value a kernel receives for a float argument"""
    return float(np.float32(x))


LR, B1, B2, EPS, L2 = f32v(1e-4), f32v(0.9), f32v(0.999), f32v(1e-8), f32v(5e-4)
GRAD_SCALE = 0.5
FINISH_REL = 2.0 ** -23


# ------------------------------------------------------------------------------------------------ one Adam step
def adam_ref(w, g, m, v, t, n_decay, grad_scale=GRAD_SCALE, lr=LR, l2=L2):
    """one TF-form step in float64 from f32 state: dict of w', m', v', g' (g*grad_scale + l2*w on [0, n_decay)) and the
    pieces the bounds need"""
    w, g, m, v = (np.asarray(a, np.float64) for a in (w, g, m, v))
    gs = g * float(grad_scale)
    dec = np.zeros_like(w)
    dec[:n_decay] = l2 * w[:n_decay]
    gp = gs + dec
    tw, tm, tv = O.adam_tf_step(torch.from_numpy(w), torch.from_numpy(gp), torch.from_numpy(m), torch.from_numpy(v), int(t),
                                lr=lr, b1=B1, b2=B2, eps=EPS)
    lr_t = lr * math.sqrt(1.0 - B2 ** t) / (1.0 - B1 ** t)
    return {"w": tw.numpy(), "m": tm.numpy(), "v": tv.numpy(), "gp": gp, "w0": w, "m0": m, "v0": v, "lr_t": lr_t,
            "cancel_g": np.abs(gs) + np.abs(dec) - np.abs(gp)}


def cancellation(r):
    """what cancellation in g' adds to the m' and v' bounds (module docstring): zeros where nothing cancels"""
    gp, c = np.abs(r["gp"]), np.maximum(r["cancel_g"], 0.0)
    xm = (1.0 - B1) * U * c
    xv = (1.0 - B2) * (2.0 * U * gp * c + U * U * (2.0 * gp + c) ** 2 * (c > 0))
    return xm, xv


def adam_bounds(r):
    """(bound_m, bound_v, bound_w) of a step ``r = adam_ref(...)``"""
    xm, xv = cancellation(r)
    bm = 2.0 ** -21 * (np.abs(B1 * r["m0"]) + np.abs((1.0 - B1) * r["gp"])) + xm
    bv = 2.0 ** -21 * r["v"] + xv
    bw = 2.0 ** -23 * np.abs(r["w"]) + 2.0 ** -20 * np.abs(r["w"] - r["w0"])
    return bm, bv, bw


def adam_f32(w, g, m, v, t, n_decay, grad_scale=GRAD_SCALE, lr=LR, l2=L2):
    """the step restated in numpy f32, operation by operation as the kernels write it (the restatement of
    test_fused_adam_matches_the_plain_sweep)"""
    f = np.float32
    w, m, v = (np.asarray(a, f) for a in (w, m, v))
    gr = np.asarray(g, f) * f(grad_scale)
    gr[:n_decay] += f(l2) * w[:n_decay]
    mr = f(B1) * m + (f(1) - f(B1)) * gr
    vr = f(B2) * v + (f(1) - f(B2)) * gr * gr
    lr_t = f(lr * math.sqrt(1.0 - B2 ** t) / (1.0 - B1 ** t))
    wr = w - lr_t * mr / (np.sqrt(vr) + f(EPS))
    return wr, mr, vr


def worst(got, want, bound):
    """largest |got - want| / bound and where; elements whose bound is 0 must match exactly"""
    err = np.abs(np.asarray(got, np.float64) - want)
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    i = int(np.argmax(ratio))
    return float(ratio[i]), i


def assert_step_within_bounds(got_w, got_m, got_v, r, what=""):
    bm, bv, bw = adam_bounds(r)
    for name, got, bound in (("m", got_m, bm), ("v", got_v, bv), ("w", got_w, bw)):
        assert np.isfinite(np.asarray(got)).all(), "%s %s': non-finite values" % (what, name)
        ratio, i = worst(got, r[name], bound)
        assert ratio <= 1.0, "%s %s': element %d is %.3g of its bound off (got %r, float64 %r)" % (
            what, name, i, ratio, float(np.asarray(got)[i]), float(r[name][i]))


# ------------------------------------------------------------------------------------------------ the l2 term
def l2_sumsq(w, n_decay) -> float:
    return float((np.asarray(w[:n_decay], np.float64) ** 2).sum())


def l2_term(w, n_decay, l2=L2) -> float:
    """0.5 * l2 * sum(w[:n_decay]^2) of the weights handed in (the pre-update ones)"""
    return 0.5 * l2 * l2_sumsq(w, n_decay)


def thread_sum_rel(n, blocks) -> float:
    """(T + 10) * 2^-24, T = elements one of the blocks*256 threads adds"""
    return (-(-int(n) // (int(blocks) * 256)) + 10) * U


def finish_ref(parts, l2=L2) -> float:
    """the float64 sum of the f32 partials times 0.5*l2"""
    return float(np.asarray(parts, np.float64).sum()) * 0.5 * l2


def sweep_blocks(n) -> int:
    """partials one sweep over n elements writes: ceil(n / 1024), at most 2048"""
    return max(1, min(2048, -(-int(n) // 1024)))


def l2_blocks(n) -> int:
    """blocks of the stand-alone l2 kernel: ceil(n / 2048), at most 1024"""
    return max(1, min(1024, -(-int(n) // 2048)))


# ------------------------------------------------------------------------------------------------ packed layouts
def fwd_layout(w_hwio: torch.Tensor) -> torch.Tensor:
    """forward operand [Cout][kh kw ci]"""
    return pack_ref(w_hwio)


def dgrad_layout(w_hwio: torch.Tensor, cout_pad: int) -> torch.Tensor:
    """data-gradient operand [Cin][taps'][cout_pad]: out[ci][t'][co] = w[taps-1-t'][ci][co], pad channels zero"""
    k, _, cin, cout = w_hwio.shape
    taps = k * k
    wt = w_hwio.reshape(taps, cin, cout)
    out = torch.zeros(cin, taps, cout_pad, dtype=w_hwio.dtype)
    for tp in range(taps):
        out[:, tp, :cout] = wt[taps - 1 - tp]
    return out.reshape(cin, taps * cout_pad)


def pack_blocks(jobs) -> int:
    """blocks of one pack-table launch; jobs = (k, Cin, Cout, cout_pad, has data-gradient operand)"""
    total = 0
    for k, cin, cout, pad, dg in jobs:
        K = k * k * cin
        total += -(-K // 64) * -(-cout // 64)
        if dg:
            total += -(-(cin * k * k * max(pad, cout)) // 4096)
    return total


# ------------------------------------------------------------------------------------------------ shared inputs
CAP_N = 2 * 2048 * 1024 + 7           # every thread of the capped sweep grid makes two grid-stride iterations
SLICES = (5000, 1100003, 3)           # contiguous slices of one arena: offsets 0, 5000, 1105003 (the last: 3 mod 4)
FINISH_NPARTS = (1, 255, 256, 257, 2053)
L2_NS = (1, 2047, 2 * 1024 * 2048 + 3)

PACK_JOBS = (
    # k, Cin, Cout, cout_pad, data-gradient operand
    (1, 1024, 72, 72, False),
    (3, 8, 24, 32, True),
    (1, 64, 64, 64, True),
    (3, 64, 128, 128, True),
    (3, 32, 9, 32, True),
    (1, 8, 8, 8, True),
    (1, 96, 24, 32, False),
)


@functools.lru_cache(maxsize=None)
def adam_inputs(n, seed=0):
    """f32 (w, g, m, v) of one step: non-zero moments of the size a few steps leave, so that a wrong moment shows in w'"""
    gen = torch.Generator().manual_seed(1000 + seed)
    w = torch.randn(n, generator=gen)
    g = torch.randn(n, generator=gen)
    m = 0.3 * torch.randn(n, generator=gen)
    v = 0.05 * torch.randn(n, generator=gen) ** 2 + 1e-6
    out = tuple(a.numpy() for a in (w, g, m, v))
    for a in out:
        a.setflags(write=False)
    return out


STEP_DEV_N = 4096 * 256 + 4099        # adam_step_dev's grid is capped at 4096 blocks: some threads make a second iteration
STEP_DEV_DECAY = 349333


def step_dev_inputs():
    """(w, g, m, v) of adam_step_dev's first step: zero moments, as a training run starts"""
    w, g, _, _ = adam_inputs(STEP_DEV_N, 30)
    z = np.zeros(STEP_DEV_N, np.float32)
    z.setflags(write=False)
    return w, g, z, z


@functools.lru_cache(maxsize=None)
def finish_parts(nparts):
    """f32 partials from 1e-8 to 1e4 that no f32 accumulation can add within 2^-23, neither a running sum nor a pairwise
    (butterfly) tree over 64 lanes.  Each run of 64 starts with 1e4 (spacing of f32 there: 2^-10); the other 63 fall into six
    groups (by the lowest set bit of their position) of 1, 2, 4 ... 32 equal values that add up, exactly, to 0.45 of that
    spacing per group: whenever a whole group, or a single value, meets the 1e4 in f32 it is rounded away, 6 * 0.45
    spacings = 2.2 * 2^-23 relative in all.  Entries beyond the first 256 are tiny (1e-8 ... 1e-7): a thread that
    strides over the partials by 256 adds them to its first one."""
    big, lost = 1e4, 0.45 * 2.0 ** -10
    i = np.arange(nparts)
    lane = i % 64
    lsb = np.where(lane > 0, lane & -lane, 64)
    p = np.where(lane == 0, big, lost * lsb / 32.0)
    gen = torch.Generator().manual_seed(77 + nparts)
    tiny = 10.0 ** (torch.rand(nparts, generator=gen, dtype=torch.float64).numpy() - 8.0)
    p = np.where(i < 256, p, tiny)
    if nparts > 37:
        p[37] = 1e-8
    out = p.astype(np.float32)
    out.setflags(write=False)
    return out


def f32_running_sum(parts) -> np.float32:
    s = np.float32(0)
    for x in np.asarray(parts, np.float32):
        s = np.float32(s + x)
    return s


def bf16_ties(e: int):
    """f32 values exactly half way between two bf16 neighbours at exponent e: odd and even mantissa below the tie, so
    round-to-nearest-even goes up for one and down for the other (and the other way round for the negatives)"""
    base = 2.0 ** e
    ulp = base * 2.0 ** -7                 # bf16 spacing in [2^e, 2^(e+1))
    return [base + ulp / 2, base + ulp + ulp / 2, -(base + ulp / 2), -(base + ulp + ulp / 2)]


@functools.lru_cache(maxsize=None)
def pack_weights_for(job_index):
    """HWIO f32 weights of PACK_JOBS[job_index], drawn from (job_index + 1) + [0.25, 0.75) with random sign -- ranges of
    different jobs do not overlap, so an output written from another job's weights cannot match -- with +0, -0 and
    exact bf16 ties planted"""
    k, cin, cout, _, _ = PACK_JOBS[job_index]
    gen = torch.Generator().manual_seed(300 + job_index)
    w = (job_index + 1) + 0.25 + 0.5 * torch.rand(k, k, cin, cout, generator=gen)
    w = w * (torch.randint(0, 2, w.shape, generator=gen) * 2 - 1).float()
    flat = w.view(-1)
    special = [0.0, -0.0] + bf16_ties(int(math.floor(math.log2(job_index + 1.25))))
    pos = torch.randperm(flat.numel(), generator=gen)[:4 * len(special)]
    for i, p in enumerate(pos.tolist()):
        flat[p] = special[i % len(special)]
    return w

"""CPU tests of tests/backward_ref.py: the float64 references agree with autograd of the oracle, and the checkers reject
planted defects of the kinds the GPU tests (tests/test_gpu_backward.py) are there to catch.  No GPU."""
from types import SimpleNamespace

import pytest
import torch

import backward_ref as R
import disyolo_oracle as O

F64 = torch.float64


def _randn(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=F64)


def _ints(lo, hi, *shape, seed=0, nonzero=False):
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(lo, hi + 1, shape, generator=g).to(F64)
    if nonzero:
        t = torch.where(t == 0, torch.ones_like(t), t)
    return t


# ------------------------------------------------------------------------------------------------ references vs autograd
def test_bn_closed_form_equals_autograd_of_the_oracle():
    B, H, W, C = 2, 5, 3, 6
    x = _randn(B, H, W, C, seed=1) * 3 + 0.5
    gamma, beta = _randn(C, seed=2) + 1.0, _randn(C, seed=3)
    params = {"yolo/convolutional7/BatchNorm/" + k: v for k, v in
              (("gamma", gamma), ("beta", beta), ("moving_mean", torch.zeros(C, dtype=F64)),
               ("moving_variance", torch.ones(C, dtype=F64)))}
    xr, gr, br = x.clone().requires_grad_(), gamma.clone().requires_grad_(), beta.clone().requires_grad_()
    params["yolo/convolutional7/BatchNorm/gamma"], params["yolo/convolutional7/BatchNorm/beta"] = gr, br
    y = O.leaky_relu(O.batch_norm(xr, params, 7, False, True, None))
    g = _randn(B, H, W, C, seed=4)
    (y * g).sum().backward()
    mean = x.mean((0, 1, 2))
    var = ((x - mean) ** 2).mean((0, 1, 2))
    rstd = 1.0 / torch.sqrt(var + O.BN_EPS)
    scale = gamma * rstd
    r = R.bn_act_bwd_ref(g, x, scale, beta - mean * scale, mean, rstd, gamma)
    assert not bool(r["amb"].any())
    torch.testing.assert_close(r["dx"], xr.grad.reshape(-1, C), rtol=1e-11, atol=1e-12)
    torch.testing.assert_close(r["dgamma"], gr.grad, rtol=1e-11, atol=1e-12)
    torch.testing.assert_close(r["dbeta"], br.grad, rtol=1e-11, atol=1e-12)


@pytest.mark.parametrize("k,stride,H,W", [(3, 1, 7, 6), (3, 2, 8, 8), (3, 2, 9, 7), (1, 1, 5, 4)])
def test_conv_gradients_equal_autograd_of_the_oracle(k, stride, H, W):
    B, C, Co = 2, 5, 4
    x = _randn(B, H, W, C, seed=5).requires_grad_()
    w = _randn(k, k, C, Co, seed=6).requires_grad_()
    y = O.conv2d_same(x, w, stride)
    dy = _randn(*y.shape, seed=7)
    (y * dy).sum().backward()
    torch.testing.assert_close(R.wgrad_ref(x.detach(), dy, k, stride), w.grad, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(R.dgrad_ref(dy, w.detach(), stride, H, W), x.grad, rtol=1e-12, atol=1e-12)


def test_concat_gradients_equal_autograd_of_the_oracle():
    B, H, W, Ca, Cb, Co = 2, 6, 4, 3, 5, 4
    a = _randn(B, H, W, Ca, seed=8).requires_grad_()
    b = _randn(B, H // 2, W // 2, Cb, seed=9).requires_grad_()
    w = _randn(1, 1, Ca + Cb, Co, seed=10).requires_grad_()
    y = O.conv2d_same(torch.cat([a, O.upsample2(b)], -1), w, 1)
    dy = _randn(*y.shape, seed=11)
    (y * dy).sum().backward()
    x = R.concat_input(a.detach(), b.detach())
    torch.testing.assert_close(R.wgrad_ref(x, dy, 1, 1), w.grad, rtol=1e-12, atol=1e-12)
    wd = w.detach()
    torch.testing.assert_close(R.dgrad_ref(dy, wd[:, :, :Ca], 1, H, W), a.grad, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(R.upsample2_bwd(R.dgrad_ref(dy, wd[:, :, Ca:], 1, H, W)), b.grad, rtol=1e-12, atol=1e-12)


def _fake_net(C=4, H=6, W=6, B=2, seed=12):
    """layer 57 with its two consumers (58: 3x3, 60: 1x1), and a concat layer 61 reading 60 as src_up"""
    mk = lambda **kw: SimpleNamespace(**{"src_up": None, "shortcut": None, **kw})
    by = {57: mk(idx=57, src=56, cout=C, H=H, W=W, k=1, stride=1),
          58: mk(idx=58, src=57, cout=6, H=H, W=W, k=3, stride=1),
          60: mk(idx=60, src=57, cout=3, H=H, W=W, k=1, stride=1),
          43: mk(idx=43, src=42, cout=2, H=2 * H, W=2 * W, k=1, stride=1),
          61: mk(idx=61, src=43, src_up=60, cout=5, H=2 * H, W=2 * W, k=1, stride=1)}
    for i, m in by.items():
        cin = {58: C, 60: C, 61: 2 + 3}.get(i, 1)
        m.w = _randn(m.k, m.k, cin, m.cout, seed=seed + i)
        m.dx = _randn(B, m.H, m.W, m.cout, seed=seed + 100 + i)
        m.act = _randn(B, m.H, m.W, m.cout, seed=seed + 200 + i)
    return by


def _output_grad(by, idx):
    return R.output_grad_ref(by[idx], by, lambda m: m.w, lambda m: m.dx, lambda m: None)


def test_output_gradient_equals_autograd_of_both_consumers_and_the_upsample():
    by = _fake_net()
    x57 = by[57].act.clone().requires_grad_()
    x60 = by[60].act.clone().requires_grad_()
    y58 = O.conv2d_same(x57, by[58].w, 1)
    y60 = O.conv2d_same(x57, by[60].w, 1)
    y61 = O.conv2d_same(torch.cat([by[43].act, O.upsample2(x60)], -1), by[61].w, 1)
    ((y58 * by[58].dx).sum() + (y60 * by[60].dx).sum() + (y61 * by[61].dx).sum()).backward()
    want, acc, twin = _output_grad(by, 57)
    torch.testing.assert_close(want, x57.grad, rtol=1e-12, atol=1e-12)
    assert bool((acc >= want.abs() - 1e-12).all()) and bool((twin >= acc - 1e-12).all())
    torch.testing.assert_close(_output_grad(by, 60)[0], x60.grad, rtol=1e-12, atol=1e-12)


# ------------------------------------------------------------------------------------------------ planted defects
def test_exact_dw_rejects_a_dropped_pixel_swapped_taps_and_shifted_concat_channels():
    B, H, W = 2, 6, 6
    a = _ints(-2, 2, B, H, W, 3, seed=20, nonzero=True)
    b = _ints(-2, 2, B, H // 2, W // 2, 2, seed=21, nonzero=True)
    dy = _ints(-2, 2, B, H, W, 4, seed=22, nonzero=True)
    x = R.concat_input(a, b)
    exact = R.wgrad_ref(x, dy, 3, 1)
    R.check_exact_f32(exact.float(), exact, "control")
    dropped = dy.clone()
    dropped[1, 2, 3] = 0
    with pytest.raises(AssertionError, match="differ"):
        R.check_exact_f32(R.wgrad_ref(x, dropped, 3, 1).float(), exact, "dropped pixel")
    swapped = exact.clone()
    swapped[0, 0], swapped[0, 1] = exact[0, 1], exact[0, 0]
    with pytest.raises(AssertionError, match="differ"):
        R.check_exact_f32(swapped.float(), exact, "swapped taps")
    shifted = x.clone()
    shifted[..., 3:] = torch.roll(x[..., 3:], 1, dims=-1)
    with pytest.raises(AssertionError, match="differ"):
        R.check_exact_f32(R.wgrad_ref(shifted, dy, 3, 1).float(), exact, "concat channels off by one")


def test_exact_bf16_rejects_one_ulp_and_truncation():
    exact = _ints(-6000, 6000, 4096, seed=23)
    R.check_exact_bf16(R.rne_bf16(exact), exact, "control")
    off = R.rne_bf16(exact).clone()
    off.view(torch.int16)[17] += 1
    with pytest.raises(AssertionError, match="1 of 4096"):
        R.check_exact_bf16(off, exact, "one ulp")
    trunc = (exact.to(torch.float32).view(torch.int32) & ~0xFFFF).view(torch.float32).to(torch.bfloat16)
    with pytest.raises(AssertionError, match="differ"):
        R.check_exact_bf16(trunc, exact, "truncation")
    with pytest.raises(AssertionError, match="integral"):
        R.check_exact_bf16(R.rne_bf16(exact), exact + 0.5, "non-integer reference")


def test_dw_bound_rejects_one_output_channel_off_by_2_to_the_minus_9():
    x = R.bf16_round(_randn(2, 8, 8, 16, seed=24))
    dy = R.bf16_round(_randn(2, 8, 8, 8, seed=25))
    want = R.wgrad_ref(x, dy, 3, 1)
    bound = R.C_DW * R.wgrad_ref(x.abs(), dy.abs(), 3, 1)
    R.check_bounded(want.float(), want, bound, "control")
    bad = want.float().clone()
    bad[..., 5] *= 1 + 2.0 ** -9
    with pytest.raises(AssertionError, match="out of bounds"):
        R.check_bounded(bad, want, bound, "dW channel 5 scaled")


def test_g_bound_rejects_a_missing_second_consumer():
    by = _fake_net()
    want, acc, twin = _output_grad(by, 57)
    bound = R.grad_bound(want, acc, twin, R.C_G_REL, R.C_G_ACC, R.C_G_TWIN)
    R.check_bounded(want.to(torch.bfloat16), want, bound, "control")
    only58 = R.dgrad_ref(by[58].dx, by[58].w, 1, 6, 6)          # 57 without 60's contribution
    with pytest.raises(AssertionError, match="out of bounds"):
        R.check_bounded(only58.to(torch.bfloat16), want, bound, "57 without 60")


def _bn_case(M=512, C=8, seed=26):
    raw = R.bf16_round(_randn(M, C, seed=seed) * 2 + 0.3)
    g = R.bf16_round(_randn(M, C, seed=seed + 1))
    mean, rstd = raw.mean(0), 1.0 / raw.std(0, unbiased=False)
    gamma = _randn(C, seed=seed + 2) + 1.5
    scale = gamma * rstd
    shift = _randn(C, seed=seed + 3) * 0.1 - mean * scale
    r = R.bn_act_bwd_ref(g, raw, scale, shift, mean, rstd, gamma)
    return raw, g, scale, shift, mean, rstd, gamma, r


def test_dx_bound_rejects_the_leaky_slope_from_the_wrong_side():
    raw, g, scale, shift, mean, rstd, gamma, r = _bn_case()
    bdx, _, _ = R.bn_bounds(r, R.C_DX_REL, R.C_DX_FIRST, R.C_SUM_SQRT_OWN, R.C_SUM_ABS_OWN)
    R.check_bounded(r["dx"].to(torch.bfloat16), r["dx"], bdx, "control")
    z = raw * scale + shift
    gp = g * torch.where(z < 0, torch.ones_like(z), torch.full_like(z, R.ALPHA))     # (the slope of the other side)
    xh = (raw - mean) * rstd
    wrong = gamma * rstd * (gp - gp.mean(0) - xh * (gp * xh).mean(0))
    with pytest.raises(AssertionError, match="out of bounds"):
        R.check_bounded(wrong.to(torch.bfloat16), r["dx"], bdx, "slope from the wrong side")


def test_dgamma_bound_rejects_missing_rows():
    _, _, _, _, _, _, _, r = _bn_case()
    _, bdg, bdb = R.bn_bounds(r, R.C_DX_REL, R.C_DX_FIRST, R.C_SUM_SQRT, R.C_SUM_ABS)
    R.check_bounded(r["dgamma"].float(), r["dgamma"], bdg, "control")
    R.check_bounded(r["dbeta"].float(), r["dbeta"], bdb, "control")
    short = (r["gp"] * r["xh"])[:-64].sum(0)
    with pytest.raises(AssertionError, match="out of bounds"):
        R.check_bounded(short.float(), r["dgamma"], bdg, "dgamma without its last 64 rows")

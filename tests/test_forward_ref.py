"""CPU checks of tests/forward_ref.py: its references agree with the oracle's network, and its checkers reject the
defects a forward kernel could plausibly have (tests/test_gpu_forward.py relies on both)."""
import pytest
import torch

import backward_ref as R
import disyolo_oracle as O
import forward_ref as FR
from disyolo_amd.net import build_topology

F64 = torch.float64


# ------------------------------------------------------------------------------------------------ against the oracle
@pytest.fixture(scope="module")
def oracle_run():
    """the oracle's stage-2 network in float64 at 64^2, B = 2, training mode: every activation and the moving-average updates"""
    torch.manual_seed(0)
    lock = O.default_lock(2)
    p = {k: v.double() for k, v in O.init_params(seed=1, lock=lock).items()}
    img = torch.rand(2, 64, 64, 3, dtype=F64)
    taps, upd = {}, {}
    O.build_network(p, img, True, lock, upd, taps)
    return p, img, taps, upd


def _layer_ref(l, by, p, img, taps, training):
    act_of = lambda m: taps["act%d" % m.idx]
    x = R.layer_input(l, by, image_bf16=img, act_of=act_of)
    w = p[O._name(l.idx, "weights")]
    if l.kind == "lin":
        return FR.stage_ref(x, w, l.stride, shift=p[O._name(l.idx, "biases")], act=False)["y"], None
    g, b = p[O._name(l.idx, "BatchNorm/gamma")], p[O._name(l.idx, "BatchNorm/beta")]
    res = taps["act%d" % l.shortcut] if l.shortcut is not None else None
    if training:
        c = FR.conv_ref(x, w, l.stride, twin=False)
        mean, var = FR.moments(c)
        sc, sh, _, _ = FR.coeffs_from(g, b, mean, 1.0 / torch.sqrt(var + FR.BN_EPS))
        y = FR.leaky(c * sc + sh)
        return (y + res if res is not None else y), (mean, var)
    sc, sh = FR.bn_fold_ref(g, b, p[O._name(l.idx, "BatchNorm/moving_mean")], p[O._name(l.idx, "BatchNorm/moving_variance")])
    return FR.stage_ref(x, w, l.stride, sc, sh, res)["y"], None


def test_references_match_the_oracle_network_layer_by_layer(oracle_run):
    p, img, taps, upd = oracle_run
    layers = build_topology(3, 3)
    by = {l.idx: l for l in layers}
    for l in layers:
        want = taps["act%d" % l.idx]
        got, mom = _layer_ref(l, by, p, img, taps, True)
        got = got.reshape(want.shape)
        assert float((got - want).abs().max()) <= 1e-9 * (1.0 + float(want.abs().max())), l.idx
        if mom is not None:
            mm0 = p[O._name(l.idx, "BatchNorm/moving_mean")]
            mv0 = p[O._name(l.idx, "BatchNorm/moving_variance")]
            # (the oracle's decay is the f64 0.997, the kernels' -- and FR's -- the f32 value: 1 - decay differs by 7e-6)
            wmm, _ = FR.moving_ref(mm0, mom[0], torch.zeros_like(mm0))
            wmv, _ = FR.moving_ref(mv0, mom[1], torch.zeros_like(mv0))
            assert torch.allclose(wmm, upd[O._name(l.idx, "BatchNorm/moving_mean")], rtol=1e-5, atol=1e-12)
            assert torch.allclose(wmv, upd[O._name(l.idx, "BatchNorm/moving_variance")], rtol=1e-6, atol=1e-12)


def test_inference_references_match_the_oracle(oracle_run):
    p, img, _, _ = oracle_run
    lock = O.default_lock(2)
    taps = {}
    O.build_network(p, img, False, lock, None, taps)
    layers = build_topology(3, 3)
    by = {l.idx: l for l in layers}
    for l in layers:
        want = taps["act%d" % l.idx]
        got = _layer_ref(l, by, p, img, taps, False)[0].reshape(want.shape)
        assert float((got - want).abs().max()) <= 1e-9 * (1.0 + float(want.abs().max())), l.idx


def test_batch_norm_statistics_match_the_oracle():
    torch.manual_seed(1)
    y = torch.randn(3, 5, 7, 6, dtype=F64) * 2 + 1
    mean, var = FR.moments(y)
    params = {O._name(9, "BatchNorm/gamma"): torch.ones(6, dtype=F64), O._name(9, "BatchNorm/beta"): torch.zeros(6, dtype=F64),
              O._name(9, "BatchNorm/moving_mean"): torch.zeros(6, dtype=F64),
              O._name(9, "BatchNorm/moving_variance"): torch.ones(6, dtype=F64)}
    xhat = O.batch_norm(y, params, 9, False, True, None)
    assert torch.allclose((y - mean) / torch.sqrt(var + O.BN_EPS), xhat, rtol=1e-12, atol=1e-12)


def test_rne_e4m3_is_torch_float8_rounding():
    # every code, every midpoint between neighbours, points just off them, beyond the range, signs, subnormals
    codes = torch.arange(256, dtype=torch.int32).to(torch.uint8)
    vals = FR.decode_e4m3(codes)
    fin = torch.sort(vals[torch.isfinite(vals)].unique()).values
    mids = (fin[1:] + fin[:-1]) / 2
    xs = torch.cat([fin, mids, mids * (1 + 2.0 ** -20), mids * (1 - 2.0 ** -20), torch.tensor([449.0, 470.0, 1e4, -1e4]),
                    torch.rand(4000, dtype=F64) * 2 ** torch.randint(-12, 10, (4000,)).double() * torch.sign(torch.randn(4000, dtype=F64))])
    want = xs.float().clamp(-448, 448).to(torch.float8_e4m3fn).float().double()
    got = FR.rne_e4m3(xs)
    assert torch.equal(got, want)


# ------------------------------------------------------------------------------------------------ planted defects
def _bf(t):
    return t.to(torch.bfloat16).to(F64)


@pytest.fixture(scope="module")
def layer():
    g = torch.Generator().manual_seed(3)
    x = _bf(torch.randn(2, 16, 16, 8, generator=g, dtype=F64))
    up = _bf(torch.randn(2, 8, 8, 4, generator=g, dtype=F64))
    w = _bf(torch.randn(3, 3, 8, 16, generator=g, dtype=F64) * 0.3)
    wc = _bf(torch.randn(1, 1, 12, 16, generator=g, dtype=F64) * 0.3)
    sc = torch.rand(16, generator=g, dtype=F64) + 0.5
    sh = torch.randn(16, generator=g, dtype=F64) * 0.3
    res = _bf(torch.randn(2, 16, 16, 16, generator=g, dtype=F64))
    return dict(x=x, up=up, w=w, wc=wc, sc=sc, sh=sh, res=res)


def _kernel_like(y):
    """what a correct kernel stores: the f32 value rounded once to bf16"""
    return y.float().to(torch.bfloat16)


def _rejects(got, want, bound):
    with pytest.raises(AssertionError):
        R.check_bounded(got, want, bound, "planted")


def test_correct_outputs_pass(layer):
    s = FR.stage_ref(layer["x"], layer["w"], 1, layer["sc"], layer["sh"], layer["res"])
    assert R.check_bounded(_kernel_like(s["y"]), s["y"], FR.bf16_bound(s), "ok") <= 1.0


def test_rejects_symmetric_padding_on_a_stride2_layer(layer):
    x, w = layer["x"], layer["w"]
    s = FR.stage_ref(x, w, 2, layer["sc"], layer["sh"])
    # TF-SAME pads a 3x3 stride-2 conv of an even size by (0, 1); symmetric (1, 1) shifts every output by one input pixel
    xs = torch.nn.functional.pad(x, (0, 0, 1, 1, 1, 1))
    bad = torch.zeros_like(s["y"])
    for ky in range(3):
        for kx in range(3):
            bad += xs[:, ky:ky + 15:2, kx:kx + 15:2, :] @ w[ky, kx]
    _rejects(_kernel_like(FR.leaky(bad * layer["sc"] + layer["sh"])), s["y"], FR.bf16_bound(s))


def test_rejects_swapped_concat_halves_and_an_offset_upsample(layer):
    x, up, wc = layer["x"], layer["up"], layer["wc"]
    s = FR.stage_ref(R.concat_input(x, up), wc, 1, layer["sc"], layer["sh"])
    swapped = torch.cat([R.upsample2(up), x], -1)
    _rejects(_kernel_like(FR.stage_ref(swapped, wc, 1, layer["sc"], layer["sh"])["y"]), s["y"], FR.bf16_bound(s))
    shifted = torch.cat([x, torch.roll(R.upsample2(up), 1, dims=2)], -1)
    _rejects(_kernel_like(FR.stage_ref(shifted, wc, 1, layer["sc"], layer["sh"])["y"]), s["y"], FR.bf16_bound(s))


def test_rejects_a_missing_residual_and_the_wrong_leaky_side(layer):
    s = FR.stage_ref(layer["x"], layer["w"], 1, layer["sc"], layer["sh"], layer["res"])
    no_res = FR.stage_ref(layer["x"], layer["w"], 1, layer["sc"], layer["sh"])["y"]
    _rejects(_kernel_like(no_res), s["y"], FR.bf16_bound(s))
    wrong = torch.minimum(FR.ALPHA * s["z"], s["z"]) + layer["res"]
    _rejects(_kernel_like(wrong), s["y"], FR.bf16_bound(s))


def test_rejects_one_ulp_off_and_truncation(layer):
    s = FR.stage_ref(layer["x"], layer["w"], 1, layer["sc"], layer["sh"], layer["res"])
    good = _kernel_like(s["y"])
    up = (good.view(torch.int16) + 1).view(torch.bfloat16)          # one bf16 ulp away from zero
    _rejects(up, s["y"], FR.bf16_bound(s))
    trunc = (s["y"].float().view(torch.int32) & ~0xffff).view(torch.float32).to(torch.bfloat16)
    _rejects(trunc, s["y"], FR.bf16_bound(s))


def _stats_case():
    g = torch.Generator().manual_seed(7)
    c = torch.randn(4, 6, 6, 8, generator=g, dtype=F64) * 1.5 + torch.linspace(-3, 3, 8, dtype=F64)
    tw = c.abs() * 4
    mean, var, bmean, bvar = FR.stats_bounds(c, FR.C_ACC * tw)
    return c, mean, var, bmean, bvar


def test_statistics_bounds_accept_one_pass_f32_and_reject_wrong_moments():
    c, mean, var, bmean, bvar = _stats_case()
    # a correct one-pass evaluation: f32 sums of x and x^2, var = E[x^2] - mean^2
    x = c.float().reshape(-1, 8)
    s1, s2 = x.sum(0).double(), (x * x).sum(0).double()
    M = x.shape[0]
    m1 = s1 / M
    v1 = s2 / M - m1 * m1
    R.check_bounded(m1.float(), mean, bmean, "mean")
    r, br = FR.rstd_ref(var, bvar)
    R.check_bounded((1.0 / torch.sqrt(v1.float() + FR.BN_EPS)), r, br, "rstd")
    # statistics over one image instead of the batch
    one = c[:1].reshape(-1, 8)
    _rejects(one.mean(0), mean, bmean)
    # unbiased instead of population variance
    n = c.reshape(-1, 8).shape[0]
    _rejects(1.0 / torch.sqrt(var * n / (n - 1) + FR.BN_EPS), r, br)


def test_moving_average_rejects_decay_twice_or_swapped():
    c, mean, var, bmean, bvar = _stats_case()
    g = torch.Generator().manual_seed(8)
    mm0 = torch.randn(8, generator=g, dtype=F64)
    want, bound = FR.moving_ref(mm0, mean, bmean)
    d = FR.BN_DECAY
    R.check_bounded((mm0 * d + mean * (1 - d)).float(), want, bound, "mm")
    _rejects(mm0 * d * d + mean * (1 - d), want, bound)                 # decay applied twice
    _rejects((mm0 * d + mean * (1 - d)) * d + mean * (1 - d), want, bound)   # the whole update applied twice
    _rejects(mm0 * (1 - d) + mean * d, want, bound)                     # decay and 1 - decay swapped


def _codes(v):
    return v.float().clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)


def test_e4m3_checker_accepts_rne_and_adjacent_only_at_midpoints():
    g = torch.Generator().manual_seed(9)
    want = torch.randn(5000, generator=g, dtype=F64) * 3
    s_out = 0.01
    bound = torch.full_like(want, 1e-9)
    bad, adj, _ = FR.check_e4m3(_codes(want / s_out), want, bound, s_out, "ok")
    assert bad == 0 and adj == 0
    # exactly on a midpoint: either neighbour is accepted and counted
    mid = torch.tensor([(1.0 + 1.125) / 2 * s_out], dtype=F64)
    up = _codes(torch.tensor([1.125]))
    bad, adj, _ = FR.check_e4m3(up, mid, torch.tensor([1e-6]), s_out, "midpoint")
    assert bad == 0 and adj == 1


def test_e4m3_checker_rejects_one_code_off_and_nan_instead_of_saturation():
    g = torch.Generator().manual_seed(10)
    want = torch.randn(5000, generator=g, dtype=F64) * 3
    s_out = 0.01
    bound = torch.full_like(want, 1e-9)
    codes = _codes(want / s_out)
    off = codes.clone()
    i = int((FR.decode_e4m3(codes).abs() > 1).nonzero()[0])
    off[i] = off[i] + 1                                                 # one code further from zero, away from a midpoint
    with pytest.raises(AssertionError):
        FR.check_e4m3(off, want, bound, s_out, "one code off")
    big = want.clone()
    big[:10] = 600.0 * s_out                                            # beyond 448: a saturating kernel stores 448
    sat = _codes(big / s_out)
    assert FR.check_e4m3(sat, big, bound, s_out, "saturated") == (0, 0, 0.0)
    nan = sat.clone()
    nan[:10] = 0x7f                                                     # the e4m3 NaN code
    with pytest.raises(AssertionError):
        FR.check_e4m3(nan, big, bound, s_out, "NaN instead of saturation")

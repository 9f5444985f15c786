"""The m = 1 mask subnet (yolo/yolo3_net_pos.py:414-461) on the GPU, the conv kernel of its 16-channel sources, and
backbone_pair / fp8 at the other strides.

conv83 concatenates act1 (32 channels) with the upsampled 16-channel act82, conv84 is a 3x3 over 16 channels, and the data
gradients of conv82 / conv83 have 16-channel sources: disyolo_conv2d_fwd runs them on conv_c16.hip's kernel.  That kernel
against float64 on bf16 operands and exactly on integer operands; the m = 1 net against the float64 restatement
(mask_stride_ref.py) with the bounds of test_gpu_kmap.test_train_step_k_matches_oracle."""
import numpy as np
import pytest
import torch

import disyolo_oracle as O
import mask_stride_ref as R
from disyolo_amd import config as cfg
from disyolo_amd import lib as L
from disyolo_amd.net import YOLONet
from forward_ref import val_test_k
from test_gpu_mask_stride import _batch, make_net
from test_gpu_net import oracle_params, rel_err

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def bf(t):
    return t.to(BF).to(torch.float64)


def conv_ref(x0, x1, w_hwio, ks, stride=1):
    """float64 conv (SAME) of [x0, up2(x1)] with HWIO weights"""
    x = x0 if x1 is None else torch.cat([x0, O.upsample2(x1)], dim=-1)
    return O.conv2d_same(x, w_hwio, stride)


def pack(w_hwio):
    """[Cout][kh kw ci] bf16 (pack_weights' forward layout)"""
    k, _, ci, co = w_hwio.shape
    return w_hwio.permute(3, 0, 1, 2).reshape(co, k * k * ci).contiguous()


def run_conv(dev, x0, x1, w_hwio, ks, Cout, stride=1, scale=None, shift=None, leaky=False, residual=None, out_f32=False,
             stats=False, tile=0):
    B, H, W, _ = x0.shape
    Ho, Wo = -(-H // stride), -(-W // stride)
    y = torch.full((B, Ho, Wo, Cout), float("nan"), dtype=torch.float32 if out_f32 else BF, device=dev)
    st = None
    x0d = x0.to(BF).to(dev)
    x1d = x1.to(BF).to(dev) if x1 is not None else None
    wp = pack(w_hwio).to(BF).to(dev)
    kw = dict(x1=x1d, tile=tile, out_f32=out_f32, leaky=leaky, alpha=0.1)
    if scale is not None:
        kw["scale"] = scale.to(dev)
    if shift is not None:
        kw["shift"] = shift.to(dev)
    if residual is not None:
        kw["residual"] = residual.to(BF).to(dev)
    d0 = L.make_conv_desc(x0d, wp, y, ks, stride, **kw)
    if stats:
        rows = L.conv2d_stats_rows(d0)
        st = torch.full((rows, Cout, 2), float("nan"), device=dev)
        kw["stats"] = st
    d = L.make_conv_desc(x0d, wp, y, ks, stride, **kw)
    assert L.conv2d_tile(d)[0] == 30
    L.conv2d_fwd(d)
    torch.cuda.synchronize()
    return y.cpu(), (st.cpu() if st is not None else None)


SHAPES = [  # (B, H, W, C0, C1, ks, Cout): conv83, conv84, the data gradients of conv83 (into act1 / act82) and conv82
    (2, 10, 6, 32, 16, 1, 16),
    (2, 13, 7, 16, 0, 3, 32),
    (1, 9, 11, 16, 0, 1, 32),
    (2, 8, 6, 16, 0, 1, 16),
    (1, 7, 5, 16, 0, 1, 64),
    (1, 6, 10, 48, 0, 3, 24),
]


@pytest.mark.parametrize("B,H,W,C0,C1,ks,Cout", SHAPES)
def test_c16_conv_matches_f64_on_bf16_operands(dev, B, H, W, C0, C1, ks, Cout):
    g = torch.Generator().manual_seed(H * W + C0 + Cout)
    x0 = bf(torch.randn(B, H, W, C0, generator=g))
    x1 = bf(torch.randn(B, H // 2, W // 2, C1, generator=g)) if C1 else None
    w = bf(torch.randn(ks, ks, C0 + C1, Cout, generator=g) / (ks * (C0 + C1) ** 0.5))
    sc, sh = torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g) * 0.2
    res = bf(torch.randn(B, H, W, Cout, generator=g))
    raw = conv_ref(x0, x1, w, ks)
    # raw + statistics (a training-mode batch-norm layer's conv)
    y, st = run_conv(dev, x0, x1, w, ks, Cout, stats=True)
    bound = 2.0 ** -8 * raw.abs() + 1e-5 * float(raw.abs().max())
    assert bool(((y.double() - raw).abs() <= bound).all())
    M = B * H * W
    assert st.shape[0] == -(-M // 64)
    np.testing.assert_allclose(st[:, :, 0].double().sum(0).numpy(), raw.reshape(M, Cout).sum(0).numpy(), rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(st[:, :, 1].double().sum(0).numpy(), (raw ** 2).reshape(M, Cout).sum(0).numpy(), rtol=1e-4)
    # folded batch norm + leaky + residual (inference layer / accumulating data gradient)
    y, _ = run_conv(dev, x0, x1, w, ks, Cout, scale=sc, shift=sh, leaky=True, residual=res)
    want = O.leaky_relu(raw * sc.double() + sh.double(), 0.1) + res
    bound = 2.0 ** -7 * want.abs() + 1e-4 * float(want.abs().max())
    assert bool(((y.double() - want).abs() <= bound).all())
    # f32 output + bias (a score layer)
    y, _ = run_conv(dev, x0, x1, w, ks, Cout, shift=sh, out_f32=True)
    want = raw + sh.double()
    assert float((y.double() - want).abs().max()) <= 1e-5 * float(want.abs().max()) + 1e-6


@pytest.mark.parametrize("B,H,W,C0,C1,ks,Cout", SHAPES)
def test_c16_conv_is_exact_on_integer_operands_under_every_tile(dev, B, H, W, C0, C1, ks, Cout):
    """small integers: every product and partial sum is exact in f32, the results exact in bf16 -- any tile code a caller
    pins (the 16-channel shapes have one kernel; the code is accepted and ignored)"""
    g = torch.Generator().manual_seed(7 + C0 + Cout)
    x0 = torch.randint(-1, 2, (B, H, W, C0), generator=g).double()
    x1 = torch.randint(-1, 2, (B, H // 2, W // 2, C1), generator=g).double() if C1 else None
    w = torch.randint(-1, 2, (ks, ks, C0 + C1, Cout), generator=g).double()
    want = conv_ref(x0, x1, w, ks)
    assert float(want.abs().max()) <= 256
    outs = []
    for tile in (0, 2, 3, 12, 16, 18, 0x20c):
        y, _ = run_conv(dev, x0, x1, w, ks, Cout, tile=tile)
        assert torch.equal(y.double(), want), tile
        outs.append(y)


def test_c16_conv_at_the_configured_size(dev):
    """conv84 (3x3, 16 -> 32) and conv83 (1x1, [32, up2(16)] -> 16) at 576^2, B = 8 against float64 (images 0 and 7)"""
    B, S = 8, 576
    g = torch.Generator().manual_seed(576)
    for (C0, C1, ks, Cout) in ((16, 0, 3, 32), (32, 16, 1, 16)):
        x0 = bf(torch.randn(B, S, S, C0, generator=g))
        x1 = bf(torch.randn(B, S // 2, S // 2, C1, generator=g)) if C1 else None
        w = bf(torch.randn(ks, ks, C0 + C1, Cout, generator=g) / (ks * (C0 + C1) ** 0.5))
        y, st = run_conv(dev, x0, x1, w, ks, Cout, stats=True)
        for b in (0, B - 1):
            raw = conv_ref(x0[b:b + 1], x1[b:b + 1] if x1 is not None else None, w, ks)
            bound = 2.0 ** -8 * raw.abs() + 1e-5 * float(raw.abs().max())
            assert bool(((y[b:b + 1].double() - raw).abs() <= bound).all()), (C0, C1, b)
        assert not torch.isnan(st).any()


# ------------------------------------------------------------------------------------------------ the m = 1 net
@pytest.mark.parametrize("stage,k", [(1, 3), (1, 5), (2, 3)])
def test_train_step_m1_matches_reference(dev, stage, k):
    """one step of the m = 1 net against the float64 restatement, teacher-forced layer by layer: losses, dscore, every
    gradient (stage 2: act1's gradient from conv2 AND conv83, accumulated), then Adam"""
    B, S = 2, 64
    net = make_net(dev, True, k, B, S, seed=1, stage=stage, m=1)
    net.fuse_first_two = net.fuse_blocks = False
    assert net.score_layer == 85
    sl = net.by_idx[85]
    assert sl.act.shape == (B, S, S, k * k)
    assert net.by_idx[83].src == 1 and not net._can_fuse_first_two(False)
    b, perms = _batch(B, S, 11)
    p0 = oracle_params(net)
    lock = R.default_lock(stage, 1)
    net.set_batch(b)
    net.compute_losses(0.1)
    torch.cuda.synchronize()
    det = net.detections.cpu().numpy()
    mp = sl.act.cpu().clone().requires_grad_(True)
    lm = R.loss_mask(det, mp, b["true_boxes"].numpy(), b["true_masks"], perms, k)
    assert int(net.roi_count.sum()) > 0, "test needs at least one positive RoI"
    lm.backward()
    np.testing.assert_allclose(float(net.mask_loss.cpu()[0]), float(lm), rtol=2e-4)
    ds = sl.dx.float().cpu()
    assert float(ds[..., k * k:].abs().max()) == 0.0
    r, _, _ = rel_err(ds[..., :k * k], mp.grad)
    assert r < 6e-3, "dscore rel err %.3g" % r
    tr = {n: p0[n].clone().requires_grad_(True) for n in net.trainable_names()}
    pp = dict(p0)
    pp.update(tr)
    upd, taps = {}, {}
    force = {"act%d" % l.idx: l.act.float().cpu() for l in net.layers}
    parts, _, _, _ = R.total_loss(pp, b, lock, 1, k, perms, upd, obj_thresh=0.1, quant=O.bf16_ste, taps=taps, force=force)
    assert sorted(taps) == sorted("act%d" % l.idx for l in net.layers)
    for l in net.layers:
        r, _, _ = rel_err(l.act, taps["act%d" % l.idx])
        assert r < 1.5e-2, "layer %d forward: rel l2 err %.3g" % (l.idx, r)
    parts["total"].backward()
    assert abs(float(net.total_loss().cpu()) - float(parts["total"])) < 1e-3 * abs(float(parts["total"]))
    assert abs(float(net.reg_loss.cpu()[0]) - float(parts["reg"])) <= 1e-4 * float(parts["reg"])
    net.backward()
    torch.cuda.synchronize()
    for name, (o, cnt) in net.arena_slices.items():
        g = net.grad_arena[o:o + cnt].cpu()
        want_g = tr[name].grad.flatten()
        if name.endswith("weights") or name.endswith("biases"):
            want_g = want_g - O.L2_WEIGHT * tr[name].detach().flatten()
        r, amax, wmax = rel_err(g, want_g)
        assert r < 0.03 or amax < 1e-3 * max(wmax, 1e-6), "grad %s: rel l2 err %.3g (max abs %.3g of %.3g)" % (name, r, amax, wmax)
    g_all = net.grad_arena.clone()
    w_before = net.arena.clone()
    net.optimizer_step()
    torch.cuda.synchronize()
    gg = g_all.cpu().double()
    gg[:net.n_decay] += O.L2_WEIGHT * w_before[:net.n_decay].cpu().double()
    wn, _, _ = O.adam_tf_step(w_before.cpu().double(), gg, torch.zeros_like(gg), torch.zeros_like(gg), 1)
    np.testing.assert_allclose(net.arena.cpu().double().numpy(), wn.numpy(), rtol=0, atol=2e-7)


@pytest.mark.parametrize("k", [3, 5])
def test_evaluation_m1_matches_val_test(dev, k):
    net = make_net(dev, False, k, 2, 96, m=1)
    b = O.synthetic_batch(2, 96, seed=6)
    det_box, det_mask = net.evaluation(b["images"], b["clip_window"], [0.05])
    torch.cuda.synchronize()
    score = net.by_idx[85].act.cpu()
    assert score.shape == (2, 96, 96, k * k)
    wb, wm = O.val_test(net.detections.cpu().numpy(), score) if k == 3 else val_test_k(net.detections.cpu().numpy(), score, k)
    assert any(np.ndim(w) for w in wm), "test needs detections"
    for i in range(2):
        np.testing.assert_array_equal(det_box[i], wb[i])
        np.testing.assert_allclose(det_mask[i], wm[i], rtol=1e-5, atol=1e-6)
    p = oracle_params(net)
    _, mq = R.build_network(p, b["images"], False, R.default_lock(1, 1), 1, k, quant=O.bf16_ste)
    r, _, _ = rel_err(score, mq)
    assert r < 2e-2, "score maps rel l2 err %.3g" % r
    net.build_infer_program(det_thresh=0.05, graph=True)
    rb, rm = net.evaluation(b["images"], b["clip_window"], [0.05])
    torch.cuda.synchronize()
    assert torch.equal(net.by_idx[85].act.cpu(), score)
    for i in range(2):
        np.testing.assert_array_equal(rb[i], det_box[i])
        np.testing.assert_array_equal(rm[i], det_mask[i])


def test_recorded_step_m1_equals_eager(dev):
    B, S = 2, 64
    b, _ = _batch(B, S, 21)
    eager = make_net(dev, True, 3, B, S, seed=4, m=1)
    rec = make_net(dev, True, 3, B, S, seed=4, m=1)
    rec.load_state_dict(eager.state_dict())
    rec.build_program(det_thresh=0.1)
    le, lr = [], []
    for _ in range(2):
        eager.set_batch(b)
        le.append(float(eager.train_step(None, det_thresh=0.1).cpu()))
        rec.set_batch(b)
        lr.append(float(rec.train_step(None).cpu()))
    torch.cuda.synchronize()
    assert le == lr
    assert torch.equal(eager.arena, rec.arena) and torch.equal(eager.adam_v, rec.adam_v)


def test_pipelined_step_m1_equals_plain_step(dev):
    B, S = 2, 64
    batches = [O.synthetic_batch(B, S, seed=40 + t) for t in range(4)]
    plain = make_net(dev, True, 3, B, S, seed=6, m=1)
    piped = make_net(dev, True, 3, B, S, seed=6, m=1)
    piped.load_state_dict(plain.state_dict())
    plain.build_program(det_thresh=0.1)
    piped.build_program(det_thresh=0.1, pipeline_backbone=True)
    assert 1 in piped._xbuf                  # act1 is a backbone output the trainable part reads: double-buffered
    piped._set_inputs(batches[0]["images"], batches[0]["clip_window"])
    piped.prime_pipeline()
    lp, lq = [], []
    for t in range(3):
        plain.set_batch(batches[t])
        lp.append(float(plain.train_step(None).cpu()))
        mixed = dict(batches[t])
        mixed["images"] = batches[t + 1]["images"]
        piped.set_batch(mixed)
        lq.append(float(piped.train_step(None).cpu()))
    torch.cuda.synchronize()
    assert lp == lq
    assert torch.equal(plain.arena, piped.arena) and torch.equal(plain.adam_v, piped.adam_v)


def test_recorded_training_m1_overfits_one_batch(dev):
    B, S = 2, 96
    net = YOLONet(training=True, device=dev, image_size=S, batch_size=B, stage=1, seed=0, mask_stride=1)
    net.set_batch(O.synthetic_batch(B, S, seed=7))
    net.shuffle_seed = 11
    net.build_program()
    losses = [float(net.train_step(None).cpu()) for _ in range(80)]
    assert all(np.isfinite(losses)), losses
    assert losses[-1] < 0.5 * losses[0], (losses[0], losses[-1])


def test_m1_at_the_configured_size(dev):
    """stage 1, B = 8, 576^2: the new layers' conv outputs (conv83 raw, conv84 raw, conv85 score maps) against float64 on the
    net's own inputs, and the data gradients with 16-channel sources (into act81 from conv82, into act82 from conv83),
    element-wise, on images 0 and 7"""
    B, S, k = 8, 576, 3
    net = make_net(dev, True, k, B, S, seed=3, m=1)
    b, _ = _batch(B, S, 31)
    net.set_batch(b)
    net.compute_losses(0.1)
    net.backward()
    torch.cuda.synchronize()
    by = net.by_idx
    assert int(net.roi_count.sum()) > 0
    wb = lambda i: by[i].w.detach().cpu().double().to(BF).double()
    for im in (0, B - 1):
        s_ = slice(im, im + 1)
        a1, a82, a83, a84 = (by[i].act[s_].cpu().double() for i in (1, 82, 83, 84))
        for got, want in ((by[83].raw[s_], conv_ref(a1, a82, wb(83), 1)), (by[84].raw[s_], conv_ref(a83, None, wb(84), 3))):
            bound = 2.0 ** -8 * want.abs() + 1e-4 * float(want.abs().max())
            assert bool(((got.cpu().double() - want).abs() <= bound).all())
        want = conv_ref(a84, None, wb(85), 1) + by[85].bias.detach().cpu().double()
        got = by[85].act[s_].cpu().double()
        assert bool(((got - want).abs() <= 2.0 ** -8 * want.abs() + 1e-4 * float(want.abs().max())).all())
        # data gradients: grad81 = dx82 . w82^T, grad82 = up2^T(dx83 . w83[32:48]^T)
        dx82, dx83 = by[82].dx[s_].cpu().double(), by[83].dx[s_].cpu().double()
        want = torch.einsum("bhwn,cn->bhwc", dx82, wb(82)[0, 0])
        got = by[81].grad[s_].cpu().double()
        assert bool(((got - want).abs() <= 2.0 ** -7 * want.abs() + 1e-3 * float(want.abs().max())).all())
        g_up = torch.einsum("bhwn,cn->bhwc", dx83, wb(83)[0, 0, 32:48])
        want = g_up.reshape(1, S // 2, 2, S // 2, 2, 16).sum(dim=(2, 4))
        got = by[82].grad[s_].cpu().double()
        assert bool(((got - want).abs() <= 2.0 ** -7 * want.abs() + 1e-3 * float(want.abs().max())).all())


# ------------------------------------------------------------------------------------------------ pair / fp8 per stride
@pytest.mark.parametrize("m", [4, 1])
def test_backbone_pair_per_stride_steps_like_the_plain_net(dev, m):
    """test_gpu_net.test_backbone_pair_step_matches_plain_steps at m = 1/4 and m = 1 (act1 / act9 halves of the 2B pass)"""
    B, S = 2, 64
    batches = [O.synthetic_batch(B, S, seed=70 + t) for t in range(5)]
    plain = make_net(dev, True, 3, B, S, seed=8, m=m)
    pair = YOLONet(training=True, device=dev, image_size=S, batch_size=B, stage=1, seed=8, backbone_pair=True, mask_stride=m)
    pair.load_state_dict(plain.state_dict())
    lp, lq = [], []
    for t in range(4):
        lp.append(float(plain.train_step(batches[t], det_thresh=0.1).cpu()))
        lq.append(float(pair.train_step((batches[t], batches[t + 1]) if t % 2 == 0 else None, det_thresh=0.1).cpu()))
    torch.cuda.synchronize()
    np.testing.assert_allclose(lq, lp, rtol=2e-3)
    for name in plain.params:
        a, b = plain.params[name], pair.params[name]
        assert float((a - b).abs().max()) <= 4.5e-4 + 1e-3 * float(a.abs().max()), name


@pytest.mark.parametrize("m", [4, 1])
def test_fp8_backbone_per_stride(dev, m):
    """dtype='fp8' (conv10-52 in e4m3) at m = 1/4 and m = 1: within test_gpu_fp8's distance of the bf16 net"""
    B, S = 2, 192
    b = O.synthetic_batch(B, S, seed=7)
    net = YOLONet(training=False, device=dev, image_size=S, batch_size=B, stage=1, seed=0, dtype="fp8", mask_stride=m)
    ref = YOLONet(training=False, device=dev, image_size=S, batch_size=B, stage=1, seed=0, mask_stride=m)
    net._set_inputs(b["images"], b["clip_window"])
    net.calibrate_fp8()
    preds, _, mask_pos = net.forward(b["images"], b["clip_window"], [0.1], is_training=False)
    preds = [p.clone() for p in preds]
    mask_pos = mask_pos.clone()
    preds_b, _, mask_b = ref.forward(b["images"], b["clip_window"], [0.1], is_training=False)
    torch.cuda.synchronize()
    assert mask_pos.shape == (B, S // m, S // m, 9)
    for a, c in list(zip(preds, preds_b)) + [(mask_pos, mask_b)]:
        r, _, _ = rel_err(a, c)
        assert r < 0.35, r

"""K_MAP = 5 and 7 on the GPU: the k x k mask path (RoI rows, mask loss, assembly, the fused conv80-82 head) and the
net around it against the float64 oracle.

The oracle's loss_mask / val_test call assemble_logits with its default k = 3; restated below with k from the oracle's
own parts (select_mask_rois, assemble_logits(..., k), sigmoid_ce, MASK_SCALE).  Bounds are those of the k = 3 tests
these restate (test_gpu_loss.py, test_gpu_net.py, test_gpu_conv.py)."""
import numpy as np
import pytest
import torch

import disyolo_oracle as O
from disyolo_amd import config as cfg
from disyolo_amd import lib as L
from disyolo_amd.net import YOLONet
from test_gpu_conv import _block32_operands, bf16r, check, pack_ref
from test_gpu_loss import assert_grad_close, mask_case
from test_gpu_net import oracle_params, rel_err
from forward_ref import val_test_k

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ oracle restated with k
def loss_mask_k(detections, mask_pos, true_boxes, true_masks, perms, k):
    """O.loss_mask (yolo/yolo3_net_pos.py:750-860) with a k x k grid"""
    B, size = mask_pos.shape[0], mask_pos.shape[1]
    total = torch.zeros((), dtype=mask_pos.dtype)
    for i in range(B):
        pd, pg = perms[i] if perms is not None else (None, None)
        pos, assign, gt_rows = O.select_mask_rois(detections[i], true_boxes[i, 0, 0, 0], pd, pg)
        if len(pos) == 0:
            continue
        step = true_masks.shape[2] // size
        gt_small = true_masks[i][gt_rows][:, ::step, ::step].astype(np.float32)
        px = np.round(pos * np.float32(size))
        per_roi = []
        for r in range(len(px)):
            logits, mobj = O.assemble_logits(mask_pos[i], px[r], k)
            gtm = torch.from_numpy(gt_small[assign[r]]).to(mask_pos.dtype)
            per_roi.append((mobj * O.sigmoid_ce(gtm, logits)).sum() / mobj.sum())
        total = total + O.MASK_SCALE * torch.stack(per_roi).mean()
    return total / B


def expected_rois_k(det, tb, perms, sm, k):
    out = []
    for i in range(det.shape[0]):
        pos, assign, gt_rows = O.select_mask_rois(det[i], tb[i, 0, 0, 0], *perms[i])
        rows = []
        for r in range(len(pos)):
            px = np.round(pos[r] * np.float32(sm))
            area = int((O.channel_index_map(px, sm, k) >= 0).sum())
            rows.append(O.kmask_edges(px[0], px[2], k) + O.kmask_edges(px[1], px[3], k) + [int(gt_rows[assign[r]]), area, 1, 0])
        out.append(rows)
    return out


def run_mask_path(dev, det, tb, tm, score, perms, sm, k):
    """mask_rois_k + psroi_loss on NaN-filled outputs"""
    B, G = det.shape[0], cfg.MAX_BOX_PER_IMAGE
    rois = torch.full((B, L.ROI_MAX, L.roi_w(k)), -1, dtype=torch.int32, device=dev)
    cnt = torch.full((B,), -1, dtype=torch.int32, device=dev)
    pd = torch.as_tensor(np.stack([p[0] for p in perms]), device=dev).int().contiguous()
    pg = torch.as_tensor(np.stack([p[1] for p in perms]), device=dev).int().contiguous()
    L.mask_rois(torch.as_tensor(det, device=dev), 30, torch.as_tensor(tb.reshape(B, G, 5), device=dev), G, pd, pg, B, sm,
                cfg.MASK_ROI_DET, cfg.MASK_ROI_GT, cfg.MASK_ROI_IOU, rois, cnt, k=k)
    pitch = (k * k + 31) // 32 * 32
    dscore = torch.full((B, sm, sm, pitch), float("nan"), dtype=torch.bfloat16, device=dev)
    loss = torch.full((1,), float("nan"), device=dev)
    if score is not None:
        L.psroi_loss(score.to(dev), torch.as_tensor(tm, device=dev).to(torch.uint8).contiguous(), G, rois, cnt, B, sm, k,
                     cfg.MASK_SCALE, dscore, loss, L.Workspace(dev))
    torch.cuda.synchronize()
    return rois.cpu().numpy(), cnt.cpu().numpy(), float(loss.cpu()[0]), dscore.float().cpu()


# ------------------------------------------------------------------------------------------------ RoI rows
def test_mask_rois_k3_is_the_twelve_word_entry_point(dev):
    det, tb, tm, perms = mask_case(8, 288, seed=296)
    B, G = 8, cfg.MAX_BOX_PER_IMAGE
    outs = []
    for fn in ("disyolo_mask_rois", "disyolo_mask_rois_k"):
        rois = torch.full((B, L.ROI_MAX, L.ROI_W), -7, dtype=torch.int32, device=dev)
        cnt = torch.full((B,), -7, dtype=torch.int32, device=dev)
        pd = torch.as_tensor(np.stack([p[0] for p in perms]), device=dev).int().contiguous()
        pg = torch.as_tensor(np.stack([p[1] for p in perms]), device=dev).int().contiguous()
        d, t = torch.as_tensor(det, device=dev), torch.as_tensor(tb.reshape(B, G, 5), device=dev)
        args = [L._p(d), 30, L._p(t), G, L._p(pd), L._p(pg), B, 288]
        args += [3] if fn.endswith("_k") else []
        args += [cfg.MASK_ROI_DET, cfg.MASK_ROI_GT, cfg.MASK_ROI_IOU, L._p(rois), L._p(cnt), L._stream()]
        L._check(getattr(L.load(), fn)(*args), fn)
        torch.cuda.synchronize()
        outs.append((rois.cpu(), cnt.cpu()))
    assert int(outs[0][1].sum()) > 20
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


@pytest.mark.parametrize("k", [5, 7])
def test_mask_rois_rows_of_a_k_grid(dev, k):
    sm = 288
    det, tb, tm, perms = mask_case(8, sm, seed=296)
    rois, cnt, _, _ = run_mask_path(dev, det, tb, tm, None, perms, sm, k)
    want = expected_rois_k(det, tb, perms, sm, k)
    assert list(cnt) == [len(w) for w in want]
    for b in range(8):
        np.testing.assert_array_equal(rois[b, :cnt[b]], np.array(want[b], np.int32).reshape(cnt[b], L.roi_w(k)))
        assert (rois[b, cnt[b]:] == 0).all()


# ------------------------------------------------------------------------------------------------ mask loss
@pytest.mark.parametrize("k", [5, 7])
@pytest.mark.parametrize("B,sm", [(8, 288), (4, 416)])
def test_mask_loss_k_matches_f64_oracle(dev, B, sm, k):
    det, tb, tm, perms = mask_case(B, sm, seed=sm + B)
    g = torch.Generator().manual_seed(sm + k)
    score = torch.randn(B, sm, sm, k * k, generator=g) * 2.0
    rois, cnt, loss, dscore = run_mask_path(dev, det, tb, tm, score, perms, sm, k)
    want = expected_rois_k(det, tb, perms, sm, k)
    assert list(cnt) == [len(w) for w in want] and sum(cnt) > 10
    sc = score.double().clone().requires_grad_(True)
    lm = loss_mask_k(det, sc, tb, tm, perms, k)
    lm.backward()
    assert np.isfinite(loss) and np.isfinite(float(lm))
    np.testing.assert_allclose(loss, float(lm), rtol=2e-5)
    assert not torch.isnan(dscore).any(), "dscore not fully written"
    assert float(dscore[..., k * k:].abs().max()) == 0.0                   # pad channels k*k .. pitch-1
    assert_grad_close(dscore[..., :k * k], sc.grad, "dscore k=%d" % k)
    cover = np.zeros((B, sm, sm), bool)
    for b in range(B):
        for row in want[b]:
            cover[b, max(row[0], 0):min(row[k], sm), max(row[k + 1], 0):min(row[2 * k + 1], sm)] = True
    assert float(dscore[torch.from_numpy(~cover)].abs().max()) == 0.0      # pixels outside every RoI


# ------------------------------------------------------------------------------------------------ assembly
def index_map_clamped(box, size, k):
    """O.channel_index_map with each bin's slice bounds clamped to [0, size].  The oracle clamps only the start of a bin, so
    a bin that lies wholly above / left of the map (end edge < 0) becomes a numpy slice with a negative end and paints
    most of the row; the reference cannot build such a bin at all (tf.zeros of a negative size).  Such a bin covers no
    pixel here, as in the kernels and in the RoI area."""
    gy, gx = O.kmask_edges(box[0], box[2], k), O.kmask_edges(box[1], box[3], k)
    c = lambda v: min(max(v, 0), size)
    m = -np.ones((size, size), dtype=np.int32)
    for by in range(k):
        for bx in range(k):
            if gy[by + 1] > gy[by] and gx[bx + 1] > gx[bx]:
                m[c(gy[by]):c(gy[by + 1]), c(gx[bx]):c(gx[bx + 1])] = by * k + bx
    return m


def _intervals(sm):
    iv = [(lo, hi) for lo in range(sm) for hi in range(lo + 1, sm + 1)]
    return iv + [(-5, 10), (-1, 1), (sm - 2, sm + 3), (40, sm + 7), (-4, sm + 4)]   # + boxes across the map's borders


@pytest.mark.parametrize("k", [5, 7])
def test_assemble_bins_every_integer_box(dev, k):
    """every integer interval 0 <= lo < hi <= Sm on each axis (paired so that both axes see all of them), plus boxes that
    straddle the map: the channel psroi_assemble picks at each pixel is channel_index_map's"""
    sm = 48
    iv = _intervals(sm)
    n = len(iv)
    det = np.zeros((1, n, 6), np.float32)
    for r in range(n):
        (y1, y2), (x1, x2) = iv[r], iv[(r * 37 + 11) % n]
        det[0, r, :4] = np.array([y1, x1, y2, x2], np.float32) / np.float32(sm)
    code = (torch.arange(k * k, dtype=torch.float32) + 1) * 0.1           # channel c -> logit 0.1 (c + 1) > 0
    score = code.expand(1, sm, sm, k * k).contiguous()
    masks = torch.full((1, n, sm, sm), float("nan"), device=dev)
    keep = torch.zeros(1, n, dtype=torch.int32, device=dev)
    L.psroi_assemble(score.to(dev), torch.as_tensor(det, device=dev), 1, n, sm, k, masks, keep)
    torch.cuda.synchronize()
    m = masks[0].cpu()
    md = m.double()
    idx = (torch.log(md / (1 - md)) / 0.1).round().numpy().astype(np.int32) - 1     # sigmoid^-1, then the code
    idx[m.numpy() == 0.5] = -1
    assert keep.all()
    px = np.round(det[0, :, :4] * np.float32(sm))
    for r in range(n):
        want = index_map_clamped(px[r], sm, k)
        if min(O.kmask_edges(px[r][0], px[r][2], k)[1:] + O.kmask_edges(px[r][1], px[r][3], k)[1:]) >= 0:
            np.testing.assert_array_equal(want, O.channel_index_map(px[r], sm, k))   # the oracle's own domain
        if not np.array_equal(idx[r], want):
            pytest.fail("k=%d box %s: %d pixels pick another bin" % (k, px[r], int((idx[r] != want).sum())))
    # mask values on random score maps vs the restated val_test
    g = torch.Generator().manual_seed(k)
    score = torch.randn(1, sm, sm, k * k, generator=g) * 2.0
    dom = [r for r in range(0, n, 23)
           if min(O.kmask_edges(px[r][0], px[r][2], k)[1:] + O.kmask_edges(px[r][1], px[r][3], k)[1:]) >= 0]
    sel = det[:, dom].copy()
    masks = torch.full((1, sel.shape[1], sm, sm), float("nan"), device=dev)
    keep = torch.zeros(1, sel.shape[1], dtype=torch.int32, device=dev)
    L.psroi_assemble(score.to(dev), torch.as_tensor(sel, device=dev), 1, sel.shape[1], sm, k, masks, keep)
    torch.cuda.synchronize()
    _, wm = val_test_k(sel, score, k)
    np.testing.assert_allclose(masks[0].cpu().numpy(), wm[0], rtol=1e-5, atol=1e-6)


# ------------------------------------------------------------------------------------------------ fused head
@pytest.mark.parametrize("k", [5, 7])
@pytest.mark.parametrize("B,H,W", [(2, 16, 32), (1, 24, 48)])
def test_block32_fused_mask_head_k(dev, B, H, W, k):
    """[1x1 (64 + up2(32)) -> 32] -> [3x3 32 -> 64] -> [1x1 64 -> k*k] + bias in one launch == the layer-by-layer path"""
    nout = k * k
    x0, x1, wA, wB, scA, shA, scB, shB = _block32_operands(B, H, W, 32, H + W + B + k)
    g = torch.Generator().manual_seed(99 + k)
    wC = bf16r(torch.randn(1, 1, 64, nout, generator=g) / 8)
    bC = torch.randn(nout, generator=g) * 0.3
    post = L.block32_post(k)
    assert L.block32_fused_ok(B, H, W, 64, 32, post)
    up = x1.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    a80 = bf16r(O.leaky_relu(O.conv2d_same(torch.cat([x0, up], dim=3), wA, 1) * scA.double() + shA.double(), 0.1).float())
    a81 = bf16r(O.leaky_relu(O.conv2d_same(a80, wB, 1) * scB.double() + shB.double(), 0.1).float())
    want = O.conv2d_same(a81, wC, 1) + bC.double()
    x0d, x1d = x0.to(torch.bfloat16).to(dev), x1.to(torch.bfloat16).to(dev)
    wAp, wBp, wCp = (pack_ref(w).to(torch.bfloat16).to(dev) for w in (wA, wB, wC))
    y = torch.full((B, H, W, nout), float("nan"), dtype=torch.float32, device=dev)
    L.block32_fused_fwd(x0d, x1d, wAp, scA.to(dev), shA.to(dev), wBp, scB.to(dev), shB.to(dev), y, post=post, wC=wCp,
                        biasC=bC.to(dev), alpha=0.1)
    torch.cuda.synchronize()
    check(y, want, 2.0 ** -7, 2e-2)
    y80 = torch.empty(B, H, W, 32, dtype=torch.bfloat16, device=dev)
    L.conv2d_fwd(L.make_conv_desc(x0d, wAp, y80, 1, 1, x1=x1d, scale=scA.to(dev), shift=shA.to(dev), leaky=True))
    y81 = torch.empty(B, H, W, 64, dtype=torch.bfloat16, device=dev)
    L.conv2d_fwd(L.make_conv_desc(y80, wBp, y81, 3, 1, scale=scB.to(dev), shift=shB.to(dev), leaky=True))
    y82 = torch.empty_like(y)
    L.conv2d_fwd(L.make_conv_desc(y81, wCp, y82, 1, 1, shift=bC.to(dev), out_f32=True))
    torch.cuda.synchronize()
    assert float((y - y82).abs().max()) <= 2e-2 * max(1.0, float(y82.abs().max()))
    assert float(((y - y82).abs() <= 1e-5 * (1 + y82.abs())).float().mean()) > 0.9


# ------------------------------------------------------------------------------------------------ the net
def make_net_k(dev, training, k, B, S, seed=0):
    net = YOLONet(training=training, device=dev, image_size=S, batch_size=B, stage=1, seed=seed, k_map=k)
    g = torch.Generator().manual_seed(7919 + seed)
    with torch.no_grad():
        for i in (59, 67, 75, 82):
            net.params["yolo/convolutional%d/weights" % i].mul_(6.0)
            b = net.params["yolo/convolutional%d/biases" % i]
            b.copy_((torch.randn(b.shape, generator=g) * 0.5).to(b.device))
    net.refresh_weights()
    return net


@pytest.mark.parametrize("k", [5, 7])
def test_train_step_k_matches_oracle(dev, k, monkeypatch):
    """test_gpu_net.test_train_step_matches_oracle (stage 1) on a k x k grid"""
    B, S = 2, 64
    net = make_net_k(dev, True, k, B, S, seed=1)
    net.fuse_first_two = net.fuse_blocks = False
    assert net.by_idx[82].dx.shape[-1] == (k * k + 31) // 32 * 32
    b = O.synthetic_batch(B, S, seed=11)
    rng = np.random.RandomState(0)
    perm_det = np.stack([rng.permutation(cfg.MAX_DETECTION) for _ in range(B)]).astype(np.int32)
    perm_gt = np.stack([rng.permutation(cfg.MAX_BOX_PER_IMAGE) for _ in range(B)]).astype(np.int32)
    b["perm_det"], b["perm_gt"] = perm_det, perm_gt
    perms = [(perm_det[i], perm_gt[i]) for i in range(B)]
    p0 = oracle_params(net)
    lock = O.default_lock(1)
    net.set_batch(b)
    net.compute_losses(0.1)
    torch.cuda.synchronize()
    yolos = [net.by_idx[i].act.cpu().view(B, net.by_idx[i].Ho, net.by_idx[i].Wo, 3, 8).clone().requires_grad_(True)
             for i in (75, 67, 59)]
    pred = O.interpret_output(yolos)
    ly = O.loss_yolo(pred, b["true_boxes"], [b["yolo3"], b["yolo2"], b["yolo1"]])
    want = [float(ly[n]) for n in ("obj", "noobj", "class", "xy", "wh")]
    np.testing.assert_allclose(net.losses.cpu().numpy()[:5], want, rtol=2e-4, atol=1e-5)
    det = net.detections.cpu().numpy()
    mp = net.by_idx[82].act.cpu().clone().requires_grad_(True)
    assert mp.shape[-1] == k * k
    lm = loss_mask_k(det, mp, b["true_boxes"].numpy(), b["true_masks"], perms, k)
    assert int(net.roi_count.sum()) > 0, "test needs at least one positive RoI"
    lm.backward()
    np.testing.assert_allclose(float(net.mask_loss.cpu()[0]), float(lm), rtol=2e-4)
    ds = net.by_idx[82].dx.float().cpu()
    assert float(ds[..., k * k:].abs().max()) == 0.0
    r, _, _ = rel_err(ds[..., :k * k], mp.grad)
    assert r < 6e-3, "dscore rel err %.3g" % r
    # the whole step, teacher-forced layer by layer; total_loss's mask term on the k x k grid
    monkeypatch.setattr(O, "loss_mask", lambda d, m, t, tm, p: loss_mask_k(d, m, t, tm, p, k))
    tr = {n: p0[n].clone().requires_grad_(True) for n in O.trainable_names(lock)}
    pp = dict(p0)
    pp.update(tr)
    upd, taps = {}, {}
    force = {"act%d" % l.idx: l.act.float().cpu() for l in net.layers}
    parts, _, _, _ = O.total_loss(pp, b, lock, True, perms, upd, obj_thresh=0.1, quant=O.bf16_ste, taps=taps, force=force)
    for l in net.layers:
        r, _, _ = rel_err(l.act, taps["act%d" % l.idx])
        assert r < 1.5e-2, "layer %d forward: rel l2 err %.3g" % (l.idx, r)
    parts["total"].backward()
    assert abs(float(net.total_loss().cpu()) - float(parts["total"])) < 1e-3 * abs(float(parts["total"]))
    net.backward()
    torch.cuda.synchronize()
    assert set(net.trainable_names()) == set(tr)
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


@pytest.mark.parametrize("k", [5, 7])
def test_evaluation_k_matches_val_test(dev, k):
    net = make_net_k(dev, False, k, 2, 96)
    assert net._fusion_plan(False, 1, 82).get(82) is not None, "the fused mask head covers k = %d" % k
    b = O.synthetic_batch(2, 96, seed=6)
    det_box, det_mask = net.evaluation(b["images"], b["clip_window"], [0.05])
    torch.cuda.synchronize()
    act82 = net.by_idx[82].act.cpu()
    assert act82.shape[-1] == k * k
    wb, wm = val_test_k(net.detections.cpu().numpy(), act82, k)
    assert any(np.ndim(w) for w in wm), "test needs detections"
    for i in range(2):
        np.testing.assert_array_equal(det_box[i], wb[i])
        np.testing.assert_allclose(det_mask[i], wm[i], rtol=1e-5, atol=1e-6)
    if k == 7:
        # the recorded inference (hipGraph replay) == eager, bit for bit
        net.build_infer_program(det_thresh=0.05, graph=True)
        rb, rm = net.evaluation(b["images"], b["clip_window"], [0.05])
        torch.cuda.synchronize()
        assert torch.equal(net.by_idx[82].act.cpu(), act82)
        for i in range(2):
            np.testing.assert_array_equal(rb[i], det_box[i])
            np.testing.assert_array_equal(rm[i], det_mask[i])


def test_recorded_training_overfits_one_batch_k5(dev):
    B, S = 2, 96
    net = YOLONet(training=True, device=dev, image_size=S, batch_size=B, stage=1, seed=0, k_map=5)
    net.set_batch(O.synthetic_batch(B, S, seed=7))
    net.shuffle_seed = 11
    net.build_program()
    losses = [float(net.train_step(None).cpu()) for _ in range(80)]
    assert all(np.isfinite(losses)), losses
    assert losses[-1] < 0.5 * losses[0], (losses[0], losses[-1])

"""The loss kernels of csrc/loss.hip -- yolo_loss, mask_rois, psroi_loss -- against the float64 oracle at the configured
sizes, teacher-forced: the kernels' own inputs (logits, labels, boxes, detections, permutations, score maps) go to
``O.loss_yolo`` / ``O.loss_mask`` in float64, so only the loss stage is under test.

Bounds (the same for every comparison here):
  * the 8 YOLO loss terms and the mask loss: rtol 2e-5.  Every term is a sum of non-negative f32 values, <= 256 per
    block summed in f32, the blocks summed in f64;
  * every gradient element: |got - want| <= 2^-8 |want| + 1e-6 max|want| (per scale / per score map).  2^-8 is one
    rounding to bf16 (7 stored mantissa bits, round to nearest); the second term covers the f32 arithmetic where an
    element is a difference of nearly equal values (sigmoid(x) - 1 at large x, the cell offset of a normalised centre);
  * the pad channels are exactly 0, nothing is left unwritten (the outputs start as NaN), a second launch is bit-identical.
"""
import numpy as np
import pytest
import torch

import disyolo_oracle as O
from disyolo_amd import config as cfg
from disyolo_amd import lib as L
from disyolo_amd.net import YOLONet
from disyolo_amd.synth import synthetic_batch
from test_gpu_kat import expected_rois, run_mask_loss

pytestmark = pytest.mark.gpu

ANCH = np.asarray(cfg.ANCHORS, np.float32)
NAMES = ("obj", "noobj", "class", "xy", "wh", "conf", "coord")
MARGIN = 1e-5        # no best IoU this close to the threshold: the f32 kernel and the f64 oracle take the same decision


def assert_grad_close(got, want, what):
    got, want = torch.as_tensor(got).double(), torch.as_tensor(want).double()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bound = 2.0 ** -8 * want.abs() + 1e-6 * float(want.abs().max())
    bad = (got - want).abs() > bound
    if bool(bad.any()):
        i = tuple(int(v) for v in bad.nonzero()[0])
        pytest.fail("%s: %d of %d elements off, first at %s: got %.9g want %.9g" % (
            what, int(bad.sum()), bad.numel(), i, float(got[i]), float(want[i])))


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32).cpu()


# ------------------------------------------------------------------------------------------------ the YOLO loss
def best_iou(heads, tb):
    """float64 best IoU of every (cell, anchor) over the GT rows -- the oracle's formula (loss_yolo, :668-680)"""
    with torch.no_grad():
        pred = O.interpret_output([torch.from_numpy(h).double() for h in heads])
        t = torch.from_numpy(tb).double()[:, None, None, None]               # [B,1,1,1,G,5]
        out = []
        for pnc in pred[5]:
            pxy, pwh = pnc[..., None, :2], pnc[..., None, 2:4]
            txy, twh = t[..., 0:2], t[..., 2:4]
            iwh = (torch.minimum(pxy + pwh / 2, txy + twh / 2) - torch.maximum(pxy - pwh / 2, txy - twh / 2)).clamp(min=0)
            inter = iwh[..., 0] * iwh[..., 1]
            uni = (pwh[..., 0] * pwh[..., 1] + twh[..., 0] * twh[..., 1] - inter).clamp(min=1e-10)
            out.append((inter / uni).clamp(0, 1).max(dim=-1).values.numpy())
        return out


def yolo_case(B, S, C, G, seed, thresh):
    """heads [B,g,g,3,5+C] f32 (yolo3, yolo2, yolo1), dense labels, true_boxes [B,G,5]: image 0 without boxes (B > 1), image
    1 with every GT row filled, the others with zero rows between the filled ones; boxes a few pixels wide, covering the
    image, touching each border.  Mostly random-normal logits, with the box of every GT planted, jittered, in its own and
    the neighbouring cells / anchors (best IoU spread over 0.2 .. 1), conf / class logits exactly 0 and at +-30."""
    rng = np.random.RandomState(seed)
    D = 5 + C
    g1 = S // 32
    grids = (4 * g1, 2 * g1, g1)
    tb = np.zeros((B, G, 5), np.float32)
    labels = [np.zeros((B, g, g, 3, D), np.float32) for g in grids]
    specials = [(S / 2, S / 2, S, S)]                                                   # the whole image
    for i in range(6):                                                                  # a few pixels wide / high
        w, h = rng.randint(2, 6), rng.randint(2, 9)
        specials.append((rng.uniform(w, S - w), rng.uniform(h, S - h), float(w), float(h)))
    for side in range(4):                                                               # touching left/right/top/bottom
        w, h = rng.uniform(0.05, 0.5) * S, rng.uniform(0.05, 0.5) * S
        xc, yc = rng.uniform(w / 2, S - w / 2), rng.uniform(h / 2, S - h / 2)
        xc = w / 2 if side == 0 else S - w / 2 if side == 1 else xc
        yc = h / 2 if side == 2 else S - h / 2 if side == 3 else yc
        specials.append((xc, yc, w, h))
    for b in range(B):
        if b == 0 and B > 1:
            rows = []
        elif b == 1 or B == 1:
            # every row of the default 20-row table; of the 64-row one, 20 rows up to the last
            rows = list(range(G)) if G <= 20 else sorted(rng.choice(G - 1, 19, replace=False).tolist()) + [G - 1]
        else:
            k = rng.randint(1, min(G, 12) + 1)
            rows = sorted(rng.choice(G, k, replace=False).tolist())
        boxes, cls = [], []
        for j, r in enumerate(rows):
            if specials and (rng.rand() < 0.5 or b == 1):
                box = specials[(b * 7 + j) % len(specials)]
            else:
                w, h = rng.uniform(0.03, 0.7) * S, rng.uniform(0.03, 0.7) * S
                box = (rng.uniform(w / 2, S - w / 2), rng.uniform(h / 2, S - h / 2), w, h)
            c = rng.randint(0, C)
            tb[b, r, :4] = np.asarray(box, np.float32) / np.float32(S)
            tb[b, r, 4] = c
            boxes.append(box)
            cls.append(c)
        t3 = O.assign_targets(np.asarray(boxes, np.float32).reshape(-1, 4), np.asarray(cls), S, num_class=C)
        for lab, t in zip(labels, t3):
            t[..., 0:4] /= S
            lab[b] = t
    heads = [rng.randn(B, g, g, 3, D).astype(np.float32) for g in grids]
    for s, (g, h) in enumerate(zip(grids, heads)):
        aw, ah = ANCH[3 * s:3 * s + 3, 0], ANCH[3 * s:3 * s + 3, 1]
        for b in range(B):
            for r in range(G):
                xc, yc, w, hh = (float(v) for v in tb[b, r, :4])
                if w == 0:
                    continue
                cx, cy = min(int(xc * g), g - 1), min(int(yc * g), g - 1)
                for y in range(max(cy - 1, 0), min(cy + 2, g)):
                    for x in range(max(cx - 1, 0), min(cx + 2, g)):
                        for a in range(3):
                            if rng.rand() < 0.4:
                                continue
                            j = rng.uniform(0, 0.45)
                            px = xc + rng.uniform(-j, j) * w
                            py = yc + rng.uniform(-j, j) * hh
                            sx = np.clip(px * g - x, 0.02, 0.98)
                            sy = np.clip(py * g - y, 0.02, 0.98)
                            pw = w * np.exp(rng.uniform(-2 * j, 2 * j))
                            ph = hh * np.exp(rng.uniform(-2 * j, 2 * j))
                            h[b, y, x, a, 0] = np.log(sx / (1 - sx))
                            h[b, y, x, a, 1] = np.log(sy / (1 - sy))
                            h[b, y, x, a, 2] = np.log(pw * S / aw[a])
                            h[b, y, x, a, 3] = np.log(ph * S / ah[a])
        u = rng.rand(*h.shape[:-1])
        h[..., 4][u < 0.05] = 0.0
        h[..., 4][(u >= 0.05) & (u < 0.08)] = 30.0
        h[..., 4][(u >= 0.08) & (u < 0.11)] = -30.0
        v = rng.rand(*h.shape[:-1], C)
        h[..., 5:][v < 0.05] = 0.0
        h[..., 5:][(v >= 0.05) & (v < 0.08)] = 30.0
        h[..., 5:][(v >= 0.08) & (v < 0.11)] = -30.0
    # keep every best IoU MARGIN away from the threshold: stretch such a candidate's width a little (deterministic)
    for _ in range(8):
        near = [np.abs(bi - thresh) < MARGIN for bi in best_iou(heads, tb)]
        if not any(n.any() for n in near):
            break
        for h, n in zip(heads, near):
            h[..., 2][n] += np.float32(1e-3)
    return heads, labels, tb


def check_yolo_preconditions(heads, labels, tb, thresh, need_mix=True):
    best = best_iou(heads, tb)
    for s, bi in enumerate(best):
        gap = float(np.abs(bi - thresh).min())
        assert gap >= MARGIN, "scale %d: a best IoU is %.3g from the ignore threshold" % (s, gap)
    if not need_mix:
        return
    for b in range(tb.shape[0]):
        if not np.abs(tb[b, :, :4]).sum(axis=1).any():
            continue
        obj = sum(int((lab[b, ..., 4] == 1).sum()) for lab in labels)
        ign = sum(int(((lab[b, ..., 4] == 0) & (bi[b] >= thresh)).sum()) for lab, bi in zip(labels, best))
        cnt = sum(int(((lab[b, ..., 4] == 0) & (bi[b] < thresh)).sum()) for lab, bi in zip(labels, best))
        assert obj > 0 and ign > 0 and cnt > 0, (b, obj, ign, cnt)


def run_yolo(dev, heads, labels, tb, S, C, thresh, scales):
    B, G = tb.shape[0], tb.shape[1]
    lg = [torch.from_numpy(h).to(dev).contiguous() for h in heads]
    lb = [torch.from_numpy(l).to(dev).contiguous() for l in labels]
    dl = [torch.full((B, h.shape[1], h.shape[2], L.GRAD_LD), float("nan"), dtype=torch.bfloat16, device=dev) for h in heads]
    losses = torch.full((8,), float("nan"), device=dev)
    L.yolo_loss(lg, lb, torch.from_numpy(tb).to(dev).contiguous(), G, B, S, C, ANCH.reshape(-1), thresh, scales, dl, losses,
                L.Workspace(dev))
    torch.cuda.synchronize()
    return losses.cpu(), [d.cpu() for d in dl]


def yolo_oracle(heads, labels, tb):
    """float64 loss terms [obj, noobj, class, xy, wh, conf, coord, conf + class + coord] and d(total)/d(head logits)"""
    B, G = tb.shape[0], tb.shape[1]
    preds = [torch.from_numpy(np.ascontiguousarray(h)).double().requires_grad_(True) for h in heads]
    ly = O.loss_yolo(O.interpret_output(preds), torch.from_numpy(tb).double().reshape(B, 1, 1, 1, G, 5),
                     [torch.from_numpy(np.ascontiguousarray(l)).double() for l in labels])
    tot = ly["conf"] + ly["class"] + ly["coord"]
    tot.backward()
    return np.array([float(ly[k].detach()) for k in NAMES] + [float(tot.detach())]), [p.grad for p in preds]


def check_yolo_outputs(losses, dl, heads, labels, tb, what):
    want, grads = yolo_oracle(heads, labels, tb)
    got = losses.double().numpy()
    assert np.isfinite(got).all(), (what, got)
    np.testing.assert_allclose(got, want, rtol=2e-5, err_msg=what + ": loss terms " + str(NAMES + ("total",)))
    for s, (d, w) in enumerate(zip(dl, grads)):
        D3 = 3 * w.shape[-1]
        assert not torch.isnan(d.float()).any(), "%s: dlogits of scale %d not fully written" % (what, s)
        assert float(d[..., D3:].float().abs().max()) == 0.0, "%s: pad channels of scale %d" % (what, s)
        assert_grad_close(d[..., :D3].float().reshape(w.shape), w, "%s: dlogits of scale %d" % (what, s))
    return want


def _yolo(dev, B, S, C=3, G=cfg.MAX_BOX_PER_IMAGE, seed=0, thresh=cfg.IGNORE_THRESH, scales=None):
    scales = scales or (O.OBJECT_SCALE, O.NOOBJECT_SCALE, O.CLASS_SCALE, O.COORD_SCALE)
    heads, labels, tb = yolo_case(B, S, C, G, seed, thresh)
    check_yolo_preconditions(heads, labels, tb, thresh)
    losses, dl = run_yolo(dev, heads, labels, tb, S, C, thresh, scales)
    want = check_yolo_outputs(losses, dl, heads, labels, tb, "B=%d S=%d C=%d G=%d" % (B, S, C, G))
    assert (want[:5] > 0).all() or C == 1
    losses2, dl2 = run_yolo(dev, heads, labels, tb, S, C, thresh, scales)
    assert torch.equal(bits(losses), bits(losses2))
    for d, d2 in zip(dl, dl2):
        assert torch.equal(bits(d), bits(d2))
    return want


@pytest.mark.parametrize("B,S", [(8, 576), (4, 832), (1, 576), (2, 64), (3, 96)])
def test_yolo_loss_matches_f64_oracle(dev, B, S):
    _yolo(dev, B, S, seed=S + B)


@pytest.mark.parametrize("C", [1, 5])
def test_yolo_loss_num_class(dev, C):
    """D = 5 + C: row widths 6 and 10, zero padding from 18 / 30 up to 32 channels (C = 3 runs above)"""
    _yolo(dev, 3, 96, C=C, seed=10 + C)


@pytest.mark.parametrize("G", [1, 64])
def test_yolo_loss_max_boxes(dev, G):
    """the best-IoU loop over 1 and over 64 GT rows (the LDS staging's cap; 20 runs above), GT in the last row"""
    _yolo(dev, 3, 96, G=G, seed=20 + G)


def test_yolo_loss_scales_and_ignore_threshold(dev, monkeypatch):
    """distinct (obj, noobj, class, coord) scales and an ignore threshold that is not 0.5: a swapped scale or a hard-coded
    threshold moves the terms and the gradients"""
    sc = (3.0, 5.0, 7.0, 11.0)
    for name, v in zip(("OBJECT_SCALE", "NOOBJECT_SCALE", "CLASS_SCALE", "COORD_SCALE"), sc):
        monkeypatch.setattr(O, name, v)
    monkeypatch.setattr(O, "IGNORE_THRESH", 0.35)
    heads, labels, tb = yolo_case(3, 96, 3, cfg.MAX_BOX_PER_IMAGE, 31, 0.35)
    # cells whose ignore decision differs between 0.35 and 0.5: the hard-coded threshold would be visible
    assert sum(int(((bi >= 0.35) & (bi < 0.5) & (lab[..., 4] == 0)).sum()) for bi, lab in zip(best_iou(heads, tb), labels)) > 0
    _yolo(dev, 3, 96, seed=31, thresh=0.35, scales=sc)


# ------------------------------------------------------------------------------------------------ the mask loss
def mask_case(B, sm, seed):
    """20 GT instances per image (ellipses at full resolution 2 sm, some touching a border), 30 detection rows per image
    jittered from the GT boxes (some IoU >= 0.5, some below), zero rows between detection rows and between GT rows, image
    0 without GT, image 1 without detections, random permutations; selected detections pushed across each map border"""
    rng = np.random.RandomState(seed)
    G, S = cfg.MAX_BOX_PER_IMAGE, 2 * sm
    tb = np.zeros((B, 1, 1, 1, G, 5), np.float32)
    tm = np.zeros((B, G, S, S), bool)
    det = np.zeros((B, cfg.MAX_DETECTION, 6), np.float32)
    for b in range(1, B):
        rows = range(G) if b % 2 else sorted(rng.choice(G, 14, replace=False))
        for j, r in enumerate(rows):
            w, h = int(rng.uniform(0.06, 0.5) * S), int(rng.uniform(0.06, 0.5) * S)
            x0, y0 = rng.randint(0, S - w + 1), rng.randint(0, S - h + 1)
            x0 = 0 if j == 0 else S - w if j == 1 else x0
            y0 = 0 if j == 2 else S - h if j == 3 else y0
            yy, xx = np.mgrid[0:h, 0:w]
            m = ((xx + 0.5 - w / 2) / (w / 2)) ** 2 + ((yy + 0.5 - h / 2) / (h / 2)) ** 2 <= 1.0
            if j == 0 or j == 1:
                m[h // 2, 0 if j == 0 else w - 1] = True          # the left / right border of the image
            elif j == 2 or j == 3:
                m[0 if j == 2 else h - 1, w // 2] = True          # the top / bottom border
            tm[b, r, y0:y0 + h, x0:x0 + w] = m
            ys, xs = np.where(tm[b, r])
            x1, x2, y1, y2 = xs.min(), xs.max(), ys.min(), ys.max()
            tb[b, 0, 0, 0, r] = [(x1 + x2) / 2.0 / S, (y1 + y2) / 2.0 / S, (x2 - x1) / S, (y2 - y1) / S, rng.randint(0, 3)]
    for b in range(B):
        if b == 1:
            continue
        gts = [r for r in range(G) if tb[b, 0, 0, 0, r, 2] > 0]
        for q in range(cfg.MAX_DETECTION):
            if q % 7 == 3:
                continue                                          # zero rows between the detection rows
            if gts and rng.rand() < 0.85:
                xc, yc, w, h = tb[b, 0, 0, 0, gts[rng.randint(len(gts))], :4]
                j = rng.choice([0.03, 0.12, 0.3])
                e = rng.uniform(-j, j, 4) * np.array([h, w, h, w])
                det[b, q, :4] = [yc - h / 2 + e[0], xc - w / 2 + e[1], yc + h / 2 + e[2], xc + w / 2 + e[3]]
            else:
                y0, x0 = rng.uniform(0, 0.7, 2)
                det[b, q, :4] = [y0, x0, y0 + rng.uniform(0.05, 0.3), x0 + rng.uniform(0.05, 0.3)]
            det[b, q, 4:] = [rng.randint(0, 3), 0.99 - 0.01 * q]
    perms = [(rng.permutation(cfg.MAX_DETECTION).astype(np.int32), rng.permutation(G).astype(np.int32)) for _ in range(B)]
    # the first two selected detections of images 2, 3, ... = a GT box that touches a border of the image, pushed 3 map
    # pixels across it (sides top, bottom, left, right in turn)
    for b in range(2, B):
        prow = [q for q in range(cfg.MAX_DETECTION) if np.abs(det[b, q, :4]).sum() != 0]
        sel = [prow[j] for j in perms[b][0] if j < len(prow)][:2]
        gts = [r for r in range(G) if tb[b, 0, 0, 0, r, 2] > 0]
        for q, side in zip(sel, ((2 * b) % 4, (2 * b + 1) % 4)):
            xc, yc, w, h = tb[b, 0, 0, 0, gts[side ^ 2], :4]          # the 1st / 2nd filled GT row touches left / right,
            box = np.array([yc - h / 2, xc - w / 2, yc + h / 2, xc + w / 2], np.float32)   # the 3rd / 4th top / bottom
            k, sgn = ((0, -1), (2, 1), (1, -1), (3, 1))[side]
            box[k] += sgn * 3.0 / sm
            det[b, q, :4] = box
    return det, tb, tm, perms


def check_mask_outputs(det, tb, tm, perms, score, rois, cnt, loss, dscore, sm, what):
    B = det.shape[0]
    want_rois = expected_rois(det, tb, perms, sm=sm)
    assert list(cnt) == [len(w) for w in want_rois], (what, list(cnt))
    for b in range(B):
        np.testing.assert_array_equal(rois[b, :cnt[b]], np.array(want_rois[b], np.int32).reshape(cnt[b], L.ROI_W))
        assert (rois[b, cnt[b]:] == 0).all()
    sc = torch.as_tensor(score).double().clone().requires_grad_(True)
    lm = O.loss_mask(det, sc, tb, tm, perms)
    lm.backward()
    assert np.isfinite(loss) and np.isfinite(float(lm))
    np.testing.assert_allclose(loss, float(lm), rtol=2e-5, err_msg=what + ": mask loss")
    assert not torch.isnan(dscore).any(), what + ": dscore not fully written"
    assert float(dscore[..., 9:].abs().max()) == 0.0
    assert_grad_close(dscore[..., :9], sc.grad, what + ": dscore")
    cover = np.zeros((B, sm, sm), np.int32)
    for b in range(B):
        for row in want_rois[b]:
            cover[b, max(row[0], 0):min(row[3], sm), max(row[4], 0):min(row[7], sm)] += 1
    assert float(dscore[torch.from_numpy(cover == 0)].abs().max()) == 0.0
    return want_rois, cover


@pytest.mark.parametrize("B,sm", [(8, 288), (4, 416)])
def test_mask_loss_matches_f64_oracle(dev, B, sm):
    det, tb, tm, perms = mask_case(B, sm, seed=sm + B)
    g = torch.Generator().manual_seed(sm)
    score = torch.randn(B, sm, sm, 9, generator=g) * 2.0
    score[torch.rand(score.shape, generator=g) < 0.02] = 0.0
    rois, cnt, loss, dscore = run_mask_loss(dev, det, tb, tm, score, perms, sm=sm, fill=float("nan"))
    want, cover = check_mask_outputs(det, tb, tm, perms, score, rois, cnt, loss, dscore, sm, "B=%d map %d" % (B, sm))
    # the cases the inputs were built for are really there
    assert cnt[0] == 0 and cnt[1] == cfg.MASK_ROI_GT                  # no GT / no detections (its 3 GT boxes)
    edges = np.array([r for w in want for r in w])
    assert (edges[:, 0] < 0).any() and (edges[:, 3] > sm).any() and (edges[:, 4] < 0).any() and (edges[:, 7] > sm).any()
    assert cover.max() >= 3
    cand = [min(cfg.MASK_ROI_DET, int((np.abs(det[b, :, :4]).sum(1) != 0).sum())) + min(cfg.MASK_ROI_GT, int(
        (np.abs(tb[b, 0, 0, 0, :, :4]).sum(1) != 0).sum())) for b in range(B)]
    assert any(c < k for c, k in zip(cnt[2:], cand[2:])), "every selected detection is positive: no negatives"
    # a RoI assigned to a GT row with an empty row in front of it: its index in the trimmed list is not its row
    assert any((np.abs(tb[b, 0, 0, 0, :r[8], :4]).sum(1) == 0).any() for b in range(B) for r in want[b])
    rois2, cnt2, loss2, dscore2 = run_mask_loss(dev, det, tb, tm, score, perms, sm=sm, fill=float("nan"))
    assert np.array_equal(rois, rois2) and np.array_equal(cnt, cnt2)
    assert np.float32(loss).view(np.int32) == np.float32(loss2).view(np.int32)
    assert torch.equal(bits(dscore.to(torch.bfloat16)), bits(dscore2.to(torch.bfloat16)))


# ------------------------------------------------------------------------------------------------ inside the net
NB, NS = 8, 576


def _net_io(net, q=None):
    """what the loss kernels of the last step consumed and produced, read back from the net (q: the pipelined step's input
    set)"""
    src = net._pipe_in[q] if q is not None else {n: getattr(net, n) for n in ("labels", "true_boxes", "true_masks",
                                                                                "perm_det", "perm_gt")}
    heads = [net.by_idx[i].act.float().cpu().view(NB, net.by_idx[i].Ho, net.by_idx[i].Wo, 3, 8).numpy().copy()
             for i in (75, 67, 59)]
    return {
        "heads": heads,
        "labels": [t.cpu().numpy().copy() for t in src["labels"]],
        "tb": src["true_boxes"].cpu().numpy().copy(),
        "tm": src["true_masks"].cpu().numpy().astype(bool),
        "perm_det": src["perm_det"].cpu().numpy().copy(),
        "perm_gt": src["perm_gt"].cpu().numpy().copy(),
        "det": net.detections.cpu().numpy().copy(),
        "score": net.by_idx[82].act.float().cpu().clone(),
        "losses": net.losses.cpu().clone(),
        "mask_loss": net.mask_loss.cpu().clone(),
        "rois": net.rois.cpu().numpy().copy(),
        "roi_count": net.roi_count.cpu().numpy().copy(),
        "dl": [net.by_idx[i].dx.cpu().clone() for i in (75, 67, 59)],
        "dscore": net.by_idx[82].dx.cpu().clone(),
    }


def _check_net_io(io, what):
    tb = io["tb"].reshape(NB, 1, 1, 1, cfg.MAX_BOX_PER_IMAGE, 5)
    check_yolo_preconditions(io["heads"], io["labels"], io["tb"], cfg.IGNORE_THRESH, need_mix=False)
    check_yolo_outputs(io["losses"], io["dl"], io["heads"], io["labels"], io["tb"], what)
    perms = [(io["perm_det"][b], io["perm_gt"][b]) for b in range(NB)]
    assert int(io["roi_count"].sum()) > 0, what + ": no positive RoI"
    check_mask_outputs(io["det"], tb, io["tm"], perms, io["score"], io["rois"], io["roi_count"], float(io["mask_loss"][0]),
                       io["dscore"].float(), NS // 2, what)


def test_losses_inside_the_net_at_the_headline_configuration(dev):
    """stage 1, 576^2, B = 8: eager compute_losses and the recorded pipelined step bench.py times (the mask path on the side
    lane, reading layer 82's output from the main lane) against the oracle on what the kernels consumed, bit-identical to
    each other; then one recorded step with the device shuffle of the RoI order"""
    net = YOLONet(training=True, device=dev, image_size=NS, batch_size=NB, stage=1, seed=0)
    with torch.no_grad():
        for i in (59, 67, 75, 82):
            net.params["yolo/convolutional%d/weights" % i].mul_(4.0)
    net.refresh_weights()
    b = synthetic_batch(NB, NS, seed=77)
    rng = np.random.RandomState(3)
    b["perm_det"] = np.stack([rng.permutation(cfg.MAX_DETECTION) for _ in range(NB)]).astype(np.int32)
    b["perm_gt"] = np.stack([rng.permutation(cfg.MAX_BOX_PER_IMAGE) for _ in range(NB)]).astype(np.int32)
    net.set_batch(b)
    net.compute_losses(0.2)
    torch.cuda.synchronize()
    eager = _net_io(net)
    assert np.array_equal(eager["perm_det"], b["perm_det"])
    _check_net_io(eager, "eager")

    net.build_program(det_thresh=0.2, pipeline_backbone=True)
    net.prime_pipeline()
    q = net._parity
    net.train_step(None, want_loss=False)
    torch.cuda.synchronize()
    rec = _net_io(net, q)
    _check_net_io(rec, "recorded pipelined step")
    assert torch.equal(bits(eager["losses"]), bits(rec["losses"])) and torch.equal(bits(eager["mask_loss"]), bits(rec["mask_loss"]))
    for d0, d1 in zip(eager["dl"] + [eager["dscore"]], rec["dl"] + [rec["dscore"]]):
        assert torch.equal(bits(d0), bits(d1))

    # the device shuffle (bench.py sets shuffle_seed): the oracle on the permutations the device drew
    net.shuffle_seed = 1234
    net.build_program(det_thresh=0.2, pipeline_backbone=True)
    net.prime_pipeline()
    q = net._parity
    net.train_step(None, want_loss=False)
    torch.cuda.synchronize()
    shuf = _net_io(net, q)
    for p, n in ((shuf["perm_det"], cfg.MAX_DETECTION), (shuf["perm_gt"], cfg.MAX_BOX_PER_IMAGE)):
        assert (np.sort(p, axis=1) == np.arange(n)).all()
    assert not np.array_equal(shuf["perm_det"], b["perm_det"])
    _check_net_io(shuf, "recorded step, device shuffle")

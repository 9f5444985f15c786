"""Cases and the CPU reference for the mask loss's RoI counts (``mask_roi_det``, ``mask_roi_gt``, ``mask_roi_iou``): the inputs of
tests/test_gpu_mask_rois.py and, without a GPU, of tests/test_mask_rois.py, which runs every case through the reference alone
and holds it to the condition it exists for.

The reference restates ``O.select_mask_rois`` / ``O.loss_mask`` (yolo/yolo3_net_pos.py:757-796, :842-858) with the 7, the 3 and
the 0.5 as arguments, on a map of Hm x Wm, composed from the oracle's ``overlaps``, ``kmask_edges``, ``sigmoid_ce`` and
``MASK_SCALE``; the loss runs in float64.  Every case is built by construction, computed once, cached and left unchanged."""
import numpy as np
import torch

import disyolo_oracle as O

ROI_MAX = 16          # the narrow table (DISYOLO_ROI_MAX)
ROI_CAP = 512         # the wide one (DISYOLO_ROI_CAP)


def roi_w(k):
    return 2 * (k + 1) + 4


# ------------------------------------------------------------------------------------------------ 1. the reference
def select(det_i, tb_i, n_det, n_gt, thr, perm_det=None, perm_gt=None):
    """``O.select_mask_rois`` with `[:7]`, `[:3]` and 0.5 replaced by n_det, n_gt and thr.  Returns (positive RoIs [P,4]
    normalised yxyx, assignment [P] into the trimmed boxes, trimmed -> row, RoI index of each positive, number of RoIs)"""
    prop = det_i[:, :4].astype(np.float32)
    prop = prop[np.abs(prop).sum(axis=1) != 0]
    gt = tb_i[:, :4].astype(np.float32)
    gt_rows = np.where(np.abs(gt).sum(axis=1) != 0)[0]
    gt = gt[gt_rows]
    xc, yc, w, h = gt[:, 0], gt[:, 1], gt[:, 2], gt[:, 3]
    two = np.float32(2.0)
    gt_yxyx = np.stack([yc - h / two, xc - w / two, yc + h / two, xc + w / two], axis=-1).astype(np.float32)
    pd = list(range(len(prop))) if perm_det is None else [q for q in perm_det if 0 <= q < len(prop)]
    pg = list(range(len(gt_yxyx))) if perm_gt is None else [q for q in perm_gt if 0 <= q < len(gt_yxyx)]
    rois = np.concatenate([prop[pd][:n_det], gt_yxyx[pg][:n_gt]], axis=0)
    if len(rois) == 0 or len(gt_yxyx) == 0:
        return np.zeros((0, 4), np.float32), np.zeros((0,), np.int64), gt_rows, np.zeros((0,), np.int64), len(rois)
    ov = O.overlaps(rois, gt_yxyx)
    ov = np.where(np.isnan(ov), -np.inf, ov)                       # NaN never wins
    pos = np.where(ov.max(axis=1) >= np.float32(thr))[0]
    return rois[pos], ov[pos].argmax(axis=1), gt_rows, pos, len(rois)


def row_of(y1, x1, y2, x2, gt_row, Hm, Wm, k):
    """the table row of an RoI whose rounded map coordinates are (y1, x1, y2, x2): [gy0..gyk, gx0..gxk, gt_row, area, 1, 0]"""
    gy, gx = O.kmask_edges(y1, y2, k), O.kmask_edges(x1, x2, k)
    area = 0
    for by in range(k):
        for bx in range(k):
            hh = min(gy[by + 1], Hm) - max(gy[by], 0)
            ww = min(gx[bx + 1], Wm) - max(gx[bx], 0)
            if hh > 0 and ww > 0:
                area += hh * ww
    return gy + gx + [int(gt_row), area, 1, 0]


def rows(det, tb, perms, Hm, Wm, k, n_det, n_gt, thr):
    """per image the rows the selection must write, and (RoI index of each positive, number of RoIs)"""
    out, info = [], []
    for i in range(det.shape[0]):
        pd, pg = perms[i] if perms is not None else (None, None)
        pos, assign, gt_rows, idx, nr = select(det[i], tb[i], n_det, n_gt, thr, pd, pg)
        r = []
        for q in range(len(pos)):
            y1, y2 = np.round(pos[q][0] * np.float32(Hm)), np.round(pos[q][2] * np.float32(Hm))
            x1, x2 = np.round(pos[q][1] * np.float32(Wm)), np.round(pos[q][3] * np.float32(Wm))
            r.append(row_of(y1, x1, y2, x2, gt_rows[assign[q]], Hm, Wm, k))
        out.append(r)
        info.append((idx, nr))
    return out, info


def table_of(rows_per_image, cap, k):
    """int32 [B, cap, roi_w(k)] and counts [B]: the rows, zeros behind them"""
    B = len(rows_per_image)
    t = np.zeros((B, cap, roi_w(k)), np.int32)
    for b, r in enumerate(rows_per_image):
        assert len(r) <= cap
        if r:
            t[b, :len(r)] = np.asarray(r, np.int32)
    return t, np.asarray([len(r) for r in rows_per_image], np.int32)


def index_map(row, Hm, Wm, k):
    """``O.channel_index_map`` from a table row, on an Hm x Wm map: by * k + bx inside bin (by, bx), -1 elsewhere"""
    gy, gx = list(row[:k + 1]), list(row[k + 1:2 * k + 2])
    m = -np.ones((Hm, Wm), np.int32)
    for by in range(k):
        for bx in range(k):
            y1, y2, x1, x2 = max(gy[by], 0), min(gy[by + 1], Hm), max(gx[bx], 0), min(gx[bx + 1], Wm)
            if y2 > y1 and x2 > x1:
                m[y1:y2, x1:x2] = by * k + bx
    return m


def table_loss(table, cnt, score, true_masks, st, k, mask_scale=O.MASK_SCALE):
    """loss_mask (:842-858) on a table of RoI rows: mask_scale * mean_r(sum BCE / area) per image, 0 without rows, the mean
    over the batch.  ``score`` [B,Hm,Wm,k*k] torch (float64 for the reference), true_masks [B,G,st*Hm,st*Wm]"""
    B, Hm, Wm = score.shape[0], score.shape[1], score.shape[2]
    total = torch.zeros((), dtype=score.dtype)
    for b in range(B):
        if cnt[b] == 0:
            continue
        per_roi = []
        for r in range(int(cnt[b])):
            row = table[b, r]
            idx = torch.from_numpy(index_map(row, Hm, Wm, k)).long()
            inside = idx >= 0
            logits = torch.gather(score[b], 2, idx.clamp(min=0).unsqueeze(-1)).squeeze(-1)
            logits = torch.where(inside, logits, torch.zeros_like(logits))
            mobj = inside.to(score.dtype)
            assert int(inside.sum()) == int(row[2 * k + 3]), "the area word is the clipped pixel count"
            gtm = torch.from_numpy(np.asarray(true_masks[b, row[2 * k + 2], ::st, ::st] != 0).astype(np.float64)).to(score.dtype)
            num = (mobj * O.sigmoid_ce(gtm, logits)).sum()
            per_roi.append(num / mobj.sum())                      # 0 / 0 -> nan
        total = total + mask_scale * torch.stack(per_roi).mean()
    return total / B


def loss_mask(det, mask_pos, tb, true_masks, n_det, n_gt, thr, perms=None, k=O.K_MAP):
    """``O.loss_mask`` with the two counts and the threshold as arguments; tb [B,G,5]"""
    Hm, Wm = mask_pos.shape[1], mask_pos.shape[2]
    r, _ = rows(det, tb, perms, Hm, Wm, k, n_det, n_gt, thr)
    cap = max(max(len(x) for x in r), 1)
    table, cnt = table_of(r, cap, k)
    return table_loss(table, cnt, mask_pos, true_masks, true_masks.shape[2] // Hm, k)


def cover_of(table, cnt, Hm, Wm, k):
    """int32 [B,Hm,Wm]: the number of rows that cover each pixel"""
    c = np.zeros((len(cnt), Hm, Wm), np.int32)
    for b in range(len(cnt)):
        for r in range(int(cnt[b])):
            row = table[b, r]
            y1, y2, x1, x2 = max(row[0], 0), min(row[k], Hm), max(row[k + 1], 0), min(row[2 * k + 1], Wm)
            if y2 > y1 and x2 > x1:
                c[b, y1:y2, x1:x2] += 1
    return c


def block_lists(table, cnt, Hm, Wm, k):
    """per image and block of 256 pixels: the rows that meet the block's span (its rows, and its columns when it lies within
    one row of the map) -- the list psroi_loss_wide_kernel culls to"""
    npx = Hm * Wm
    out = []
    for b in range(len(cnt)):
        per = []
        for i0 in range(0, npx, 256):
            i1 = min(i0 + 255, npx - 1)
            ylo, yhi = i0 // Wm, i1 // Wm
            xlo, xhi = (i0 - ylo * Wm, i1 - ylo * Wm) if ylo == yhi else (0, Wm - 1)
            per.append([r for r in range(int(cnt[b])) if table[b, r, 0] <= yhi and table[b, r, k] > ylo
                        and table[b, r, k + 1] <= xhi and table[b, r, 2 * k + 1] > xlo])
        out.append(per)
    return out


# ------------------------------------------------------------------------------------------------ 2. selection cases
SEL_MAP = (24, 40)
SEL_CASES = ((17, 0, 30, 20), (0, 17, 30, 20), (30, 20, 30, 20), (100, 65, 100, 65), (256, 256, 256, 256))   # n_det, n_gt, D, G
OLD_CASES = ((7, 3), (10, 6))                                     # against the old entry point, roi_cap = 16
OLD_SIZES = ((30, 20), (100, 65))
_SEL = {}


def lattice(n, Hm, Wm, side):
    """n boxes of side x side map pixels on a regular lattice of the map, in pixels (y1, x1, y2, x2); distinct positions"""
    ys = list(range(1, Hm - side - 1))
    xs = list(range(1, Wm - side - 1))
    assert len(ys) * len(xs) >= n, "the lattice holds %d boxes" % (len(ys) * len(xs))
    step = (len(ys) * len(xs)) // n
    out = []
    for q in range(n):
        p = q * step
        out.append((ys[p // len(xs)], xs[p % len(xs)], ys[p // len(xs)] + side, xs[p % len(xs)] + side))
    return out


def sel_case(D, G, B=3):
    """detections [B,D,6], true_boxes [B,G,5], perms.  On the 24 x 40 map:
    image 0: every second row of true_boxes holds a 16-pixel box of a lattice (zero rows between them); every detection row but
             each fifth holds such a box moved by one map pixel down and right -- IoU 15 * 15 / (2 * 256 - 225) = 225/287 with
             its original, so it is positive whatever the other boxes add -- or, each seventh filled row, a 3-pixel box on the
             top edge (IoU at most 9/256 with any 16-pixel box: negative);
    image 1: boxes as image 0, but only 5 non-zero detections (fewer than any n_det here above 5);
    image 2: detections as image 0 and no box at all: no positive.
    The permutations are non-identity and hold every index."""
    key = (D, G, B)
    if key in _SEL:
        return _SEL[key]
    Hm, Wm = SEL_MAP
    rng = np.random.RandomState(4000 + D + G)
    det = np.zeros((B, D, 6), np.float32)
    tb = np.zeros((B, G, 5), np.float32)
    perms = []
    grow = list(range(0, G, 2))
    boxes = lattice(len(grow), Hm, Wm, 16)                        # 6 x 22 = 132 positions >= the 128 boxes of G = 256
    for b in range(B):
        if b < 2:
            for r, (y1, x1, y2, x2) in zip(grow, boxes):
                tb[b, r] = [(x1 + x2) / 2.0 / Wm, (y1 + y2) / 2.0 / Hm, (x2 - x1) / float(Wm), (y2 - y1) / float(Hm), r % 3]
        prow = [q for q in range(D) if q % 5 != 4]
        if b == 1:
            prow = prow[:5]
        for j, q in enumerate(prow):
            if j % 7 == 6:
                det[b, q] = [0.0, (j % 30) / 40.0, 3.0 / Hm, (j % 30 + 3) / 40.0, 0, 0.5]       # a 3-pixel box on the top edge
            else:
                y1, x1, y2, x2 = boxes[(j * 3) % len(boxes)]
                det[b, q] = [(y1 + 1.0) / Hm, (x1 + 1.0) / Wm, (y2 + 1.0) / Hm, (x2 + 1.0) / Wm, j % 3, 0.9]
        perms.append((rng.permutation(D).astype(np.int32), rng.permutation(G).astype(np.int32)))
    _SEL[key] = (det, tb, perms)
    return _SEL[key]


# ------------------------------------------------------------------------------------------------ 3. loss cases
LOSS_MAPS = ((24, 40), (36, 36))
LOSS_ROWS = (17, 64, 512)
LOSS_G = 24
_TAB = {}


def loss_table(nrow, Hm, Wm, k, B=3):
    """a table of ``nrow`` rows per image and its counts, on an Hm x Wm map, G = LOSS_G:
    image 0: up to twenty concentric boxes around the map's centre (the centre pixel is covered by all of them), one small box
             over the last map row's first columns, one box across each of the four borders, then boxes of sides 3 .. 16 on a
             lattice that reaches 2 pixels past the borders; nrow rows in all, every one with pixels on the map;
    image 1: min(nrow, 9) rows, all within the map's first 6 rows -- the blocks behind them cull to an empty list;
    image 2: no row."""
    key = (nrow, Hm, Wm, k, B)
    if key in _TAB:
        return _TAB[key]
    cy, cx = Hm // 2, Wm // 2
    px = []
    for j in range(min(20, nrow)):
        h = 1 + j // 2
        px.append((cy - h, cx - h - (j % 2), cy + h + (j % 2), cx + h))
    px.append((Hm - 2, 2, Hm + 1, 10))                            # the last rows of the map, the first columns
    px += [(-2, 3, 4, 9), (Hm - 3, 5, Hm + 2, 12), (1, -2, 6, 5), (1, Wm - 4, 6, Wm + 2)]    # one across each border
    sides = (3, 5, 8, 12, 16)
    q = 0
    while len(px) < nrow:
        s = sides[q % len(sides)]
        span_y, span_x = max(Hm + 4 - s, 0), max(Wm + 4 - s, 0)   # y1 in -2 .. Hm + 2 - s: at least one row on the map
        y1 = -2 + (q * 7) % (span_y + 1)
        x1 = -2 + (q * 11) % (span_x + 1)
        px.append((y1, x1, y1 + s, x1 + s + (q % 3)))
        q += 1
    px = px[:nrow]
    img0 = [row_of(y1, x1, y2, x2, (j * 5) % LOSS_G, Hm, Wm, k) for j, (y1, x1, y2, x2) in enumerate(px)]
    img1 = [row_of(j % 3, 2 * j, j % 3 + 3, 2 * j + 6, j % LOSS_G, Hm, Wm, k) for j in range(min(nrow, 9))]
    _TAB[key] = table_of([img0, img1, []][:B], nrow, k)
    return _TAB[key]


def loss_inputs(Hm, Wm, k, st, B=3, seed=0):
    """score f32 [B,Hm,Wm,k*k] (a few exact zeros) and true_masks uint8 [B,LOSS_G,st*Hm,st*Wm]"""
    g = torch.Generator().manual_seed(1000 * k + 10 * st + seed + Hm)
    score = torch.randn(B, Hm, Wm, k * k, generator=g) * 2.0
    score[torch.rand(score.shape, generator=g) < 0.02] = 0.0
    tm = (torch.rand(B, LOSS_G, st * Hm, st * Wm, generator=g) < 0.5).to(torch.uint8)
    return score, tm


def loss_want(table, cnt, score, tm, st, k):
    """(float64 loss, gradient wrt the score maps [B,Hm,Wm,k*k])"""
    sc = score.double().clone().requires_grad_(True)
    lm = table_loss(table, cnt, sc, tm.numpy(), st, k)
    if lm.requires_grad:
        lm.backward()
    grad = sc.grad if sc.grad is not None else torch.zeros_like(sc)
    return float(lm.detach()), grad.detach()


# ------------------------------------------------------------------------------------------------ 4. the whole net
NET_B, NET_S, NET_G, NET_D = 2, 64, 40, 40
NET_ROWS = tuple(range(0, 40, 2))                               # twenty instances per image: twenty positives by themselves
PLANT_MIN = 8.0                                                 # pixels: a planted detection covers at least 4 x 4 of the map


def plant_detections(batch, det, anchors, n=3, num_class=3):
    """The detections of an untrained net overlap the boxes of a synthetic batch, but none by half.  So that detections are
    positive by construction, the first ``n`` detections of each image that are at least PLANT_MIN pixels on both sides become
    ground truth: each replaces one filled row of true_boxes (its box), of true_masks (the box, filled) and the image's
    targets are assigned again.  The forward pass does not read the labels, so the net yields the same detections on the new
    batch, each of them with IoU 1 (to rounding) with its row.  Returns (the new batch, planted rows per image)."""
    S = batch["images"].shape[1]
    b = dict(batch)
    tb = batch["true_boxes"].numpy().copy()
    tm = np.array(batch["true_masks"], copy=True)
    ys = [batch[k].numpy().copy() for k in ("yolo3", "yolo2", "yolo1")]
    planted = []
    for i in range(tb.shape[0]):
        rows = [r for r in range(tb.shape[4]) if np.abs(tb[i, 0, 0, 0, r, :4]).sum() != 0]
        d = det[i].astype(np.float32)
        big = [q for q in range(len(d)) if (d[q, 2] - d[q, 0]) * S >= PLANT_MIN and (d[q, 3] - d[q, 1]) * S >= PLANT_MIN][:n]
        for q, r in zip(big, rows):
            y1, x1, y2, x2 = d[q, :4]
            tb[i, 0, 0, 0, r, :4] = [(x1 + x2) / np.float32(2), (y1 + y2) / np.float32(2), x2 - x1, y2 - y1]
            tm[i, r] = False
            tm[i, r, max(int(np.floor(y1 * S)), 0):int(np.ceil(y2 * S)), max(int(np.floor(x1 * S)), 0):int(np.ceil(x2 * S))] = True
        planted.append(list(zip(big, rows)))
        boxes = tb[i, 0, 0, 0, rows, :4] * np.float32(S)
        for dst, t in zip(ys, O.assign_targets(boxes.astype(np.float32), tb[i, 0, 0, 0, rows, 4].astype(np.int64), S, anchors=anchors,
                                               num_class=num_class)):
            t[..., 0:4] /= S
            dst[i] = t
    b["true_boxes"], b["true_masks"] = torch.from_numpy(tb), tm
    b["yolo3"], b["yolo2"], b["yolo1"] = (torch.from_numpy(y) for y in ys)
    return b, planted

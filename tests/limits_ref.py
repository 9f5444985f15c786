"""Cases and CPU references for the per-net limits (anchors, max_box_per_image, max_detection up to 256): the inputs of
tests/test_gpu_limits.py and, without a GPU, of tests/test_limits.py, which runs every case through the oracle alone and holds
it to the condition that makes it a case at all (more than 64 kept rows, a ``noobj`` term that rows >= 64 decide, a selected
row >= 64).  Every case is computed once, cached, and left unchanged.

The oracle takes the three values as arguments (``interpret_output(anchors=)``, ``filter_detections(max_detection=)``,
``assign_targets(anchors=)``) or from the array shapes (``loss_yolo``, ``loss_mask``, ``select_mask_rois``); only
``O.total_loss`` bakes the defaults in, so ``total_loss`` here composes it from those functions."""
import numpy as np
import torch

import disyolo_oracle as O
import nms_modes_ref as R
from disyolo_amd import config as cfg

ANCH = np.asarray(cfg.ANCHORS, np.float32)
NET_ANCH = (ANCH * np.float32(0.11)).astype(np.float32)         # the whole-net cases: non-integer anchors
OLD = 64                                                        # the limit of the entry points from before


# ------------------------------------------------------------------------------------------------ 1. the filter
FILTER_S, FILTER_B = 96, 2                                       # 567 candidates: the smallest net with more than 256
FILTER_THR, FILTER_NMS = 0.25, 0.45
FILTER_WIN = [[0.0, 0.0, 1.0, 1.0], [0.1, 0.05, 0.9, 0.95]]      # the second image has a window of its own
FILTER_D = (65, 100, 256)
FILTER_C = (3, 80)
# small boxes (a few pixels of a 96-pixel image), so that greedy NMS leaves most candidates standing
FILTER_ANCH = np.array([[4, 5], [7, 4], [5, 8], [9, 9], [12, 7], [7, 13], [14, 15], [19, 11], [12, 21]], np.float32)
_FILTER = {}


def n_cand(S):
    return 3 * ((S // 8) ** 2 + (S // 16) ** 2 + (S // 32) ** 2)


def filter_logits(C, S=FILTER_S, B=FILTER_B):
    """random logits [B,g,g,3,5+C] x 3, shifted so that far more than 256 of the 567 candidates pass the threshold; conf and
    class logits rounded (class margin 40: the softmax maximum is 1, 1/2, 1/3 ... exactly), so that scores tie"""
    key = (C, S, B)
    if key not in _FILTER:
        g = torch.Generator().manual_seed(100 + C)
        ys = [torch.randn(B, S // d, S // d, 3, 5 + C, generator=g) for d in (8, 16, 32)]
        for y in ys:
            y[..., 2:4] *= 0.3
            y[..., 4] = torch.round(y[..., 4] * 1.5) + 3.0
            y[..., 5:] = torch.round(y[..., 5:]) * 40.0
        _FILTER[key] = ys
    return _FILTER[key]


def filter_want(ys, D, mode, S=FILTER_S, anchors=FILTER_ANCH, win=FILTER_WIN, thr=FILTER_THR, nms=FILTER_NMS):
    """(rows [B,D,6], counts, candidates above the threshold per image) from the oracle's own decode"""
    pred = O.interpret_output(ys, anchors=anchors)
    B = ys[0].shape[0]
    rows, cnt, above = np.zeros((B, D, 6), np.float32), [], []
    for i in range(B):
        boxes, scores, classes = R.decode(pred[2], pred[3], pred[5], np.asarray(win[i], np.float32), i)
        idx = R.select(boxes, scores, classes, thr, nms, D, mode)
        rows[i] = R.rows_of(boxes, scores, classes, idx, D)
        cnt.append(len(idx))
        above.append(int((scores > np.float32(thr)).sum()))
    return rows, cnt, above


def restated(dec, thr, nms_thr, mode, max_det):
    """tests/test_gpu_nms_modes.py ``restated``: the filter on the boxes / scores / classes the decode kernel wrote"""
    boxes, scores, classes = dec
    rows, cnt = np.zeros((len(boxes), max_det, 6), np.float32), []
    for b in range(len(boxes)):
        idx = R.select(boxes[b], scores[b], classes[b], thr, nms_thr, max_det, mode)
        rows[b] = R.rows_of(boxes[b], scores[b], classes[b], idx, max_det)
        cnt.append(len(idx))
    return rows, cnt


# ------------------------------------------------------------------------------------------------ 2. shuffle_perm
def hash32(x):
    x = np.asarray(x, np.uint64) & np.uint64(0xffffffff)
    m = np.uint64(0xffffffff)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7feb352d)) & m
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846ca68b)) & m
    x ^= x >> np.uint64(16)
    return x


def shuffle_perm_want(n, B, which, seed, step):
    """the permutation rows shuffle_perm_kernel writes: the key of index t is a counter-based hash of (seed, step, image,
    which, t); position rank(t) receives t, ranks by (key, index)"""
    m = np.uint64(0xffffffff)
    base = hash32((np.uint64(seed) + np.uint64(0x9e3779b9) * np.uint64(step & 0xffffffff)) & m)
    out = np.zeros((B, n), np.int32)
    for b in range(B):
        t = np.arange(n, dtype=np.uint64)
        keys = hash32(base ^ hash32(((np.uint64(b * 2 + which) * np.uint64(0x85ebca6b)) & m) + t))
        order = np.lexsort((np.arange(n), keys))
        out[b] = order.astype(np.int32)
    return out


# ------------------------------------------------------------------------------------------------ 3. the RoI selection
ROI_MAP = (24, 40)                                               # a rectangular score map (Hm, Wm)
ROI_CASES = ((100, 65), (256, 256))
_ROI = {}


def roi_case(D, G, B=2):
    """detections [B,D,6], true_boxes [B,1,1,1,G,5], perms [(perm_det [D], perm_gt [G])] per image.  Non-zero rows are
    scattered with zero rows between them, up to the last row; at (256, 256) more than 64 of each are non-zero (several
    rounds of ballots, several ground-truth rows per lane).  Two ground-truth rows hold the same box -- at (256, 256) 64
    trimmed positions apart, the same lane -- and a detection on that box is among the first picked: the lower row must win.
    The permutations put trimmed positions whose rows are >= 64 first."""
    key = (D, G, B)
    if key in _ROI:
        return _ROI[key]
    rng = np.random.RandomState(1000 + D + G)
    det = np.zeros((B, D, 6), np.float32)
    tb = np.zeros((B, 1, 1, 1, G, 5), np.float32)
    perms = []
    for b in range(B):
        if G > 200:
            grow = sorted(rng.choice(G - 1, 150, replace=False).tolist() + [G - 1])
            prow = sorted(rng.choice(D - 1, 170, replace=False).tolist() + [D - 1])
        else:
            grow = sorted(rng.choice(OLD, 6, replace=False).tolist()) + list(range(OLD, G))
            prow = sorted(rng.choice(OLD, 8, replace=False).tolist() + rng.choice(np.arange(OLD, D - 1), 9, replace=False).tolist()
                          + [D - 1])
        for r in grow:
            w, h = rng.uniform(0.08, 0.5, size=2)
            tb[b, 0, 0, 0, r] = [rng.uniform(w / 2, 1 - w / 2), rng.uniform(h / 2, 1 - h / 2), w, h, rng.randint(0, 3)]
        # the twin: trimmed positions t0 and t1 hold the same box (t1 = t0 + 64 where the list is that long)
        t0 = 3
        t1 = t0 + 64 if len(grow) > t0 + 64 else t0 + 2
        tb[b, 0, 0, 0, grow[t1], :4] = tb[b, 0, 0, 0, grow[t0], :4]
        # detections: jittered copies of ground-truth boxes (IoU mostly above 0.5), a few far off
        for q, r in enumerate(prow):
            src = grow[t0] if q == len(prow) - 1 else grow[-1] if q == len(prow) - 2 else grow[rng.randint(0, len(grow))]
            xc, yc, w, h = tb[b, 0, 0, 0, src, :4]
            j = (rng.rand(4) - 0.5) * (0.06 if q % 5 else 0.5)
            if q == len(prow) - 1:
                j = j * 0.0                                       # exactly the twins' box: IoU 1 with both
            elif q == len(prow) - 2:
                j = j * 0.1                                       # on the last ground-truth row (G - 1 >= 64)
            det[b, r] = [yc - h / 2 + j[0], xc - w / 2 + j[1], yc + h / 2 + j[2], xc + w / 2 + j[3], q % 3, 0.9 - 0.001 * q]
        # permutations of 0..D-1 / 0..G-1 whose first entries are trimmed positions of rows >= 64
        hi_p = [q for q, r in enumerate(prow) if r >= OLD]
        hi_g = [q for q, r in enumerate(grow) if r >= OLD]
        first_p = [len(prow) - 1, len(prow) - 2] + [int(v) for v in rng.choice(hi_p[:-2], 3, replace=False)]
        first_g = [int(v) for v in rng.choice(hi_g, min(2, len(hi_g)), replace=False)]
        pd = first_p + [int(v) for v in rng.permutation(D) if v not in first_p]
        pg = first_g + [int(v) for v in rng.permutation(G) if v not in first_g]
        perms.append((np.asarray(pd, np.int32), np.asarray(pg, np.int32)))
    _ROI[key] = (det, tb, perms)
    return _ROI[key]


def roi_rows(det, tb, perms, Hm, Wm, k):
    """the RoI table mask_rois must write on an Hm x Wm map with a k x k grid (tests/test_gpu_kat.py ``expected_rois`` with
    each axis scaled by its own side): per image a list of rows [gy0..gyk, gx0..gxk, gt_row, area, 1, 0], and the selection"""
    out, picked = [], []
    for i in range(det.shape[0]):
        pos, assign, gt_rows = O.select_mask_rois(det[i], tb[i, 0, 0, 0], perms[i][0], perms[i][1])
        rows = []
        for r in range(len(pos)):
            y1, y2 = np.round(pos[r][0] * np.float32(Hm)), np.round(pos[r][2] * np.float32(Hm))
            x1, x2 = np.round(pos[r][1] * np.float32(Wm)), np.round(pos[r][3] * np.float32(Wm))
            gy, gx = O.kmask_edges(y1, y2, k), O.kmask_edges(x1, x2, k)
            area = 0
            for by in range(k):
                for bx in range(k):
                    hh = min(gy[by + 1], Hm) - max(gy[by], 0)
                    ww = min(gx[bx + 1], Wm) - max(gx[bx], 0)
                    if hh > 0 and ww > 0:
                        area += hh * ww
            rows.append(gy + gx + [int(gt_rows[assign[r]]), area, 1, 0])
        out.append(rows)
        picked.append((pos, assign, gt_rows))
    return out, picked


# ------------------------------------------------------------------------------------------------ 4. the YOLO loss
LOSS_S, LOSS_B = 64, 2
LOSS_G = (65, 256)
LOSS_C = (3, 80)
_LOSS = {}


def loss_case(C, G):
    """tests/test_gpu_loss.py ``yolo_case`` at B = 2, 64^2 with its boxes moved to rows >= 64 of a G-row table (rows < 64 are
    zero): image 0 has no box, image 1 has one box in row 64 (G = 65) or twelve spread over 64..255 (G = 256).  The labels
    do not depend on the row a box sits in."""
    from test_gpu_loss import check_yolo_preconditions, yolo_case
    key = (C, G)
    if key not in _LOSS:
        n = 1 if G == 65 else 12
        heads, labels, tb_n = yolo_case(LOSS_B, LOSS_S, C, n, 700 + C + G, cfg.IGNORE_THRESH)
        check_yolo_preconditions(heads, labels, tb_n, cfg.IGNORE_THRESH, need_mix=False)
        rows = [64] if G == 65 else [64, 65, 80, 100, 127, 128, 129, 191, 192, 200, 254, 255]
        tb = np.zeros((LOSS_B, G, 5), np.float32)
        tb[:, rows] = tb_n
        _LOSS[key] = (heads, labels, tb)
    return _LOSS[key]


def loss_terms(heads, labels, tb):
    """float64 [obj, noobj, class, xy, wh, conf, coord, total] (tests/test_gpu_loss.py ``yolo_oracle`` without the gradient)"""
    B, G = tb.shape[0], tb.shape[1]
    with torch.no_grad():
        ly = O.loss_yolo(O.interpret_output([torch.from_numpy(h).double() for h in heads]),
                         torch.from_numpy(tb).double().reshape(B, 1, 1, 1, G, 5), [torch.from_numpy(l).double() for l in labels])
    names = ("obj", "noobj", "class", "xy", "wh", "conf", "coord")
    return np.array([float(ly[k]) for k in names] + [float(ly["conf"] + ly["class"] + ly["coord"])])


# ------------------------------------------------------------------------------------------------ 5. the batched paste
def paste_case(n, h, w, ng, size, seed):
    """masks f32 [n,size,size], rects int32 [n,8], class ids, ground truth uint8 [ng,h,w] with classes, a true class map.
    Detections 3 and 70 -- either side of the first cover word's end -- overlap with different classes, and so do 63 and 64
    and the last two: the later one must own the overlap in the merged map."""
    rng = np.random.RandomState(seed)
    m = rng.rand(n, size, size).astype(np.float32)
    flat = m.reshape(-1)
    at = rng.choice(flat.size, size=200, replace=False)
    flat[at[::2]] = np.float32(0.5)
    flat[at[1::2]] = np.nextafter(np.float32(0.5), np.float32(1.0))
    r = np.zeros((n, 8), np.int32)
    cls = rng.randint(0, 3, size=n).astype(np.int32)
    for k in range(n):
        cy1, cx1 = rng.randint(0, size, size=2)
        cy2, cx2 = rng.randint(cy1, size + 1), rng.randint(cx1, size + 1)
        y1, x1 = rng.randint(0, h), rng.randint(0, w)
        y2, x2 = rng.randint(y1, min(h, y1 + max(h // 3, 2)) + 1), rng.randint(x1, min(w, x1 + max(w // 3, 2)) + 1)
        r[k] = [cy1, cx1, cy2, cx2, y1, x1, y2, x2]
    # planted pairs: a solid mask (every tap above 0.5) over the same destination, different classes
    for a, b, (y1, x1, y2, x2) in ((3, 70, (2, 3, h // 2, w // 2)), (63, 64, (h // 2, w // 2, h - 1, w - 2)),
                                   (n - 2, n - 1, (h // 3, 1, h // 3 + 5, w - 1))):
        for k, c in ((a, 0), (b, 2)):
            m[k] = np.float32(0.9)
            r[k] = [0, 0, size, size, y1, x1, y2, x2]
            cls[k] = c
    r[0] = [7, 3, 7, 20, 0, 0, h, w]                             # an empty crop
    r[1] = [2, 2, 30, 30, 0, w // 2, h, w // 2]                  # an empty destination
    gt = (rng.rand(ng, h, w) < 0.4).astype(np.uint8)
    gt_cls = rng.randint(0, 3, size=ng).astype(np.int32)
    tm = rng.randint(0, 6, size=(h, w)).astype(np.uint8)
    return m, r, cls, gt, gt_cls, tm


# ------------------------------------------------------------------------------------------------ 6. the whole net
NET_B, NET_S, NET_G, NET_D = 2, 64, 100, 100
NET_ROWS = (0, 23, 64, 77, 99)                                   # the rows of the five instances


def net_batch(seed, B=NET_B, S=NET_S, G=NET_G, anchors=NET_ANCH, rows=NET_ROWS, num_class=3):
    """the feed of tests' synthetic batches with G rows: five ellipses per image in rows ``rows`` of true_boxes / true_masks,
    targets assigned with ``anchors`` by the oracle, and injected permutations of D and G entries"""
    rng = np.random.RandomState(seed)
    images = torch.from_numpy(rng.rand(B, S, S, 3).astype(np.float32))
    true_boxes = np.zeros((B, 1, 1, 1, G, 5), np.float32)
    true_masks = np.zeros((B, G, S, S), bool)
    ys = [np.zeros((B, S // d, S // d, 3, 5 + num_class), np.float32) for d in (8, 16, 32)]
    yy, xx = np.mgrid[0:S, 0:S]
    for b in range(B):
        bx, cl = [], []
        for j in rows:
            while True:
                w, h = rng.uniform(0.08, 0.5, size=2) * S
                cx, cy = rng.uniform(w / 2, S - w / 2), rng.uniform(h / 2, S - h / 2)
                m = ((xx - cx) / (w / 2)) ** 2 + ((yy - cy) / (h / 2)) ** 2 <= 1.0
                rws, cols = np.where(m)
                if m.any() and cols.max() > cols.min() and rws.max() > rws.min():
                    break
            x1, x2, y1, y2 = cols.min(), cols.max(), rws.min(), rws.max()
            c = rng.randint(0, num_class)
            box = [(x1 + x2) / 2.0, (y1 + y2) / 2.0, float(x2 - x1), float(y2 - y1)]
            true_masks[b, j] = m
            true_boxes[b, 0, 0, 0, j, :4] = np.asarray(box, np.float32) / np.float32(S)
            true_boxes[b, 0, 0, 0, j, 4] = c
            bx.append(box)
            cl.append(c)
        for dst, t in zip(ys, O.assign_targets(np.asarray(bx, np.float32).reshape(-1, 4), np.asarray(cl), S, anchors=anchors,
                                               num_class=num_class)):
            t[..., 0:4] /= S
            dst[b] = t
    batch = {"images": images, "clip_window": torch.tensor([[0.0, 0.0, 1.0, 1.0]] * B), "true_boxes": torch.from_numpy(true_boxes),
             "true_masks": true_masks, "yolo3": torch.from_numpy(ys[0]), "yolo2": torch.from_numpy(ys[1]),
             "yolo1": torch.from_numpy(ys[2])}
    return batch


def with_perms(batch, D=NET_D, seed=0):
    B, G = batch["true_boxes"].shape[0], batch["true_boxes"].shape[4]
    rng = np.random.RandomState(seed)
    b = dict(batch)
    b["perm_det"] = np.stack([rng.permutation(D) for _ in range(B)]).astype(np.int32)
    b["perm_gt"] = np.stack([rng.permutation(G) for _ in range(B)]).astype(np.int32)
    return b, [(b["perm_det"][i], b["perm_gt"][i]) for i in range(B)]


def total_loss(params, batch, lock, anchors, max_detection, perms=None, updates=None, obj_thresh=O.OBJ_THRESHOLD, quant=None,
               taps=None, force=None):
    """``O.total_loss`` with the net's anchors and max_detection (G comes from the shapes of true_boxes / true_masks)"""
    yolos, mask_pos = O.build_network(params, batch["images"], True, lock, updates, taps, quant, force)
    pred = O.interpret_output(yolos, anchors=anchors)
    with torch.no_grad():
        det = O.filter_detections(pred[2], pred[3], pred[5], batch["clip_window"], obj_thresh, max_detection=max_detection)
    ly = O.loss_yolo(pred, batch["true_boxes"], [batch["yolo3"], batch["yolo2"], batch["yolo1"]])
    lm = O.loss_mask(det, mask_pos, batch["true_boxes"].detach().numpy(), batch["true_masks"], perms)
    reg = O.l2_regularization(params, lock)
    parts = dict(ly)
    parts["mask"] = lm
    parts["reg"] = reg
    parts["total"] = ly["conf"] + ly["class"] + ly["coord"] + lm + reg
    return parts, det, yolos, mask_pos


# ------------------------------------------------------------------------------------------------ 7. defect_train records
def rectangle_record(rng, h, w, n, classes):
    """a record of ``defect_train`` with n rectangular instances (one 'out' polygon each) on an h x w image"""
    polys, names = [], []
    for _ in range(n):
        bw, bh = rng.randint(6, w // 3), rng.randint(6, h // 3)
        x1, y1 = rng.randint(0, w - bw), rng.randint(0, h - bh)
        polys.append([{"type": "out", "all_points_x": [x1, x1 + bw, x1 + bw, x1], "all_points_y": [y1, y1, y1 + bh, y1 + bh]}])
        names.append(classes[rng.randint(0, len(classes))])
    return {"image": rng.randint(0, 256, (h, w, 3)).astype(np.uint8), "class_names": names, "polygons": polys}

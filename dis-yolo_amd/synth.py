"""Seeded synthetic training batches of the reference's feed_dict shape.

Restates the two pieces of the reference's CPU data path that define the tensors the hot
path consumes: the batch layout of ``defect_train.get`` (utils/train_data.py:44-52,258-265)
and the anchor/cell target assignment (utils/train_data.py:149-178).  Images are uniform
noise and instances are axis-aligned ellipses -- there is no dataset in the reference tree.
"""
from __future__ import annotations

import numpy as np

from . import config as cfg


def net_hw(S):
    """(net_h, net_w) of a net size given as one int S (square) or as a pair (H, W)"""
    if isinstance(S, (int, np.integer)):
        return int(S), int(S)
    h, w = S
    return int(h), int(w)


def assign_target_entries(boxes_px, cls, S, num_class: int, anchors=None):
    """utils/train_data.py:149-178 as a sparse list: best-IoU anchor of the 9 (boxes centred at the origin),
    cell = (int(xc * grid_w / net_w), int(yc * grid_h / net_h)); an occupied (cell, anchor) keeps its first box.  ``S``: the
    net's size, an int or (H, W).  Returns, per scale (yolo3, yolo2, yolo1), {(yi, xi, anchor): row float32 [5 + C]} in
    assignment order -- the non-zero rows of the dense target grids.  ``anchors``: the net's nine (w, h), cfg.ANCHORS unless
    given."""
    H, W = net_hw(S)
    sizes = [(H // d, W // d) for d in (8, 16, 32)]
    out = [dict() for _ in sizes]
    amax = np.asarray(cfg.ANCHORS if anchors is None else anchors, np.float32) / 2.0
    a_area = amax[:, 0] * amax[:, 1] * 4
    for b, c in zip(boxes_px, cls):
        half = np.asarray(b[2:4], np.float32) / 2.0
        inter = np.maximum(2 * np.minimum(half[None, :], amax), 0.0)
        ia = inter[:, 0] * inter[:, 1]
        iou = ia / (half[0] * half[1] * 4 + a_area - ia)
        if iou.max() <= 0:
            continue
        idx = int(np.argmax(iou))
        gh, gw = sizes[idx // 3]
        xi, yi = int(b[0] * gw / W), int(b[1] * gh / H)
        key = (yi, xi, idx % 3)
        if key in out[idx // 3]:
            continue
        row = np.zeros(5 + num_class, np.float32)
        row[0:4] = b[:4]
        row[4] = 1
        row[5 + int(c)] = 1.0
        out[idx // 3][key] = row
    return out


def assign_targets(boxes_px, cls, S, num_class: int, anchors=None):
    """the dense grids of utils/train_data.py:149-178: [gh, gw, 3, 5 + C] per scale (yolo3, yolo2, yolo1)"""
    H, W = net_hw(S)
    yolos = [np.zeros((H // d, W // d, 3, 5 + num_class), np.float32) for d in (8, 16, 32)]
    for y, ent in zip(yolos, assign_target_entries(boxes_px, cls, S, num_class, anchors)):
        for (yi, xi, a), row in ent.items():
            y[yi, xi, a] = row
    return yolos


def synthetic_batch(B: int, S, seed: int = 1234, num_class: int = 3, anchors=None, max_box_per_image=None):
    """dict of numpy arrays for a net of size ``S`` (an int, or (H, W)): images f32 [B,H,W,3] in [0,1), clip_window [B,4] =
    (0,0,1,1), true_boxes [B,1,1,1,20,5] (xc,yc,w,h normalised -- x, w by W and y, h by H --, class), true_masks bool
    [B,20,H,W], yolo1/2/3 targets [B,gh,gw,3,5+C] with normalised boxes.  The order and count of the RNG draws do not depend
    on the shape.  ``anchors`` / ``max_box_per_image``: the net's (the 20 above becomes G); the cfg values unless given."""
    H, W = net_hw(S)
    norm = np.asarray([W, H, W, H], np.float32)
    rng = np.random.RandomState(seed)
    G = cfg.MAX_BOX_PER_IMAGE if max_box_per_image is None else int(max_box_per_image)
    images = rng.rand(B, H, W, 3).astype(np.float32)
    true_boxes = np.zeros((B, 1, 1, 1, G, 5), np.float32)
    true_masks = np.zeros((B, G, H, W), bool)
    ys = [np.zeros((B, H // d, W // d, 3, 5 + num_class), np.float32) for d in (8, 16, 32)]
    yy, xx = np.mgrid[0:H, 0:W]
    for b in range(B):
        bx, cl = [], []
        for j in range(min(rng.randint(1, 6), G)):             # (one to five instances; no more than the table's rows)
            w, h = rng.uniform(0.05, 0.6, size=2) * np.asarray([W, H])
            cx, cy = rng.uniform(w / 2, W - w / 2), rng.uniform(h / 2, H - h / 2)
            m = ((xx - cx) / (w / 2)) ** 2 + ((yy - cy) / (h / 2)) ** 2 <= 1.0
            if not m.any():
                continue
            rows, cols = np.where(m)
            x1, x2, y1, y2 = cols.min(), cols.max(), rows.min(), rows.max()
            if x2 <= x1 or y2 <= y1:
                continue
            c = rng.randint(0, num_class)
            box = [(x1 + x2) / 2.0, (y1 + y2) / 2.0, float(x2 - x1), float(y2 - y1)]
            true_masks[b, j] = m
            true_boxes[b, 0, 0, 0, j, :4] = np.asarray(box, np.float32) / norm
            true_boxes[b, 0, 0, 0, j, 4] = c
            bx.append(box)
            cl.append(c)
        for dst, t in zip(ys, assign_targets(np.asarray(bx, np.float32).reshape(-1, 4), cl, (H, W), num_class, anchors)):
            t[..., 0:4] /= norm
            dst[b] = t
    return {"images": images, "clip_window": np.tile(np.array([[0, 0, 1, 1]], np.float32), (B, 1)),
            "true_boxes": true_boxes, "true_masks": true_masks, "yolo3": ys[0], "yolo2": ys[1], "yolo1": ys[2]}

"""The definition of window training (``defect_train(placement="window")``) in numpy: what a net-size window
of a record at scale 1 holds -- the visible part of every instance, which instances are kept, their boxes, the three target
grids, the mask planes and the image.  The full-image raster is the oracle's (``disyolo_oracle.instance_mask``); everything
after it is the loader's own host arithmetic (``train_data.static_box`` / ``window_candidates``, ``synth.assign_target_entries``
and the flip / normalise lines of ``defect_train._fill``), in f32, operation by operation.  The kernels of csrc/augment.hip
(window_visible, window_targets, window_place_masks) are held to this, bit for bit."""
import numpy as np

import disyolo_oracle as O
from disyolo_amd import config as cfg
from disyolo_amd.synth import assign_target_entries
from disyolo_amd.train_data import static_box, window_candidates

NET = (64, 96)            # the net of the scene's sweep (H, W)


def polygon12(cx, cy, rx, ry, kind="out"):
    t = np.arange(12) * (2 * np.pi / 12)          # (i times the step: the areas test_windows.py pins belong to this form)
    return {"type": kind, "all_points_x": [int(cx + rx * np.cos(a)) for a in t], "all_points_y": [int(cy + ry * np.sin(a)) for a in t]}


def scene():
    """a 150 x 200 record with five instances in record order: a crack (a thin band through the image), a spall with a hole, a
    rebar, a rebar inside the spall, a tiny spall"""
    xs = list(range(5, 186, 10))
    crack = {"type": "out", "all_points_x": xs + xs[::-1],
             "all_points_y": [int(20 + 0.6 * x) for x in xs] + [int(23 + 0.6 * x) for x in xs[::-1]]}
    hole = {"type": "in", "all_points_x": [135, 145, 140], "all_points_y": [36, 36, 44]}
    image = np.random.RandomState(7).randint(0, 256, (150, 200, 3)).astype(np.uint8)
    return {"image": image, "class_names": ["crack", "spall", "rebar", "rebar", "spall"],
            "polygons": [[crack], [polygon12(140, 40, 30, 22), hole], [polygon12(40, 110, 18, 14)], [polygon12(150, 45, 6, 5)],
                         [polygon12(100, 75, 3, 3)]]}


_FULL = {}


def record(label):
    """(image uint8 [h,w,3], full-image masks bool [n,h,w], static boxes [(x1,y1,x2,y2)], class names) of the record's instances
    with a non-empty static box, in record order; rasterised once per record object"""
    hit = _FULL.get(id(label))
    if hit is None:
        image = np.asarray(label["image"], np.uint8)
        h, w = image.shape[:2]
        masks, boxes, names = [], [], []
        for polys, name in zip(label["polygons"], label["class_names"]):
            box = static_box(polys, h, w)
            if box[2] <= box[0] or box[3] <= box[1]:
                continue
            masks.append(O.instance_mask(polys, h, w))
            boxes.append(box)
            names.append(name)
        hit = _FULL[id(label)] = (label, image, np.asarray(masks, bool).reshape(-1, h, w), boxes, names)
    return hit[1:]


def visible(mask, x0, y0, net_hw):
    """the visible part of a full-image mask in the window at (x0, y0): bool [net_h, net_w] in window coordinates, unflipped
    (what lies outside the image is not visible)"""
    H, W = net_hw
    out = np.zeros((H, W), bool)
    part = mask[y0:y0 + H, x0:x0 + W]
    out[:part.shape[0], :part.shape[1]] = part
    return out


def vis_row(v):
    """(count, x1, y1, x2, y2) of a visible part: its pixels and their tight box, x2 / y2 one past; zeros when empty"""
    n = int(v.sum())
    if n == 0:
        return [0, 0, 0, 0, 0]
    cols, rows = np.nonzero(v.any(axis=0))[0], np.nonzero(v.any(axis=1))[0]
    return [n, int(cols[0]), int(rows[0]), int(cols[-1]) + 1, int(rows[-1]) + 1]


def _flip(a, flip):
    return a[:, ::-1] if flip == 2 else (a[::-1] if flip == 3 else a)


def window_image(image, x0, y0, flip, net_hw):
    """uint8 [net_h, net_w, 3]: the window of the record's bytes, 127 where the window leaves the image, flipped"""
    H, W = net_hw
    out = np.full((H, W, 3), 127, np.uint8)
    part = image[y0:y0 + H, x0:x0 + W]
    out[:part.shape[0], :part.shape[1]] = part
    return np.ascontiguousarray(_flip(out, flip))


def window_ref(label, x0, y0, flip=1, net_hw=NET, min_visible=8, G=cfg.MAX_BOX_PER_IMAGE, classes=cfg.CLASSES, anchors=None,
               want_masks=True):
    """One window of one record.  Returns a dict:
      cand   the candidate instances (indices into ``record(label)``), vis int32 [ncand,5], rows int32 [ncand] (-1 = dropped)
      true_boxes f32 [G,5], yolo3 / yolo2 / yolo1 f32 [net/d, net/d, 3, 5+C], true_masks bool [G,net_h,net_w], image uint8"""
    H, W = net_hw
    C = len(classes)
    image, masks, boxes, names = record(label)
    cand = window_candidates(boxes, x0, y0, H, W)
    vis = np.zeros((len(cand), 5), np.int32)
    rows = np.full(len(cand), -1, np.int32)
    true_masks = np.zeros((G, H, W), bool) if want_masks else None
    bx, cls = [], []
    for k, i in enumerate(cand):
        v = visible(masks[i], x0, y0, net_hw)
        vis[k] = vis_row(v)
        n, x1, y1, x2, y2 = (int(t) for t in vis[k])
        # defect_train._fill's lines with sx = sy = 1, dx = dy = 0
        x1 = max(min(float(x1) * 1.0 + 0, W - 1), 0)
        y1 = max(min(float(y1) * 1.0 + 0, H - 1), 0)
        x2 = max(min(float(x2) * 1.0 + 0, W - 1), 0)
        y2 = max(min(float(y2) * 1.0 + 0, H - 1), 0)
        if n < min_visible or not x2 - x1 > 0 or not y2 - y1 > 0 or len(bx) >= G:
            continue
        rows[k] = len(bx)
        if want_masks:
            true_masks[len(bx)] = _flip(v, flip)
        bx.append([(x2 + x1) / 2.0, (y2 + y1) / 2.0, x2 - x1, y2 - y1])
        cls.append(list(classes).index(names[i]))
    bx = np.asarray(bx, np.float32).reshape(-1, 4)
    grids = assign_target_entries(bx, cls, (H, W), C, anchors)
    sizes = [(H // d, W // d) for d in (8, 16, 32)]
    # the loader's flip: the grids mirrored and the stored centres reflected
    if flip == 2:
        bx[:, 0] = W - 1 - bx[:, 0]
        for k, ent in enumerate(grids):
            for row in ent.values():
                row[0] = np.float32(W - 1) - row[0]
            grids[k] = {(yi, sizes[k][1] - 1 - xi, a): row for (yi, xi, a), row in ent.items()}
    elif flip == 3:
        bx[:, 1] = H - 1 - bx[:, 1]
        for k, ent in enumerate(grids):
            for row in ent.values():
                row[1] = np.float32(H - 1) - row[1]
            grids[k] = {(sizes[k][0] - 1 - yi, xi, a): row for (yi, xi, a), row in ent.items()}
    norm = np.asarray([W, H, W, H], np.float32)
    true_boxes = np.zeros((G, 5), np.float32)
    true_boxes[:len(bx), :4] = bx / norm
    true_boxes[:len(bx), 4] = cls
    ys = [np.zeros((gh, gw, 3, 5 + C), np.float32) for gh, gw in sizes]
    cells = 0
    for k, ent in enumerate(grids):
        for (yi, xi, a), row in ent.items():
            row[0:4] = row[0:4] / norm
            ys[k][yi, xi, a] = row
            cells += 1
    return {"cand": cand, "vis": vis, "rows": rows, "true_boxes": true_boxes, "yolo3": ys[0], "yolo2": ys[1], "yolo1": ys[2],
            "true_masks": true_masks, "image": window_image(image, x0, y0, flip, net_hw), "cells": cells}


def origins(label, net_hw=NET):
    """every window origin (x0, y0) of the record"""
    h, w = np.asarray(label["image"]).shape[:2]
    return [(x0, y0) for y0 in range(max(h - net_hw[0], 0) + 1) for x0 in range(max(w - net_hw[1], 0) + 1)]

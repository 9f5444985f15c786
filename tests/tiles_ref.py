"""Tiled detection (disyolo_amd.tiles), restated in numpy for the tests.

The reference project has no tiling, so there is no text of it to restate: this file IS the definition the HIP path is held
to.  It is composed from what the tests already trust -- rect_ref.paste_detections (the reference's paste, with the tile as
the "image", so the scale is 1) -- and plain integer / boolean numpy:

  plan      per axis: one origin 0 if n <= N, else cnt = ceil((n - o) / (N - o)) origins (i * (n - N)) // (cnt - 1)
  gather    inside the image (float)((double)v / 255.0), outside 127 through the same division; a tile index >= T is all pad
  instances the kept rows with a non-empty paste, numbered in (tile, row) order
  pairs     instances of different tiles and the same class whose image-space rects intersect
  counts    |A n R|, |B n R|, |A n B| with R = the two tiles' windows n the image
  join      ni > 0 and ni >= merge_overlap * min(na, nb) (float64); union-find
  groups    score = max of the members, box = union of the members' rects clipped to the image; order: score descending, ties
            to the lower first member
  compose   group mask = OR of the members, cropped to the box; owner = 1 + rank of the LAST covering group; merged = class
            of the owner + 1

Every quantity is an integer or a bit, so the tests compare with equality."""
from collections import namedtuple

import numpy as np

import disyolo_oracle as O
import rect_ref as RR


def plan_axis(n: int, N: int, o: int):
    if n <= N:
        return [0]
    cnt = -(-(n - o) // (N - o))
    return [(i * (n - N)) // (cnt - 1) for i in range(cnt)]


def plan_tiles(image_h: int, image_w: int, net_size, overlap) -> np.ndarray:
    H, W = RR.hw(net_size)
    oy, ox = RR.hw(overlap)
    ys, xs = plan_axis(image_h, H, oy), plan_axis(image_w, W, ox)
    return np.array([(y, x) for y in ys for x in xs], np.int32).reshape(-1, 2)


def tile_window(origin, image_hw, net_size) -> np.ndarray:
    H, W = RR.hw(net_size)
    return np.array([0.0, 0.0, min(H, image_hw[0] - int(origin[0])) / H, min(W, image_hw[1] - int(origin[1])) / W], np.float32)


def tile_gather(image_rgb: np.ndarray, tiles: np.ndarray, t0: int, t1: int, net_size) -> np.ndarray:
    H, W = RR.hw(net_size)
    h, w = image_rgb.shape[:2]
    out = np.full((t1 - t0, H, W, 3), 127, np.uint8)
    for t in range(t0, min(t1, len(tiles))):
        y0, x0 = (int(v) for v in tiles[t])
        hh, ww = min(H, h - y0), min(W, w - x0)
        out[t - t0, :hh, :ww] = image_rgb[y0:y0 + hh, x0:x0 + ww]
    return (out.astype(np.float64) / 255.0).astype(np.float32)


Instance = namedtuple("Instance", "tile row classid score rect mask")     # rect (y1,x1,y2,x2) in the image, mask bool [H,W] of the tile


def instances(tiles, image_hw, net_size, detections, keep, masks):
    """the kept rows with a non-empty paste, in (tile, row) order; ``masks`` [T,D,Hm,Wm]"""
    H, W = RR.hw(net_size)
    h, w = image_hw
    out = []
    for t in range(len(tiles)):
        rows = np.flatnonzero(np.asarray(keep[t]).astype(bool))
        if rows.size == 0:
            continue
        box = np.asarray(detections[t], np.float32)[rows]
        entries, _ = RR.paste_detections(box, np.asarray(masks[t], np.float32)[rows], H, W, H, W)
        y0, x0 = (int(v) for v in tiles[t])
        for e in entries:
            b = box[e["index"]]
            x1, y1, x2, y2 = O.correct_yolo_boxes(np.float32(b[1]), np.float32(b[0]), np.float32(b[3]), np.float32(b[2]), H, W, H, W)
            rect = (min(max(y0 + int(y1), 0), h), min(max(x0 + int(x1), 0), w), min(max(y0 + int(y2), 0), h), min(max(x0 + int(x2), 0), w))
            out.append(Instance(t, int(rows[e["index"]]), e["classid"], np.float32(b[5]), rect, e["mask"]))
    return out


def seam_rect(oa, ob, image_hw, net_size):
    """R: the intersection of two tiles' windows and the image, (y1, x1, y2, x2); empty when y2 <= y1 or x2 <= x1"""
    H, W = RR.hw(net_size)
    return (max(int(oa[0]), int(ob[0]), 0), max(int(oa[1]), int(ob[1]), 0),
            min(int(oa[0]) + H, int(ob[0]) + H, image_hw[0]), min(int(oa[1]) + W, int(ob[1]) + W, image_hw[1]))


def seam_counts(mask_a, oa, mask_b, ob, image_hw, net_size):
    """(|A n R|, |B n R|, |A n B|) of two tile-local bool masks [H,W] at origins oa, ob"""
    y1, x1, y2, x2 = seam_rect(oa, ob, image_hw, net_size)
    if y2 <= y1 or x2 <= x1:
        return 0, 0, 0
    a = mask_a[y1 - int(oa[0]):y2 - int(oa[0]), x1 - int(oa[1]):x2 - int(oa[1])]
    b = mask_b[y1 - int(ob[0]):y2 - int(ob[0]), x1 - int(ob[1]):x2 - int(ob[1])]
    return int(a.sum()), int(b.sum()), int((a & b).sum())


def rects_intersect(ra, rb) -> bool:
    return min(ra[2], rb[2]) > max(ra[0], rb[0]) and min(ra[3], rb[3]) > max(ra[1], rb[1])


def pair_table(inst):
    return [(a, b) for a in range(len(inst)) for b in range(a + 1, len(inst))
            if inst[a].tile != inst[b].tile and inst[a].classid == inst[b].classid and rects_intersect(inst[a].rect, inst[b].rect)]


Merged = namedtuple("Merged", "boxes classid score members masks owner merged instances pairs counts")


def merge_tiles(tiles, image_hw, net_size, detections, keep, masks, merge_overlap=0.5):
    """-> boxes int32 [G,4] (y1,x1,y2,x2), classid int32 [G], score f32 [G], members [[(tile,row)]], masks [bool [bh,bw]]
    (cropped to the boxes), owner int32 [h,w], merged uint8 [h,w]; and the intermediate instances, pairs and counts"""
    h, w = image_hw
    inst = instances(tiles, image_hw, net_size, detections, keep, masks)
    pairs = pair_table(inst)
    counts = [seam_counts(inst[a].mask, tiles[inst[a].tile], inst[b].mask, tiles[inst[b].tile], image_hw, net_size)
              for a, b in pairs]
    parent = list(range(len(inst)))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    for (a, b), (na, nb, ni) in zip(pairs, counts):
        if ni > 0 and float(ni) >= float(merge_overlap) * float(min(na, nb)):
            ra, rb = find(a), find(b)
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)
    groups = {}
    for i in range(len(inst)):
        groups.setdefault(find(i), []).append(i)
    order = sorted(groups.values(), key=lambda g: (-float(max(inst[i].score for i in g)), g[0]))
    boxes = np.zeros((len(order), 4), np.int32)
    classid = np.zeros(len(order), np.int32)
    score = np.zeros(len(order), np.float32)
    members, gmasks = [], []
    owner = np.zeros((h, w), np.int32)
    merged = np.zeros((h, w), np.uint8)
    H, W = RR.hw(net_size)
    for g, mem in enumerate(order):
        r = np.array([inst[i].rect for i in mem])
        boxes[g] = (r[:, 0].min(), r[:, 1].min(), r[:, 2].max(), r[:, 3].max())
        classid[g] = inst[mem[0]].classid
        score[g] = max(inst[i].score for i in mem)
        members.append([(inst[i].tile, inst[i].row) for i in mem])
        canvas = np.zeros((h, w), bool)
        for i in mem:
            y0, x0 = (int(v) for v in tiles[inst[i].tile])
            hh, ww = min(H, h - y0), min(W, w - x0)
            canvas[y0:y0 + hh, x0:x0 + ww] |= inst[i].mask[:hh, :ww]
        y1, x1, y2, x2 = boxes[g]
        crop = np.zeros((h, w), bool)
        crop[y1:y2, x1:x2] = canvas[y1:y2, x1:x2]
        gmasks.append(crop[y1:y2, x1:x2].copy())
        owner[crop] = g + 1
        merged[crop] = classid[g] + 1
    return Merged(boxes, classid, score, members, gmasks, owner, merged, inst, pairs, counts)


# ------------------------------------------------------------------------------------------------ the scene of the tests
SCENE_HW = (150, 200)


def scene_objects(image_hw=SCENE_HW):
    """five objects [(classid, bool [h,w])]: a crack through the image, an ellipse in four tiles, and three more"""
    h, w = image_hw
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    p0, p1 = np.array([10.0, 10.0]), np.array([140.0, 190.0])
    d = p1 - p0
    s = np.clip(((yy - p0[0]) * d[0] + (xx - p0[1]) * d[1]) / (d @ d), 0.0, 1.0)
    band = np.hypot(yy - (p0[0] + s * d[0]), xx - (p0[1] + s * d[1])) <= 4.0

    def ellipse(cy, cx, ry, rx):
        return ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
    return [(0, band), (1, ellipse(53, 74, 8, 14)), (1, ellipse(125, 40, 10, 12)), (2, ellipse(75, 100, 12, 20)),
            (0, ellipse(30, 160, 8, 10))]


Scene = namedtuple("Scene", "image_hw net_size tiles objects detections keep masks")


def scene(net_size=(64, 96), overlap=16, mask_stride=2, max_det=8, image_hw=SCENE_HW):
    """per tile every object with >= 12 visible pixels is a detection: the tight box of the visible part, the mask
    0.9 * (m x m mean) + 0.05 at map size, the score 0.9 - 0.01 object - 0.001 tile, rows by descending score"""
    H, W = RR.hw(net_size)
    h, w = image_hw
    m = mask_stride
    objects = scene_objects(image_hw)
    tiles = plan_tiles(h, w, net_size, overlap)
    T = len(tiles)
    det = np.zeros((T, max_det, 6), np.float32)
    keep = np.zeros((T, max_det), np.int32)
    masks = np.zeros((T, max_det, H // m, W // m), np.float32)
    for t, (y0, x0) in enumerate(tiles):
        row = 0
        for k, (cid, obj) in enumerate(objects):                  # (scores fall with k: already in descending order)
            vis = np.zeros((H, W), bool)
            hh, ww = min(H, h - y0), min(W, w - x0)
            vis[:hh, :ww] = obj[y0:y0 + hh, x0:x0 + ww]
            if vis.sum() < 12:
                continue
            ys, xs = np.flatnonzero(vis.any(1)), np.flatnonzero(vis.any(0))
            det[t, row] = (ys[0] / H, xs[0] / W, (ys[-1] + 1) / H, (xs[-1] + 1) / W, cid, 0.9 - 0.01 * k - 0.001 * t)
            masks[t, row] = 0.9 * vis.reshape(H // m, m, W // m, m).mean(axis=(1, 3)) + 0.05
            keep[t, row] = 1
            row += 1
    return Scene(image_hw, (H, W), tiles, objects, det, keep, masks)


def iou(a, b) -> float:
    return float((a & b).sum()) / float((a | b).sum())


def full_mask(res, g, image_hw):
    out = np.zeros(image_hw, bool)
    y1, x1, y2, x2 = res.boxes[g]
    out[y1:y2, x1:x2] = res.masks[g]
    return out

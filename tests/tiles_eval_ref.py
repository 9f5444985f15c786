"""Tiled evaluation (MAP.collect_tiled, disyolo_tile_group_counts), restated in numpy for the tests.

Like tiles_ref.py this file IS the definition: the reference project letter-boxes every image and has no tiled metric.  It is
composed from what the tests already trust -- tiles_ref.merge_tiles / full_mask and voc_eval (pinned by
tests/golden/voc_eval.json) -- and plain boolean numpy:

  group_counts   per pair (g, j): |mask_g n gt_j| over full-size boolean masks, j = -1: |mask_g|; mask_g is read out of the
                 compose arena the way disyolo_tile_compose lays it out (bytes != 0, row-major over the box, at 16 * off16)
  pack_gt        the bit-plane layout of the ground truth, written pixel by pixel; unpack_gt is its inverse
  collect_tiled  the detfile entries of one image: every merged group is a detection, classes ascending, groups in rank order
                 within a class; with ``ov`` the IoU rows compute_overlaps_masks gives (f32), otherwise the full-size masks
  ap_table       voc_eval per class -> [(recall, precision, ap)]

Every quantity is an integer, a bit, or an f32 quotient of two integers below 2^24: the tests compare with equality."""
import numpy as np

import tiles_ref as TR
from disyolo_amd.voc_eval import compute_overlaps_masks, voc_eval


def group_mask(groups, arena, g: int, image_hw) -> np.ndarray:
    """bool [h,w]: group g's mask out of the arena"""
    y1, x1, y2, x2 = (int(v) for v in groups[g][2:6])
    n = (y2 - y1) * (x2 - x1)
    off = int(groups[g][7]) * 16
    out = np.zeros(image_hw, bool)
    out[y1:y2, x1:x2] = np.asarray(arena[off:off + n]).reshape(y2 - y1, x2 - x1) != 0
    return out


def group_counts(groups, arena, gt_masks, pairs) -> np.ndarray:
    """int64 [P]: per pair (g, j) the pixels of group g that lie in ground-truth mask j (bool [h,w]); j = -1: all of them"""
    image_hw = gt_masks[0].shape if len(gt_masks) else (max([int(g[4]) for g in groups] + [1]), max([int(g[5]) for g in groups] + [1]))
    out = np.zeros(len(pairs), np.int64)
    for p, (g, j) in enumerate(pairs):
        m = group_mask(groups, arena, int(g), image_hw)
        out[p] = int(m.sum()) if j < 0 else int((m & np.asarray(gt_masks[j], bool)).sum())
    return out


def pack_gt(masks):
    """bool masks [h,w] -> (gt int32 [ng,8] = y1, x1, y2, x2, 0, pitch, off, area; words uint32): bit i of word off + r * pitch
    + k is pixel (y1 + r, x1 + 32 k + i) of the instance's tight box; an empty mask has the box (0, 0, 0, 0)"""
    gt = np.zeros((len(masks), 8), np.int32)
    words = []
    for j, m in enumerate(masks):
        m = np.asarray(m, bool)
        ys, xs = np.nonzero(m)
        gt[j, 6] = len(words)
        if ys.size == 0:
            continue
        y1, x1, y2, x2 = ys.min(), xs.min(), ys.max() + 1, xs.max() + 1
        pitch = (x2 - x1 + 31) // 32
        plane = [0] * ((y2 - y1) * pitch)
        for y, x in zip(ys.tolist(), xs.tolist()):
            plane[(y - y1) * pitch + (x - x1) // 32] |= 1 << ((x - x1) % 32)
        gt[j, :4], gt[j, 5], gt[j, 7] = (y1, x1, y2, x2), pitch, ys.size
        words += plane
    return gt, np.array(words, np.uint32)


def unpack_gt(gt, words, image_hw):
    """the inverse of pack_gt: [bool [h,w]]"""
    out = []
    for y1, x1, y2, x2, _, pitch, off, _ in np.asarray(gt).tolist():
        m = np.zeros(image_hw, bool)
        for y in range(y1, y2):
            for x in range(x1, x2):
                m[y, x] = (int(words[off + (y - y1) * pitch + (x - x1) // 32]) >> ((x - x1) % 32)) & 1
        out.append(m)
    return out


def records(objects, imageid="scene"):
    """[(classid, bool [h,w])] -> the recs_mask list of one image (nothing is difficult)"""
    return [{"imageid": imageid, "classid": int(c), "difficult": 0, "mask": np.asarray(m, bool)} for c, m in objects]


def class_map(objects, image_hw) -> np.ndarray:
    """uint8 [h,w]: classid + 1, painted in object order"""
    out = np.zeros(image_hw, np.uint8)
    for c, m in objects:
        out[np.asarray(m, bool)] = c + 1
    return out


def collect_tiled(res, recs, imageid, image_hw, classids, ov=False):
    """res: a tiles_ref.Merged (or anything with boxes, classid, score, masks); recs: image id -> records -> the detfile
    {str(classid): [entries]} of this image"""
    detfile = {str(c): [] for c in classids}
    for c in sorted({int(v) for v in res.classid}):
        objs = [o for o in recs[imageid] if o["classid"] == c]
        for g in np.flatnonzero(np.asarray(res.classid) == c):
            full = TR.full_mask(res, int(g), image_hw)
            entry = {"imageid": imageid, "score": float(res.score[g])}
            if not ov:
                entry["mask"] = full
            elif not objs:
                entry["ov"] = np.zeros(0, np.float32)
            else:
                stack = np.stack([np.asarray(o["mask"]) for o in objs], axis=-1).astype(float)
                entry["ov"] = compute_overlaps_masks(full.astype(float)[..., None], stack)[0].astype(np.float32)
            detfile[str(c)].append(entry)
    return detfile


def extend(detfile, more):
    for k, v in more.items():
        detfile[k] += v
    return detfile


def ap_table(detfile, recs, index, classids):
    """[(recall, precision, ap)] per class; (0, 0, 0) for a class without detections, like MAP._ap_table"""
    return [tuple(float(v) for v in voc_eval(detfile[str(c)], recs, index, c, ovthresh=0.5, use_07_metric=False))
            if detfile[str(c)] else (0.0, 0.0, 0.0) for c in classids]


def confusion(true_map, pred_map, nlabel: int) -> np.ndarray:
    """int64 [nlabel * nlabel]: conf[true * nlabel + pred]"""
    conf = np.zeros(nlabel * nlabel, np.int64)
    np.add.at(conf, np.asarray(true_map, np.int64).reshape(-1) * nlabel + np.asarray(pred_map, np.int64).reshape(-1), 1)
    return conf


def mask_acc(conf, nlabel: int):
    """SegmentationAccuracy.result's arithmetic"""
    c = np.asarray(conf).reshape(nlabel, nlabel).astype(np.float64)
    with np.errstate(invalid="ignore"):                  # a label in neither map: 0 / 0, as in SegmentationAccuracy
        ious = [c[k, k] / (c[k, :].sum() + c[:, k].sum() - c[k, k]) for k in range(nlabel)]
    return ious + [float(np.mean(ious))]

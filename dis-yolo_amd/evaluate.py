"""Test / validation driver: the counterpart of ``calculate_test_map.py`` (``image_read`` :149-176,
``evaluate`` :180-347, class ``MAP``) and of ``utils/validation_map.py`` (``MAP.do_python_eval``
:104-198), on top of ``YOLONet.evaluation``.

Same flow as the reference -- letter box -> ``sess.run(net.evaluation)`` -> un-letterbox boxes, crop /
resize / threshold / paste masks -> per-class mask AP at IoU 0.5 (``voc_eval``) -> 4x4 pixel confusion ->
mIoU -- with the pixel work on the GPU (``disyolo_letterbox``, ``disyolo_mask_paste``,
``disyolo_confusion16``) instead of cv2 on the host.  Image files are decoded with PIL (host).
"""
from __future__ import annotations

import os
import time
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import config as cfg
from . import lib as L
from .postprocess import SegmentationAccuracy, correct_yolo_boxes, paste_detections, paste_rects
from .voc_eval import voc_eval


def image_read(image_rgb, image_size, device=None, out: Optional[torch.Tensor] = None):
    """calculate_test_map.py:149-176: RGB uint8 [H,W,3] (numpy or CUDA tensor) -> (letter-boxed image f32
    CUDA [net_h,net_w,3] in [0,1], clip window f32 [4] = top, left, bottom, right).  ``image_size``: the net's size, an int
    or (net_h, net_w)."""
    if not torch.is_tensor(image_rgb):
        image_rgb = torch.from_numpy(np.ascontiguousarray(image_rgb))
    if device is None:
        device = image_rgb.device if image_rgb.is_cuda else torch.device("cuda", torch.cuda.current_device())
    rgb = image_rgb.to(device, torch.uint8).contiguous()
    if out is None:
        out = torch.empty(*L.hw_of(image_size), 3, dtype=torch.float32, device=device)
    window = L.letterbox(rgb, out, image_size)
    return out, window


def load_image_rgb(path: str) -> np.ndarray:
    """cv2.cvtColor(cv2.imread(path), COLOR_BGR2RGB) (calculate_test_map.py:208) via PIL"""
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert("RGB"))


def gt_bit_planes(masks) -> Tuple[np.ndarray, np.ndarray]:
    """ground-truth masks [h,w] (> 0.5 is set) -> (gt int32 [ng,8] = y1, x1, y2, x2, 0, pitch, off, area; words uint32): each
    instance as a bit plane cropped to its tight box, pitch = ceil((x2 - x1) / 32) words per row from word ``off``; bit i of
    word k of row r is pixel (y1 + r, x1 + 32 k + i) and the bits past the box's last column are zero (disyolo_tile_group_counts'
    layout).  An instance without pixels has an empty box and area 0.  Column 4 (the class id) is the caller's."""
    gt = np.zeros((len(masks), 8), np.int32)
    words, off = [], 0
    for j, mask in enumerate(masks):
        m = np.asarray(mask).astype(float) > 0.5
        ys, xs = np.flatnonzero(m.any(1)), np.flatnonzero(m.any(0))
        if ys.size == 0:
            gt[j, 6] = off
            continue
        y1, x1, y2, x2 = int(ys[0]), int(xs[0]), int(ys[-1]) + 1, int(xs[-1]) + 1
        pitch = -(-(x2 - x1) // 32)
        rows = np.zeros((y2 - y1, pitch * 32), bool)
        rows[:, :x2 - x1] = m[y1:y2, x1:x2]
        words.append(np.packbits(rows, axis=1, bitorder="little").view("<u4").reshape(-1))
        gt[j] = (y1, x1, y2, x2, 0, pitch, off, int(rows.sum()))
        off += (y2 - y1) * pitch
    if off >= 1 << 31:
        raise ValueError("gt_bit_planes: the instances' boxes hold too many words for int32 offsets")
    return gt, (np.concatenate(words) if words else np.zeros(0, "<u4")).astype(np.uint32)


class MAP(object):
    """Ground truth + metric, like the reference's two ``MAP`` classes.  ``groundtruth`` =
    [recs_mask, recs_mergemask or recs_size, ..., index] is passed in (the reference builds it from its
    pickle cache with skimage; ``train_data.rasterize_polygons`` is the counterpart here):
      recs_mask: image id -> [{'imageid', 'classid', 'difficult', 'mask' bool [H,W]}]
      sizes:     image id -> [image_h, image_w]
      merged:    image id -> uint8 [H,W] class map (0 background, classid + 1), for mIoU; optional
      index:     list of image ids in evaluation order.
    ``net_size``: the size of the net whose detections are collected, an int or (H, W)."""

    def __init__(self, recs_mask: Dict[str, List[Dict]], sizes: Dict[str, Sequence[int]], index: Sequence[str],
                 merged: Optional[Dict[str, np.ndarray]] = None, net_size=cfg.TEST_SIZE,
                 classes: Optional[Sequence[str]] = None):
        from .net import check_classes
        self.classes = check_classes(cfg.CLASSES if classes is None else classes)
        self.num_class = len(self.classes)
        self.classid = list(range(self.num_class))
        self.class_to_ind = dict(zip(self.classes, range(self.num_class)))
        self.recs_mask, self.sizes, self.index, self.merged = recs_mask, sizes, list(index), merged
        self.net_size = net_size
        self.groundtruth = [recs_mask, merged, sizes, self.index]
        self._gt_cache = {}

    @staticmethod
    def correct_yolo_boxes(x1, y1, x2, y2, image_h, image_w, net_h, net_w):
        """calculate_test_map.py:121-138 (one box; returns x1, y1, x2, y2 integer pixel corners)"""
        b = correct_yolo_boxes(np.array([[y1, x1, y2, x2]], np.float32), image_h, image_w, net_h, net_w)[0]
        return int(b[0]), int(b[1]), int(b[2]), int(b[3])

    def _ap_table(self, detfile: Dict[str, List[Dict]], thresh: float = 0.5):
        """calculate_test_map.py:275-299 / validation_map.py:170-197"""
        res, pres, aps = [], [], []
        for clsid in self.classid:
            if not detfile[str(clsid)]:
                res, pres, aps = res + [0.0], pres + [0.0], aps + [0.0]
                continue
            recall, precision, ap = voc_eval(detfile[str(clsid)], self.recs_mask, self.index, clsid, ovthresh=thresh,
                                             use_07_metric=False)
            res, pres, aps = res + [recall], pres + [precision], aps + [ap]
        return [{"thresh": thresh, "AP": aps, "mAP": [float(np.mean(res)), float(np.mean(pres)), float(np.mean(aps))]}]

    def collect(self, imageid: str, det_box, det_mask, detfile: Dict[str, List[Dict]]) -> torch.Tensor:
        """the per-image body of both reference loops: paste this image's detections, append them to the
        per-class lists, return the merged class map (uint8 CUDA [H,W])"""
        image_h, image_w = self.sizes[imageid]
        entries, merged = paste_detections(det_box, det_mask, image_h, image_w, self.net_size)
        if entries and os.environ.get("DISYOLO_EVAL_GPU_IOU", "1") != "0":
            # round 6: the mask IoUs voc_eval needs (compute_overlaps_masks: every detection against the image's ground-truth
            # instances of its class) are taken HERE, on the GPU, from the pasted masks -- pixel counts as exact integers
            # ([nd, HW] x [HW, ng] in f32: every partial sum is an integer below 2^24), divided on the host in f32 exactly as
            # numpy does; the 0.5-MB-per-detection copies to the host and the numpy pass over them (145 ms per image) are gone
            for c in sorted({e["classid"] for e in entries}):
                dets = [e for e in entries if e["classid"] == c]
                gt = self._gt_stack(imageid, c, merged.device)
                if gt is None:
                    rows = [np.zeros(0, np.float32)] * len(dets)
                else:
                    d = torch.stack([e["mask"] for e in dets]).reshape(len(dets), -1).to(torch.float32)
                    inter = (d @ gt[0]).cpu().numpy()                                    # [nd, ng] f32, exact counts
                    union = d.sum(1).cpu().numpy()[:, None] + gt[1][None, :] - inter
                    rows = list((inter / union).astype(np.float32))
                for e, ov in zip(dets, rows):
                    detfile[str(c)].append({"imageid": imageid, "score": e["score"], "ov": ov})
            return merged
        for e in entries:
            detfile[str(e["classid"])].append({"imageid": imageid, "score": e["score"], "mask": e["mask"].cpu().numpy()})
        return merged

    def _gt_stack(self, imageid: str, classid: int, device):
        """the ground-truth instances of one class of one image, in ``recs_mask`` order (voc_eval's ``objs``): ([HW, ng] f32
        0 / 1 on the GPU, pixel counts [ng] f32 on the host); None without such instances.  Cached: a validation set is
        swept many times."""
        key = (imageid, classid)
        hit = self._gt_cache.get(key)
        if hit is None:
            objs = [o for o in self.recs_mask[imageid] if o["classid"] == classid]
            if not objs:
                hit = (None,)
            else:
                g = torch.from_numpy(np.stack([np.asarray(o["mask"]).astype(float) > 0.5 for o in objs]).reshape(len(objs), -1))
                g = g.to(device).to(torch.float32)
                hit = ((g.t().contiguous(), g.sum(1).cpu().numpy()),)
            self._gt_cache[key] = hit
        return hit[0]

    def _gt_image(self, imageid: str, device):
        """all ground-truth instances of one image for ``collect_batch``: (uint8 [ng,H,W] 0 / 1 stack on the GPU or None, int32
        [ng] class ids on the GPU or None, {classid: (stack rows of that class in ``recs_mask`` order = voc_eval's ``objs``
        order, their pixel counts f32 [ngc] on the host)}).  Cached like ``_gt_stack``."""
        key = ("image", imageid)
        hit = self._gt_cache.get(key)
        if hit is None:
            objs = self.recs_mask[imageid]
            if not objs:
                hit = (None, None, {})
            else:
                g = np.stack([np.asarray(o["mask"]).astype(float) > 0.5 for o in objs])
                cls = np.array([o["classid"] for o in objs], np.int32)
                area = g.reshape(len(objs), -1).sum(1)
                per_class = {int(c): (np.nonzero(cls == c)[0], area[cls == c].astype(np.float32)) for c in np.unique(cls)}
                hit = (torch.from_numpy(g.astype(np.uint8)).to(device), torch.from_numpy(cls).to(device), per_class)
            self._gt_cache[key] = hit
        return hit

    def _true_map(self, imageid: str, true_map, device) -> torch.Tensor:
        """a ground-truth class map on the GPU (uint8 [H,W]); host arrays are uploaded once per image id and cached"""
        if torch.is_tensor(true_map) and true_map.is_cuda:
            return true_map.to(device, torch.uint8).contiguous()
        key = ("true_map", imageid)
        hit = self._gt_cache.get(key)
        if hit is None:
            hit = torch.as_tensor(np.ascontiguousarray(true_map)).to(device, torch.uint8).contiguous()
            self._gt_cache[key] = hit
        return hit

    def _add_confusion(self, true_map: torch.Tensor, merged: torch.Tensor, conf: torch.Tensor) -> None:
        """the confusion counts of one image into ``conf``: int64 [16] for 3 classes, [(C + 1)^2] for any other list"""
        if conf.numel() != (self.num_class + 1) ** 2:
            raise ValueError("conf holds %d counts; a list of %d classes needs %d" %
                             (conf.numel(), self.num_class, (self.num_class + 1) ** 2))
        if tuple(true_map.shape) != tuple(merged.shape):
            raise ValueError("class maps differ in shape: %s vs %s" % (tuple(true_map.shape), tuple(merged.shape)))
        if self.num_class == 3:
            L.confusion16(true_map, merged, conf)
        else:
            L.confusion_n(true_map, merged.contiguous(), conf, self.num_class + 1)

    def collect_batch(self, imageids: Sequence[str], detections: torch.Tensor, keep: torch.Tensor, masks: torch.Tensor,
                      detfile: Dict[str, List[Dict]], true_maps: Optional[Sequence] = None,
                      conf: Optional[torch.Tensor] = None) -> List[torch.Tensor]:
        """``collect`` for a batch, on the device-resident outputs of ``YOLONet.evaluation_device`` / ``infer``: detections
        [B,max_det,6], keep [B,max_det], masks [B,max_det,Hm,Wm]; ``imageids`` names the first len(imageids) <= B images
        (a short last batch leaves the other rows unused).  Per batch: one fetch of detections + keep, the job table on the
        host, one upload (jobs, rects, class ids), ONE launch (disyolo_mask_paste_iou_batch: merged maps, pixel counts,
        intersections and -- with ``true_maps`` (one uint8 [H,W] class map per image) and ``conf`` (int64 [16] on the GPU, e.g.
        ``SegmentationAccuracy.conf``) -- the confusion counts), one fetch of the counts.  Appends to ``detfile`` exactly what
        ``collect`` appends image by image, in its order (per image, classes ascending, detections in row order); returns the
        merged class maps (uint8 CUDA [H,W] each).

        The ``ov`` rows are inter / (area_det + area_gt - inter) in f32 from integer counts converted to f32 -- ``collect``'s
        arithmetic, whose counts are f32 sums; the two agree exactly while an image has fewer than 2^24 pixels (every count is
        then an integer that f32 holds)."""
        nb = len(imageids)
        B, max_det = int(detections.shape[0]), int(detections.shape[1])
        if nb > B:
            raise ValueError("collect_batch: %d image ids for a batch of %d" % (nb, B))
        if nb == 0:
            return []
        dev = masks.device
        if os.environ.get("DISYOLO_EVAL_GPU_IOU", "1") == "0":
            det, kp = detections.cpu().numpy(), keep.cpu().numpy().astype(bool)
            out = []
            for b, imageid in enumerate(imageids):
                if kp[b].any():
                    merged = self.collect(imageid, det[b][kp[b]], masks[b][torch.from_numpy(kp[b]).to(dev)], detfile)
                else:
                    merged = torch.zeros(*self.sizes[imageid], dtype=torch.uint8, device=dev)
                if true_maps is not None and conf is not None:
                    self._add_confusion(self._true_map(imageid, true_maps[b], dev), merged, conf)
                out.append(merged)
            return out
        map_h, map_w = int(masks.shape[-2]), int(masks.shape[-1])
        size = (map_h, map_w)
        masks = masks.contiguous()
        # the paste's own confusion counts are the 4x4 table of 3 classes; any other class list counts after the launch
        fused_conf = self.num_class == 3
        host = torch.cat([detections.reshape(B, -1), keep.reshape(B, -1).to(torch.float32)], 1).cpu().numpy()     # the one fetch
        det = host[:nb, :max_det * 6].reshape(nb, max_det, 6)
        kp = host[:nb, max_det * 6:] != 0
        # ---- the job table, rects and class ids in one host buffer -> one upload
        jobs = np.zeros(nb, L.PASTE_JOB)
        off_rects = (jobs.nbytes + 15) // 16 * 16
        off_cls = off_rects + nb * max_det * 8 * 4
        hbuf = np.zeros(off_cls + nb * max_det * 4, np.uint8)
        rects_all = hbuf[off_rects:off_cls].view(np.int32).reshape(nb, max_det, 8)
        cls_all = hbuf[off_cls:].view(np.int32).reshape(nb, max_det)
        oks, gts, npix, cnt_off = [], [], 0, [0]
        for b, imageid in enumerate(imageids):
            image_h, image_w = self.sizes[imageid]
            rects, ok = paste_rects(det[b], image_h, image_w, self.net_size, size)
            ok &= kp[b]
            rects[~ok] = 0
            rects_all[b], cls_all[b] = rects, det[b][:, 4].astype(np.int32)
            oks.append(ok)
            gts.append(self._gt_image(imageid, dev))
            ng = 0 if gts[b][0] is None else int(gts[b][0].shape[0])
            cnt_off.append(cnt_off[-1] + max_det * (1 + ng))
            npix += int(image_h) * int(image_w)
        dbuf = torch.empty(hbuf.size, dtype=torch.uint8, device=dev)
        counts = torch.zeros(cnt_off[-1], dtype=torch.int32, device=dev)
        merged_all = torch.empty(npix, dtype=torch.uint8, device=dev)
        out, tms, pix0 = [], [], 0
        for b, imageid in enumerate(imageids):
            image_h, image_w = self.sizes[imageid]
            gt, gt_cls, _ = gts[b]
            merged = merged_all[pix0:pix0 + image_h * image_w].view(image_h, image_w)
            pix0 += image_h * image_w
            out.append(merged)
            j = jobs[b]
            j["masks"] = masks.data_ptr() + b * max_det * map_h * map_w * 4
            j["rects"] = dbuf.data_ptr() + off_rects + b * max_det * 32
            j["classids"] = dbuf.data_ptr() + off_cls + b * max_det * 4
            j["gt"], j["gt_class"] = (0, 0) if gt is None else (gt.data_ptr(), gt_cls.data_ptr())
            j["merged"] = merged.data_ptr()
            if true_maps is not None and conf is not None:
                tm = self._true_map(imageid, true_maps[b], dev)
                if tuple(tm.shape) != (image_h, image_w):
                    raise ValueError("class maps differ in shape: %s vs %s" % (tuple(tm.shape), (image_h, image_w)))
                tms.append(tm)                       # (kept alive until the launch has been issued on this stream)
                if fused_conf:
                    j["true_map"] = tm.data_ptr()
            j["counts"] = counts.data_ptr() + cnt_off[b] * 4
            j["n"], j["ng"] = max_det, 0 if gt is None else int(gt.shape[0])
            j["image_h"], j["image_w"] = image_h, image_w
        wide = max_det > 64                                  # more detections than one cover word per pixel holds
        L.paste_job_plan(jobs, wide=wide)
        hbuf[:jobs.nbytes] = jobs.view(np.uint8)
        dbuf.copy_(torch.from_numpy(hbuf))                                                       # the one upload
        L.mask_paste_iou_batch(jobs, dbuf, size, conf if (tms and fused_conf) else None, wide=wide)
        if tms and not fused_conf:
            for tm, merged in zip(tms, out):
                self._add_confusion(tm, merged, conf)
        cnt = counts.cpu().numpy()                                                               # the one fetch of the counts
        for b, imageid in enumerate(imageids):
            ok, per_class = oks[b], gts[b][2]
            c_b = cnt[cnt_off[b]:cnt_off[b + 1]].reshape(max_det, -1)
            cls_b = cls_all[b]
            for c in sorted({int(v) for v in cls_b[ok]}):
                rows = np.nonzero(ok & (cls_b == c))[0]
                if c not in per_class:
                    ovs = [np.zeros(0, np.float32)] * len(rows)
                else:
                    cols, gt_area = per_class[c]
                    inter = c_b[rows][:, 1 + cols].astype(np.float32)                            # [nd, ng] exact counts
                    union = c_b[rows, 0].astype(np.float32)[:, None] + gt_area[None, :] - inter
                    ovs = list((inter / union).astype(np.float32))
                for k, ov in zip(rows, ovs):
                    detfile[str(c)].append({"imageid": imageid, "score": float(det[b][k, 5]), "ov": ov})
        return out

    def _gt_planes(self, imageid: str, device):
        """all ground-truth instances of one image for ``collect_tiled``, as bit planes cropped to their tight boxes
        (``gt_bit_planes``): (gt int32 [ng,8] on the host, its CUDA copy, the words int32 CUDA, {classid: (instance indices of
        that class in ``recs_mask`` order = voc_eval's ``objs`` order, their pixel counts f32 on the host)}).  Cached like
        ``_gt_image``, whose uint8 [ng,H,W] stack is 8 x H x W / box area times larger."""
        key = ("planes", imageid)
        hit = self._gt_cache.get(key)
        if hit is None:
            objs = self.recs_mask[imageid]
            gt, words = gt_bit_planes([o["mask"] for o in objs])
            cls = np.array([o["classid"] for o in objs], np.int32).reshape(-1)
            gt[:, 4] = cls
            per_class = {int(c): (np.nonzero(cls == c)[0], gt[cls == c, 7].astype(np.float32)) for c in np.unique(cls)}
            hit = (gt, torch.from_numpy(gt).to(device), torch.from_numpy(words.view(np.int32)).to(device), per_class)
            self._gt_cache[key] = hit
        return hit

    def collect_tiled(self, imageid: str, res, detfile: Dict[str, List[Dict]], true_map=None,
                      conf: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``collect`` for what ``tiles.detect_tiled`` / ``tiles.merge_tiles`` returned for one whole image (``res``, a
        ``TiledDetections`` in image pixels: ``net_size`` plays no part).  Every merged group is a detection.  Its mask stays
        cropped to its box in the merge's arena and the ground truth stays cropped bit planes (``_gt_planes``): one upload (the
        pair table: per group its own pixel count, and one row per ground-truth instance of its class whose box meets the
        group's), ONE launch (disyolo_tile_group_counts), one fetch of the counts.  Appends to ``detfile`` what ``collect`` would
        append for the groups' full-size masks, in its order (classes ascending, groups in rank order within a class); with
        ``true_map`` (uint8 [h,w]) and ``conf`` adds the image's confusion counts; returns ``res.merged``.

        The ``ov`` rows are inter / (area_group + area_gt - inter) in f32 from integer counts converted to f32 --
        ``collect_batch``'s arithmetic, equal to ``compute_overlaps_masks`` bit for bit while the image has fewer than 2^24
        pixels.  Above that (3000 x 4000 is 1.2e7, 5000 x 4000 is past it) the counts here are still exact integers, where the
        reference's f32 sums of ones stop counting at 2^24: the rows can then differ, and these are the right ones.
        ``DISYOLO_EVAL_GPU_IOU=0`` takes the host path instead (full-size masks to ``voc_eval``), the built-in comparator."""
        image_hw = tuple(int(v) for v in self.sizes[imageid])
        if tuple(res.image_hw) != image_hw:
            raise ValueError("collect_tiled: the result is of a %s image, %r is %s" % (tuple(res.image_hw), imageid, image_hw))
        G = len(res)
        classid = np.asarray(res.classid, np.int64).reshape(-1)
        if G and os.environ.get("DISYOLO_EVAL_GPU_IOU", "1") == "0":
            for c in sorted({int(v) for v in classid}):
                for g in np.nonzero(classid == c)[0]:
                    detfile[str(c)].append({"imageid": imageid, "score": float(res.score[g]),
                                            "mask": res.full_mask(int(g)).cpu().numpy()})
        elif G:
            dev = res.arena.device
            gt, gt_dev, gt_bits, per_class = self._gt_planes(imageid, dev)
            boxes = np.asarray(res.boxes, np.int64).reshape(-1, 4)
            # ---- the pair table in one pass: (g, -1) per group, (g, j) per instance of the group's class whose box meets its box
            meet = ((classid[:, None] == gt[None, :, 4])
                    & (np.minimum(boxes[:, None, 2], gt[None, :, 2]) > np.maximum(boxes[:, None, 0], gt[None, :, 0]))
                    & (np.minimum(boxes[:, None, 3], gt[None, :, 3]) > np.maximum(boxes[:, None, 1], gt[None, :, 1])))
            pg, pj = np.nonzero(meet)
            pairs2 = np.concatenate([np.stack([np.arange(G), np.full(G, -1)], 1), np.stack([pg, pj], 1)])
            pairs, _ = L.tile_group_counts_plan(res.groups, gt, pairs2)
            cnt = L.tile_group_counts(res.groups, res.arena, gt, gt_bits, pairs, image_hw, groups_dev=res.groups_dev,
                                      gt_dev=gt_dev, arena_bytes=res.arena_bytes).cpu().numpy()   # one upload, launch, fetch
            area = cnt[:G].astype(np.float32)
            inter_all = np.zeros((G, gt.shape[0]), np.float32)                                  # a missing pair is inter = 0
            inter_all[pg, pj] = cnt[G:]
            for c in sorted({int(v) for v in classid}):
                rows = np.nonzero(classid == c)[0]
                if c not in per_class:
                    ovs = [np.zeros(0, np.float32)] * len(rows)
                else:
                    cols, gt_area = per_class[c]
                    inter = inter_all[rows][:, cols]                                             # [nd, ng] exact counts
                    union = area[rows][:, None] + gt_area[None, :] - inter
                    with np.errstate(divide="ignore", invalid="ignore"):
                        ovs = list((inter / union).astype(np.float32))
                for g, ov in zip(rows, ovs):
                    detfile[str(c)].append({"imageid": imageid, "score": float(res.score[g]), "ov": ov})
        if true_map is not None and conf is not None:
            self._add_confusion(self._true_map(imageid, true_map, res.merged.device), res.merged, conf)
        return res.merged

    def do_python_eval(self, detdata: List[Dict]):
        """utils/validation_map.py:104-198: detdata = [{'boxes' [n,6], 'masks' [n,S,S] (CUDA tensor or numpy)
        or the scalar 0.0, 'imname'}] in ``index`` order -> [{'thresh', 'AP' [3], 'mAP' [recall, precision, mAP]}]"""
        assert len(detdata) == len(self.index)
        detfile = {str(c): [] for c in self.classid}
        for i, d in enumerate(detdata):
            assert d["imname"] == self.index[i]
            masks = d["masks"]
            if not torch.is_tensor(masks):
                if np.isscalar(masks) or np.ndim(masks) == 0 or np.sum(masks) == 0.0:
                    continue
                masks = torch.from_numpy(np.ascontiguousarray(masks, np.float32)).cuda()
            self.collect(d["imname"], d["boxes"], masks, detfile)
        return self._ap_table(detfile)


def evaluate(net, images: Dict[str, np.ndarray], eval_map: MAP, det_thresh: float = cfg.OBJ_THRESHOLD,
             weights_file: Optional[str] = None, tiled: Optional[Dict] = None):
    """calculate_test_map.py:180-347.  ``images``: image id -> RGB uint8 array (or a path to decode);
    ``net``: a YOLONet built with batch size 1 like the reference's test graph (:354), or with a larger one: B images are then
    letter-boxed into one frame, run as one batch and collected by ``MAP.collect_batch`` (a short last batch runs with the
    stale frames of the one before left in place).  Returns
    (thresh_out, mask_acc, timing) = ([{'thresh', 'AP', 'mAP'}], [bg, crack, spall, rebar, mIoU] or None,
    {'prediction_s', 'crop_assemble_s', 'per_image_s'}).  The class list is ``eval_map``'s (``MAP(classes=...)``, the net's must
    have as many): one AP per class, and mask_acc = background, one IoU per class, their mean.

    ``tiled``: None (the letter-boxed loops above), or a dict {"overlap": 64, "merge_overlap": 0.5} (either key may be left
    out): every image runs whole through ``tiles.detect_tiled`` -- any image size, any batch size and option set of an
    inference net -- and its merged instances are scored in image pixels by ``MAP.collect_tiled``.  ``prediction_s`` is then
    the time in ``detect_tiled``, ``crop_assemble_s`` the time in ``collect_tiled``."""
    if tiled is not None:
        unknown = sorted(set(tiled) - {"overlap", "merge_overlap"})
        if unknown:
            raise ValueError("evaluate: tiled takes the keys 'overlap' and 'merge_overlap' (got %s)" %
                             ", ".join(repr(k) for k in unknown))
        if net.training:
            raise ValueError("evaluate: tiled evaluation takes an inference net (training=False)")
    if weights_file is not None:
        from .checkpoint import restore_net
        restore_net(net, weights_file)                       # saver.restore (:184-185)
    S, B = (net.H, net.W), net.B
    if (not net.training and getattr(net, "_infer_prog", None) is None and os.environ.get("DISYOLO_EVAL_REPLAY", "1") != "0"):
        # an inference net: record forward + detection filter + mask assembly once for this threshold (a hipGraph of one lane);
        # every image is then one replay (YOLONet.evaluation uses the recording when the threshold matches)
        net.build_infer_program(float(det_thresh), graph=True)
    detfile = {str(c): [] for c in eval_map.classid}
    if getattr(net, "num_class", eval_map.num_class) != eval_map.num_class:
        raise ValueError("evaluate: the net has %d classes, the MAP %d" % (net.num_class, eval_map.num_class))
    seg = SegmentationAccuracy(net.device, eval_map.num_class) if eval_map.merged is not None else None
    t_pred = t_crop = 0.0
    if tiled is not None:
        t_pred, t_crop = _evaluate_tiled(net, images, eval_map, det_thresh, detfile, seg, tiled.get("overlap", 64),
                                         tiled.get("merge_overlap", 0.5))
        return _evaluate_result(eval_map, detfile, seg, t_pred, t_crop)
    if B > 1:
        t_pred, t_crop = _evaluate_batches(net, images, eval_map, det_thresh, detfile, seg)
        return _evaluate_result(eval_map, detfile, seg, t_pred, t_crop)
    frame = torch.empty(1, S[0], S[1], 3, dtype=torch.float32, device=net.device)
    for index in eval_map.index:
        src = images[index]
        rgb = load_image_rgb(src) if isinstance(src, str) else np.asarray(src)
        image_h, image_w = rgb.shape[:2]
        assert [image_h, image_w] == list(eval_map.sizes[index])
        _, window = image_read(rgb, S, net.device, out=frame[0])
        torch.cuda.synchronize()
        t = time.time()
        det_box, det_mask = net.evaluation(frame, window[None], [np.float32(det_thresh)], masks_on_device=True)
        torch.cuda.synchronize()
        t_pred += time.time() - t
        t = time.time()
        if torch.is_tensor(det_mask[0]):
            merged = eval_map.collect(index, det_box[0], det_mask[0], detfile)
        else:                                                # np.sum(det_mask[0]) == 0.0 (:221-224)
            merged = torch.zeros(image_h, image_w, dtype=torch.uint8, device=net.device)
        if seg is not None:
            seg.add(eval_map.merged[index], merged)
        torch.cuda.synchronize()
        t_crop += time.time() - t
    return _evaluate_result(eval_map, detfile, seg, t_pred, t_crop)


def _evaluate_result(eval_map: MAP, detfile, seg, t_pred: float, t_crop: float):
    thresh_out = eval_map._ap_table(detfile)
    mask_acc = seg.result() if seg is not None else None
    n = max(len(eval_map.index), 1)
    return thresh_out, mask_acc, {"prediction_s": t_pred, "crop_assemble_s": t_crop, "per_image_s": (t_pred + t_crop) / n}


def _evaluate_batches(net, images, eval_map: MAP, det_thresh: float, detfile, seg) -> Tuple[float, float]:
    """evaluate()'s loop for a net of batch size B > 1: B letter boxes into one frame, one pass of the net, one
    ``MAP.collect_batch``; the last batch may hold fewer images -- the frames (and clip windows) of the batch before stay in the
    unused rows, and only the real images get a job.  Returns (prediction seconds, crop + assemble seconds)."""
    S, B = (net.H, net.W), net.B
    t_pred = t_crop = 0.0
    frame = torch.zeros(B, S[0], S[1], 3, dtype=torch.float32, device=net.device)
    windows = np.tile(np.array([0.0, 0.0, 1.0, 1.0], np.float32), (B, 1))
    for a in range(0, len(eval_map.index), B):
        ids = eval_map.index[a:a + B]
        for i, index in enumerate(ids):
            src = images[index]
            rgb = load_image_rgb(src) if isinstance(src, str) else np.asarray(src)
            assert list(rgb.shape[:2]) == list(eval_map.sizes[index])
            _, windows[i] = image_read(rgb, S, net.device, out=frame[i])
        torch.cuda.synchronize()
        t = time.time()
        dets, keep, masks = net.evaluation_device(frame, windows, [np.float32(det_thresh)])
        torch.cuda.synchronize()
        t_pred += time.time() - t
        t = time.time()
        eval_map.collect_batch(ids, dets, keep, masks, detfile,
                               true_maps=[eval_map.merged[i] for i in ids] if seg is not None else None,
                               conf=seg.conf if seg is not None else None)
        torch.cuda.synchronize()
        t_crop += time.time() - t
    return t_pred, t_crop


def _evaluate_tiled(net, images, eval_map: MAP, det_thresh: float, detfile, seg, overlap, merge_overlap) -> Tuple[float, float]:
    """evaluate()'s loop over whole images: ``tiles.detect_tiled`` (the tiles run as batches of the net's size), then
    ``MAP.collect_tiled``.  Returns (seconds in detect_tiled, seconds in collect_tiled)."""
    from .tiles import detect_tiled
    t_pred = t_crop = 0.0
    for index in eval_map.index:
        src = images[index]
        rgb = load_image_rgb(src) if isinstance(src, str) else np.asarray(src)
        assert list(rgb.shape[:2]) == list(eval_map.sizes[index])
        rgb = torch.from_numpy(np.ascontiguousarray(rgb)).to(net.device)
        torch.cuda.synchronize()
        t = time.time()
        res = detect_tiled(net, rgb, overlap, det_thresh, merge_overlap)
        torch.cuda.synchronize()
        t_pred += time.time() - t
        t = time.time()
        eval_map.collect_tiled(index, res, detfile, true_map=eval_map.merged[index] if seg is not None else None,
                               conf=seg.conf if seg is not None else None)
        torch.cuda.synchronize()
        t_crop += time.time() - t
    return t_pred, t_crop

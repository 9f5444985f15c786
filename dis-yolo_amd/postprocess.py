"""Caller side of ``YOLONet.evaluation``: the per-image post-processing of the reference's
``evaluate`` loop (calculate_test_map.py:203-269) -- letter-box window, box un-letterboxing, mask
crop / bilinear resize / threshold / paste -- with the pixel work on the GPU (disyolo_mask_paste).
The reference does it on the host with cv2 at ~0.1 s per image; at thousands of images per second
it has to sit next to the network.  SURVEY.md 8(f3)."""
from __future__ import annotations

from typing import Dict, List, Tuple

import numpy as np
import torch

from . import lib as L


def letterbox_window(image_h: int, image_w: int, size) -> np.ndarray:
    """``image_read``'s clip window (calculate_test_map.py:151-169): [top, left, bottom, right], normalised by
    (net_h, net_w), of the aspect-preserving resize centred in the letter box of a net of ``size`` (an int, or
    (net_h, net_w)); the width binds when net_w / image_w < net_h / image_h."""
    net_h, net_w = L.hw_of(size)
    imgh, imgw = image_h, image_w
    if (float(net_w) / imgw) < (float(net_h) / imgh):
        imgh = (imgh * net_w) // imgw
        imgw = net_w
    else:
        imgw = (imgw * net_h) // imgh
        imgh = net_h
    top, left = (net_h - imgh) // 2, (net_w - imgw) // 2
    return np.array([top / net_h, left / net_w, (imgh + top) / net_h, (imgw + left) / net_w], np.float32)


def correct_yolo_boxes(boxes_yxyx: np.ndarray, image_h: int, image_w: int, net_h: int, net_w: int) -> np.ndarray:
    """calculate_test_map.py:121-138 for an [n,4] array of normalised (y1,x1,y2,x2) boxes: integer
    (x1,y1,x2,y2) pixel corners in the original image (half-to-even rounding, clamped)."""
    b = np.asarray(boxes_yxyx, np.float32).reshape(-1, 4)
    if (float(net_w) / image_w) < (float(net_h) / image_h):
        new_w, new_h = net_w, (image_h * net_w) // image_w
    else:
        new_h, new_w = net_h, (image_w * net_h) // image_h
    x_off, x_scale = float((net_w - new_w) // 2) / net_w, float(new_w) / net_w
    y_off, y_scale = float((net_h - new_h) // 2) / net_h, float(new_h) / net_h

    def corner(v, off, scale, n):
        return np.clip(np.around((v - off) / scale * n).astype(np.int32), 0, n)
    return np.stack([corner(b[:, 1], x_off, x_scale, image_w), corner(b[:, 0], y_off, y_scale, image_h),
                     corner(b[:, 3], x_off, x_scale, image_w), corner(b[:, 2], y_off, y_scale, image_h)], axis=1)


def paste_rects(box: np.ndarray, image_h: int, image_w: int, net_size, map_size) -> Tuple[np.ndarray, np.ndarray]:
    """The rect arithmetic of the paste (calculate_test_map.py:244-251) for an [n,6] detection array (normalised y1,x1,y2,x2,
    class, score) on an image_h x image_w image, the letter box of a net of ``net_size`` and masks of ``map_size`` (each an int,
    or a (height, width) pair): (rects int32 [n,8] = cy1,cx1,cy2,cx2 on the mask map -- around(y * Hm), around(x * Wm) --,
    y1,x1,y2,x2 in the image -- what disyolo_mask_paste takes --, ok bool [n]); the rows with an empty crop or destination are
    not ``ok`` and have zero rects."""
    box = np.asarray(box, np.float32).reshape(-1, 6)
    net_h, net_w = L.hw_of(net_size)
    map_h, map_w = L.hw_of(map_size)
    dst = correct_yolo_boxes(box[:, :4], image_h, image_w, net_h, net_w)                # x1,y1,x2,y2
    crop = np.around(box[:, :4] * np.asarray([map_h, map_w, map_h, map_w], np.float32)).astype(np.int32)   # y1,x1,y2,x2 on the map
    rects = np.concatenate([crop, dst[:, [1, 0, 3, 2]]], axis=1).astype(np.int32)          # cy1,cx1,cy2,cx2,y1,x1,y2,x2
    ok = ((dst[:, 3] - dst[:, 1]) * (dst[:, 2] - dst[:, 0]) > 0) & (crop[:, 2] > crop[:, 0]) & (crop[:, 3] > crop[:, 1])
    rects[~ok] = 0
    return rects, ok


def paste_detections(det_box, det_mask, image_h: int, image_w: int, net_size,
                     want_full: bool = True) -> Tuple[List[Dict], torch.Tensor]:
    """One image of ``evaluation``'s result -> (entries, merged) like the reference loop body
    (calculate_test_map.py:220-266): ``entries`` = [{index, classid, score, mask (bool CUDA tensor
    [H,W])}] for the detections with a non-empty box, ``merged`` = uint8 CUDA tensor [H,W] with
    class id + 1.  ``det_box`` [n,6] (numpy or tensor), ``det_mask`` CUDA f32 [n,Hm,Wm] or the
    scalar 0.0 the reference returns for an image without detections; ``net_size``: the net's size, an int or (H, W)."""
    dev = det_mask.device if torch.is_tensor(det_mask) else torch.device("cuda", torch.cuda.current_device())
    merged = torch.zeros(image_h, image_w, dtype=torch.uint8, device=dev)
    box = det_box.detach().cpu().numpy() if torch.is_tensor(det_box) else np.asarray(det_box)
    if not torch.is_tensor(det_mask) or box.size == 0:
        return [], merged
    box = box.reshape(-1, 6).astype(np.float32)
    n, size = box.shape[0], (int(det_mask.shape[-2]), int(det_mask.shape[-1]))
    rects, ok = paste_rects(box, image_h, image_w, net_size, size)
    rects_d = torch.from_numpy(rects).to(dev)
    cls_d = torch.from_numpy(box[:, 4].astype(np.int32)).to(dev)
    full = torch.empty(n, image_h, image_w, dtype=torch.uint8, device=dev) if want_full else None
    L.mask_paste(det_mask.contiguous(), rects_d, cls_d, image_h, image_w, full, merged)
    entries = []
    for k in range(n):
        if ok[k]:
            entries.append({"index": k, "classid": int(box[k, 4]), "score": float(box[k, 5]),
                            "mask": full[k].bool() if want_full else None})
    return entries, merged


class SegmentationAccuracy:
    """the mIoU block of ``evaluate`` (calculate_test_map.py:303-346): accumulate the pixel confusion
    counts of (ground-truth class map, merged detection map) pairs on the GPU, image by image."""

    def __init__(self, device, num_class: int = 3):
        # background + num_class labels; 3 classes keep the 4x4 table the batched paste fills in its own pass
        if not 1 <= int(num_class) <= 80:
            raise ValueError("num_class must be in 1..80 (got %r)" % (num_class,))
        self.num_class = int(num_class)
        self.nlabel = self.num_class + 1
        self.conf = torch.zeros(self.nlabel * self.nlabel, dtype=torch.int64, device=device)

    def add(self, true_map, pred_map: torch.Tensor) -> None:
        t = torch.as_tensor(true_map).to(self.conf.device, torch.uint8).contiguous()
        p = pred_map.to(self.conf.device, torch.uint8).contiguous()
        if t.shape != p.shape:
            raise ValueError("class maps differ in shape: %s vs %s" % (tuple(t.shape), tuple(p.shape)))
        if self.num_class == 3:
            L.confusion16(t, p, self.conf)
        else:
            L.confusion_n(t, p, self.conf, self.nlabel)

    def result(self) -> List[float]:
        """[bg_iou, crack_iou, spall_iou, rebar_iou, miou]; with another class list: background, one IoU per class, the mean"""
        n = self.nlabel
        c = self.conf.cpu().numpy().reshape(n, n).astype(np.float64)
        ious = [c[k, k] / (c[k, :].sum() + c[:, k].sum() - c[k, k]) for k in range(n)]
        return ious + [float(np.mean(ious))]

"""Rectangular nets (image_size = (H, W)), restated on top of the oracle for the tests.

The oracle's decode, detection filter, YOLO loss and network (O.interpret_output, O.filter_detections, O.loss_yolo,
O.build_network, MR.build_network) already keep net_h / net_w and grid_h / grid_w apart, as the reference's text does
(yolo/yolo3_net_pos.py:473-506, :646, :709-718).  What the oracle restates for a square only -- because the reference
multiplies all four normalised coordinates of a box by the one ``size = shape(pred_masks)[1]`` (:772, :842, :873, :876) or
is written with one ``image_size`` -- is restated here with the two sides apart, composed from the oracle's primitives
(kmask_edges, select_mask_rois, sigmoid_ce, correct_yolo_boxes, resize_linear):

  mask branch   y-coordinates x Hm, x-coordinates x Wm, each through np.round (half to even); bin edges from O.kmask_edges per
                axis; ground truth sampled at [::m, ::m]; area = pixel count; 0.5 outside the box
  loader        net_h = H, net_w = W; boxes and grid rows normalised x, w by net_w and y, h by net_h; same RNG draws
  letter box    width binds when net_w / imgw < net_h / imgh; pad 127; window normalised by (net_h, net_w)
  paste         crop = around(y * Hm), around(x * Wm); destination from O.correct_yolo_boxes(..., net_h, net_w)

At H = W every function returns exactly what the oracle's square function returns (tests/test_rect.py)."""
from typing import Sequence

import numpy as np
import torch

import disyolo_oracle as O
import mask_stride_ref as MR


def hw(size):
    if isinstance(size, (int, np.integer)):
        return int(size), int(size)
    h, w = size
    return int(h), int(w)


# ------------------------------------------------------------------------------------------------ mask branch
def round_box(box_norm: np.ndarray, Hm: int, Wm: int) -> np.ndarray:
    """normalised (y1, x1, y2, x2) rows -> map pixels: y x Hm, x x Wm, f32 products, np.round = half to even"""
    b = np.asarray(box_norm, np.float32)
    return np.round(b * np.asarray([Hm, Wm, Hm, Wm], np.float32))


def channel_index_map(box_px: Sequence[float], Hm: int, Wm: int, k: int) -> np.ndarray:
    """int32 [Hm, Wm]: by * k + bx inside bin (by, bx) of the box, -1 elsewhere; edges from O.kmask_edges per axis"""
    gy = O.kmask_edges(box_px[0], box_px[2], k)
    gx = O.kmask_edges(box_px[1], box_px[3], k)
    m = -np.ones((Hm, Wm), dtype=np.int32)
    for by in range(k):
        for bx in range(k):
            y1, y2, x1, x2 = gy[by], gy[by + 1], gx[bx], gx[bx + 1]
            if y2 > y1 and x2 > x1:
                m[max(y1, 0):min(y2, Hm), max(x1, 0):min(x2, Wm)] = by * k + bx
    return m


def assemble_logits(score_maps: torch.Tensor, box_px: Sequence[float], k: int):
    """(logits [Hm, Wm] -- 0 outside the box --, mask_object [Hm, Wm] in {0, 1}) of one box on score maps [Hm, Wm, k*k]"""
    Hm, Wm = score_maps.shape[0], score_maps.shape[1]
    idx = torch.from_numpy(channel_index_map(box_px, Hm, Wm, k)).long()
    inside = idx >= 0
    logits = torch.gather(score_maps, 2, idx.clamp(min=0).unsqueeze(-1)).squeeze(-1)
    logits = torch.where(inside, logits, torch.zeros_like(logits))
    return logits, inside.to(score_maps.dtype)


def loss_mask(detections, mask_pos, true_boxes, true_masks, perms, k: int):
    """the mask term on score maps [B, Hm, Wm, k*k]; true_masks [B, G, m Hm, m Wm] sampled at [::m, ::m]"""
    B, Hm, Wm = mask_pos.shape[0], mask_pos.shape[1], mask_pos.shape[2]
    step = true_masks.shape[2] // Hm
    assert true_masks.shape[2] == step * Hm and true_masks.shape[3] == step * Wm
    total = torch.zeros((), dtype=mask_pos.dtype)
    for i in range(B):
        pd, pg = perms[i] if perms is not None else (None, None)
        pos, assign, gt_rows = O.select_mask_rois(detections[i], true_boxes[i, 0, 0, 0], pd, pg)
        if len(pos) == 0:
            continue
        gt_small = true_masks[i][gt_rows][:, ::step, ::step].astype(np.float32)
        px = round_box(pos, Hm, Wm)
        per_roi = []
        for r in range(len(px)):
            logits, mobj = assemble_logits(mask_pos[i], px[r], k)
            gtm = torch.from_numpy(gt_small[assign[r]]).to(mask_pos.dtype)
            per_roi.append((mobj * O.sigmoid_ce(gtm, logits)).sum() / mobj.sum())
        total = total + O.MASK_SCALE * torch.stack(per_roi).mean()
    return total / B


def val_test(detections: np.ndarray, mask_pos: torch.Tensor, k: int):
    """(det_box list of [n, 6], det_mask list of [n, Hm, Wm] f32 or scalar 0.0): sigmoid of the selected channel inside the
    box, sigmoid(0) = 0.5 outside; rows kept where the rounded box has positive height and width"""
    det_box, det_mask = [], []
    B, Hm, Wm = mask_pos.shape[0], mask_pos.shape[1], mask_pos.shape[2]
    for i in range(B):
        prop = detections[i].astype(np.float32)
        pb = round_box(prop[:, :4], Hm, Wm)
        keep = np.where(((pb[:, 2] - pb[:, 0]) > 0) & ((pb[:, 3] - pb[:, 1]) > 0))[0]
        prop, pb = prop[keep], pb[keep]
        if prop.size > 0:
            masks = [torch.sigmoid(assemble_logits(mask_pos[i], pb[r], k)[0]) for r in range(len(pb))]
            det_mask.append(torch.stack(masks).float().numpy())
        else:
            det_mask.append(np.float32(0.0))
        det_box.append(prop)
    return det_box, det_mask


def total_loss(params, batch, lock, mask_stride: int, k: int, perms=None, updates=None, obj_thresh=O.OBJ_THRESHOLD,
               quant=None, taps=None, force=None):
    """MR.total_loss with the rectangular mask term; everything else is the oracle's own code, which reads the two sides
    off the tensors"""
    yolos, mask_pos = MR.build_network(params, batch["images"], True, lock, mask_stride, k, updates, taps, quant, force)
    pred = O.interpret_output(yolos)
    with torch.no_grad():
        det = O.filter_detections(pred[2], pred[3], pred[5], batch["clip_window"], obj_thresh)
    ly = O.loss_yolo(pred, batch["true_boxes"], [batch["yolo3"], batch["yolo2"], batch["yolo1"]])
    lm = loss_mask(det, mask_pos, batch["true_boxes"].detach().numpy(), batch["true_masks"], perms, k)
    reg = None
    for n in MR.regularized_names(params, lock):
        t = O.L2_WEIGHT * 0.5 * (params[n] ** 2).sum()
        reg = t if reg is None else reg + t
    parts = dict(ly)
    parts["mask"] = lm
    parts["reg"] = reg
    parts["total"] = ly["conf"] + ly["class"] + ly["coord"] + lm + reg
    return parts, det, yolos, mask_pos


# ------------------------------------------------------------------------------------------------ synthetic batch
def assign_targets(boxes_px: np.ndarray, cls: np.ndarray, H: int, W: int, anchors=O.ANCHORS, num_class=3):
    """O.assign_targets with x_ind = int(xc * grid_w / net_w), y_ind = int(yc * grid_h / net_h)
    (utils/train_data.py:170-173)"""
    yolos = [np.zeros((H // d, W // d, 3, 5 + num_class), np.float32) for d in (8, 16, 32)]
    amax = np.asarray(anchors, np.float32) / 2.0
    a_area = amax[:, 0] * amax[:, 1] * 4
    for b, c in zip(boxes_px, cls):
        half = np.asarray(b[2:4], np.float32) / 2.0
        imax = np.minimum(half[None, :], amax)
        inter = np.maximum(2 * imax, 0.0)
        ia = inter[:, 0] * inter[:, 1]
        iou = ia / (half[0] * half[1] * 4 + a_area - ia)
        if iou.max() <= 0:
            continue
        idx = int(np.argmax(iou))
        y = yolos[idx // 3]
        xi = int(b[0] * y.shape[1] / W)
        yi = int(b[1] * y.shape[0] / H)
        if y[yi, xi, idx % 3, 4] == 1:
            continue
        y[yi, xi, idx % 3, 0:4] = b[:4]
        y[yi, xi, idx % 3, 4] = 1
        y[yi, xi, idx % 3, 5 + int(c)] = 1.0
    return yolos


def synthetic_batch(B: int, H: int, W: int, seed: int = 1234, dtype=torch.float32, num_class: int = 3):
    """O.synthetic_batch on an H x W net: the same RNG draws in the same order, x and w scaled by W, y and h by H"""
    rng = np.random.RandomState(seed)
    norm = np.asarray([W, H, W, H], np.float32)
    images = rng.rand(B, H, W, 3).astype(np.float32)
    true_boxes = np.zeros((B, 1, 1, 1, O.MAX_BOX_PER_IMAGE, 5), np.float32)
    true_masks = np.zeros((B, O.MAX_BOX_PER_IMAGE, H, W), bool)
    ys = [np.zeros((B, H // d, W // d, 3, 5 + num_class), np.float32) for d in (8, 16, 32)]
    yy, xx = np.mgrid[0:H, 0:W]
    for b in range(B):
        n = rng.randint(1, 6)
        bx, cl = [], []
        for j in range(n):
            w = rng.uniform(0.05, 0.6) * W
            h = rng.uniform(0.05, 0.6) * H
            cx = rng.uniform(w / 2, W - w / 2)
            cy = rng.uniform(h / 2, H - h / 2)
            m = ((xx - cx) / (w / 2)) ** 2 + ((yy - cy) / (h / 2)) ** 2 <= 1.0
            if not m.any():
                continue
            rows, cols = np.where(m)
            x1, x2, y1_, y2_ = cols.min(), cols.max(), rows.min(), rows.max()
            true_masks[b, j] = m
            c = rng.randint(0, num_class)
            box = [(x1 + x2) / 2.0, (y1_ + y2_) / 2.0, float(x2 - x1), float(y2_ - y1_)]
            if box[2] <= 0 or box[3] <= 0:
                true_masks[b, j] = False
                continue
            true_boxes[b, 0, 0, 0, j, :4] = np.asarray(box, np.float32) / norm
            true_boxes[b, 0, 0, 0, j, 4] = c
            bx.append(box)
            cl.append(c)
        ts = assign_targets(np.asarray(bx, np.float32).reshape(-1, 4), np.asarray(cl), H, W, num_class=num_class)
        for dst, t in zip(ys, ts):
            t[..., 0:4] /= norm
            dst[b] = t
    window = np.tile(np.array([[0.0, 0.0, 1.0, 1.0]], np.float32), (B, 1))
    return {"images": torch.from_numpy(images).to(dtype), "clip_window": window,
            "true_boxes": torch.from_numpy(true_boxes).to(dtype), "true_masks": true_masks,
            "yolo1": torch.from_numpy(ys[2]).to(dtype), "yolo2": torch.from_numpy(ys[1]).to(dtype),
            "yolo3": torch.from_numpy(ys[0]).to(dtype)}


# ------------------------------------------------------------------------------------------------ letter box and paste
def _fit(image_h: int, image_w: int, net_h: int, net_w: int):
    """(new_h, new_w) of calculate_test_map.py:151-160 with the two sides apart: the width binds when
    net_w / imgw < net_h / imgh"""
    if (float(net_w) / image_w) < (float(net_h) / image_h):
        return (image_h * net_w) // image_w, net_w
    return net_h, (image_w * net_h) // image_h


def letterbox_window(image_h: int, image_w: int, net_h: int, net_w: int) -> np.ndarray:
    imgh, imgw = _fit(image_h, image_w, net_h, net_w)
    top, left = (net_h - imgh) // 2, (net_w - imgw) // 2
    return np.array([top / net_h, left / net_w, (imgh + top) / net_h, (imgw + left) / net_w], np.float32)


def image_read(image_rgb: np.ndarray, net_h: int, net_w: int):
    """O.image_read into a net_h x net_w letter box"""
    imgh, imgw = _fit(image_rgb.shape[0], image_rgb.shape[1], net_h, net_w)
    img = image_rgb.astype(np.float32)
    small = np.stack([O.resize_linear(img[:, :, c], imgw, imgh) for c in range(3)], axis=-1)
    canvas = np.ones((net_h, net_w, 3)) * 127.0
    top, left = (net_h - imgh) // 2, (net_w - imgw) // 2
    canvas[top:top + imgh, left:left + imgw, :] = small
    return (canvas / 255.0).astype(np.float32), letterbox_window(image_rgb.shape[0], image_rgb.shape[1], net_h, net_w)


def paste_detections(det_box: np.ndarray, det_mask, image_h: int, image_w: int, net_h: int, net_w: int):
    """O.paste_detections with masks [n, Hm, Wm]: crop = around(y * Hm), around(x * Wm); destination from
    O.correct_yolo_boxes(..., net_h, net_w)"""
    merged = np.zeros((image_h, image_w), np.uint8)
    entries = []
    if np.isscalar(det_mask) or np.sum(det_mask) == 0.0:
        return entries, merged
    for k in range(det_box.shape[0]):
        y1n, x1n, y2n, x2n = (np.float32(v) for v in det_box[k, :4])
        x1, y1, x2, y2 = O.correct_yolo_boxes(x1n, y1n, x2n, y2n, image_h, image_w, net_h, net_w)
        if (y2 - y1) * (x2 - x1) <= 0:
            continue
        Hm, Wm = det_mask[k].shape
        cy1, cy2 = (int(np.around(v * Hm).astype(np.int32)) for v in (y1n, y2n))
        cx1, cx2 = (int(np.around(v * Wm).astype(np.int32)) for v in (x1n, x2n))
        crop = np.asarray(det_mask[k], np.float32)[cy1:cy2, cx1:cx2]
        if crop.size == 0:
            continue
        m = O.resize_linear(crop, x2 - x1, y2 - y1) > 0.5
        full = np.zeros((image_h, image_w), bool)
        full[y1:y2, x1:x2] = m
        cid = int(det_box[k, 4])
        entries.append({"index": k, "classid": cid, "score": float(det_box[k, 5]), "mask": full})
        merged[full] = cid + 1
    return entries, merged


# ------------------------------------------------------------------------------------------------ the rows of the tests
# (B, H, W, C, k, m, lock): the smallest shapes at which each thing can go wrong; shared by tests/test_rect.py (CPU: the
# oracle is finite with a positive RoI at the row's seed) and tests/test_gpu_rect.py
from collections import namedtuple      # noqa: E402

Row = namedtuple("Row", "name B H W C k m lock seed values extras")


def _row(B, H, W, C, k, m, lock, seed, values=True, extras=()):
    return Row("b%d_%dx%d_c%d_k%d_m%d_%s" % (B, H, W, C, k, m, lock), B, H, W, C, k, m, lock, seed, values, tuple(extras))


ROWS = [
    _row(2, 64, 128, 3, 3, 2, "stage1", 11, extras=("anchor", "pair", "fp8")),   # wide; every fused launch of 64^2 can be admitted
    _row(2, 128, 64, 3, 3, 2, "stage2", 11),                                      # tall: a swapped axis shows here or above
    _row(3, 96, 160, 6, 5, 4, "stage1", 11, extras=("map",)),                     # 3 x 5 coarse grid, odd B, wide loss, m = 4
    _row(1, 160, 96, 5, 7, 1, "stage1", 11),                                      # m = 1 on a tall map
    _row(2, 32, 96, 6, 3, 2, "stage1", 11, values=False),                         # 1 x 3 coarse grid: bit identity, detections
]
VALUE_ROWS = [r for r in ROWS if r.values]


def ids(rows):
    return [r.name for r in rows]


def describe(row) -> str:
    return "row %s (B=%d, H=%d, W=%d, %d classes, k_map=%d, mask_stride=%d, lock=%s, batch seed %d)" % (
        row.name, row.B, row.H, row.W, row.C, row.k, row.m, row.lock, row.seed)


def names(n):
    return ["class%02d" % i for i in range(n)]


def lock_of_row(row):
    return MR.default_lock(int(row.lock[-1]), row.m)


def locked_prefix(row) -> int:
    lock, n = lock_of_row(row), 0
    while lock.get(n + 1, False):
        n += 1
    return n


def net_kwargs(row) -> dict:
    """YOLONet(..., **net_kwargs(row)): everything but training / device / seed"""
    return dict(image_size=(row.H, row.W), batch_size=row.B, classes=names(row.C), k_map=row.k, mask_stride=row.m,
                lock=lock_of_row(row))


def trainable_names(row):
    lock = lock_of_row(row)
    if row.m == 2:
        return O.trainable_names(lock)
    return [n for n in MR.variable_shapes(row.m, row.k) if not lock[int(n.split("convolutional")[1].split("/")[0])]
            and not n.split("/")[-1].startswith("moving_")]


def row_batch(row, seed=None):
    """the row's batch with the RoI permutations of the per-option tests (tests/test_gpu_class_list.py::class_batch)"""
    b = synthetic_batch(row.B, row.H, row.W, seed=row.seed if seed is None else seed, num_class=row.C)
    rng = np.random.RandomState(0)
    b["perm_det"] = np.stack([rng.permutation(O.MAX_DETECTION) for _ in range(row.B)]).astype(np.int32)
    b["perm_gt"] = np.stack([rng.permutation(O.MAX_BOX_PER_IMAGE) for _ in range(row.B)]).astype(np.int32)
    return b, [(b["perm_det"][i], b["perm_gt"][i]) for i in range(row.B)]


def oracle_total_loss(row, params, batch, perms, updates=None, taps=None, force=None, quant=O.bf16_ste):
    return total_loss(params, batch, lock_of_row(row), row.m, row.k, perms, updates, obj_thresh=0.1, quant=quant, taps=taps,
                      force=force)


# ------------------------------------------------------------------------------------------------ the loader
def scale_and_crop(im_sized: np.ndarray, new_w: int, new_h: int, dx: int, dy: int, net_h: int, net_w: int, pad_value) -> np.ndarray:
    """O.scale_and_crop into a net_h x net_w frame (utils/train_data.py:452-464 pads to net_w along x and net_h along y)"""
    if dx > 0:
        im_sized = np.pad(im_sized, ((0, 0), (dx, 0), (0, 0)), mode="constant", constant_values=pad_value)
    else:
        im_sized = im_sized[:, -dx:, :]
    if (new_w + dx) < net_w:
        im_sized = np.pad(im_sized, ((0, 0), (0, net_w - (new_w + dx)), (0, 0)), mode="constant", constant_values=pad_value)
    if dy > 0:
        im_sized = np.pad(im_sized, ((dy, 0), (0, 0), (0, 0)), mode="constant", constant_values=pad_value)
    else:
        im_sized = im_sized[-dy:, :, :]
    if (new_h + dy) < net_h:
        im_sized = np.pad(im_sized, ((0, net_h - (new_h + dy)), (0, 0), (0, 0)), mode="constant", constant_values=pad_value)
    return im_sized[:net_h, :net_w, :]


def place_image(image_u8, net_h: int, net_w: int, new_w: int, new_h: int, dx: int, dy: int, flip: int) -> np.ndarray:
    return np.ascontiguousarray(O._flip(scale_and_crop(O.resize_linear_u8(image_u8, new_w, new_h), new_w, new_h, dx, dy,
                                                       net_h, net_w, 127), flip))


def place_mask(mask, net_h: int, net_w: int, new_w: int, new_h: int, dx: int, dy: int, flip: int) -> np.ndarray:
    m = O.resize_linear(np.asarray(mask, np.float32), new_w, new_h)[:, :, None]
    m = O._flip(scale_and_crop(m, new_w, new_h, dx, dy, net_h, net_w, 0.0), flip)
    return np.around(np.squeeze(m, -1)).astype(bool)


def motion_blur3(img: np.ndarray, angle: int, line_type: int) -> np.ndarray:
    """O.motion_blur3 on an [H, W, 3] image: the same kernel (O.pyblur_line_kernel3), the same 255 border"""
    k = O.pyblur_line_kernel3(angle, line_type)
    H, W = img.shape[:2]
    pad = np.full((H + 2, W + 2, 3), 255.0, np.float32)
    pad[1:-1, 1:-1] = img.astype(np.float32)
    out = np.zeros(img.shape, np.float32)
    for i in range(3):
        for j in range(3):
            if k[i, j] != 0:
                dy, dx = i - 1, j - 1
                out = out + pad[1 - dy:1 - dy + H, 1 - dx:1 - dx + W] * k[i, j]
    return np.clip(out.astype(np.int64), 0, 255).astype(np.uint8)


def loader_sample(rng, image_h: int, image_w: int, boxes_xyxy: np.ndarray, cls, net_h: int, net_w: int, num_class: int = 3,
                  flipped: bool = True, blur_noise_light: bool = True):
    """one sample of defect_train.get (utils/train_data.py:86-133, 134-178, 187-249, 511-531) with net_h and net_w apart,
    drawing from ``rng`` in the reference's order.  The two ``new_ar < 1`` tests are ``new_ar < net_w / net_h``: which
    side binds the fit.  Returns (decisions, true_box rows [n, 4] normalised x, w by net_w and y, h by net_h, the three
    target grids normalised likewise)."""
    import math
    scale_crop = int(rng.randint(low=1, high=3))
    if scale_crop == 2:
        jitter = 0.2
        new_ar = image_w / image_h * rng.uniform(1 - jitter, 1 + jitter) / rng.uniform(1 - jitter, 1 + jitter)
        scale = rng.uniform(0.75, 1.5)
        if new_ar < net_w / net_h:
            new_h = int(scale * net_h)
            new_w = int(new_h * new_ar)
        else:
            new_w = int(scale * net_w)
            new_h = int(new_w / new_ar)
        dx = int(rng.uniform(0, net_w - new_w))
        dy = int(rng.uniform(0, net_h - new_h))
        sx, sy = float(new_w) / image_w, float(new_h) / image_h
        if len(boxes_xyxy):
            b = np.asarray(boxes_xyxy, np.float32)
            if ((b[:, 0] * sx + dx).min() < 0 or (b[:, 1] * sy + dy).min() < 0 or (b[:, 2] * sx + dx).max() >= net_w
                    or (b[:, 3] * sy + dy).max() >= net_h):
                scale_crop = 1
    if scale_crop == 1:
        new_ar = image_w / image_h
        if new_ar < net_w / net_h:
            new_h = int(1.0 * net_h)
            new_w = int(new_h * new_ar)
        else:
            new_w = int(1.0 * net_w)
            new_h = int(new_w / new_ar)
        dx, dy = (net_w - new_w) // 2, (net_h - new_h) // 2
        sx, sy = float(new_w) / image_w, float(new_h) / image_h
    bx = np.zeros((len(boxes_xyxy), 4), np.float32)
    for j, (x1, y1, x2, y2) in enumerate(boxes_xyxy):
        x1 = max(min(float(x1) * sx + dx, net_w - 1), 0)
        y1 = max(min(float(y1) * sy + dy, net_h - 1), 0)
        x2 = max(min(float(x2) * sx + dx, net_w - 1), 0)
        y2 = max(min(float(y2) * sy + dy, net_h - 1), 0)
        bx[j] = [(x2 + x1) / 2.0, (y2 + y1) / 2.0, x2 - x1, y2 - y1]
    ys = assign_targets(bx, cls, net_h, net_w, num_class=num_class)
    flip = int(rng.randint(low=1, high=4)) if flipped else 1
    if flip == 2:                                   # :195-215
        bx[:, 0] = net_w - 1 - bx[:, 0]
        for k in range(3):
            ys[k] = ys[k][:, ::-1].copy()
            on = ys[k][..., 4] == 1
            ys[k][on, 0] = np.float32(net_w - 1) - ys[k][on, 0]
    elif flip == 3:                                 # :216-236
        bx[:, 1] = net_h - 1 - bx[:, 1]
        for k in range(3):
            ys[k] = ys[k][::-1].copy()
            on = ys[k][..., 4] == 1
            ys[k][on, 1] = np.float32(net_h - 1) - ys[k][on, 1]
    bnl = int(rng.randint(low=1, high=5)) if blur_noise_light else 1
    dec = {"scale_crop": scale_crop, "new_w": new_w, "new_h": new_h, "dx": dx, "dy": dy, "flip": flip, "bnl": bnl}
    if bnl == 2:                                    # add_salt_pepper_noise: index ranges (H, W, 3)
        n_el = net_h * net_w * 3
        ns, npp = int(math.ceil(0.004 * n_el * 0.2)), int(math.ceil(0.004 * n_el * 0.8))
        cs = [rng.randint(0, i - 1, ns) for i in (net_h, net_w, 3)]
        cp = [rng.randint(0, i - 1, npp) for i in (net_h, net_w, 3)]
        dec.update(salt=(cs[0], cs[1]), pepper=(cp[0], cp[1]))
    elif bnl == 3:
        dec["coeff"] = rng.uniform() + 0.5
    elif bnl == 4:
        rng.randint(0, 1)
        type_idx = int(rng.randint(0, 3))
        angles = np.linspace(0, 180, 4, endpoint=False)
        dec.update(angle=int(angles[rng.randint(0, len(angles))]), line_type=("right", "left", "full")[type_idx])
    norm = np.asarray([net_w, net_h, net_w, net_h], np.float32)
    for k in range(3):
        ys[k][..., 0:4] = ys[k][..., 0:4] / norm
    return dec, bx / norm, ys

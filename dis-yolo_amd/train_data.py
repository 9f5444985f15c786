"""Training data pipeline: the counterpart of ``utils/train_data.py`` (``defect_train`` :18-531).

``defect_train.get()`` of the reference builds every batch on the host, synchronously, with cv2 and
scikit-image (:44-276) -- decode, rasterise the annotation polygons, random scale / crop, flip, motion blur /
noise / light change, YOLO target assignment.  At the step rates of the HIP path that loader would be three
orders of magnitude too slow, so here the HOST only draws the random decisions (in the
reference's order, from an injectable ``numpy.random.RandomState``), transforms the handful of boxes and
assigns the targets, and the GPU does all pixel work (``csrc/augment.hip``): polygon rasterisation, bilinear
resize + place + pad + flip of image and masks, the three photometric augmentations, /255 -- straight into the
batch buffers ``YOLONet.set_batch`` consumes.

Same ``get()`` contract, for ``image_size`` = S or (H, W): (images [B,H,W,3] f32, true_masks [B,20,H,W] bool, true_boxes [B,1,1,1,20,5],
yolo_3, yolo_2, yolo_1, clip_window [B,4]); tensors live on the GPU (``.cpu().numpy()`` for a host caller).  The two device
tensors are views of the loader's own batch buffers, of which there are two sets: what a ``get()`` returns stays intact through the
NEXT ``get()`` and is overwritten by the one after it (a training loop that reads one batch ahead, ``Solver.train``, holds two).

Round 6: what does not depend on the random draws is computed ONCE per record and kept on the GPU -- the decoded image, the
rasterised instance masks, their boxes (``load_mask`` / ``load_box`` of the reference run again on every visit of an image and return
the same arrays every time).  A 1000 x 1000 image with three instances is 6 MB; ``cache_bytes`` (default 16 GiB of the 288) bounds
it, records beyond the budget are recomputed per visit as before.  With it ``get()`` has no host synchronisation left; with the
target grids kept sparse on the host (a dozen rows in 5 MB of zeros) and uploaded from pinned staging, and all placements of a batch (images and instance masks) in one launch: 7.5 -> 1.4 ms per batch of 8
at 576^2; ``Solver.train`` end to end 630 -> 2100 images/s in stage 1 (the step's own rate), 806 in stage 2 (the step: 833)
(``tools/solver_rate.py``).

``placement="window"`` (the reference has nothing like it): every batch image is a net-size window of its record at
scale 1, the training counterpart of ``tiles.detect_tiled``.  The host draws the window's origin; which instances the window keeps,
their boxes and the three target grids come from the visible pixels and are computed on the GPU (window_visible, window_targets,
window_place_masks of ``csrc/augment.hip``), so ``get_device()`` still has no host synchronisation and ``get()`` downloads the
four small arrays with one.  The record cache keeps each instance's mask cropped to its static box.  tests/window_ref.py is the
definition.
"""
from __future__ import annotations

import copy
import math
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import config as cfg
from . import lib as L
from .synth import assign_target_entries


def rasterize_instance(polys: Sequence[Dict], image_h: int, image_w: int, device, out: Optional[torch.Tensor] = None,
                       origin=(0, 0)) -> torch.Tensor:
    """``load_mask`` for one instance (utils/train_data.py:325-336) on the GPU: polys = [{'type': 'out'|'in',
    'all_points_x': [...], 'all_points_y': [...]}] -> uint8 CUDA [image_h, image_w].  ``origin`` = (x, y), integers: the
    raster's pixel (0, 0) is the image's pixel (x, y) -- with ``image_h`` / ``image_w`` the crop's size this rasterises a crop
    of the instance without the full-size mask (the kernel works on vertex - pixel, so an integer shift changes no pixel)."""
    xs = np.concatenate([np.asarray(p["all_points_x"], np.float32) for p in polys]) if polys else np.zeros(0, np.float32)
    ys = np.concatenate([np.asarray(p["all_points_y"], np.float32) for p in polys]) if polys else np.zeros(0, np.float32)
    if tuple(origin) != (0, 0):
        xs = (xs.astype(np.float64) - int(origin[0])).astype(np.float32)
        ys = (ys.astype(np.float64) - int(origin[1])).astype(np.float32)
    start = np.cumsum([0] + [len(p["all_points_x"]) for p in polys]).astype(np.int32)
    is_out = np.asarray([1 if p["type"] == "out" else 0 for p in polys], np.int32)
    if out is None:
        out = torch.empty(image_h, image_w, dtype=torch.uint8, device=device)
    if len(polys) == 0:
        out.zero_()
        return out
    L.polygon_mask(torch.from_numpy(xs).to(device), torch.from_numpy(ys).to(device), torch.from_numpy(start).to(device),
                   torch.from_numpy(is_out).to(device), image_h, image_w, out)
    return out


def static_box(polys: Sequence[Dict], image_h: int, image_w: int):
    """(x1, y1, x2, y2) of an instance from its annotation alone: the min and the max + 1 of its polygons' vertices, clipped to
    the image (every pixel ``rasterize_instance`` sets lies inside it); x2 <= x1 or y2 <= y1 when nothing of it is in the
    image.  Host arithmetic: no raster, no synchronisation."""
    if not polys or not any(len(p["all_points_x"]) for p in polys):
        return 0, 0, 0, 0
    xs = np.concatenate([np.asarray(p["all_points_x"], np.float64) for p in polys])
    ys = np.concatenate([np.asarray(p["all_points_y"], np.float64) for p in polys])
    return (max(int(math.floor(xs.min())), 0), max(int(math.floor(ys.min())), 0),
            min(int(math.ceil(xs.max())) + 1, int(image_w)), min(int(math.ceil(ys.max())) + 1, int(image_h)))


WINDOW_CANDIDATES = 256      # instances of a record a window looks at: the first 256 whose static box meets it


def window_candidates(boxes, x0: int, y0: int, net_h: int, net_w: int) -> List[int]:
    """the indices of the static boxes (x1, y1, x2, y2) that meet the window [x0, x0 + net_w) x [y0, y0 + net_h), in order,
    the first WINDOW_CANDIDATES of them"""
    out = []
    for i, (x1, y1, x2, y2) in enumerate(boxes):
        if x1 < x0 + net_w and x2 > x0 and y1 < y0 + net_h and y2 > y0:
            out.append(i)
            if len(out) == WINDOW_CANDIDATES:
                break
    return out


def draw_window(rng, boxes, image_h: int, image_w: int, net_h: int, net_w: int, positive_fraction: float) -> Dict:
    """the window draws of one image, in this order: u = uniform(); with instances and u < positive_fraction an
    instance j, a point (px, py) of its static box and where in the window that point falls (ox, oy); otherwise the origin
    itself, x then y.  ``boxes``: the record's static boxes (the non-empty ones).  Returns x0, y0 (and what was drawn)."""
    max_x, max_y = max(image_w - net_w, 0), max(image_h - net_h, 0)
    u = rng.uniform()
    if len(boxes) and u < positive_fraction:
        j = int(rng.randint(0, len(boxes)))
        bx1, by1, bx2, by2 = boxes[j]
        px, py = int(rng.randint(bx1, bx2)), int(rng.randint(by1, by2))
        ox, oy = int(rng.randint(0, net_w)), int(rng.randint(0, net_h))
        return {"x0": min(max(px - ox, 0), max_x), "y0": min(max(py - oy, 0), max_y), "instance": j, "point": (px, py)}
    x0 = int(rng.randint(0, max_x + 1))
    y0 = int(rng.randint(0, max_y + 1))
    return {"x0": x0, "y0": y0, "instance": None, "point": None}


def extract_bboxes(mask: torch.Tensor):
    """utils/train_data.py:357-373: x1, y1, x2, y2 with x2 / y2 one past the last set pixel"""
    cols = torch.nonzero(mask.any(dim=0)).flatten()
    rows = torch.nonzero(mask.any(dim=1)).flatten()
    return int(cols[0]), int(rows[0]), int(cols[-1]) + 1, int(rows[-1]) + 1


def letterbox_boxes(labels: Sequence[Dict], image_size) -> np.ndarray:
    """float64 [N, 2]: the (w, h) of every instance of ``labels`` (``defect_train``'s records) in the pixels of a net of
    ``image_size`` (an int or (H, W)), i.e. scaled by the letter-box factor ``evaluate.image_read`` applies to the record's
    image.  An instance's box spans its polygon points, x2 / y2 one past the last one like ``extract_bboxes``.  A record
    gives its image size as ``'image'`` (the array), ``'image_size'`` = (h, w) or ``'imname'`` (decoded)."""
    from .net import check_image_size
    net_h, net_w = check_image_size(image_size)
    out = []
    for label in labels:
        if "image" in label:
            image_h, image_w = np.asarray(label["image"]).shape[:2]
        elif "image_size" in label:
            image_h, image_w = label["image_size"]
        else:
            from .evaluate import load_image_rgb
            image_h, image_w = load_image_rgb(label["imname"]).shape[:2]
        image_h, image_w = int(image_h), int(image_w)
        # the letter box of disyolo_letterbox_hw: the width binds when net_w / image_w < net_h / image_h
        if net_w / image_w < net_h / image_h:
            new_w, new_h = net_w, (image_h * net_w) // image_w
        else:
            new_w, new_h = (image_w * net_h) // image_h, net_h
        for polys in label["polygons"]:
            xs = np.concatenate([np.asarray(p["all_points_x"], np.float64) for p in polys]) if polys else np.zeros(0)
            ys = np.concatenate([np.asarray(p["all_points_y"], np.float64) for p in polys]) if polys else np.zeros(0)
            if xs.size == 0:
                continue
            out.append(((xs.max() + 1 - xs.min()) * new_w / image_w, (ys.max() + 1 - ys.min()) * new_h / image_h))
    return np.asarray(out, np.float64).reshape(-1, 2)


def cluster_anchors(labels, image_size, n: int = 9) -> np.ndarray:
    """The "dimension clustering" that yolo/config.py names for its ANCHORS and the reference does not ship: k-means over the
    instances' (w, h) at the net's size with the distance 1 - IoU of co-centred boxes (YOLOv2).  ``labels``: ``defect_train``'s
    records (``letterbox_boxes`` scales their boxes to ``image_size``).  Deterministic -- no random draw:
      * initial centroids: the boxes at the n evenly spaced quantiles (i + 1/2) / n of the boxes sorted by area;
      * a box joins the centroid of highest IoU (the first among equals); a centroid becomes the mean of its boxes, an empty
        cluster keeps its centroid;
      * stop when no assignment changes, or after 300 rounds.
    Returns float32 [n, 2], (w, h) in net pixels sorted by area ascending: rows [0:3] for the H/8 grid, as YOLONet's and
    defect_train's ``anchors`` take them.  Host numpy, once per dataset."""
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 1:
        raise ValueError("cluster_anchors: n must be a positive int (got %r)" % (n,))
    boxes = letterbox_boxes(labels, image_size)
    if len(boxes) < n:
        raise ValueError("cluster_anchors: %d clusters need at least as many instances (got %d)" % (n, len(boxes)))
    if not np.all(np.isfinite(boxes)) or not np.all(boxes > 0):
        raise ValueError("cluster_anchors: every instance must have a finite positive width and height")
    area = boxes[:, 0] * boxes[:, 1]
    order = np.argsort(area, kind="stable")
    pick = np.minimum(((np.arange(n) + 0.5) / n * len(boxes)).astype(np.int64), len(boxes) - 1)
    cent = boxes[order[pick]].copy()
    assign = np.full(len(boxes), -1, np.int64)
    for _ in range(300):
        inter = np.minimum(boxes[:, None, 0], cent[None, :, 0]) * np.minimum(boxes[:, None, 1], cent[None, :, 1])
        iou = inter / (area[:, None] + (cent[:, 0] * cent[:, 1])[None, :] - inter)
        new = np.argmax(iou, axis=1)                           # smallest 1 - IoU, the first among equals
        if np.array_equal(new, assign):
            break
        assign = new
        for c in range(n):
            mine = boxes[assign == c]
            if len(mine):
                cent[c] = mine.mean(axis=0)
    cent = cent[np.argsort(cent[:, 0] * cent[:, 1], kind="stable")]
    return np.ascontiguousarray(cent.astype(np.float32))


class defect_train(object):
    """labels: [{'image': RGB uint8 array [H,W,3] (or 'imname': path decoded with PIL), 'class_names': [...],
    'polygons': [[{'type', 'all_points_x', 'all_points_y'}, ...] per instance]}] -- the ``gt_labels`` structure of
    the reference's cache (utils/train_data.py:278-319)."""

    def __init__(self, labels: List[Dict], batch_size: Optional[int] = None, image_size=None, device=None,
                 rng: Optional[np.random.RandomState] = None, flipped: Optional[bool] = None,
                 blur_noise_light: Optional[bool] = None, cache_bytes: int = 16 << 30,
                 classes: Optional[Sequence[str]] = None, anchors=None, max_box_per_image: Optional[int] = None,
                 placement: str = "letterbox", min_visible: int = 8, positive_fraction: float = 1.0):
        # placement: "letterbox" = the reference's loader (the whole record fitted into the net); "window" = each batch image
        # a net-size window of its record at scale 1: min_visible = the visible pixels an instance needs to be
        # kept, positive_fraction = the share of windows drawn around a point of an instance (the rest anywhere in the image)
        if placement not in ("letterbox", "window"):
            raise ValueError("placement must be 'letterbox' or 'window' (got %r)" % (placement,))
        if isinstance(min_visible, bool) or not isinstance(min_visible, (int, np.integer)) or min_visible < 1:
            raise ValueError("min_visible must be an int >= 1 (got %r)" % (min_visible,))
        if isinstance(positive_fraction, bool) or not isinstance(positive_fraction, (int, float, np.integer, np.floating)) \
                or not 0.0 <= float(positive_fraction) <= 1.0:
            raise ValueError("positive_fraction must be a number in [0, 1] (got %r)" % (positive_fraction,))
        self.placement, self.min_visible, self.positive_fraction = placement, int(min_visible), float(positive_fraction)
        self.batch_size = cfg.BATCH_SIZE if batch_size is None else batch_size
        # image_size: an int S or a pair (net_h, net_w), like YOLONet's; the attribute keeps the caller's form
        from .net import check_image_size
        self.image_size = cfg.IMAGE_SIZE if image_size is None else image_size
        self.net_h, self.net_w = check_image_size(self.image_size)
        self.base_grid = self.net_h // 32 if self.net_h == self.net_w else (self.net_h // 32, self.net_w // 32)
        # the net's anchors and its ground-truth rows per image (YOLONet's options of the same names); cfg's unless given
        from .net import check_anchors, check_classes, check_limit
        self.max_box_per_image = check_limit(cfg.MAX_BOX_PER_IMAGE if max_box_per_image is None else max_box_per_image,
                                             "max_box_per_image")
        self.anchors = check_anchors(cfg.ANCHORS if anchors is None else anchors)
        self.num_anchor = 3
        self.classes = check_classes(cfg.CLASSES if classes is None else classes)     # cfg.CLASSES unless given
        self.num_class = len(self.classes)
        self.class_to_ind = dict(zip(self.classes, range(self.num_class)))
        self.flipped = cfg.FLIPPED if flipped is None else flipped
        self.blur_noise_light = cfg.BLUR_NOISE_LIGHT if blur_noise_light is None else blur_noise_light
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.rng = rng if rng is not None else np.random.RandomState()
        self.cursor, self.epoch = 0, 1
        self.gt_labels = list(labels)
        self.rng.shuffle(self.gt_labels)                       # :40
        self.random_labels = copy.copy(self.gt_labels)
        B, G = self.batch_size, self.max_box_per_image
        NH, NW = self.net_h, self.net_w
        dev = self.device
        # batch buffers, written in place by the kernels: two sets, used in turn
        self._sets = [(torch.zeros(B, NH, NW, 3, dtype=torch.float32, device=dev),
                       torch.zeros(B, G, NH, NW, dtype=torch.uint8, device=dev)) for _ in range(2)]
        self._turn = 0
        self.images, self.true_masks = self._sets[0]
        # the small host-built arrays (true_boxes, the three target grids, the clip windows): per set a staging copy on the host
        # (pinned where there is a GPU: its upload is asynchronous), the device copy get_device() hands out, the cells the
        # last fill of the set wrote (only those are cleared again: the grids are 5 MB of zeros around a dozen rows) and an
        # event behind the set's last upload
        cuda = dev.type == "cuda"
        shapes = [(B, 1, 1, 1, G, 5)] + [(B, NH // d, NW // d, 3, 5 + self.num_class) for d in (8, 16, 32)] + [(B, 4)]
        self._host = [[torch.zeros(sh, dtype=torch.float32, pin_memory=cuda) for sh in shapes] for _ in range(2)]
        self._dev = [[torch.zeros(sh, dtype=torch.float32, device=dev) for sh in shapes] for _ in range(2)]
        self._written = [[], []]
        self._uploaded = [None, None]
        for st in self._host:
            st[4][:, 2:] = 1.0                                 # window = (0, 0, 1, 1), :46-47
        self._last = None
        # uint8 frames of the batch (the placed images, augmented in place) + one scratch frame for the motion blur; the
        # placement jobs of a batch (images and instance masks: ONE launch, csrc/augment.hip place_batch_kernel) are written
        # into pinned staging and uploaded with the batch's other small arrays
        self._frames = torch.zeros(B, NH, NW, 3, dtype=torch.uint8, device=dev)
        self._blur = torch.zeros(NH, NW, 3, dtype=torch.uint8, device=dev)
        njob = B * (1 + G)
        job_bytes = njob * L.PLACE_JOB.itemsize
        if placement == "window":
            # the B image placements, then the window jobs (one per image and candidate instance) in the same staging: one
            # upload; the visible-part table and the jobs' rows stay on the device, and so do the four target arrays (the
            # clip windows never change: uploaded here, once)
            job_bytes = B * L.PLACE_JOB.itemsize + B * WINDOW_CANDIDATES * L.WINDOW_JOB.itemsize
            self._vis = torch.zeros(B * WINDOW_CANDIDATES, 5, dtype=torch.int32, device=dev)
            self._rows = torch.zeros(B * WINDOW_CANDIDATES, dtype=torch.int32, device=dev)
            self._anchors_dev = torch.from_numpy(self.anchors).to(dev)
            for st, d in zip(self._host, self._dev):
                d[4].copy_(st[4])
        # the salt-and-pepper coordinates of a batch (rows, cols per image) go through pinned staging too: an upload from
        # pageable memory waits for the stream, and get_device() must only enqueue
        n_el = NH * NW * 3
        n_sp = int(math.ceil(0.004 * n_el * 0.2)) + int(math.ceil(0.004 * n_el * 0.8))
        self._sp_host = [torch.zeros(B, 2, n_sp, dtype=torch.int32, pin_memory=cuda) for _ in range(2)]
        self._sp_dev = [torch.zeros(B, 2, n_sp, dtype=torch.int32, device=dev) for _ in range(2)]
        self._jobs_host = [torch.zeros(job_bytes, dtype=torch.uint8, pin_memory=dev.type == "cuda") for _ in range(2)]
        self._jobs_dev = [torch.zeros(job_bytes, dtype=torch.uint8, device=dev) for _ in range(2)]
        self.last_decisions: List[Dict] = []                   # the random draws of the last get(), for tests / logging
        # per-record static part (image on the GPU, instance masks, boxes, classes), keyed by the record object
        self.cache_bytes = int(cache_bytes)
        self._cache: Dict[int, tuple] = {}
        self._cached = 0

    def _image(self, label) -> np.ndarray:
        if "image" in label:
            return np.asarray(label["image"], np.uint8)
        from .evaluate import load_image_rgb
        return load_image_rgb(label["imname"])

    def _record(self, label):
        """what ``get()`` needs of a record that no random draw touches: (image_h, image_w, image uint8 on the GPU, the
        non-empty instance masks, their boxes [n,4], their class indices) -- :77-88 of the reference (load_mask, load_box)"""
        hit = self._cache.get(id(label))
        if hit is not None:
            return hit[1]
        dev, G = self.device, self.max_box_per_image
        image = self._image(label)
        image_h, image_w = image.shape[:2]
        polygons, class_names = label["polygons"][:G], label["class_names"][:G]           # :77-81
        masks = [rasterize_instance(p, image_h, image_w, dev) for p in polygons]          # load_mask
        keep = [i for i, m in enumerate(masks) if bool(m.any())]                          # load_box: non-empty masks
        assert len(keep) == len(class_names), "an annotated instance rasterised to nothing"
        boxes = np.array([extract_bboxes(masks[i]) for i in keep], np.float32).reshape(-1, 4)
        cls = [self.class_to_ind[class_names[i]] for i in keep]
        src = torch.from_numpy(np.ascontiguousarray(image)).to(dev)
        entry = (image_h, image_w, src, [masks[i] for i in keep], boxes, cls)
        nbytes = src.numel() + sum(m.numel() for m in entry[3])
        if self._cached + nbytes <= self.cache_bytes:
            self._cache[id(label)] = (label, entry)        # (the record itself is held: its id stays its own)
            self._cached += nbytes
        return entry

    def get(self):
        """the reference's tuple: (images, true_masks) on the GPU, (true_boxes, yolo_3, yolo_2, yolo_1, window) numpy.  In
        window mode the host never has the boxes and grids (they come from the visible pixels): this call downloads the four
        arrays, with ONE synchronisation; a training loop takes ``get_device()``, which has none."""
        self._fill()
        h = self._host[self._last]
        if self.placement == "window":
            small = [t.numpy() for t in torch.cat([d.reshape(-1) for d in self._dev[self._last][:4]]).cpu().split(
                [d.numel() for d in self._dev[self._last][:4]])]
            small = [a.reshape(d.shape) for a, d in zip(small, self._dev[self._last][:4])]
            return (self.images, self.true_masks.view(torch.bool), small[0], small[1], small[2], small[3], h[4].numpy())
        return (self.images, self.true_masks.view(torch.bool), h[0].numpy(), h[1].numpy(), h[2].numpy(), h[3].numpy(), h[4].numpy())

    def get_device(self) -> Dict[str, torch.Tensor]:
        """the same batch as ``YOLONet.set_batch``'s dict with EVERY array on the GPU (the small ones uploaded from pinned
        staging on the current stream, asynchronously): a training loop fed this way never waits for the device
        (``Solver.train`` uses it when the data object has it)"""
        self._fill()
        d = self._dev[self._last]
        return {"images": self.images, "true_masks": self.true_masks.view(torch.bool), "true_boxes": d[0], "yolo3": d[1],
                "yolo2": d[2], "yolo1": d[3], "clip_window": d[4]}

    def _record_window(self, label):
        """the static part of a record in window mode: (image_h, image_w, image uint8 on the GPU, per instance with a
        non-empty static box its byte mask CROPPED to that box (rasterised once, with the vertices shifted by the crop's
        origin), the static boxes [(x1, y1, x2, y2)], the class indices).  Nothing full-size per instance is kept, no box is
        fetched from the device, and the record is not cut to its first max_box_per_image instances."""
        hit = self._cache.get(id(label))
        if hit is not None:
            return hit[1]
        dev = self.device
        image = self._image(label)
        image_h, image_w = image.shape[:2]
        crops, boxes, cls = [], [], []
        for polys, name in zip(label["polygons"], label["class_names"]):
            x1, y1, x2, y2 = static_box(polys, image_h, image_w)
            if x2 <= x1 or y2 <= y1:
                continue
            crops.append(rasterize_instance(polys, y2 - y1, x2 - x1, dev, origin=(x1, y1)))
            boxes.append((x1, y1, x2, y2))
            cls.append(self.class_to_ind[name])
        src = torch.from_numpy(np.ascontiguousarray(image)).to(dev)
        entry = (image_h, image_w, src, crops, boxes, cls)
        nbytes = src.numel() + sum(m.numel() for m in crops)
        if self._cached + nbytes <= self.cache_bytes:
            self._cache[id(label)] = (label, entry)
            self._cached += nbytes
        return entry

    def _draw_photo(self, count: int, bnl: int, dec: Dict, photo: List) -> None:
        """the draws of the photometric step of image ``count`` (:228-241, 466-535) in the reference's order; the step itself is
        noted in ``photo`` for after the placement launch"""
        rng = self.rng
        net_h, net_w = self.net_h, self.net_w
        if bnl == 2:                                                                    # salt & pepper (:511-525)
            n_el = net_h * net_w * 3
            ns, npp = int(math.ceil(0.004 * n_el * 0.2)), int(math.ceil(0.004 * n_el * 0.8))
            cs = [rng.randint(0, i - 1, ns) for i in (net_h, net_w, 3)]
            cp = [rng.randint(0, i - 1, npp) for i in (net_h, net_w, 3)]
            photo.append((count, "salt_pepper", (np.concatenate([cs[0], cp[0]]).astype(np.int32),
                                                 np.concatenate([cs[1], cp[1]]).astype(np.int32), ns, npp)))
            dec.update(salt=(cs[0], cs[1]), pepper=(cp[0], cp[1]))
        elif bnl == 3:                                                                  # light (:527-535)
            coeff = rng.uniform() + 0.5
            photo.append((count, "light", (coeff,)))
            dec["coeff"] = coeff
        elif bnl == 4:                                                                  # motion blur (:466-494)
            length_idx = rng.randint(0, 1)                                              # lineLengths = [3]
            type_idx = int(rng.randint(0, 3))                                           # right, left, full
            angles = np.linspace(0, 180, 4, endpoint=False)                             # kernel centre 1 -> 4 lines
            angle = int(angles[rng.randint(0, len(angles))])
            photo.append((count, "blur", (angle, {0: 1, 1: 2, 2: 0}[type_idx])))
            dec.update(angle=angle, line_type=("right", "left", "full")[type_idx], _len=int(length_idx))

    def _next_record(self) -> None:
        self.cursor += 1
        if self.cursor >= len(self.gt_labels):                                          # :266-271
            self.rng.shuffle(self.gt_labels)
            self.random_labels = copy.copy(self.gt_labels)
            self.cursor = 0
            self.epoch += 1

    def _photo_and_float(self, photo: List, turn: int) -> None:
        """the photometric steps noted by ``_draw_photo`` on the placed frames, then the batch's one /255 (the caller records
        the set's upload event after this: the salt-and-pepper staging of ``turn`` is read by copies enqueued here)"""
        S = (self.net_h, self.net_w)
        for count, what, a in photo:
            f = self._frames[count]
            if what == "salt_pepper":
                h, d = self._sp_host[turn][count], self._sp_dev[turn][count]
                h.numpy()[0], h.numpy()[1] = a[0], a[1]
                d.copy_(h, non_blocking=True)
                L.aug_salt_pepper(f, S, d[0], d[1], a[2], a[3])
            elif what == "light":
                L.aug_change_light(f, S, a[0])
            else:
                L.aug_motion_blur3(f, self._blur, S, a[0], a[1])
                f.copy_(self._blur)
        L.aug_to_float(self._frames, self.images)

    def _fill_window(self) -> None:
        """a batch of windows: the host draws the origins and builds one job per image and candidate instance;
        image placement, visible parts, target assignment and mask placement are launches on the current stream, and nothing
        comes back to the host"""
        B, rng = self.batch_size, self.rng
        S = NH, NW = self.net_h, self.net_w
        turn = self._turn
        self._turn ^= 1
        self._last = turn
        self.images, self.true_masks = self._sets[turn]
        if self._uploaded[turn] is not None:
            self._uploaded[turn].synchronize()                 # (the upload of two batches ago: long done)
        self.true_masks.zero_()
        self.last_decisions = []
        place_bytes = B * L.PLACE_JOB.itemsize
        raw = self._jobs_host[turn].numpy()
        jobs, wjobs = raw[:place_bytes].view(L.PLACE_JOB), raw[place_bytes:].view(L.WINDOW_JOB)
        nwin = 0
        photo, alive = [], []
        for count in range(B):
            label = self.random_labels[self.cursor]
            image_h, image_w, src, crops, boxes, cls = self._record_window(label)
            dec = {"placement": "window"}
            dec.update(draw_window(rng, boxes, image_h, image_w, NH, NW, self.positive_fraction))
            x0, y0 = dec["x0"], dec["y0"]
            flip = 1
            if self.flipped:
                flip = int(rng.randint(low=1, high=4))
            bnl = 1
            if self.blur_noise_light:
                bnl = int(rng.randint(low=1, high=5))
            dec.update(flip=flip, bnl=bnl)
            # the image: the existing placement at scale 1 (taps a = 0: a copy) with the 127 pad
            alive.append((src, crops))
            jobs[count] = (src.data_ptr(), self._frames[count].data_ptr(), 0, image_h, image_w, image_w, image_h, -x0, -y0, flip)
            for i in window_candidates(boxes, x0, y0, NH, NW):
                x1, y1, x2, y2 = boxes[i]
                wjobs[nwin] = (crops[i].data_ptr(), y2 - y1, x2 - x1, x1, y1, x0, y0, image_h, image_w, count, cls[i], flip, 0)
                nwin += 1
            self._draw_photo(count, bnl, dec, photo)
            self.last_decisions.append(dec)
            self._next_record()
        nbytes = place_bytes + nwin * L.WINDOW_JOB.itemsize
        jd = self._jobs_dev[turn]
        jd[:nbytes].copy_(self._jobs_host[turn][:nbytes], non_blocking=True)
        L.aug_place_batch(jd, B, S)
        d, wj = self._dev[turn], jd[place_bytes:]
        self._last_window = (wj, nwin)                         # (what the three launches below were given: tools/window_rate.py)
        L.window_visible(wj, nwin, S, self._vis)
        L.window_targets(wj, nwin, self._vis, self._anchors_dev, S, self.min_visible, d[0], d[1], d[2], d[3], self._rows)
        L.window_place_masks(wj, nwin, self._rows, self.true_masks, S)
        self._photo_and_float(photo, turn)
        if self.device.type == "cuda":
            self._uploaded[turn] = torch.cuda.current_stream().record_event()      # (behind the set's last upload)
        del alive

    def _fill(self) -> None:
        if self.placement == "window":
            return self._fill_window()
        B, G, rng = self.batch_size, self.max_box_per_image, self.rng
        S = (self.net_h, self.net_w)
        norm = np.asarray([self.net_w, self.net_h, self.net_w, self.net_h], np.float32)      # x, w by net_w; y, h by net_h
        dev = self.device
        turn = self._turn
        self._turn ^= 1
        self._last = turn
        self.images, self.true_masks = self._sets[turn]
        if self._uploaded[turn] is not None:
            self._uploaded[turn].synchronize()                 # (the upload of two batches ago: long done)
        host = self._host[turn]
        true_boxes, ys = host[0].numpy(), [host[1].numpy(), host[2].numpy(), host[3].numpy()]   # yolo3, yolo2, yolo1
        true_boxes[...] = 0.0
        for k, b, yi, xi, a in self._written[turn]:
            ys[k][b, yi, xi, a] = 0.0
        written = self._written[turn] = []
        self.true_masks.zero_()
        self.last_decisions = []
        jobs = self._jobs_host[turn].numpy().view(L.PLACE_JOB)
        njobs = 0
        photo = []          # (image index, what, arguments): the photometric step of the images that drew one
        alive = []          # sources of records beyond the cache budget: held until the launch that reads them is enqueued
        for count in range(B):
            label = self.random_labels[self.cursor]
            image_h, image_w, src, masks, boxes, cls = self._record(label)
            # ---- augmentation step 1: random scale and crop (:90-133); the draws happen in the reference's order
            net_h, net_w = S
            fit_ar = net_w / net_h           # which side binds the fit: the reference's ``new_ar < 1`` at net_w = net_h
            scale_crop = int(rng.randint(low=1, high=3))
            if scale_crop == 2:
                jitter = 0.2
                new_ar = image_w / image_h * rng.uniform(1 - jitter, 1 + jitter) / rng.uniform(1 - jitter, 1 + jitter)
                scale = rng.uniform(0.75, 1.5)
                if new_ar < fit_ar:
                    new_h = int(scale * net_h)
                    new_w = int(new_h * new_ar)
                else:
                    new_w = int(scale * net_w)
                    new_h = int(new_w / new_ar)
                dx = int(rng.uniform(0, net_w - new_w))
                dy = int(rng.uniform(0, net_h - new_h))
                sx, sy = float(new_w) / image_w, float(new_h) / image_h
                if len(boxes):
                    x1, y1 = boxes[:, 0] * sx + dx, boxes[:, 1] * sy + dy
                    x2, y2 = boxes[:, 2] * sx + dx, boxes[:, 3] * sy + dy
                    if x1.min() < 0 or y1.min() < 0 or x2.max() >= net_w or y2.max() >= net_h:
                        scale_crop = 1                                                     # keep every defect inside
            if scale_crop == 1:
                new_ar = image_w / image_h
                if new_ar < fit_ar:
                    new_h = int(1.0 * net_h)
                    new_w = int(new_h * new_ar)
                else:
                    new_w = int(1.0 * net_w)
                    new_h = int(new_w / new_ar)
                dx, dy = (net_w - new_w) // 2, (net_h - new_h) // 2
                sx, sy = float(new_w) / image_w, float(new_h) / image_h
            # ---- boxes into the net frame (:136-147) and the three YOLO target grids (:149-178)
            bx = np.zeros((len(boxes), 4), np.float32)
            for j, (x1, y1, x2, y2) in enumerate(boxes):
                x1 = max(min(float(x1) * sx + dx, net_w - 1), 0)
                y1 = max(min(float(y1) * sy + dy, net_h - 1), 0)
                x2 = max(min(float(x2) * sx + dx, net_w - 1), 0)
                y2 = max(min(float(y2) * sy + dy, net_h - 1), 0)
                bx[j] = [(x2 + x1) / 2.0, (y2 + y1) / 2.0, x2 - x1, y2 - y1]
            # (the non-zero rows of the three grids, {(yi, xi, anchor): row}: pixel units, like the reference here)
            grids = assign_target_entries(bx, cls, S, self.num_class, self.anchors)
            # ---- step 2: flip (:187-226) -- the grids are mirrored and the stored centres reflected
            flip = 1
            if self.flipped:
                flip = int(rng.randint(low=1, high=4))
            if flip == 2:
                bx[:, 0] = net_w - 1 - bx[:, 0]
                for k, ent in enumerate(grids):
                    gsz = ys[k].shape[2]
                    for row in ent.values():
                        row[0] = np.float32(net_w - 1) - row[0]
                    grids[k] = {(yi, gsz - 1 - xi, a): row for (yi, xi, a), row in ent.items()}
            elif flip == 3:
                bx[:, 1] = net_h - 1 - bx[:, 1]
                for k, ent in enumerate(grids):
                    gsz = ys[k].shape[1]
                    for row in ent.values():
                        row[1] = np.float32(net_h - 1) - row[1]
                    grids[k] = {(gsz - 1 - yi, xi, a): row for (yi, xi, a), row in ent.items()}
            # ---- step 3: blur / noise / light (:228-241)
            bnl = 1
            if self.blur_noise_light:
                bnl = int(rng.randint(low=1, high=5))
            dec = {"scale_crop": scale_crop, "new_w": new_w, "new_h": new_h, "dx": dx, "dy": dy, "flip": flip, "bnl": bnl}
            # ---- pixels (image_read :376-416, resize_mask :418-444) on the GPU: the placements as jobs of the batch's one
            #      launch, the photometric step noted for after it (the draws happen here, in the reference's order)
            alive.append((src, masks))
            jobs[njobs] = (src.data_ptr(), self._frames[count].data_ptr(), 0, image_h, image_w, new_w, new_h, dx, dy, flip)
            njobs += 1
            for j, m in enumerate(masks):
                jobs[njobs] = (m.data_ptr(), self.true_masks[count, j].data_ptr(), 1, image_h, image_w, new_w, new_h, dx, dy, flip)
                njobs += 1
            self._draw_photo(count, bnl, dec, photo)
            # ---- normalise (:250-257)
            true_boxes[count, 0, 0, 0, :len(bx), :4] = bx / norm
            true_boxes[count, 0, 0, 0, :len(bx), 4] = cls
            for k, ent in enumerate(grids):
                for (yi, xi, a), row in ent.items():
                    row[0:4] = row[0:4] / norm
                    ys[k][count, yi, xi, a] = row
                    written.append((k, count, yi, xi, a))
            self.last_decisions.append(dec)
            self._next_record()
        # ---- the batch's pixel work: one placement launch, the photometric steps, one /255
        jd = self._jobs_dev[turn]
        jd[:njobs * L.PLACE_JOB.itemsize].copy_(self._jobs_host[turn][:njobs * L.PLACE_JOB.itemsize], non_blocking=True)
        L.aug_place_batch(jd, njobs, S)
        self._photo_and_float(photo, turn)
        del alive
        if dev.type == "cuda":
            for h, d in zip(host, self._dev[turn]):
                d.copy_(h, non_blocking=True)
            self._uploaded[turn] = torch.cuda.current_stream().record_event()
        else:
            for h, d in zip(host, self._dev[turn]):
                d.copy_(h)

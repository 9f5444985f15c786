"""The second option matrix: whole-net rows that combine the options merged after tests/option_matrix.py -- image_size=(H, W),
nms=, anchors= / max_box_per_image= / max_detection=, mask_roi_det= / mask_roi_gt= / mask_roi_iou= and tiles.detect_tiled --
with each other and with the class list, k_map, mask_stride and the lock map.  Shared by tests/test_option_matrix2.py (CPU: the
table's coverage, the composed oracle on every row, every option biting on its row) and tests/test_gpu_option_matrix2.py (GPU:
the step, its recorded forms, inference, evaluation, tiled detection and the loader on the rows).  Importing it needs no GPU.

Every whole-net test of the per-option files holds the OTHER options at their defaults, so the kernels' branch points -- the
loss pitch (C > 5), the RoI table (more than 16 RoIs), the per-class filter's three forms (rank merge; k-way merge at C <= 16
with C D > 512; bucketed segments at C > 16), the winner lists (D > 64), the image-wide filters, the paste jobs (D > 64) and the
rectangular score map at m = 4 / 2 / 1 -- are reached one at a time there.  The rows below cross them.  Factors:

  frame (B, H, W)  (2, 64, 64); (2, 64, 96): W/4 no multiple of 16, no fused 64-channel block; (3, 96, 64): tall, odd B;
                   (1, 64, 128): every fused launch admitted, B = 1
  C                3 (the narrow YOLO loss), 6 (the first wide one), 16 (the last count with a block per class; 16 D > 512 takes
                   the k-way merge), 17 (the first bucketed one), 80
  k                3, 5, 7        m   4, 2, 1
  lock             the stage-1 map, the stage-2 map, a holed map of tests/lock_maps.py valid for the row's m
  nms              per_class, agnostic, none
  limits (G, D)    (20, 30) configured; (40, 40); (100, 100); (256, 256)
  anchors          cfg.ANCHORS; limits_ref.NET_ANCH (non-integer)
  rois             (n_det, n_gt, iou): (7, 3, 0.5) configured; (10, 6, 0.4): 16 rows, the narrow kernels with other counts and
                   another threshold; (40, 40, 0.5); (0, 256, 0.5): ground truth only, "more than there are takes all";
                   (40, 0, 0.5): detections only

Every pair of values of two different factors occurs in a row (tests/test_option_matrix2.py checks the table as written), with
two exceptions, PAIRS_LEFT_OUT: the rows at B = 1 keep the stage-1 map, since batch norms over 4 values per channel make the
bf16 gradient distance depend on the seed (the docstring of tests/option_matrix.py has the figures).  TRIPLES lists the
crossings of three values that a row must hold; the CPU test asserts them.

The table was made by a greedy search over the pairs under conditions that keep a row a well-posed case for the oracle alone
(the CPU test holds every row to them): a row with D > 64 needs more than 64 kept detections per image, which per-class NMS
yields only with 16 or more classes and agnostic NMS only with the small anchors; a detections-only row needs more than 16
detections that cover 4 x 4 of the score map (``plant_min``).  The rows were then fixed; ``seed`` is the batch seed, 11 throughout.

Extras: "map" (evaluate() end to end, stage-1 rows), "tiled" (tiles.detect_tiled with the row's inference net), "loader"
(defect_train on the row's net)."""
from collections import namedtuple
from typing import Dict

import numpy as np
import torch

import disyolo_oracle as O
import limits_ref as LR
import mask_roi_ref as RR
import mask_stride_ref as MR
import nms_modes_ref as NR
import rect_ref as RECT
from disyolo_amd import config as cfg
from lock_maps import lock_of, pass_through

Row = namedtuple("Row", "name B H W C k m lock nms G D anchors rois seed extras")

FRAMES = [(2, 64, 64), (2, 64, 96), (3, 96, 64), (1, 64, 128)]
CLASS_COUNTS = [3, 6, 16, 17, 80]
K_MAPS = [3, 5, 7]
MASK_STRIDES = [4, 2, 1]
LOCK_KINDS = ["stage1", "stage2", "holed"]
NMS = ["per_class", "agnostic", "none"]
LIMITS = [(20, 30), (40, 40), (100, 100), (256, 256)]
ANCHORS = ["cfg", "net"]
ROIS = [(7, 3, 0.5), (10, 6, 0.4), (40, 40, 0.5), (0, 256, 0.5), (40, 0, 0.5)]

PAIRS_LEFT_OUT = [("frame", (1, 64, 128), "lock", "stage2"), ("frame", (1, 64, 128), "lock", "holed")]
DET_THRESH = 0.1          # the training steps' detection threshold in the tests
INFER_THRESH = 0.02       # the inference tests' (80 classes share the probability: tests/test_gpu_option_matrix.py)


def _row(frame, C, k, m, lock, nms, limits, anchors, rois, seed=11, extras=()):
    B, H, W = frame
    name = "b%d_%dx%d_c%d_k%d_m%d_%s_%s_g%dd%d_%s_r%d+%d" % (B, H, W, C, k, m, lock, nms, limits[0], limits[1], anchors,
                                                            rois[0], rois[1])
    return Row(name, B, H, W, C, k, m, lock, nms, limits[0], limits[1], anchors, tuple(rois), seed, tuple(extras))


ROWS = [
    _row((2, 64, 96), 17, 5, 2, "stage1_hole", "agnostic", (100, 100), "net", (7, 3, 0.5)),
    _row((3, 96, 64), 80, 3, 4, "stage2", "none", (256, 256), "cfg", (40, 40, 0.5)),
    _row((2, 64, 64), 16, 7, 1, "m1_hole", "per_class", (40, 40), "cfg", (0, 256, 0.5)),
    _row((1, 64, 128), 16, 3, 4, "stage1", "per_class", (100, 100), "net", (10, 6, 0.4), extras=("tiled",)),
    _row((2, 64, 96), 6, 7, 1, "stage1", "none", (20, 30), "cfg", (40, 0, 0.5), extras=("map",)),
    _row((2, 64, 64), 17, 7, 4, "stage2", "agnostic", (20, 30), "net", (0, 256, 0.5)),
    _row((2, 64, 64), 3, 5, 2, "stage2", "none", (100, 100), "cfg", (40, 0, 0.5)),
    _row((3, 96, 64), 17, 5, 2, "stage1", "per_class", (40, 40), "net", (40, 40, 0.5), extras=("loader",)),
    _row((1, 64, 128), 3, 3, 1, "stage1", "agnostic", (20, 30), "cfg", (7, 3, 0.5)),
    _row((2, 64, 96), 6, 3, 2, "stage2", "per_class", (40, 40), "cfg", (10, 6, 0.4)),
    _row((3, 96, 64), 3, 7, 1, "stage1_hole_m1", "agnostic", (256, 256), "net", (10, 6, 0.4)),
    _row((1, 64, 128), 6, 5, 2, "stage1", "none", (256, 256), "cfg", (0, 256, 0.5)),
    _row((2, 64, 96), 17, 3, 4, "frozen_heads_m4", "none", (256, 256), "cfg", (40, 0, 0.5)),
    _row((2, 64, 96), 16, 5, 1, "stage1_hole_m1", "agnostic", (20, 30), "net", (40, 40, 0.5)),
    _row((1, 64, 128), 80, 7, 1, "stage1", "agnostic", (40, 40), "net", (7, 3, 0.5)),
    _row((3, 96, 64), 16, 7, 4, "stage2", "none", (40, 40), "net", (7, 3, 0.5)),
    _row((2, 64, 64), 80, 5, 2, "stage1", "per_class", (20, 30), "cfg", (10, 6, 0.4)),
    _row((2, 64, 64), 6, 7, 2, "hole_5_9", "agnostic", (100, 100), "net", (40, 40, 0.5)),
    _row((2, 64, 64), 17, 3, 1, "stage2", "per_class", (256, 256), "net", (7, 3, 0.5)),
    _row((2, 64, 96), 3, 3, 4, "stage1_hole_m4", "per_class", (40, 40), "cfg", (0, 256, 0.5)),
    _row((3, 96, 64), 6, 5, 4, "stage2", "none", (100, 100), "net", (0, 256, 0.5)),
    _row((1, 64, 128), 17, 7, 1, "stage1", "none", (100, 100), "cfg", (10, 6, 0.4), extras=("tiled",)),
    _row((3, 96, 64), 16, 5, 2, "stage2", "per_class", (256, 256), "net", (40, 0, 0.5)),
    _row((1, 64, 128), 3, 5, 2, "stage1", "agnostic", (256, 256), "net", (40, 40, 0.5)),
    _row((3, 96, 64), 6, 7, 2, "stage2", "none", (20, 30), "cfg", (7, 3, 0.5)),
    _row((3, 96, 64), 80, 7, 4, "stage2", "none", (100, 100), "cfg", (0, 256, 0.5)),
    # ---- beside the search's rows: where its conditions were too weak for the oracle (the CPU test), a row was changed and the
    #      pairs it gave up are held here
    _row((2, 64, 96), 6, 5, 1, "stage1", "agnostic", (256, 256), "net", (40, 0, 0.5), extras=("map",)),
    _row((1, 64, 128), 80, 3, 1, "stage1", "none", (40, 40), "cfg", (40, 0, 0.5)),
    _row((2, 64, 96), 80, 7, 2, "stage1_hole", "per_class", (40, 40), "net", (10, 6, 0.4)),
]

# (what the row must hold, a predicate on the row)
_rect = lambda r: r.H != r.W
_wide = lambda r: r.rois[0] + r.rois[1] > 16
TRIPLES = [
    ("agnostic x D > 64 x C > 16", lambda r: r.nms == "agnostic" and r.D > 64 and r.C > 16),
    ("none x D = 256 x rectangular", lambda r: r.nms == "none" and r.D == 256 and _rect(r)),
    ("per_class x C = 16 x D = 40 (k-way merge, 64-entry lists)", lambda r: r.nms == "per_class" and r.C == 16 and r.D == 40),
    ("per_class x C = 16 x D >= 100 (k-way merge, 256-entry lists)", lambda r: r.nms == "per_class" and r.C == 16 and r.D >= 100),
    ("rois > 16 x m = 1 x rectangular", lambda r: _wide(r) and r.m == 1 and _rect(r)),
    ("rois > 16 x k = 7 x m = 4", lambda r: _wide(r) and r.k == 7 and r.m == 4),
    ("G = 256 x C = 80", lambda r: r.G == 256 and r.C == 80),
    ("stage 2 x rois > 16 x D > 64", lambda r: r.lock == "stage2" and _wide(r) and r.D > 64),
    ("holed x agnostic", lambda r: lock_kind(r) == "holed" and r.nms == "agnostic"),
    ("rectangular x non-default anchors x C > 5", lambda r: _rect(r) and r.anchors == "net" and r.C > 5),
]


def ids(rows):
    return [r.name for r in rows]


def describe(row: Row) -> str:
    """what a failure message says about the row, so that a report reads without the table"""
    return ("row %s (B=%d, H=%d, W=%d, %d classes, k_map=%d, mask_stride=%d, lock=%s, nms=%s, G=%d, D=%d, anchors=%s, "
            "rois=%s, batch seed %d)" % (row.name, row.B, row.H, row.W, row.C, row.k, row.m, row.lock, row.nms, row.G, row.D,
                                         row.anchors, row.rois, row.seed))


def names(n):
    return ["class%02d" % i for i in range(n)]


def factors(row: Row) -> dict:
    return {"frame": (row.B, row.H, row.W), "C": row.C, "k": row.k, "m": row.m, "lock": lock_kind(row), "nms": row.nms,
            "limits": (row.G, row.D), "anchors": row.anchors, "rois": row.rois}


VALUES = {"frame": FRAMES, "C": CLASS_COUNTS, "k": K_MAPS, "m": MASK_STRIDES, "lock": LOCK_KINDS, "nms": NMS, "limits": LIMITS,
          "anchors": ANCHORS, "rois": ROIS}


def lock_kind(row: Row) -> str:
    return row.lock if row.lock in ("stage1", "stage2") else "holed"


def lock_of_row(row: Row) -> Dict[int, bool]:
    if row.lock in ("stage1", "stage2"):
        return MR.default_lock(int(row.lock[-1]), row.m)
    m, lock = lock_of(row.lock)
    assert m == row.m, "%s: map %s is a map of mask_stride %d" % (row.name, row.lock, m)
    return lock


def locked_prefix(row: Row) -> int:
    lock, n = lock_of_row(row), 0
    while lock.get(n + 1, False):
        n += 1
    return n


def expected_pass_through(row: Row):
    return pass_through(row.m, lock_of_row(row))


def anchors_of(row: Row) -> np.ndarray:
    return np.asarray(cfg.ANCHORS, np.float32) if row.anchors == "cfg" else LR.NET_ANCH


def net_kwargs(row: Row) -> dict:
    """YOLONet(..., **net_kwargs(row)): everything but training / device / seed"""
    return dict(image_size=(row.H, row.W), batch_size=row.B, classes=names(row.C), k_map=row.k, mask_stride=row.m,
                lock=lock_of_row(row), nms=row.nms, anchors=anchors_of(row), max_box_per_image=row.G, max_detection=row.D,
                mask_roi_det=row.rois[0], mask_roi_gt=row.rois[1], mask_roi_iou=row.rois[2])


def trainable_names(row: Row):
    lock = lock_of_row(row)
    if row.m == 2:
        return O.trainable_names(lock)
    return [n for n in MR.variable_shapes(row.m, row.k) if not lock[int(n.split("convolutional")[1].split("/")[0])]
            and not n.split("/")[-1].startswith("moving_")]


# ------------------------------------------------------------------------------------------------ the batch
N_INSTANCES = 20


def instance_rows(G):
    """the rows of true_boxes / true_masks that hold the twenty instances: spread over 0..G-1, so that the first 16 rows are not
    the only ones used and, where G > 64, rows >= 64 are"""
    return [int(v) for v in np.linspace(0, G - 1, N_INSTANCES).round()]


def bare_batch(row: Row, seed=None):
    """``limits_ref.net_batch`` on an H x W net: twenty ellipses per image in rows ``instance_rows(G)`` of G-row tables, classes
    of the row's list, targets assigned with the row's anchors by ``rect_ref.assign_targets``"""
    B, H, W, G, C = row.B, row.H, row.W, row.G, row.C
    anchors = anchors_of(row)
    rng = np.random.RandomState(row.seed if seed is None else seed)
    norm = np.asarray([W, H, W, H], np.float32)
    images = torch.from_numpy(rng.rand(B, H, W, 3).astype(np.float32))
    true_boxes = np.zeros((B, 1, 1, 1, G, 5), np.float32)
    true_masks = np.zeros((B, G, H, W), bool)
    ys = [np.zeros((B, H // d, W // d, 3, 5 + C), np.float32) for d in (8, 16, 32)]
    yy, xx = np.mgrid[0:H, 0:W]
    for b in range(B):
        bx, cl = [], []
        for j in instance_rows(G):
            while True:
                w, h = rng.uniform(0.08, 0.5, size=2) * np.asarray([W, H])
                cx, cy = rng.uniform(w / 2, W - w / 2), rng.uniform(h / 2, H - h / 2)
                m = ((xx - cx) / (w / 2)) ** 2 + ((yy - cy) / (h / 2)) ** 2 <= 1.0
                rws, cols = np.where(m)
                # (more than a pixel and a half of the score map on both sides: the box's RoI cannot round to zero area -- the NaN
                #  mask term of the reference, SURVEY B14 -- where every box is an RoI)
                if m.any() and cols.max() - cols.min() >= 1.5 * row.m and rws.max() - rws.min() >= 1.5 * row.m:
                    break
            x1, x2, y1, y2 = cols.min(), cols.max(), rws.min(), rws.max()
            c = rng.randint(0, C)
            box = [(x1 + x2) / 2.0, (y1 + y2) / 2.0, float(x2 - x1), float(y2 - y1)]
            true_masks[b, j] = m
            true_boxes[b, 0, 0, 0, j, :4] = np.asarray(box, np.float32) / norm
            true_boxes[b, 0, 0, 0, j, 4] = c
            bx.append(box)
            cl.append(c)
        for dst, t in zip(ys, RECT.assign_targets(np.asarray(bx, np.float32).reshape(-1, 4), np.asarray(cl), H, W, anchors=anchors,
                                                  num_class=C)):
            t[..., 0:4] /= norm
            dst[b] = t
    window = np.tile(np.array([[0.0, 0.0, 1.0, 1.0]], np.float32), (B, 1))
    return {"images": images, "clip_window": window, "true_boxes": torch.from_numpy(true_boxes), "true_masks": true_masks,
            "yolo3": torch.from_numpy(ys[0]), "yolo2": torch.from_numpy(ys[1]), "yolo1": torch.from_numpy(ys[2])}


PLANT_SHRINK = 0.45      # the planted box of a row with another IoU threshold: the detection's left 45 % -- IoU 0.45 with it


def plant_min(row: Row) -> float:
    """pixels: a planted detection covers at least 4 x 4 of the score map (mask_roi_ref.PLANT_MIN is this at m = 2)"""
    return RR.PLANT_MIN * row.m / 2.0


def plant_detections(row: Row, batch, det, n=N_INSTANCES, shrink=1.0):
    """``mask_roi_ref.plant_detections`` with the two sides apart: the first ``n`` detections of each image that are at least
    ``plant_min`` pixels on both sides replace filled rows of true_boxes (the box) and true_masks (the box, filled), and the
    image's targets are assigned again.  The forward pass does not read the labels, so the net yields the same detections on the
    new batch, each planted one with IoU 1 (to rounding) with its row.  ``shrink`` < 1 plants the left part of the box only:
    the detection's IoU with its row is ``shrink``, between a threshold below it and the configured 0.5 (the planted part is
    half of ``plant_min`` wide at least).  Returns (the new batch, [(detection, row)] per image)."""
    H, W, C = row.H, row.W, row.C
    anchors = anchors_of(row)
    norm = np.asarray([W, H, W, H], np.float32)
    b = dict(batch)
    tb = batch["true_boxes"].numpy().copy()
    tm = np.array(batch["true_masks"], copy=True)
    ys = [batch[k].numpy().copy() for k in ("yolo3", "yolo2", "yolo1")]
    planted = []
    side = plant_min(row)
    side_x = side if shrink == 1.0 else side / 2
    for i in range(tb.shape[0]):
        rows = [r for r in range(tb.shape[4]) if np.abs(tb[i, 0, 0, 0, r, :4]).sum() != 0]
        d = np.asarray(det[i], np.float32)
        big = [q for q in range(len(d)) if (d[q, 2] - d[q, 0]) * H >= side and (d[q, 3] - d[q, 1]) * W * shrink >= side_x][:n]
        for q, r in zip(big, rows):
            y1, x1, y2, x2 = d[q, :4]
            x2 = x1 + np.float32(shrink) * (x2 - x1)
            tb[i, 0, 0, 0, r, :4] = [(x1 + x2) / np.float32(2), (y1 + y2) / np.float32(2), x2 - x1, y2 - y1]
            tm[i, r] = False
            tm[i, r, max(int(np.floor(y1 * H)), 0):int(np.ceil(y2 * H)), max(int(np.floor(x1 * W)), 0):int(np.ceil(x2 * W))] = True
        planted.append(list(zip(big, rows)))
        boxes = tb[i, 0, 0, 0, rows, :4] * norm
        for dst, t in zip(ys, RECT.assign_targets(boxes.astype(np.float32), tb[i, 0, 0, 0, rows, 4].astype(np.int64), H, W,
                                                  anchors=anchors, num_class=C)):
            t[..., 0:4] /= norm
            dst[i] = t
    b["true_boxes"], b["true_masks"] = torch.from_numpy(tb), tm
    b["yolo3"], b["yolo2"], b["yolo1"] = (torch.from_numpy(y) for y in ys)
    return b, planted


def needs_plants(row: Row) -> bool:
    """detections-only rows (every positive is a planted detection) and rows with another IoU threshold (three detections
    whose best IoU lies between the row's threshold and the configured one)"""
    return row.rois[1] == 0 or row.rois[2] != cfg.MASK_ROI_IOU


def with_perms(row: Row, batch, planted=None, seed=0):
    """injected permutations of D and G entries.  On a row that plants detections they come first in perm_det, so that the
    n_det picked ones hold them whatever D is"""
    rng = np.random.RandomState(seed)
    b = dict(batch)
    pd, pg = [], []
    for i in range(row.B):
        p = [int(v) for v in rng.permutation(row.D)]
        if planted is not None:
            first = [int(q) for q, _ in planted[i]]
            p = first + [v for v in p if v not in first]
        pd.append(p)
        pg.append([int(v) for v in rng.permutation(row.G)])
    b["perm_det"], b["perm_gt"] = np.asarray(pd, np.int32), np.asarray(pg, np.int32)
    return b, [(b["perm_det"][i], b["perm_gt"][i]) for i in range(row.B)]


def row_batch(row: Row, det_of=None, seed=None):
    """(batch, perms, planted) of the row.  ``det_of(batch)``: the training-mode detections [B, D, 6] of the net under test on
    the batch's images (the oracle's on the CPU, a first pass of the same net on the GPU); called on the rows that plant
    detections (``needs_plants``), with the batch before planting"""
    b = bare_batch(row, seed)
    planted = None
    if needs_plants(row):
        assert det_of is not None, "%s plants detections: pass det_of" % row.name
        if row.rois[1] == 0:
            b, planted = plant_detections(row, b, det_of(b))
        else:
            b, planted = plant_detections(row, b, det_of(b), n=3, shrink=PLANT_SHRINK)
    b, perms = with_perms(row, b, planted)
    return b, perms, planted


def infer_batch(row: Row, seed=3):
    """the inference tests' batch: other images, a clip window of its own on the last image"""
    b = bare_batch(row, seed)
    b["clip_window"][-1] = [0.1, 0.05, 0.9, 0.8]
    return b


# ------------------------------------------------------------------------------------------------ the composed oracle
def oracle_forward(row: Row, params, images, is_training=True, updates=None, taps=None, force=None, quant=O.bf16_ste):
    return MR.build_network(params, images, is_training, lock_of_row(row), row.m, row.k, updates, taps, quant, force)


def oracle_detections(row: Row, yolos, window, obj_thresh, nms=None, D=None, anchors=None):
    """the oracle's filter on head logits, with the row's anchors, D and mode unless given"""
    pred = O.interpret_output([y.detach() for y in yolos], anchors=anchors_of(row) if anchors is None else anchors)
    return NR.filter_detections(pred[2], pred[3], pred[5], np.asarray(window, np.float32), obj_thresh, O.IOU_THRESHOLD,
                                row.D if D is None else D, row.nms if nms is None else nms)


def oracle_losses(row: Row, params, yolos, mask_pos, batch, perms, obj_thresh=DET_THRESH, nms=None, D=None, anchors=None,
                  rois=None):
    """the loss parts on the forward pass's outputs, composed of what exists: O.interpret_output(anchors=),
    nms_modes_ref.filter_detections(mode=, max_detection=), O.loss_yolo, mask_roi_ref.loss_mask(n_det, n_gt, iou, perms, k) and
    the l2 term over mask_stride_ref.regularized_names.  The keywords replace one option of the row (the CPU test's
    "every option bites")"""
    anchors = anchors_of(row) if anchors is None else anchors
    n_det, n_gt, iou = row.rois if rois is None else rois
    pred = O.interpret_output(yolos, anchors=anchors)
    with torch.no_grad():
        det = oracle_detections(row, yolos, batch["clip_window"], obj_thresh, nms, D, anchors)
    ly = O.loss_yolo(pred, batch["true_boxes"], [batch["yolo3"], batch["yolo2"], batch["yolo1"]])
    tb = batch["true_boxes"].detach().numpy()[:, 0, 0, 0]
    lm = RR.loss_mask(det, mask_pos, tb, batch["true_masks"], n_det, n_gt, iou, perms, row.k)
    reg = None
    for n in MR.regularized_names(params, lock_of_row(row)):
        t = O.L2_WEIGHT * 0.5 * (params[n] ** 2).sum()
        reg = t if reg is None else reg + t
    parts = dict(ly)
    parts["mask"] = lm
    parts["reg"] = reg
    parts["total"] = ly["conf"] + ly["class"] + ly["coord"] + lm + reg
    return parts, det


def oracle_total_loss(row: Row, params, batch, perms, updates=None, taps=None, force=None, quant=O.bf16_ste):
    """(parts, detections, head logits, score maps) of the row's training step"""
    yolos, mask_pos = oracle_forward(row, params, batch["images"], True, updates, taps, force, quant)
    parts, det = oracle_losses(row, params, yolos, mask_pos, batch, perms)
    return parts, det, yolos, mask_pos


def positives(row: Row, det, batch, perms, rois=None):
    """per image: the number of positive RoIs of the reference's selection"""
    n_det, n_gt, iou = row.rois if rois is None else rois
    Hm, Wm = row.H // row.m, row.W // row.m
    r, _ = RR.rows(det, batch["true_boxes"].numpy()[:, 0, 0, 0], perms, Hm, Wm, row.k, n_det, n_gt, iou)
    return [len(x) for x in r]

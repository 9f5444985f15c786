"""CPU restatement of the detection filter's three NMS modes (filter_detections, yolo/yolo3_net_pos.py:517-628), built on the
oracle's own interpret_output / clip_boxes / _tf_iou / non_max_suppression:

* ``"per_class"``: Method 1 (:564-592) -- what ``O.filter_detections`` computes (tests/test_nms_modes.py holds the two equal);
* ``"agnostic"``: Method 2 (:594-605) -- ONE greedy NMS over all candidates above the threshold, whatever their class;
* ``"none"``: nms=False (:518, 585) -- the max_detection highest scores.

All modes share everything up to and including ``score > obj_thresh`` on the clipped boxes (:558) and the output: rows
(y1, x1, y2, x2, classid, score) in tf.nn.top_k order (score descending, ties to the lower candidate index), zero padded.

Two entry points: ``filter_detections`` decodes logits like the oracle; ``select`` works on decoded (boxes, scores, classes) of
one image -- what the GPU tests read back from the decode kernel's workspace, so that their comparison is exact.  ``select``
runs the greedy loop with the IoU of the winner against ALL remaining candidates at once in numpy f32 (``iou_many``, the
operation order of ``O._tf_iou``): the oracle's pure-Python loop is too slow for an image-wide list of 20,000."""
import numpy as np
import torch

import disyolo_oracle as O

MODES = ("per_class", "agnostic", "none")


def iou_many(box, boxes):
    """O._tf_iou(box, boxes[j]) for every j, f32, operation by operation"""
    f = np.float32
    boxes = np.asarray(boxes, f).reshape(-1, 4)
    box = np.asarray(box, f)
    ya1, xa1 = np.minimum(box[0], box[2]), np.minimum(box[1], box[3])
    ya2, xa2 = np.maximum(box[0], box[2]), np.maximum(box[1], box[3])
    yb1, xb1 = np.minimum(boxes[:, 0], boxes[:, 2]), np.minimum(boxes[:, 1], boxes[:, 3])
    yb2, xb2 = np.maximum(boxes[:, 0], boxes[:, 2]), np.maximum(boxes[:, 1], boxes[:, 3])
    area_a = f(f(ya2 - ya1) * f(xa2 - xa1))
    area_b = ((yb2 - yb1).astype(f) * (xb2 - xb1).astype(f)).astype(f)
    iy1, ix1 = np.maximum(ya1, yb1), np.maximum(xa1, xb1)
    iy2, ix2 = np.minimum(ya2, yb2), np.minimum(xa2, xb2)
    inter = (np.maximum((iy2 - iy1).astype(f), f(0)) * np.maximum((ix2 - ix1).astype(f), f(0))).astype(f)
    with np.errstate(divide="ignore", invalid="ignore"):
        iou = (inter / ((area_a + area_b).astype(f) - inter).astype(f)).astype(f)
    return np.where((area_a <= 0) | (area_b <= 0), f(0), iou)


def greedy(boxes, scores, max_out, iou_thresh):
    """O.non_max_suppression: positions into (boxes, scores) in selection order.  ``iou_thresh`` None: no suppression."""
    scores = np.asarray(scores, np.float32)
    order = np.lexsort((np.arange(len(scores)), -scores.astype(np.float64)))      # score descending, ties: lower index
    boxes = np.asarray(boxes, np.float32).reshape(-1, 4)[order]
    alive = np.ones(len(order), bool)
    thr = None if iou_thresh is None else np.float32(iou_thresh)                    # the kernel compares in f32
    keep, at = [], 0
    while len(keep) < max_out:
        rest = np.flatnonzero(alive[at:])
        if not len(rest):
            break
        at += int(rest[0])
        keep.append(int(order[at]))
        alive[at] = False
        if thr is not None:
            alive[at:] &= ~(iou_many(boxes[at], boxes[at:]) > thr)
        at += 1
    return keep


def select(boxes, scores, classes, obj_thresh, nms_thresh, max_detection, mode):
    """candidate indices of one image's detections in output order, from its decoded candidates"""
    assert mode in MODES
    scores = np.asarray(scores, np.float32)
    keep = np.where(scores > np.float32(obj_thresh))[0]                             # :558
    if mode == "per_class":
        nms_keep = []
        for c in np.unique(classes[keep]):                                          # :565-589
            ixs = keep[classes[keep] == c]
            nms_keep.extend(int(ixs[q]) for q in greedy(boxes[ixs], scores[ixs], max_detection, nms_thresh))
        kept = np.array(sorted(set(nms_keep)), dtype=np.int64)                      # :590-592 ascending ids
        order = np.lexsort((np.arange(len(kept)), -scores[kept].astype(np.float64)))[:max_detection]   # :608-612
        return [int(kept[q]) for q in order]
    # one list per image: the selection order already is the top_k order
    sel = greedy(boxes[keep], scores[keep], max_detection, nms_thresh if mode == "agnostic" else None)
    return [int(keep[q]) for q in sel]


def rows_of(boxes, scores, classes, idx, max_detection):
    out = np.zeros((max_detection, 6), np.float32)
    for r, i in enumerate(idx):
        out[r, :4] = boxes[i]
        out[r, 4] = np.float32(classes[i])
        out[r, 5] = scores[i]
    return out


def select_slow(boxes, scores, classes, obj_thresh, nms_thresh, max_detection, mode):
    """``select`` through the oracle's own pure-Python non_max_suppression (small lists only): holds ``greedy`` to it"""
    keep = np.where(np.asarray(scores, np.float32) > np.float32(obj_thresh))[0]
    if mode == "none":
        order = sorted(range(len(keep)), key=lambda q: (-float(scores[keep[q]]), q))[:max_detection]
        return [int(keep[q]) for q in order]
    assert mode == "agnostic"
    return [int(keep[q]) for q in O.non_max_suppression(boxes[keep], scores[keep], max_detection, float(np.float32(nms_thresh)))]


def decode(conf_logit, class_logit, pred_norm_coord, window, i):
    """image i's candidates as O.filter_detections forms them (:527-555): clipped boxes, scores, arg-max classes"""
    confs, clss, boxes = [], [], []
    for j in (0, 1, 2):
        confs.append(torch.sigmoid(conf_logit[j][i].detach().float()).reshape(-1))
        clss.append(torch.softmax(class_logit[j][i].detach().float(), dim=-1).reshape(-1, class_logit[j].shape[-1]))
        boxes.append(pred_norm_coord[j][i].detach().float().reshape(-1, 4))
    pred_conf, pred_class, box = torch.cat(confs).numpy(), torch.cat(clss).numpy(), torch.cat(boxes).numpy()
    classid = np.argmax(pred_class, axis=-1).astype(np.int32)
    score = (pred_conf * pred_class[np.arange(pred_class.shape[0]), classid]).astype(np.float32)
    xc, yc, w, h = box[:, 0], box[:, 1], box[:, 2], box[:, 3]
    half = np.float32(2.0)
    yxyx = np.stack([yc - h / half, xc - w / half, yc + h / half, xc + w / half], axis=-1).astype(np.float32)
    return O.clip_boxes(yxyx, np.asarray(window, dtype=np.float32)), score, classid


def filter_detections(conf_logit, class_logit, pred_norm_coord, batch_window, obj_thresh=O.OBJ_THRESHOLD,
                      nms_thresh=O.IOU_THRESHOLD, max_detection=O.MAX_DETECTION, mode="per_class"):
    """O.filter_detections with the NMS mode: float32 [B, max_detection, 6]"""
    B = conf_logit[0].shape[0]
    out = np.zeros((B, max_detection, 6), np.float32)
    for i in range(B):
        boxes, scores, classes = decode(conf_logit, class_logit, pred_norm_coord, batch_window[i], i)
        idx = select(boxes, scores, classes, obj_thresh, nms_thresh, max_detection, mode)
        out[i] = rows_of(boxes, scores, classes, idx, max_detection)
    return out


def filter_logits(ys, window, obj_thresh, nms_thresh, max_detection, mode, anchors=None):
    """the filter on raw head logits [B,g,g,3,5+C] x 3"""
    pred = O.interpret_output(ys) if anchors is None else O.interpret_output(ys, anchors=anchors)
    return filter_detections(pred[2], pred[3], pred[5], np.asarray(window, np.float32), obj_thresh, nms_thresh, max_detection, mode)


# ---- hand cases in the style of tests/test_gpu_kat.py: S = 64 (grids 8 / 4 / 2), dyadic anchors, logits 0 / +-40, so every
#      box coordinate and every score is exact in f32 on both sides
KAT_S = 64
KAT_ANCH = np.array([[16, 16], [32, 32], [8, 24],        # 8-grid
                     [32, 32], [16, 48], [48, 16],       # 4-grid
                     [32, 32], [64, 32], [32, 64]], np.float32)


def blank_logits(B):
    """conf logit -40 everywhere: sigmoid = 4e-18, far below any threshold"""
    ys = [torch.zeros(B, g, g, 3, 8) for g in (8, 4, 2)]
    for y in ys:
        y[..., 4] = -40.0
    return ys


def put(y, b, cy, cx, a, cls, conf=0.0):
    """a candidate with score sigmoid(conf) * 1.0 exactly (class margin 40 -> softmax max == 1.0f), centred in its cell, anchor-sized"""
    y[b, cy, cx, a, :4] = 0.0
    y[b, cy, cx, a, 4] = conf
    y[b, cy, cx, a, 5:] = 0.0
    y[b, cy, cx, a, 5 + cls] = 40.0


def pair_one_cell_apart(cls_a, cls_b):
    """two 0.5 x 0.5 boxes, centres one 4-grid cell apart (inter .125, union .375: IoU = 1/3 in f32), scores sigmoid(2) and
    sigmoid(1)"""
    ys = blank_logits(1)
    put(ys[1], 0, 1, 1, 0, cls=cls_a, conf=2.0)
    put(ys[1], 0, 1, 2, 0, cls=cls_b, conf=1.0)
    return ys


THIRD = float(np.float32(0.125) / np.float32(0.375))

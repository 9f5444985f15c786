"""The reference's m = 1/4 and m = 1 mask subnets (yolo/yolo3_net_pos.py:361-378, 414-461), restated in float64 on top of
the oracle, whose build_network is fixed to the active m = 1/2 subnet (:380-412).

The backbone and the three heads come from O.build_network itself; its m = 1/2 tail runs on stand-in variables (the shapes
of the m = 1/2 layers it needs) and is thrown away.  The variant's own layers are applied with O.conv_bn, O.conv_lin and
O.upsample2 to the oracle's taps (act1, act73 / act78 / act81), straight-through forced like the oracle's own taps."""
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

import disyolo_oracle as O

# (idx, cin, cout, ksize, stride, kind, src, src_up) of the layers from conv76 on, read off the reference's text
MASK_LAYERS = {
    4: [(76, 128, 64, 1, 1, "bn", 73, None),           # :362-364
        (77, 192, 64, 1, 1, "bn", 9, 76),              # :366-372 [skip3, up2(act76)]
        (78, 64, 128, 3, 1, "bn", 77, None),           # :373-375
        (79, 128, None, 1, 1, "lin", 78, None)],       # :376-378, k^2 score maps at S/4
    2: [(76, 128, 64, 1, 1, "bn", 73, None),
        (77, 192, 64, 1, 1, "bn", 9, 76),
        (78, 64, 128, 3, 1, "bn", 77, None),
        (79, 128, 32, 1, 1, "bn", 78, None),
        (80, 96, 32, 1, 1, "bn", 4, 79),
        (81, 32, 64, 3, 1, "bn", 80, None),
        (82, 64, None, 1, 1, "lin", 81, None)],
    1: [(76, 128, 64, 1, 1, "bn", 73, None),           # :415-431 as m = 1/2
        (77, 192, 64, 1, 1, "bn", 9, 76),
        (78, 64, 128, 3, 1, "bn", 77, None),
        (79, 128, 32, 1, 1, "bn", 78, None),
        (80, 96, 32, 1, 1, "bn", 4, 79),
        (81, 32, 64, 3, 1, "bn", 80, None),
        (82, 64, 16, 1, 1, "bn", 81, None),            # :449-451
        (83, 48, 16, 1, 1, "bn", 1, 82),               # :453-459 [skip1, up2(act82)]
        (84, 16, 32, 3, 1, "bn", 83, None),
        (85, 32, None, 1, 1, "lin", 84, None)],         # :460-461, k^2 score maps at S
}
SCORE_LAYER = {4: 79, 2: 82, 1: 85}


def mask_layers(mask_stride: int, k: int) -> List[Tuple]:
    return [(i, cin, cout if cout is not None else k * k, ks, s, kind, src, up)
            for (i, cin, cout, ks, s, kind, src, up) in MASK_LAYERS[mask_stride]]


def variable_shapes(mask_stride: int, k: int) -> Dict[str, tuple]:
    """name -> shape of every variable: the oracle's for conv1-75, the table's for the mask subnet"""
    base = {n: tuple(t.shape) for n, t in O.init_params(k=k, lock=O.default_lock(1)).items()
            if int(n.split("convolutional")[1].split("/")[0]) <= 75}
    for (i, cin, cout, ks, _, kind, _, _) in mask_layers(mask_stride, k):
        base[O._name(i, "weights")] = (ks, ks, cin, cout)
        leaves = ("biases",) if kind == "lin" else ("BatchNorm/gamma", "BatchNorm/beta", "BatchNorm/moving_mean",
                                                   "BatchNorm/moving_variance")
        for leaf in leaves:
            base[O._name(i, leaf)] = (cout,)
    return base


def default_lock(stage: int, mask_stride: int) -> Dict[int, bool]:
    return {i: (stage == 1 and i <= 52) for i in range(1, SCORE_LAYER[mask_stride] + 1)}


def regularized_names(params: Dict[str, torch.Tensor], lock: Dict[int, bool]) -> List[str]:
    """l2_regularizer(1e-4) (:38,120,123,140): weights of every unlocked conv, biases of the four linear convs (59 / 67 / 75
    and the variant's score layer)"""
    out = []
    for n in params:
        i = int(n.split("convolutional")[1].split("/")[0])
        if not lock[i] and (n.endswith("/weights") or n.endswith("/biases")):
            out.append(n)
    return out


def _layer(n: str) -> int:
    return int(n.split("convolutional")[1].split("/")[0])


def build_network(params, images, is_training, lock, mask_stride: int, k: int, updates=None, taps=None, quant=None,
                  force=None):
    """(yolos, mask_pos) of the variant; ``taps`` / ``force`` as O.build_network (act{i} of every layer of the variant)"""
    if mask_stride == 2:
        return O.build_network(params, images, is_training, lock, updates, taps, quant, force)
    # stand-ins for the m = 1/2 layers the oracle runs that this variant lacks or shapes differently
    first_stand_in = 79 if mask_stride == 4 else 82
    stand = O.init_params(k=k, lock={i: False for i in range(1, 83)})
    base = {n: t for n, t in params.items() if _layer(n) < first_stand_in}
    dtype = next(iter(params.values())).dtype
    base.update({n: t.to(dtype) for n, t in stand.items() if _layer(n) >= first_stand_in})
    lock82 = {i: lock.get(i, False) for i in range(1, 83)}
    tp: Dict[str, torch.Tensor] = {}
    up: Dict[str, torch.Tensor] = {}
    force_base = None if force is None else {n: v for n, v in force.items() if _layer_of_tap(n) < first_stand_in}
    yolos, _ = O.build_network(base, images, is_training, lock82, up if updates is not None else None, tp, quant,
                               force_base)
    if updates is not None:
        updates.update({n: v for n, v in up.items() if _layer(n) < first_stand_in})

    def forced(name):
        t = tp[name]
        if force is not None and name in force:
            t = t + (force[name].to(t.dtype) - t).detach()
        return t

    def tap(name, t, score=False):
        if quant is not None and not score:
            t = quant(t)
        tp[name] = t
        return forced(name)

    cb = lambda x, i: O.conv_bn(x, params, i, 1, lock[i], is_training, updates, quant=quant)
    if mask_stride == 4:
        mask_pos = tap("act79", O.conv_lin(forced("act78"), params, 79, quant), score=True)
    else:
        net = tap("act82", cb(forced("act81"), 82))
        net = torch.cat([forced("act1"), O.upsample2(net)], dim=-1)          # :455-456 [skip1, up]
        net = tap("act83", cb(net, 83))
        net = tap("act84", cb(net, 84))
        mask_pos = tap("act85", O.conv_lin(net, params, 85, quant), score=True)
    if taps is not None:
        taps.update({n: t for n, t in tp.items() if _layer_of_tap(n) < first_stand_in or n in _variant_taps(mask_stride)})
    return yolos, mask_pos


def _layer_of_tap(name: str) -> int:
    return int(name[3:])


def _variant_taps(mask_stride: int):
    return {4: ("act79",), 1: ("act82", "act83", "act84", "act85")}[mask_stride]


def loss_mask(detections, mask_pos, true_boxes, true_masks, perms, k: int):
    """O.loss_mask (:750-860) on a k x k grid; the GT masks are sampled at [::S/size, ::S/size] as there"""
    if k == 3:
        return O.loss_mask(detections, mask_pos, true_boxes, true_masks, perms)
    B, size = mask_pos.shape[0], mask_pos.shape[1]
    total = torch.zeros((), dtype=mask_pos.dtype)
    for i in range(B):
        pd, pg = perms[i] if perms is not None else (None, None)
        pos, assign, gt_rows = O.select_mask_rois(detections[i], true_boxes[i, 0, 0, 0], pd, pg)
        if len(pos) == 0:
            continue
        step = true_masks.shape[2] // size
        gt_small = true_masks[i][gt_rows][:, ::step, ::step].astype(np.float32)
        px = np.round(pos * np.float32(size))
        per_roi = []
        for r in range(len(px)):
            logits, mobj = O.assemble_logits(mask_pos[i], px[r], k)
            gtm = torch.from_numpy(gt_small[assign[r]]).to(mask_pos.dtype)
            per_roi.append((mobj * O.sigmoid_ce(gtm, logits)).sum() / mobj.sum())
        total = total + O.MASK_SCALE * torch.stack(per_roi).mean()
    return total / B


def total_loss(params, batch, lock, mask_stride: int, k: int, perms=None, updates=None, obj_thresh=O.OBJ_THRESHOLD,
               quant=None, taps=None, force=None):
    """O.total_loss (:47-61) with the variant's mask subnet and its L2 set"""
    yolos, mask_pos = build_network(params, batch["images"], True, lock, mask_stride, k, updates, taps, quant, force)
    pred = O.interpret_output(yolos)
    with torch.no_grad():
        det = O.filter_detections(pred[2], pred[3], pred[5], batch["clip_window"], obj_thresh)
    ly = O.loss_yolo(pred, batch["true_boxes"], [batch["yolo3"], batch["yolo2"], batch["yolo1"]])
    lm = loss_mask(det, mask_pos, batch["true_boxes"].detach().numpy(), batch["true_masks"], perms, k)
    reg = None
    for n in regularized_names(params, lock):
        t = O.L2_WEIGHT * 0.5 * (params[n] ** 2).sum()
        reg = t if reg is None else reg + t
    parts = dict(ly)
    parts["mask"] = lm
    parts["reg"] = reg
    parts["total"] = ly["conf"] + ly["class"] + ly["coord"] + lm + reg
    return parts, det, yolos, mask_pos

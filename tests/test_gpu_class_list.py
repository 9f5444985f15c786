"""Class lists of 1 to 80 classes on the GPU: the wide YOLO loss against the float64 oracle, the bucketed detection filter
against the oracle's filter (known answers, more than 512 survivors, long / short / tied lists, the 80-term decode), the
n-label confusion counts, whole training steps and ``evaluate`` with other class lists than the configured three.

Helpers come from the test modules that own them (test_gpu_loss, test_gpu_lock_map, test_gpu_eval_batch)."""
import numpy as np
import pytest
import torch

import disyolo_oracle as O
from disyolo_amd import config as cfg
from disyolo_amd import evaluate as E
from disyolo_amd import lib as L
from disyolo_amd.net import YOLONet
from disyolo_amd.postprocess import SegmentationAccuracy, paste_detections
from disyolo_amd.synth import synthetic_batch
from disyolo_amd.voc_eval import voc_eval
from test_gpu_eval_batch import randomize_heads
from test_gpu_lock_map import _same_state, make_net, oracle_params, rel_err
from test_gpu_loss import ANCH as ANCH_CFG, bits, check_yolo_outputs, check_yolo_preconditions, yolo_case

pytestmark = pytest.mark.gpu


def names(n):
    return ["class%02d" % i for i in range(n)]


# ------------------------------------------------------------------------------------------------ the wide YOLO loss
_CASES = {}


def wide_case(C):
    """B = 3, S = 96, seed 10 + C: computed once per class count and left unchanged"""
    if C not in _CASES:
        heads, labels, tb = yolo_case(3, 96, C, cfg.MAX_BOX_PER_IMAGE, 10 + C, cfg.IGNORE_THRESH)
        check_yolo_preconditions(heads, labels, tb, cfg.IGNORE_THRESH)
        _CASES[C] = (heads, labels, tb)
    return _CASES[C]


def run_wide(dev, heads, labels, tb, S, C, ld):
    B, G = tb.shape[0], tb.shape[1]
    lg = [torch.from_numpy(h).to(dev).contiguous() for h in heads]
    lb = [torch.from_numpy(l).to(dev).contiguous() for l in labels]
    dl = [torch.full((B, h.shape[1], h.shape[2], ld), float("nan"), dtype=torch.bfloat16, device=dev) for h in heads]
    losses = torch.full((8,), float("nan"), device=dev)
    scales = (O.OBJECT_SCALE, O.NOOBJECT_SCALE, O.CLASS_SCALE, O.COORD_SCALE)
    L.yolo_loss_wide(lg, lb, torch.from_numpy(tb).to(dev).contiguous(), G, B, S, C, ld, ANCH_CFG.reshape(-1),
                     cfg.IGNORE_THRESH, scales, dl, losses, L.Workspace(dev))
    torch.cuda.synchronize()
    return losses.cpu(), [d.cpu() for d in dl]


@pytest.mark.parametrize("C,ld", [(6, 64), (11, 64), (12, 64), (27, 96), (80, 256), (6, 128)])
def test_wide_yolo_loss_matches_f64_oracle(dev, C, ld):
    """row widths 11 (the first past the 32-channel entry), 16 and 17 (either side of the old per-thread array), 32 (3 D = 96:
    no pad channel), 85 (3 D = 255: one pad channel), each at its minimal pitch, and 11 again at pitch 128: the pitch is an
    argument.  The bounds are those of tests/test_gpu_loss.py (loss terms rtol 2e-5, gradients 2^-8 |want| + 1e-6 max)."""
    heads, labels, tb = wide_case(C)
    assert 3 * (5 + C) <= ld and (ld == 128 or ld - 32 < 3 * (5 + C))
    losses, dl = run_wide(dev, heads, labels, tb, 96, C, ld)
    assert all(d.shape[-1] == ld for d in dl)
    # (check_yolo_outputs takes the maximum over the pad channels: a row without any gets one zero channel appended for it)
    shown = dl if ld > 3 * (5 + C) else [torch.cat([d, torch.zeros_like(d[..., :1])], -1) for d in dl]
    want = check_yolo_outputs(losses, shown, heads, labels, tb, "wide C=%d ld=%d" % (C, ld))
    assert (want[:5] > 0).all()
    losses2, dl2 = run_wide(dev, heads, labels, tb, 96, C, ld)
    assert torch.equal(bits(losses), bits(losses2))
    for d, d2 in zip(dl, dl2):
        assert torch.equal(bits(d), bits(d2))


# ------------------------------------------------------------------------------------------------ the filter: known answers
S = 64                                   # grids 8 / 4 / 2: cell centres and anchor/S are dyadic (tests/test_gpu_kat.py)
ANCH = np.array([[16, 16], [32, 32], [8, 24], [32, 32], [16, 48], [48, 16], [32, 32], [64, 32], [32, 64]], np.float32)


def blank_logits(B, C, grids=(8, 4, 2)):
    """conf logit -40 everywhere: sigmoid = 4e-18, far below any threshold"""
    ys = [torch.zeros(B, g, g, 3, 5 + C) for g in grids]
    for y in ys:
        y[..., 4] = -40.0
    return ys


def put(y, b, cy, cx, a, cls, conf=0.0):
    """a candidate with score sigmoid(conf) * 1.0 exactly (class margin 40 -> softmax max == 1.0f at any class count)"""
    y[b, cy, cx, a, :4] = 0.0
    y[b, cy, cx, a, 4] = conf
    y[b, cy, cx, a, 5:] = 0.0
    y[b, cy, cx, a, 5 + cls] = 40.0


def run_detect(dev, ys, C, window, thr, nms_thr, max_det=cfg.MAX_DETECTION, size=S, anchors=ANCH, oracle_max_det=None):
    B = ys[0].shape[0]
    det = torch.full((B, max_det, 6), float("nan"), device=dev)
    cnt = torch.full((B,), -7, dtype=torch.int32, device=dev)
    logits = [y.reshape(B, y.shape[1], y.shape[2], 3 * (5 + C)).contiguous().to(dev) for y in ys]
    ws = L.Workspace(dev)
    L.detect(logits[0], logits[1], logits[2], B, size, C, anchors.reshape(-1), torch.as_tensor(window, device=dev).float(),
             float(thr), float(nms_thr), max_det, det, cnt, ws)
    torch.cuda.synchronize()
    pred = O.interpret_output(ys, anchors=anchors)
    want = O.filter_detections(pred[2], pred[3], pred[5], np.asarray(window, np.float32), thr, nms_thr,
                               oracle_max_det or max_det)
    return det.cpu().numpy(), cnt.cpu().numpy(), want


@pytest.mark.parametrize("C", [17, 80])
def test_filter_score_exactly_at_threshold_is_dropped(dev, C):
    ys = blank_logits(1, C)
    put(ys[1], 0, 1, 1, 0, cls=C - 1)                 # score = 0.5 exactly
    win = [[0, 0, 1, 1]]
    got, cnt, want = run_detect(dev, ys, C, win, 0.5, 0.3)
    assert (want == 0).all() and cnt[0] == 0          # strict '>'
    np.testing.assert_array_equal(got, want)
    below = float(np.nextafter(np.float32(0.5), np.float32(0)))
    got, cnt, want = run_detect(dev, ys, C, win, below, 0.3)
    assert cnt[0] == 1 and want[0, 0, 5] == 0.5 and want[0, 0, 4] == C - 1
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got[0, 0, :4], np.float32([0.125, 0.125, 0.625, 0.625]))


@pytest.mark.parametrize("C", [17, 80])
def test_filter_iou_exactly_at_threshold_and_other_classes(dev, C):
    # two 0.5 x 0.5 boxes, centres one 4-grid cell apart: inter .125, union .375 -> IoU = 1/3 in f32
    ys = blank_logits(1, C)
    put(ys[1], 0, 1, 1, 0, cls=16, conf=2.0)
    put(ys[1], 0, 1, 2, 0, cls=16, conf=1.0)
    win = [[0, 0, 1, 1]]
    third = float(np.float32(0.125) / np.float32(0.375))
    got, cnt, want = run_detect(dev, ys, C, win, 0.25, third)
    assert cnt[0] == 2                                # IoU > thr is false at equality
    np.testing.assert_array_equal(got, want)
    got, cnt, want = run_detect(dev, ys, C, win, 0.25, float(np.nextafter(np.float32(third), np.float32(0))))
    assert cnt[0] == 1 and (want[0, 0, 5] > 0.8)
    np.testing.assert_array_equal(got, want)
    # a different class is never suppressed by it
    put(ys[1], 0, 1, 2, 0, cls=0, conf=1.0)
    got, cnt, want = run_detect(dev, ys, C, win, 0.25, 0.1)
    assert cnt[0] == 2
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("C", [17, 80])
def test_filter_equal_scores_across_classes_and_scales_keep_candidate_order(dev, C):
    top = min(17, C - 1)
    ys = blank_logits(2, C)
    # image 0: two overlapping equal-score boxes of one class -> the first in candidate order survives
    put(ys[1], 0, 2, 1, 0, cls=top, conf=1.0)
    put(ys[1], 0, 2, 2, 0, cls=top, conf=1.0)
    # image 1: equal-score boxes far apart on three scales, classes 0, 16, 17 (16 at C = 17) and C - 1 all present
    put(ys[2], 1, 0, 0, 0, cls=16, conf=1.0)
    put(ys[0], 1, 6, 6, 0, cls=C - 1, conf=1.0)
    put(ys[0], 1, 1, 6, 0, cls=0, conf=1.0)
    put(ys[1], 1, 3, 0, 0, cls=top, conf=1.0)
    put(ys[0], 1, 3, 6, 0, cls=C - 1, conf=2.0)          # (touches none of the others)
    win = [[0, 0, 1, 1], [0, 0, 1, 1]]
    got, cnt, want = run_detect(dev, ys, C, win, 0.25, 0.2)
    assert list(cnt) == [1, 5]
    np.testing.assert_array_equal(got, want)
    assert want[0, 0, 3] == np.float32(0.625)          # the x = 1 cell's box won
    # image 1: the higher score first, then candidate index order: 8-grid (1,6), 8-grid (6,6), 4-grid, 2-grid
    np.testing.assert_array_equal(want[1, :5, 4], [C - 1, 0, C - 1, top, 16])


def test_filter_merges_more_than_512_survivors(dev):
    """576 disjoint boxes of 80 classes all survive their class's NMS (more than the 512 the old merge holds in LDS); the
    output is the top 30 by score, ties by candidate index; the second image is empty"""
    C, size = 80, 192
    anchors = ANCH.copy()
    anchors[0] = [8, 8]                                # anchor 0 of the 24-grid: a box the size of its cell
    ys = blank_logits(2, C, grids=(24, 12, 6))
    for cy in range(24):
        for cx in range(24):
            put(ys[0], 0, cy, cx, 0, cls=(cy * 24 + cx) % 80, conf=float((cy * 24 + cx) % 5))
    win = [[0, 0, 1, 1], [0, 0, 1, 1]]
    _, _, all_kept = run_detect(dev, ys, C, win, 0.25, 0.3, size=size, anchors=anchors, oracle_max_det=600)
    assert int((all_kept[0, :, 5] > 0).sum()) == 576 and not all_kept[1].any()      # the precondition: nothing is suppressed
    got, cnt, want = run_detect(dev, ys, C, win, 0.25, 0.3, size=size, anchors=anchors)
    assert list(cnt) == [30, 0]
    np.testing.assert_array_equal(want, all_kept[:, :30])
    np.testing.assert_array_equal(got, want)


# ------------------------------------------------------------------------------------------------ the filter: long and short lists
def read_decode(ws, B, NC):
    raw = ws.buf.cpu().numpy()
    boxes = raw[:B * NC * 16].view(np.float32).reshape(B, NC, 4)
    scores = raw[B * NC * 16:B * NC * 20].view(np.float32).reshape(B, NC)
    classes = raw[B * NC * 20:B * NC * 24].view(np.int32).reshape(B, NC)
    return boxes, scores, classes


@pytest.mark.parametrize("case", ["balanced", "one_class", "sparse", "ties"])
def test_bucketed_filter_on_long_and_short_lists(dev, case):
    """the recipe of tests/test_gpu_kat.py::test_detect_greedy_nms_on_thousands_of_candidates on the path of more than 16
    classes (C = 20, 384^2: 9,072 candidates): the decode results are read back from the workspace prefix and the oracle's
    non_max_suppression + top-k merge is replayed on them, so any difference is a different bucketing / NMS / merge decision"""
    S_, B, C = 384, 1, 20
    g = torch.Generator().manual_seed({"balanced": 1, "one_class": 2, "sparse": 3, "ties": 4}[case])
    ys = [torch.randn(B, gs, gs, 3, 5 + C, generator=g) for gs in (48, 24, 12)]
    thr = 0.25
    for y in ys:
        y[..., 2:4] *= 0.5
        if case == "one_class":
            y[..., 4] += 6.0
            y[..., 5 + 7] += 10.0                 # nearly every candidate is class 7 and passes: > 8,192 in one segment
        elif case == "sparse":
            y[..., 4] -= 2.0
            y[..., 5 + 19] += 6.0                 # what passes is class 19 or 3: most classes stay empty
            y[..., 5 + 3] += 5.5
        elif case == "ties":
            y[..., 4] = torch.round(y[..., 4])               # few distinct scores: long runs of equal ones
            y[..., 5:] = torch.round(y[..., 5:]) * 40.0
        else:
            y[..., 4] += 1.5
            y[..., 5:] *= 3.0
    anchors = np.asarray(cfg.ANCHORS, np.float32).reshape(-1)
    win = torch.tensor([[0.1, 0.05, 0.9, 0.95]], device=dev)
    max_det = cfg.MAX_DETECTION
    nms_f32 = float(np.float32(cfg.IOU_THRESHOLD))     # the kernel compares in f32
    det = torch.full((B, max_det, 6), float("nan"), device=dev)
    cnt = torch.zeros(B, dtype=torch.int32, device=dev)
    logits = [y.reshape(B, y.shape[1], y.shape[2], 3 * (5 + C)).contiguous().to(dev) for y in ys]
    ws = L.Workspace(dev)
    L.detect(logits[0], logits[1], logits[2], B, S_, C, anchors, win, thr, cfg.IOU_THRESHOLD, max_det, det, cnt, ws)
    torch.cuda.synchronize()
    NC = 3 * (48 * 48 + 24 * 24 + 12 * 12)
    boxes, scores, classes = read_decode(ws, B, NC)
    want = np.zeros((B, max_det, 6), np.float32)
    sizes = np.zeros(C, np.int64)
    for b in range(B):
        keep = np.where(scores[b] > np.float32(thr))[0]
        kept = []
        for c in np.unique(classes[b][keep]):
            ixs = keep[classes[b][keep] == c]
            sizes[c] = len(ixs)
            order = np.lexsort((np.arange(len(ixs)), -scores[b][ixs].astype(np.float64)))
            sel = []
            for j in order:
                if len(sel) >= max_det:
                    break
                if all(O._tf_iou(boxes[b][ixs[j]], boxes[b][ixs[q]]) <= nms_f32 for q in sel):
                    sel.append(j)
            kept.extend(int(ixs[q]) for q in sel)
        kept = np.array(sorted(set(kept)), dtype=np.int64)
        order = sorted(range(len(kept)), key=lambda q: (-float(scores[b][kept[q]]), q))[:max_det]
        for r, q in enumerate(order):
            want[b, r, :4] = boxes[b][kept[q]]
            want[b, r, 4] = classes[b][kept[q]]
            want[b, r, 5] = scores[b][kept[q]]
        assert int(cnt[b]) == len(order)
    print(case, "candidates per class:", sizes.tolist())
    if case == "one_class":
        assert sizes.max() > 8192                         # the list in global memory
    elif case == "balanced":
        assert (sizes > 64).all() and sizes.max() <= 8192
    elif case == "ties":
        assert (sizes > 64).all() and len(np.unique(scores[0][scores[0] > np.float32(thr)])) < 64
    else:
        assert 0 < (sizes > 0).sum() <= C // 2 and sizes.max() < 1024
    np.testing.assert_array_equal(det.cpu().numpy(), want)


def test_decode_of_80_classes_matches_the_f32_softmax(dev):
    """scores / classes of the workspace prefix at C = 80 against the oracle's f32 softmax: the class exact wherever the top two
    class logits differ by more than 1e-3, the score within rtol 1e-5 (the 80-term sum may be ordered differently)"""
    C, B = 80, 2
    g = torch.Generator().manual_seed(80)
    ys = [torch.randn(B, gs, gs, 3, 5 + C, generator=g) * 2.0 for gs in (8, 4, 2)]
    det = torch.zeros(B, 30, 6, device=dev)
    cnt = torch.zeros(B, dtype=torch.int32, device=dev)
    logits = [y.reshape(B, y.shape[1], y.shape[2], 3 * (5 + C)).contiguous().to(dev) for y in ys]
    ws = L.Workspace(dev)
    win = torch.tensor([[0.0, 0.0, 1.0, 1.0]] * B, device=dev)
    L.detect(logits[0], logits[1], logits[2], B, S, C, ANCH.reshape(-1), win, 0.25, 0.3, 30, det, cnt, ws)
    torch.cuda.synchronize()
    NC = 3 * (64 + 16 + 4)
    _, scores, classes = read_decode(ws, B, NC)
    flat = torch.cat([y.reshape(B, -1, 5 + C) for y in ys], 1)
    want_sc = (torch.sigmoid(flat[..., 4]) * torch.softmax(flat[..., 5:], -1).max(-1).values).numpy()
    top2 = flat[..., 5:].topk(2, -1).values
    clear = ((top2[..., 0] - top2[..., 1]) > 1e-3).numpy()
    assert clear.mean() > 0.9
    np.testing.assert_array_equal(classes[clear], flat[..., 5:].argmax(-1).numpy()[clear])
    assert classes.min() >= 0 and classes.max() < C and len(np.unique(classes)) > 40
    np.testing.assert_allclose(scores, want_sc, rtol=1e-5, atol=0)


# ------------------------------------------------------------------------------------------------ confusion counts
@pytest.mark.parametrize("nlabel", [2, 4, 81])
def test_confusion_n_matches_bincount(dev, nlabel):
    rng = np.random.RandomState(nlabel)
    t = rng.randint(0, nlabel + 3, (257, 131)).astype(np.uint8)          # values up to nlabel + 2: the last three are ignored
    p = rng.randint(0, nlabel + 3, (257, 131)).astype(np.uint8)
    ok = (t < nlabel) & (p < nlabel)
    want = np.bincount(t[ok].astype(np.int64) * nlabel + p[ok], minlength=nlabel * nlabel)
    td, pd = torch.from_numpy(t).to(dev), torch.from_numpy(p).to(dev)
    conf = torch.zeros(nlabel * nlabel, dtype=torch.int64, device=dev)
    L.confusion_n(td, pd, conf, nlabel)
    np.testing.assert_array_equal(conf.cpu().numpy(), want)
    assert want.sum() == ok.sum() and (~ok).any()
    L.confusion_n(td, pd, conf, nlabel)
    np.testing.assert_array_equal(conf.cpu().numpy(), 2 * want)          # it adds
    if nlabel == 4:
        c16 = torch.zeros(16, dtype=torch.int64, device=dev)
        L.confusion16(td, pd, c16)
        np.testing.assert_array_equal(c16.cpu().numpy(), want)
    with pytest.raises(L.DisyoloError):
        L.confusion_n(td, pd, torch.zeros(16, dtype=torch.int64, device=dev), 5)


# ------------------------------------------------------------------------------------------------ whole steps
def class_batch(B, S_, seed, C):
    b = O.synthetic_batch(B, S_, seed=seed, num_class=C)
    rng = np.random.RandomState(0)
    b["perm_det"] = np.stack([rng.permutation(cfg.MAX_DETECTION) for _ in range(B)]).astype(np.int32)
    b["perm_gt"] = np.stack([rng.permutation(cfg.MAX_BOX_PER_IMAGE) for _ in range(B)]).astype(np.int32)
    return b, [(b["perm_det"][i], b["perm_gt"][i]) for i in range(B)]


@pytest.mark.parametrize("C", [1, 6, 80])
def test_train_step_with_a_class_list_matches_oracle(dev, C):
    """the recipe and bounds of tests/test_gpu_lock_map.py::test_train_step_with_a_holed_map_matches_oracle on the stage-1
    map with a class list of 1, 6 and 80 names: total loss within 1e-3, every trainable gradient within 3 % relative l2 (or
    1e-3 of the largest element)"""
    B, S_ = 2, 64
    lock = O.default_lock(1)
    net = make_net(dev, None, B=B, S=S_, seed=1, classes=names(C))
    assert net.num_class == C and net.by_idx[59].cout == 3 * (5 + C)
    net.fuse_first_two = net.fuse_blocks = False
    b, perms = class_batch(B, S_, 11, C)
    p0 = oracle_params(net)
    assert {n: tuple(v.shape) for n, v in p0.items()} == {n: tuple(v.shape) for n, v in O.init_params(num_class=C).items()}
    net.set_batch(b)
    net.compute_losses(0.1)
    torch.cuda.synchronize()
    assert int(net.roi_count.sum()) > 0, "test needs at least one positive RoI"
    want_names = O.trainable_names(lock)
    tr = {n: p0[n].clone().requires_grad_(True) for n in want_names}
    pp = dict(p0)
    pp.update(tr)
    force = {"act%d" % l.idx: l.act.float().cpu() for l in net.layers}
    parts, _, _, _ = O.total_loss(pp, b, lock, True, perms, {}, obj_thresh=0.1, quant=O.bf16_ste, taps={}, force=force)
    parts["total"].backward()
    total = float(net.total_loss().cpu())
    print("C=%d: total loss %.6f (oracle %.6f)" % (C, total, float(parts["total"])))
    assert abs(total - float(parts["total"])) < 1e-3 * abs(float(parts["total"]))
    net.backward()
    torch.cuda.synchronize()
    assert set(net.trainable_names()) == set(want_names)
    fails = []
    for nm, (o, cnt) in net.arena_slices.items():
        g = net.grad_arena[o:o + cnt].cpu()
        assert tr[nm].grad is not None, nm
        want_g = tr[nm].grad.flatten()
        if nm.endswith("weights") or nm.endswith("biases"):
            want_g = want_g - O.L2_WEIGHT * tr[nm].detach().flatten()   # (the kernel adds l2*w inside Adam)
        r, amax, wmax = rel_err(g, want_g)
        if not (r < 0.03 or amax < 1e-3 * max(wmax, 1e-6)):
            fails.append("grad %s: rel l2 err %.3g (max abs %.3g of %.3g)" % (nm, r, amax, wmax))
    assert not fails, "%d checks failed:\n%s" % (len(fails), "\n".join(fails[:40]))


@pytest.mark.parametrize("C", [1, 6, 80])
def test_recorded_step_with_a_class_list_equals_eager(dev, C):
    B, S_ = 2, 64
    batches = [O.synthetic_batch(B, S_, seed=500 + t, num_class=C) for t in range(2)]
    eager, rec = (make_net(dev, None, B=B, S=S_, seed=4, classes=names(C)) for _ in range(2))
    for n in (eager, rec):
        n.set_batch(batches[0])
    rec.build_program(det_thresh=0.1)
    la = [float(eager.train_step(batches[t], det_thresh=0.1).cpu()) for t in range(2)]
    lb = [float(rec.train_step(batches[t]).cpu()) for t in range(2)]
    torch.cuda.synchronize()
    print("C=%d: losses eager %s recorded %s" % (C, la, lb))
    # (an RoI that rounds to zero area makes the mask term NaN, as in the reference -- SURVEY B14; the variables stay finite)
    assert np.isfinite(la).any()
    assert np.array_equal(np.asarray(la), np.asarray(lb), equal_nan=True)
    assert bool(torch.isfinite(eager.arena).all())
    _same_state(eager, rec)
    assert eager.step_count == rec.step_count == 2


@pytest.mark.parametrize("C", [1, 6, 80])
def test_inference_with_a_class_list_returns_the_oracle_detections(dev, C):
    """forward + evaluation of an inference net: the detections are the oracle's filter applied to the kernel's own logits"""
    B, S_ = 2, 64
    net = YOLONet(training=False, device=dev, image_size=S_, batch_size=B, stage=1, seed=0, classes=names(C))
    randomize_heads(net, 5)
    batch = O.synthetic_batch(B, S_, seed=3, num_class=C)
    thr = 0.02                      # (80 classes share the probability: the best class of an untrained head stays below 0.1)
    preds, det, _ = net.forward(batch["images"], batch["clip_window"], [thr], is_training=False)
    torch.cuda.synchronize()
    assert [tuple(p.shape) for p in preds] == [(B, g, g, 3, 5 + C) for g in (8, 4, 2)]
    pred = O.interpret_output([t.cpu() for t in preds])
    want = O.filter_detections(pred[2], pred[3], pred[5], batch["clip_window"], thr)
    got = det.cpu().numpy()
    assert (want[:, :, 5] > 0).sum() >= 4, "fixture needs detections"
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-6)
    if C > 1:
        assert len(np.unique(want[want[:, :, 5] > 0][:, 4])) > 1
    boxes, masks = net.evaluation(batch["images"], batch["clip_window"], [thr])
    for b in range(B):
        n = len(boxes[b])
        assert n > 0 and np.asarray(masks[b]).shape[0] == n
        assert all(any(np.array_equal(row, w) for w in got[b]) for row in np.asarray(boxes[b]))


# ------------------------------------------------------------------------------------------------ evaluate
def class_ground_truth(shapes, seed, C):
    """tests/test_gpu_eval_batch.py::synth_ground_truth with the instances' classes drawn from C classes"""
    rng = np.random.RandomState(seed)
    images, recs, sizes, merged, index = {}, {}, {}, {}, []
    for k, (h, w) in enumerate(shapes):
        name = "img%03d" % k
        index.append(name)
        images[name] = rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
        sizes[name] = [h, w]
        batch = synthetic_batch(1, (max(h, w) + 31) // 32 * 32, seed=seed + k, num_class=C)
        objs, mm = [], np.zeros((h, w), np.uint8)
        for j in range(batch["true_masks"].shape[1]):
            m = batch["true_masks"][0, j][:h, :w]
            if m.any():
                c = int(batch["true_boxes"][0, 0, 0, 0, j, 4])
                objs.append({"imageid": name, "classid": c, "difficult": 0, "mask": m.copy()})
                mm[m] = c + 1
        recs[name], merged[name] = objs, mm
    return images, recs, sizes, merged, index


def test_evaluate_with_a_6_class_map(dev):
    """two synthetic images, a net and a MAP of 6 classes: 6 AP rows and background + 6 IoUs + their mean, both equal to the
    host computation (voc_eval on the pasted masks, numpy confusion counts)"""
    check_evaluate_with_a_6_class_map(dev)


def check_evaluate_with_a_6_class_map(dev, **net_options):
    """the body of the test above; ``net_options`` are further YOLONet arguments (tests/test_gpu_option_matrix.py runs it with
    another k_map and mask_stride)"""
    S_, B, thr, C = 96, 2, 0.05, 6
    net = YOLONet(training=False, device=dev, image_size=S_, batch_size=B, stage=1, seed=0, classes=names(C), **net_options)
    randomize_heads(net, 7)
    images, recs, sizes, merged, index = class_ground_truth([(70, 120), (96, 96)], 33, C)
    emap = E.MAP(recs, sizes, index, merged, net_size=S_, classes=names(C))
    thresh_out, mask_acc, _ = E.evaluate(net, images, emap, det_thresh=thr)
    assert len(thresh_out) == 1 and len(thresh_out[0]["AP"]) == C and len(mask_acc) == C + 2
    with pytest.raises(ValueError, match="6 classes"):
        E.evaluate(net, images, E.MAP(recs, sizes, index, merged, net_size=S_))
    # the host computation on the same net's outputs
    frame = torch.zeros(B, S_, S_, 3, dtype=torch.float32, device=dev)
    windows = np.stack([E.image_read(images[n], S_, dev, out=frame[i])[1] for i, n in enumerate(index)])
    det_box, det_mask = net.evaluation(frame, windows, [np.float32(thr)], masks_on_device=True)
    detfile = {str(c): [] for c in range(C)}
    conf = np.zeros((C + 1, C + 1), np.int64)
    ndet = 0
    for i, n in enumerate(index):
        h, w = sizes[n]
        entries, mm = paste_detections(det_box[i], det_mask[i], h, w, S_)
        ndet += len(entries)
        for e in entries:
            detfile[str(e["classid"])].append({"imageid": n, "score": e["score"], "mask": e["mask"].cpu().numpy()})
        conf += np.bincount(merged[n].astype(np.int64).ravel() * (C + 1) + mm.cpu().numpy().ravel(),
                            minlength=(C + 1) ** 2).reshape(C + 1, C + 1)
    assert ndet >= 10 and len({c for c in detfile if detfile[c]}) >= 3, "fixture needs detections of several classes"
    res, pres, aps = [], [], []
    for c in range(C):
        if not detfile[str(c)]:
            r, p, a = 0.0, 0.0, 0.0
        else:
            r, p, a = voc_eval(detfile[str(c)], recs, index, c, ovthresh=0.5, use_07_metric=False)
        res, pres, aps = res + [r], pres + [p], aps + [a]
    assert repr(thresh_out[0]["AP"]) == repr(aps)
    assert repr(thresh_out[0]["mAP"]) == repr([float(np.mean(res)), float(np.mean(pres)), float(np.mean(aps))])
    cf = conf.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        ious = [cf[k, k] / (cf[k].sum() + cf[:, k].sum() - cf[k, k]) for k in range(C + 1)]
    np.testing.assert_array_equal(np.asarray(mask_acc[:-1]), np.asarray(ious))
    np.testing.assert_array_equal(mask_acc[-1], float(np.mean(ious)))
    seg = SegmentationAccuracy(dev, C)
    assert seg.conf.numel() == 49

"""The detection filter's NMS modes on the CPU: the restatement the GPU tests compare against (tests/nms_modes_ref.py) is held
to the oracle, the hand cases have the answers the reference's two methods and its nms=False give
(yolo/yolo3_net_pos.py:564-592, 594-605, 518), and the option reaches the net."""
import numpy as np
import pytest
import torch

import disyolo_oracle as O
import nms_modes_ref as R
from disyolo_amd import config as cfg
from disyolo_amd import lib as L
from disyolo_amd.net import YOLONet

FULL = [[0.0, 0.0, 1.0, 1.0]]


def hand_cases():
    eq = R.blank_logits(2)                                   # tests/test_gpu_kat.py::test_detect_equal_scores_keep_candidate_order
    R.put(eq[1], 0, 2, 1, 0, cls=0, conf=1.0)
    R.put(eq[1], 0, 2, 2, 0, cls=0, conf=1.0)
    R.put(eq[2], 1, 0, 0, 0, cls=1, conf=1.0)
    R.put(eq[0], 1, 6, 6, 0, cls=2, conf=1.0)
    R.put(eq[0], 1, 1, 6, 0, cls=1, conf=1.0)
    R.put(eq[1], 1, 3, 0, 0, cls=2, conf=1.0)
    return [("cross", R.pair_one_cell_apart(1, 0), FULL, 0.25, 0.1), ("same", R.pair_one_cell_apart(1, 1), FULL, 0.25, 0.1),
            ("at_iou", R.pair_one_cell_apart(1, 1), FULL, 0.25, R.THIRD), ("ties", eq, FULL * 2, 0.25, 0.2)]


def random_logits(seed, B=2, S=64):
    g = torch.Generator().manual_seed(seed)
    ys = [torch.randn(B, S // d, S // d, 3, 8, generator=g) for d in (8, 16, 32)]
    for y in ys:
        y[..., 2:4] *= 0.5
        y[..., 4] += 1.0
    return ys


def test_per_class_restatement_is_the_oracles_filter():
    ys = random_logits(5)
    win = [[0.0, 0.0, 1.0, 1.0], [0.1, 0.05, 0.9, 0.95]]
    pred = O.interpret_output(ys)
    want = O.filter_detections(pred[2], pred[3], pred[5], np.asarray(win, np.float32), 0.25)
    got = R.filter_logits(ys, win, 0.25, O.IOU_THRESHOLD, O.MAX_DETECTION, "per_class")
    assert (want[:, :, 5] > 0).sum() >= 40 and len(np.unique(want[:, :, 4])) == 3
    np.testing.assert_array_equal(got, want)
    for name, ys, win, thr, nms_thr in hand_cases():
        pred = O.interpret_output(ys, anchors=R.KAT_ANCH)
        want = O.filter_detections(pred[2], pred[3], pred[5], np.asarray(win, np.float32), thr, nms_thr)
        got = R.filter_logits(ys, win, thr, nms_thr, O.MAX_DETECTION, "per_class", anchors=R.KAT_ANCH)
        np.testing.assert_array_equal(got, want, err_msg=name)


@pytest.mark.parametrize("mode", ["agnostic", "none"])
def test_vectorised_greedy_loop_is_the_oracles_non_max_suppression(mode):
    ys = random_logits(6)
    pred = O.interpret_output(ys)
    for i in range(2):
        boxes, scores, classes = R.decode(pred[2], pred[3], pred[5], [0.05, 0.0, 1.0, 0.9], i)
        for max_det in (30, 7):
            fast = R.select(boxes, scores, classes, 0.25, O.IOU_THRESHOLD, max_det, mode)
            slow = R.select_slow(boxes, scores, classes, 0.25, O.IOU_THRESHOLD, max_det, mode)
            assert 7 <= len(fast) <= max_det and fast == slow       # (the cap binds at 7, and at 30 without suppression)
            assert len(fast) == max_det or (mode, max_det) == ("agnostic", 30)
    # the modes are different filters on these logits
    rows = {m: R.filter_logits(ys, FULL * 2, 0.25, O.IOU_THRESHOLD, 30, m) for m in R.MODES}
    assert not np.array_equal(rows["per_class"], rows["agnostic"]) and not np.array_equal(rows["agnostic"], rows["none"])
    # "none" = the 30 highest scores above the threshold, in order
    boxes, scores, classes = R.decode(pred[2], pred[3], pred[5], FULL[0], 0)
    top = np.sort(scores[scores > np.float32(0.25)])[::-1][:30]
    np.testing.assert_array_equal(rows["none"][0, :, 5], top)


def counts(ys, thr, nms_thr, win=FULL):
    out = {}
    for m in R.MODES:
        rows = R.filter_logits(ys, win, thr, nms_thr, O.MAX_DETECTION, m, anchors=R.KAT_ANCH)
        out[m] = rows, int((rows[0, :, 5] > 0).sum())
    return out


def test_hand_case_two_boxes_of_different_classes():
    c = counts(R.pair_one_cell_apart(1, 0), 0.25, 0.1)
    assert [c[m][1] for m in R.MODES] == [2, 1, 2]
    hi = np.float32(torch.sigmoid(torch.tensor(2.0)).item())
    row = c["agnostic"][0][0, 0]
    assert row[5] == hi and row[4] == 1                        # the higher score survives, with its own class
    np.testing.assert_array_equal(row[:4], np.float32([0.125, 0.125, 0.625, 0.625]))
    np.testing.assert_array_equal(c["none"][0], c["per_class"][0])


def test_hand_case_two_boxes_of_one_class():
    c = counts(R.pair_one_cell_apart(1, 1), 0.25, 0.1)
    assert [c[m][1] for m in R.MODES] == [1, 1, 2]
    np.testing.assert_array_equal(c["agnostic"][0], c["per_class"][0])


def test_hand_case_iou_at_the_threshold_and_a_score_at_the_threshold():
    ys = R.pair_one_cell_apart(2, 0)
    assert counts(ys, 0.25, R.THIRD)["agnostic"][1] == 2        # IoU > thr is false at equality
    assert counts(ys, 0.25, float(np.nextafter(np.float32(R.THIRD), np.float32(0))))["agnostic"][1] == 1
    one = R.blank_logits(1)
    R.put(one[1], 0, 1, 1, 0, cls=2)                            # score = 0.5 exactly
    for m in ("agnostic", "none"):
        assert counts(one, 0.5, 0.3)[m][1] == 0                 # strict '>' (:558)
        assert counts(one, float(np.nextafter(np.float32(0.5), np.float32(0))), 0.3)[m][1] == 1


def test_config_names_the_default_mode():
    assert cfg.NMS_METHOD == "per_class"
    assert list(L.NMS_MODES) == list(R.MODES) and [L.NMS_MODES[m] for m in R.MODES] == [0, 1, 2]


def test_plan_only_net_takes_the_mode():
    kw = dict(training=False, image_size=64, batch_size=1, plan_only=True)
    assert YOLONet(**kw).nms == "per_class"
    for m in R.MODES:
        assert YOLONet(nms=m, **kw).nms == m
    for bad in ("soft", "", "PER_CLASS", 1, True):
        with pytest.raises(ValueError, match="per_class.*agnostic.*none"):
            YOLONet(nms=bad, **kw)

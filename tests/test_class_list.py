"""Class lists of 1 to 80 classes, the parts that need no GPU: the net's plan and argument checks, checkpoints across class
lists, the argument errors of the new entry points (reported before any launch) and the host-side class tables.

The reference takes its list from CLASSES of yolo/config.py; here it is the ``classes`` argument of YOLONet, defect_train
and MAP (default cfg.CLASSES)."""
import ctypes

import numpy as np
import pytest
import torch

import disyolo_oracle as O
from disyolo_amd import checkpoint
from disyolo_amd import config as cfg
from disyolo_amd import lib as L
from disyolo_amd.evaluate import MAP
from disyolo_amd.net import YOLONet
from disyolo_amd.postprocess import SegmentationAccuracy

HEADS = ((59, 1024), (67, 512), (75, 256))


def names(n):
    return ["class%02d" % i for i in range(n)]


# ------------------------------------------------------------------------------------------------ plan and arguments
@pytest.mark.parametrize("C", [1, 6, 80])
def test_plan_sizes_the_heads_from_the_class_list(C):
    net = YOLONet(plan_only=True, classes=names(C))
    assert net.classes == names(C) and net.num_class == C and net.output_depth == 3 * (5 + C)
    for i, cin in HEADS:
        assert tuple(net.params["yolo/convolutional%d/weights" % i].shape) == (1, 1, cin, 3 * (5 + C))
        assert tuple(net.params["yolo/convolutional%d/biases" % i].shape) == (3 * (5 + C),)
    want = O.init_params(num_class=C)
    assert {n: tuple(v.shape) for n, v in net.params.items()} == {n: tuple(v.shape) for n, v in want.items()}
    assert sum(v.numel() for v in net.params.values()) == sum(v.numel() for v in want.values())


def test_default_class_list_is_the_configured_one():
    net = YOLONet(plan_only=True)
    assert net.classes == list(cfg.CLASSES) and net.num_class == 3 and net.output_depth == 24


@pytest.mark.parametrize("classes", [[], names(81), ["a", "b", "a"], ["a", ""], "crack", ["a", 3]])
def test_bad_class_lists_raise_naming_the_limit(classes):
    with pytest.raises(ValueError, match="80"):
        YOLONet(plan_only=True, classes=classes)
    with pytest.raises(ValueError, match="80"):
        MAP({}, {}, [], classes=classes)


# ------------------------------------------------------------------------------------------------ checkpoints
def test_80_class_checkpoint_round_trip(tmp_path):
    a = YOLONet(plan_only=True, classes=names(80), seed=1)
    prefix = str(tmp_path / "model.ckpt")
    checkpoint.save_net(a, prefix)
    b = YOLONet(plan_only=True, classes=names(80), seed=2)
    restored = checkpoint.restore_net(b, prefix)
    assert sorted(restored) == sorted(a.params) and b.restore_skipped == []
    for n, v in a.params.items():
        assert torch.equal(v, b.params[n]), n


def test_new_class_list_from_a_3_class_checkpoint(tmp_path):
    a = YOLONet(plan_only=True, seed=1)
    prefix = str(tmp_path / "model.ckpt")
    checkpoint.save_net(a, prefix)
    b = YOLONet(plan_only=True, classes=names(6), seed=2)
    with pytest.raises(ValueError, match="convolutional(59|67|75)"):
        checkpoint.restore_net(b, prefix)
    b = YOLONet(plan_only=True, classes=names(6), seed=2)
    init = {n: v.clone() for n, v in b.params.items()}
    restored = checkpoint.restore_net(b, prefix, reinit_mismatched_heads=True)
    heads = sorted("yolo/convolutional%d/%s" % (i, leaf) for i, _ in HEADS for leaf in ("weights", "biases"))
    assert sorted(b.restore_skipped) == heads
    assert sorted(restored) == sorted(set(a.params) - set(heads))
    for n in b.params:
        if n in heads:
            assert torch.equal(b.params[n], init[n]), n          # stays at its initialiser
        else:
            assert torch.equal(b.params[n], a.params[n]), n
    assert not torch.equal(init["yolo/convolutional1/weights"], a.params["yolo/convolutional1/weights"])
    # the flag forgives nothing but the heads' class dimension: another score-map grid still raises
    c = YOLONet(plan_only=True, classes=names(6), k_map=5)
    with pytest.raises(ValueError, match="convolutional82"):
        checkpoint.restore_net(c, prefix, reinit_mismatched_heads=True)


# ------------------------------------------------------------------------------------------------ ABI argument errors
def test_wide_loss_and_confusion_reject_bad_arguments_before_any_launch():
    """host buffers as in tests/test_abi.py: a launch would fault on them"""
    lib = L.load()
    buf = ctypes.create_string_buffer(1 << 16)
    p = ctypes.cast(buf, ctypes.c_void_p)
    three = (ctypes.c_void_p * 3)(p, p, p)
    anchors = (ctypes.c_float * 18)(*([32.0] * 18))
    scales = (ctypes.c_float * 4)(2.0, 1.0, 1.0, 1.0)
    B, S = 2, 64
    need = lib.disyolo_yolo_loss_workspace(B, S, 80)
    assert 0 < need <= len(buf)

    def wide(num_class=80, ld=256, max_boxes=20, S=S, ws_bytes=len(buf)):
        return lib.disyolo_yolo_loss_wide(three, three, p, max_boxes, B, S, num_class, ld, anchors, 0.5, scales, three, p,
                                          p, ws_bytes, None)

    for kw in (dict(num_class=0), dict(num_class=81), dict(num_class=6, ld=32), dict(num_class=80, ld=224),
               dict(num_class=6, ld=48), dict(num_class=6, ld=288), dict(S=80)):
        assert wide(**kw) == -1 and b"bad sizes" in lib.disyolo_last_error(), kw
    assert wide(max_boxes=65) == -1 and b"max_boxes" in lib.disyolo_last_error()
    assert wide(ws_bytes=need - 1) == -2 and b"workspace" in lib.disyolo_last_error()
    for nlabel in (1, 82, 0, -4):
        assert lib.disyolo_confusion_n(p, p, 16, nlabel, p, None) == -1 and b"nlabel" in lib.disyolo_last_error()
    assert lib.disyolo_confusion_n(p, p, 0, 4, p, None) == -1
    # the detection filter: 80 classes are accepted, 81 are not; the workspace no longer grows with B * C * NC
    assert lib.disyolo_detect_workspace(2, 64, 80) > 0
    assert lib.disyolo_detect(p, p, p, 2, 64, 81, anchors, p, 0.25, 0.3, 30, p, p, p, len(buf), None) == -1
    assert b"bad sizes" in lib.disyolo_last_error()
    assert lib.disyolo_detect(p, p, p, 2, 64, 80, anchors, p, 0.25, 0.3, 65, p, p, p, len(buf), None) == -1
    assert b"max_det" in lib.disyolo_last_error()
    assert lib.disyolo_detect(p, p, p, 2, 64, 80, anchors, p, 0.25, 0.3, 30, p, p, p, 1024, None) == -2
    w80, w16 = lib.disyolo_detect_workspace(32, 576, 80), lib.disyolo_detect_workspace(32, 576, 16)
    assert w80 < 3 * w16
    NC = 20412
    assert w80 > 32 * NC * 24 and lib.disyolo_detect_workspace(32, 576, 17) > 32 * NC * 24      # the decode prefix
    assert w16 == 32 * NC * 24 + 32 * 16 * NC * 8 + 32 * 16 * (64 * 8 + 4) + 256                 # the old formula, as it was


# ------------------------------------------------------------------------------------------------ host class tables
@pytest.mark.parametrize("C", [1, 6, 80])
def test_map_tables_follow_the_class_list(C):
    m = MAP({"a": []}, {"a": [8, 8]}, ["a"], classes=names(C))
    assert m.num_class == C and m.classid == list(range(C))
    assert m.class_to_ind == {n: i for i, n in enumerate(names(C))}
    table = m._ap_table({str(c): [] for c in m.classid})
    assert len(table) == 1 and len(table[0]["AP"]) == C and table[0]["AP"] == [0.0] * C


def test_map_default_is_the_configured_list():
    m = MAP({}, {}, [])
    assert m.classes == list(cfg.CLASSES) and m.class_to_ind == {"crack": 0, "spall": 1, "rebar": 2}


@pytest.mark.parametrize("C", [1, 3, 6, 80])
def test_segmentation_accuracy_has_one_iou_per_label_and_the_mean(C):
    seg = SegmentationAccuracy(torch.device("cpu"), num_class=C)
    n = C + 1
    assert seg.conf.numel() == n * n and seg.conf.dtype == torch.int64
    c = np.arange(n * n, dtype=np.int64).reshape(n, n) + 1
    seg.conf.copy_(torch.from_numpy(c.reshape(-1)))
    res = seg.result()
    assert len(res) == C + 2
    want = [c[k, k] / (c[k].sum() + c[:, k].sum() - c[k, k]) for k in range(n)]
    np.testing.assert_allclose(res[:-1], want, rtol=1e-15)
    assert res[-1] == pytest.approx(float(np.mean(want)), rel=1e-15)
    assert SegmentationAccuracy(torch.device("cpu")).conf.numel() == 16
    with pytest.raises(ValueError):
        SegmentationAccuracy(torch.device("cpu"), num_class=81)


def test_solver_refuses_mixed_class_lists(tmp_path):
    from disyolo_amd.solver import Solver

    class Data:
        num_class = 3

    net = YOLONet(plan_only=True, classes=names(6))
    net.shuffle_seed = None
    with pytest.raises(ValueError, match="6 classes.*data has 3"):
        Solver(net, Data(), output_dir=str(tmp_path))
    with pytest.raises(ValueError, match="6 classes.*evalu has 3"):
        Solver(net, object(), evalu=MAP({}, {}, []), output_dir=str(tmp_path))

"""Anchors and per-image limits per net, the parts that need no GPU: the three options of YOLONet and of the loader and
their checks, the Solver's refusal of a net and a loader that differ, the argument errors of the new and the widened entry
points (reported before any launch; the old ones keep their limit of 64), ``cluster_anchors``, and every case of
tests/test_gpu_limits.py run through the oracle alone and held to the condition that makes it a case (tests/limits_ref.py).

The reference has ANCHORS, MAX_BOX_PER_IMAGE = 20 and MAX_DETECTION = 30 in yolo/config.py and no answer beyond editing it."""
import ctypes

import numpy as np
import pytest
import torch

import disyolo_oracle as O
import limits_ref as LR
from disyolo_amd import config as cfg
from disyolo_amd import lib as L
from disyolo_amd.net import YOLONet
from disyolo_amd.synth import assign_targets, synthetic_batch
from disyolo_amd.train_data import cluster_anchors, defect_train, letterbox_boxes

ANCH = np.asarray(cfg.ANCHORS, np.float32)


# ------------------------------------------------------------------------------------------------ the options and their checks
def test_defaults_are_the_configured_values():
    net = YOLONet(plan_only=True)
    assert net.anchors.dtype == np.float32 and net.anchors.shape == (9, 2)
    np.testing.assert_array_equal(net.anchors, ANCH)
    assert net.max_box_per_image == cfg.MAX_BOX_PER_IMAGE == 20 and net.max_detection == cfg.MAX_DETECTION == 30


def test_defaults_are_read_at_construction(monkeypatch):
    monkeypatch.setattr(cfg, "MAX_DETECTION", 41)
    monkeypatch.setattr(cfg, "MAX_BOX_PER_IMAGE", 33)
    monkeypatch.setattr(cfg, "ANCHORS", (ANCH * 2).tolist())
    net = YOLONet(plan_only=True)
    monkeypatch.undo()
    assert (net.max_detection, net.max_box_per_image) == (41, 33)
    np.testing.assert_array_equal(net.anchors, ANCH * 2)
    assert YOLONet(plan_only=True).max_detection == 30       # a second net in the same process has its own


def test_two_nets_in_one_process_differ():
    a = YOLONet(plan_only=True, anchors=LR.NET_ANCH, max_box_per_image=100, max_detection=256)
    b = YOLONet(plan_only=True, anchors=ANCH.tolist(), max_box_per_image=1, max_detection=1)
    assert (a.max_box_per_image, a.max_detection, b.max_box_per_image, b.max_detection) == (100, 256, 1, 1)
    np.testing.assert_array_equal(a.anchors, LR.NET_ANCH)
    np.testing.assert_array_equal(b.anchors, ANCH)
    assert {n: tuple(v.shape) for n, v in a.params.items()} == {n: tuple(v.shape) for n, v in b.params.items()}


BAD_ANCHORS = [ANCH[:8], ANCH.reshape(-1), np.zeros((9, 2)), -ANCH, np.full((9, 2), np.nan), np.full((9, 2), np.inf),
               np.full((9, 2), 1e39), "auto", [[1, 2]] * 8 + [[1, "x"]], 5]


@pytest.mark.parametrize("bad", BAD_ANCHORS, ids=lambda v: str(np.shape(v)) + str(type(v).__name__))
def test_bad_anchors_raise(bad):
    with pytest.raises(ValueError, match="anchors must be 9 rows of 2 finite positive numbers"):
        YOLONet(plan_only=True, anchors=bad)
    with pytest.raises(ValueError, match="anchors must be 9 rows of 2 finite positive numbers"):
        defect_train([], batch_size=1, image_size=64, device="cpu", anchors=bad)


@pytest.mark.parametrize("bad", [0, 257, -1, True, False, 20.0, "20", None.__class__])
@pytest.mark.parametrize("name", ["max_box_per_image", "max_detection"])
def test_bad_limits_raise_naming_the_range(name, bad):
    with pytest.raises(ValueError, match=name + ".*1\\.\\.256"):
        YOLONet(plan_only=True, **{name: bad})
    if name == "max_box_per_image":
        with pytest.raises(ValueError, match=name + ".*1\\.\\.256"):
            defect_train([], batch_size=1, image_size=64, device="cpu", max_box_per_image=bad)


@pytest.mark.parametrize("v", [1, 64, 65, 256, np.int64(100)])
def test_limits_of_1_to_256_are_taken(v):
    net = YOLONet(plan_only=True, max_box_per_image=v, max_detection=v)
    assert net.max_box_per_image == net.max_detection == int(v) and type(net.max_detection) is int


def test_loader_takes_the_options_and_sizes_its_buffers():
    data = defect_train([], batch_size=2, image_size=(64, 96), device="cpu", anchors=LR.NET_ANCH, max_box_per_image=100)
    assert data.max_box_per_image == 100
    np.testing.assert_array_equal(data.anchors, LR.NET_ANCH)
    assert tuple(data.true_masks.shape) == (2, 100, 64, 96)
    assert tuple(data._host[0][0].shape) == (2, 1, 1, 1, 100, 5)
    assert data._jobs_host[0].numel() == 2 * (1 + 100) * L.PLACE_JOB.itemsize
    plain = defect_train([], batch_size=2, image_size=64, device="cpu")
    assert plain.max_box_per_image == 20 and tuple(plain.true_masks.shape) == (2, 20, 64, 64)
    np.testing.assert_array_equal(plain.anchors, ANCH)


def test_solver_refuses_a_net_and_a_loader_that_differ(tmp_path):
    from disyolo_amd.solver import Solver

    class Data:
        num_class = 3
        max_box_per_image = 20
        anchors = cfg.ANCHORS

    net = YOLONet(plan_only=True, max_box_per_image=100)
    net.shuffle_seed = None
    with pytest.raises(ValueError, match="100 boxes per image.*data has 20"):
        Solver(net, Data(), output_dir=str(tmp_path))
    net = YOLONet(plan_only=True, anchors=LR.NET_ANCH)
    net.shuffle_seed = None
    with pytest.raises(ValueError, match="anchors differ.*same anchors"):
        Solver(net, Data(), output_dir=str(tmp_path))
    # a loader with the same values, and an object that says nothing about either, pass
    net = YOLONet(plan_only=True)
    net.shuffle_seed = None
    Solver(net, Data(), output_dir=str(tmp_path), max_iter=0)
    Solver(net, object(), output_dir=str(tmp_path), max_iter=0)


def test_targets_follow_the_anchors():
    """the package's target assignment with ``anchors=`` equals the oracle's; with other anchors a box lands on another scale"""
    boxes = np.array([[30.0, 20.0, 6.0, 4.0], [40.0, 40.0, 30.0, 28.0], [10.0, 50.0, 3.0, 9.0]], np.float32)
    cls = [0, 2, 1]
    for anchors in (ANCH, LR.NET_ANCH):
        got = assign_targets(boxes, cls, 64, 3, anchors)
        want = O.assign_targets(boxes, np.asarray(cls), 64, anchors=anchors, num_class=3)
        for g, w in zip(got, want):
            np.testing.assert_array_equal(g, w)
    a = assign_targets(boxes, cls, 64, 3, ANCH)
    b = assign_targets(boxes, cls, 64, 3, LR.NET_ANCH)
    assert [int(t[..., 4].sum()) for t in a] != [int(t[..., 4].sum()) for t in b]
    batch = synthetic_batch(2, 64, seed=3, anchors=LR.NET_ANCH, max_box_per_image=100)
    assert batch["true_boxes"].shape == (2, 1, 1, 1, 100, 5) and batch["true_masks"].shape == (2, 100, 64, 64)
    assert synthetic_batch(2, 64, seed=3)["true_boxes"].shape == (2, 1, 1, 1, 20, 5)
    # a table of fewer rows than the helper's five instances: no more instances than rows (G is taken from 1)
    for G in (1, 2, 4):
        for seed in range(6):
            small = synthetic_batch(3, 64, seed=seed, max_box_per_image=G)
            assert small["true_boxes"].shape == (3, 1, 1, 1, G, 5) and small["true_masks"].shape == (3, G, 64, 64)
            assert small["true_masks"][:, 0].any()
    same = synthetic_batch(2, 64, seed=3, max_box_per_image=20)
    np.testing.assert_array_equal(same["true_boxes"], synthetic_batch(2, 64, seed=3)["true_boxes"])


def test_detect_picks_the_entry_point_by_the_sizes():
    """the old entry point wherever it takes the sizes; disyolo_detect_x above 64 rows and, up to 16 classes, above the 512
    survivors of the old merge"""
    lib = L.load()
    for Cn, D, x in ((3, 30, False), (3, 64, False), (8, 64, False), (16, 32, False), (17, 64, False), (80, 64, False),
                     (9, 57, True), (10, 64, True), (16, 33, True), (16, 40, True), (3, 65, True), (80, 65, True), (1, 256, True)):
        assert L.detect_takes_x(Cn, D) is x, (Cn, D)
        want = lib.disyolo_detect_workspace_x(2, 64, 64, Cn, D) if x else lib.disyolo_detect_workspace_hw(2, 64, 64, Cn)
        assert L.detect_workspace(2, 64, Cn, D) == want > 0
    # every size in range is taken by one of the two: what the old one refuses is exactly what goes to the new one
    buf, p = _host(1 << 20)
    anchors = (ctypes.c_float * 18)(*([32.0] * 18))
    for Cn in (1, 8, 9, 16, 17, 80):
        for D in (1, 32, 33, 56, 57, 64):
            rc = lib.disyolo_detect_nms_hw(p, p, p, 2, 64, 64, Cn, anchors, p, 0.25, 0.3, D, 0, p, p, p, 16, None)
            assert (rc == -1) == L.detect_takes_x(Cn, D), (Cn, D, rc)         # (-2: sizes accepted, the 16-byte workspace not)
    # a net in that band sizes its filter workspace for the entry point it will call
    net = YOLONet(plan_only=True, classes=["c%d" % i for i in range(16)], max_detection=40)
    assert L.detect_takes_x(net.num_class, net.max_detection)


# ------------------------------------------------------------------------------------------------ ABI
def _host(nbytes=1 << 16):
    buf = ctypes.create_string_buffer(nbytes)
    return buf, ctypes.cast(buf, ctypes.c_void_p)


def test_header_names_the_limits():
    import os
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "disyolo.h")).read()
    assert "#define DISYOLO_MAX_BOXES 256" in src and "#define DISYOLO_MAX_DET 256" in src
    assert L.MAX_BOXES == L.MAX_DET == 256


def test_detect_x_rejects_bad_arguments_before_any_launch():
    """host buffers as in tests/test_abi.py: a launch would fault on them"""
    lib = L.load()
    buf, p = _host(1 << 19)
    anchors = (ctypes.c_float * 18)(*([32.0] * 18))
    B, S = 2, 64
    need = lib.disyolo_detect_workspace_x(B, S, S, 80, 256)
    assert 0 < need <= len(buf)

    def detect(max_det=256, C=80, mode=0, ws=p, ws_bytes=len(buf), l3=p, win=p, det=p, cnt=p, anc=anchors):
        return lib.disyolo_detect_x(l3, p, p, B, S, S, C, anc, win, 0.25, 0.3, max_det, mode, det, cnt, ws, ws_bytes, None)

    for bad in (0, 257, -5):
        assert detect(max_det=bad) == -1 and b"1..256" in lib.disyolo_last_error(), bad
    for kw in (dict(l3=None), dict(win=None), dict(det=None), dict(cnt=None), dict(anc=None)):
        assert detect(**kw) == -1 and b"null pointer" in lib.disyolo_last_error(), kw
    assert detect(C=81) == -1 and b"bad sizes" in lib.disyolo_last_error()
    assert detect(mode=3) == -1 and b"nms_mode" in lib.disyolo_last_error()
    assert detect(ws_bytes=need - 1) == -2 and b"workspace" in lib.disyolo_last_error()       # DISYOLO_E_WORKSPACE
    assert detect(ws=None) == -2
    # a workspace of the old size is too short above 64 rows, and exactly enough up to 64
    old = lib.disyolo_detect_workspace_hw(B, S, S, 80)
    assert old < need and detect(ws_bytes=old) == -2
    assert lib.disyolo_detect_workspace_x(B, S, S, 80, 64) == lib.disyolo_detect_workspace_x(B, S, S, 80, 1) == old
    assert lib.disyolo_detect_workspace_x(B, S, S, 3, 256) - lib.disyolo_detect_workspace_hw(B, S, S, 3) == B * 3 * (256 - 64) * 8
    for bad in (0, 257):
        assert lib.disyolo_detect_workspace_x(B, S, S, 3, bad) == 0
    assert lib.disyolo_detect_workspace_x(B, 80, S, 3, 100) == 0 and lib.disyolo_detect_workspace_x(B, S, S, 81, 100) == 0
    # the old entry points keep their limit, their message and their workspace
    assert lib.disyolo_detect(p, p, p, B, S, 80, anchors, p, 0.25, 0.3, 65, p, p, p, len(buf), None) == -1
    assert b"max_det must be <= 64" in lib.disyolo_last_error()
    assert lib.disyolo_detect_nms_hw(p, p, p, B, S, S, 3, anchors, p, 0.25, 0.3, 65, 1, p, p, p, len(buf), None) == -1
    assert lib.disyolo_detect_nms_hw(p, p, p, B, S, S, 16, anchors, p, 0.25, 0.3, 33, 0, p, p, p, len(buf), None) == -1   # 16 * 33 > 512
    NC = 20412
    assert lib.disyolo_detect_workspace(32, 576, 16) == 32 * NC * 24 + 32 * 16 * NC * 8 + 32 * 16 * (64 * 8 + 4) + 256
    with pytest.raises(L.DisyoloError, match="1..256"):
        L.detect(None, None, None, B, S, 3, [1.0] * 18, None, 0.25, 0.3, 257, None, None, None)
    assert L.detect_workspace(B, S, 3, 256) == lib.disyolo_detect_workspace_x(B, S, S, 3, 256)
    assert L.detect_workspace(B, S, 3) == L.detect_workspace(B, S, 3, 64) == lib.disyolo_detect_workspace_hw(B, S, S, 3)


def test_loss_entry_points_take_256_boxes_and_the_old_ones_64():
    lib = L.load()
    buf, p = _host()
    three = (ctypes.c_void_p * 3)(p, p, p)
    anchors = (ctypes.c_float * 18)(*([32.0] * 18))
    scales = (ctypes.c_float * 4)(2.0, 1.0, 1.0, 1.0)
    B, S = 2, 64
    need = lib.disyolo_yolo_loss_workspace_hw(B, S, S, 80)
    assert 0 < need <= len(buf)

    def hw(max_boxes=256, C=3, ld=0, tb=p, ws=p, ws_bytes=len(buf), lg=three):
        return lib.disyolo_yolo_loss_hw(lg, three, tb, max_boxes, B, S, S, C, ld, anchors, 0.5, scales, three, p, ws, ws_bytes,
                                        None)

    for C, ld in ((3, 0), (80, 256)):
        for bad in (0, 257, -1):
            assert hw(max_boxes=bad, C=C, ld=ld) == -1 and b"max_boxes must be in 1..256" in lib.disyolo_last_error()
        assert hw(C=C, ld=ld, tb=None) == -1 and b"null pointer" in lib.disyolo_last_error()
        assert hw(C=C, ld=ld, lg=None) == -1 and b"null pointer" in lib.disyolo_last_error()
        assert hw(C=C, ld=ld, ws_bytes=need // 2 - 1 if C == 3 else need - 1) == -2 and b"workspace" in lib.disyolo_last_error()
        assert hw(C=C, ld=ld, ws=None) == -2
    # the old entry points still reject 65
    assert lib.disyolo_yolo_loss(three, three, p, 65, B, S, 3, anchors, 0.5, scales, three, p, p, len(buf), None) == -1
    assert b"max_boxes must be in 1..64" in lib.disyolo_last_error()
    assert lib.disyolo_yolo_loss_wide(three, three, p, 65, B, S, 80, 256, anchors, 0.5, scales, three, p, p, len(buf), None) == -1
    assert b"max_boxes must be in 1..64" in lib.disyolo_last_error()


def test_roi_and_shuffle_entry_points_take_256_rows():
    lib = L.load()
    buf, p = _host()

    def rois(max_det=256, G=256, det=p, tb=p, out=p, cnt=p, n_det=7, n_gt=3):
        return lib.disyolo_mask_rois_hw(det, max_det, tb, G, p, p, 2, 24, 40, 3, n_det, n_gt, 0.5, out, cnt, None)

    for kw in (dict(max_det=0), dict(max_det=257), dict(G=0), dict(G=257)):
        assert rois(**kw) == -1 and b"1..256" in lib.disyolo_last_error(), kw
    for kw in (dict(det=None), dict(tb=None), dict(out=None), dict(cnt=None)):
        assert rois(**kw) == -1 and b"null pointer" in lib.disyolo_last_error(), kw
    assert rois(n_det=9, n_gt=8) == -1 and b"n_det + n_gt" in lib.disyolo_last_error()     # DISYOLO_ROI_MAX stays 16

    def shuffle(n_det=256, n_gt=256, a=p, b=p, B=2):
        return lib.disyolo_shuffle_perm(a, n_det, b, n_gt, B, 1, None, None)

    for kw in (dict(n_det=0), dict(n_det=257), dict(n_gt=0), dict(n_gt=257)):
        assert shuffle(**kw) == -1 and b"1..256" in lib.disyolo_last_error(), kw
    for kw in (dict(a=None), dict(b=None), dict(B=0)):
        assert shuffle(**kw) == -1 and b"shuffle_perm" in lib.disyolo_last_error(), kw


def _job(buf, n=5, ng=2, h=37, w=53):
    j = np.zeros(1, L.PASTE_JOB)
    for f in ("masks", "rects", "classids", "gt", "gt_class", "merged", "true_map", "counts"):
        j[f] = ctypes.addressof(buf)
    j["n"], j["ng"], j["image_h"], j["image_w"] = n, ng, h, w
    return j


def test_paste_x_takes_256_detections_and_the_old_plan_64():
    lib = L.load()
    buf, p = _host()
    conf = ctypes.cast(ctypes.create_string_buffer(128), ctypes.c_void_p)

    def call(j, njobs=1, mh=32, mw=32, table=True, dev=p, conf=conf):
        return lib.disyolo_mask_paste_iou_batch_x(j.ctypes.data if table else None, dev, njobs, mh, mw, conf, None)

    for n in (65, 100, 256):
        j = _job(buf, n=n)
        assert lib.disyolo_paste_job_plan_x(j.ctypes.data, 1) == 2 and j["block0"][0] == 0
        assert L.paste_job_plan(j, wide=True) == 2
        assert lib.disyolo_paste_job_plan(j.ctypes.data, 1) == -1 and b"0..64" in lib.disyolo_last_error()
        assert lib.disyolo_mask_paste_iou_batch_hw(j.ctypes.data, p, 1, 32, 32, conf, None) == -1
        assert b"0..64" in lib.disyolo_last_error()
        with pytest.raises(L.DisyoloError, match="0..64"):
            L.paste_job_plan(j)
    for n in (257, -1):
        j = _job(buf, n=n)
        assert lib.disyolo_paste_job_plan_x(j.ctypes.data, 1) == -1 and b"0..256" in lib.disyolo_last_error()
        assert call(j) == -1 and b"0..256" in lib.disyolo_last_error()
        with pytest.raises(L.DisyoloError, match="0..256"):
            L.paste_job_plan(j, wide=True)
    good = _job(buf, n=100)
    assert lib.disyolo_paste_job_plan_x(good.ctypes.data, 1) == 2
    assert call(good, table=False) == -1 and b"null table" in lib.disyolo_last_error()
    assert call(good, dev=None) == -1 and b"null table" in lib.disyolo_last_error()
    assert call(good, njobs=0) == -1
    assert call(good, mh=0) == -1 and b"size" in lib.disyolo_last_error()
    assert call(good, conf=None) == -1 and b"conf" in lib.disyolo_last_error()
    assert lib.disyolo_paste_job_plan_x(None, 1) == -1
    two = np.concatenate([_job(buf, n=100), _job(buf, n=256)])
    assert lib.disyolo_paste_job_plan_x(two.ctypes.data, 2) == 4 and list(two["block0"]) == [0, 2]
    two["block0"][1] = 1
    assert call(two, njobs=2) == -1 and b"not planned" in lib.disyolo_last_error()


# ------------------------------------------------------------------------------------------------ cluster_anchors
PLANTED = np.array([[6, 9], [14, 8], [11, 22], [30, 19], [22, 44], [58, 38], [40, 90], [120, 70], [150, 160]], np.float64)


def planted_records(image_hw, net_size, per=40, seed=0):
    """records whose instances, letter-boxed to ``net_size``, are the nine planted (w, h) with +-3 % jitter"""
    from disyolo_amd.net import check_image_size
    rng = np.random.RandomState(seed)
    h, w = image_hw
    net_h, net_w = check_image_size(net_size)
    f = min(net_w / w, net_h / h)                      # the letter box keeps the aspect: one factor (up to the integer fit)
    recs = []
    for i in range(per):
        polys = []
        for pw, ph in PLANTED:
            bw = pw * rng.uniform(0.97, 1.03) / f
            bh = ph * rng.uniform(0.97, 1.03) / f
            x1, y1 = rng.uniform(0, w - bw - 1), rng.uniform(0, h - bh - 1)
            # (float vertices: the box spans max + 1 - min, like extract_bboxes on the rasterised mask)
            polys.append([{"type": "out", "all_points_x": [x1, x1 + bw - 1, x1 + bw - 1, x1],
                           "all_points_y": [y1, y1, y1 + bh - 1, y1 + bh - 1]}])
        recs.append({"image_size": (h, w), "class_names": ["a"] * len(polys), "polygons": polys})
    return recs


@pytest.mark.parametrize("image_hw,net_size", [((1000, 1000), 576), ((600, 900), (128, 192)), ((480, 640), (192, 128))])
def test_cluster_anchors_recovers_planted_clusters(image_hw, net_size):
    recs = planted_records(image_hw, net_size)
    boxes = letterbox_boxes(recs, net_size)
    assert boxes.shape == (40 * 9, 2)
    got = cluster_anchors(recs, net_size)
    assert got.dtype == np.float32 and got.shape == (9, 2)
    area = got[:, 0] * got[:, 1]
    assert (np.diff(area) > 0).all(), "sorted by area ascending"
    # within the jitter (3 %) plus the half-percent of the letter box's integer fit
    np.testing.assert_allclose(got, PLANTED, rtol=0.035)
    again = cluster_anchors(planted_records(image_hw, net_size), net_size)
    assert got.tobytes() == again.tobytes(), "no random draw: the same labels give the same anchors"
    YOLONet(plan_only=True, image_size=net_size, anchors=got)           # what the net takes


def test_cluster_anchors_edge_cases():
    recs = planted_records((500, 500), 64, per=1)
    np.testing.assert_allclose(cluster_anchors(recs, 64), letterbox_boxes(recs, 64)[np.argsort(
        letterbox_boxes(recs, 64).prod(axis=1))].astype(np.float32), rtol=1e-6)      # 9 boxes, 9 clusters: the boxes
    assert cluster_anchors(recs, 64, n=3).shape == (3, 2)
    with pytest.raises(ValueError, match="at least as many instances"):
        cluster_anchors(recs[:1], 64, n=10)
    with pytest.raises(ValueError, match="positive int"):
        cluster_anchors(recs, 64, n=0)
    with pytest.raises(ValueError, match="multiple of 32"):
        cluster_anchors(recs, 100)
    # an image from an array, and the letter box of a tall image in a wide net: the height binds
    rec = {"image": np.zeros((200, 100, 3), np.uint8), "class_names": ["a"],
           "polygons": [[{"type": "out", "all_points_x": [10, 49], "all_points_y": [20, 119]}]]}
    np.testing.assert_allclose(letterbox_boxes([rec], (64, 128)), [[40 * 32 / 100, 100 * 64 / 200]])
    # an empty cluster keeps its centroid: two distinct boxes, many copies, three clusters
    two = {"image_size": (64, 64), "class_names": ["a"] * 8,
           "polygons": [[{"type": "out", "all_points_x": [0, 9], "all_points_y": [0, 9]}]] * 4
           + [[{"type": "out", "all_points_x": [0, 39], "all_points_y": [0, 29]}]] * 4}
    got = cluster_anchors([two], 64, n=3)
    assert sorted(map(tuple, got.tolist())) == [(10.0, 10.0), (40.0, 30.0), (40.0, 30.0)]


# ------------------------------------------------------------------------------------------------ the GPU cases, oracle only
@pytest.mark.parametrize("C", LR.FILTER_C)
def test_filter_cases_keep_more_than_64_rows_in_every_image(C):
    ys = LR.filter_logits(C)
    assert LR.n_cand(LR.FILTER_S) == 567
    by_mode = {}
    for D in LR.FILTER_D:
        for mode in ("per_class", "agnostic", "none"):
            rows, cnt, above = LR.filter_want(ys, D, mode)
            assert min(above) > D, "more than D candidates must pass: %s" % above
            assert min(cnt) > 64 and max(cnt) <= D, (C, D, mode, cnt)
            for i in range(LR.FILTER_B):
                sc = rows[i, :cnt[i], 5]
                assert (np.diff(sc) <= 0).all() and len(np.unique(sc)) < cnt[i], "score descending, with ties"
                assert (rows[i, cnt[i]:] == 0).all()
            by_mode[(D, mode)] = rows
            if mode == "per_class":         # the oracle's own filter agrees with the restatement
                pred = O.interpret_output(ys, anchors=LR.FILTER_ANCH)
                want = O.filter_detections(pred[2], pred[3], pred[5], np.asarray(LR.FILTER_WIN, np.float32), LR.FILTER_THR,
                                           LR.FILTER_NMS, max_detection=D)
                np.testing.assert_array_equal(rows, want)
    # the three modes are told apart, and the window of the second image clips
    assert not np.array_equal(by_mode[(256, "agnostic")], by_mode[(256, "none")])
    assert not np.array_equal(by_mode[(256, "agnostic")], by_mode[(256, "per_class")])
    second = by_mode[(256, "none")][1]
    assert second[:, 0].min() >= np.float32(0.1) and second[:, 3].max() <= np.float32(0.95)
    if C == 3:
        assert 3 * 100 <= 512 < 3 * 256, "D = 100 and 256 sit either side of the rank merge's capacity"


@pytest.mark.parametrize("G", LR.LOSS_G)
@pytest.mark.parametrize("C", LR.LOSS_C)
def test_loss_cases_depend_on_rows_past_64(C, G):
    heads, labels, tb = LR.loss_case(C, G)
    assert tb.shape == (LR.LOSS_B, G, 5) and not tb[:, :64].any() and np.abs(tb[1, 64:, :4]).sum(axis=1).all() == (G == 65)
    full = LR.loss_terms(heads, labels, tb)
    cut = tb.copy()
    cut[:, 64:] = 0
    short = LR.loss_terms(heads, labels, cut)
    assert np.isfinite(full).all() and (full[:5] > 0).all()
    assert full[1] < short[1] and abs(full[1] - short[1]) > 1e-3 * full[1], "rows >= 64 must decide the noobj term"
    np.testing.assert_array_equal(full[[0, 2, 3, 4]], short[[0, 2, 3, 4]])      # the labels carry the other terms


@pytest.mark.parametrize("D,G", LR.ROI_CASES)
def test_roi_cases_select_rows_past_64(D, G):
    det, tb, perms = LR.roi_case(D, G)
    Hm, Wm = LR.ROI_MAP
    for k in (3, 7):
        rows, picked = LR.roi_rows(det, tb, perms, Hm, Wm, k)
        for b in range(det.shape[0]):
            pos, assign, gt_rows = picked[b]
            assert len(rows[b]) >= 6 and len(rows[b][0]) == L.roi_w(k)
            assert any(r[2 * k + 2] >= 64 for r in rows[b]), "a ground-truth row >= 64 must be assigned"
            from_row = [[q for q in range(D) if np.array_equal(det[b, q, :4], p)] for p in pos]
            assert any(q and q[0] >= 64 for q in from_row), "a detection row >= 64 must be selected"
            # zero rows between the non-zero ones, and the twins: the detection on their box takes the lower row
            nz = np.flatnonzero(np.abs(tb[b, 0, 0, 0, :, :4]).sum(axis=1))
            assert len(nz) < G and nz[-1] == G - 1 and (G < 200 or len(nz) > 64)
            t0, t1 = nz[3], nz[3 + 64] if len(nz) > 3 + 64 else nz[5]
            np.testing.assert_array_equal(tb[b, 0, 0, 0, t0, :4], tb[b, 0, 0, 0, t1, :4])
            twin = [r for r, p in zip(rows[b], pos) if np.array_equal(p, det[b, D - 1, :4])]
            assert twin and twin[0][2 * k + 2] == t0
        assert max(len(r) for r in rows) <= cfg.MASK_ROI_DET + cfg.MASK_ROI_GT


def test_paste_cases_have_an_overlap_across_the_word_boundary():
    for n, (h, w) in ((100, (37, 53)), (256, (130, 257))):
        m, r, cls, gt, gt_cls, tm = LR.paste_case(n, h, w, 5, 32, seed=n)
        assert m.shape == (n, 32, 32) and h * w > 1024, "more than one block's chunk of pixels"
        for a, b in ((3, 70), (63, 64), (n - 2, n - 1)):
            assert cls[a] != cls[b] and np.array_equal(r[a, 4:], r[b, 4:]) and (r[a, 6] - r[a, 4]) * (r[a, 7] - r[a, 5]) > 0
        assert 3 // 64 != 70 // 64


def test_whole_net_batch_and_composed_loss():
    """the batch of the whole-net case (five instances in rows 0..99) and the composed total loss at the default values equal
    to ``O.total_loss``"""
    b = LR.net_batch(11)
    tb = b["true_boxes"].numpy()
    for i in range(LR.NET_B):
        assert np.flatnonzero(np.abs(tb[i, 0, 0, 0, :, :4]).sum(axis=1)).tolist() == list(LR.NET_ROWS)
        assert [int(m.any()) for m in b["true_masks"][i]] == [int(j in LR.NET_ROWS) for j in range(LR.NET_G)]
    assert sum(int(b[k][..., 4].sum()) for k in ("yolo1", "yolo2", "yolo3")) >= 6
    assert not np.array_equal(LR.NET_ANCH, np.round(LR.NET_ANCH)), "non-integer anchors"
    bb, perms = LR.with_perms(b)
    assert bb["perm_det"].shape == (2, 100) and bb["perm_gt"].shape == (2, 100)
    # composed == O.total_loss where the latter's baked-in values apply
    ob = O.synthetic_batch(1, 64, seed=5)
    params = O.init_params(seed=1)
    lock = O.default_lock(1)
    with torch.no_grad():
        want, wdet, _, _ = O.total_loss(params, ob, lock, True, None, {}, obj_thresh=0.1)
        got, gdet, _, _ = LR.total_loss(params, ob, lock, O.ANCHORS, O.MAX_DETECTION, None, {}, obj_thresh=0.1)
    np.testing.assert_array_equal(gdet, wdet)
    for k in want:
        assert float(got[k]) == float(want[k]) or (np.isnan(float(got[k])) and np.isnan(float(want[k]))), k


def test_shuffle_reference_rows_are_permutations():
    for n in (20, 30, 100, 256):
        a = LR.shuffle_perm_want(n, 3, 0, 20190530, 7)
        assert all(sorted(r.tolist()) == list(range(n)) for r in a)
        assert not np.array_equal(a[0], a[1]) and not np.array_equal(a, LR.shuffle_perm_want(n, 3, 0, 20190530, 8))
        assert not np.array_equal(a, LR.shuffle_perm_want(n, 3, 1, 20190530, 7))

"""The detection filter's NMS modes on the GPU: "per_class" (Method 1 of filter_detections, yolo/yolo3_net_pos.py:564-592),
"agnostic" (Method 2, :594-605) and "none" (nms=False, :518).

Every comparison with the restatement (tests/nms_modes_ref.py) is ``assert_array_equal`` on the boxes / scores / classes the
decode kernel itself wrote (read back from the workspace, like tests/test_gpu_kat.py's many-candidates test): any difference
is a different decision of the filter, not rounding."""
import ctypes as C

import numpy as np
import pytest
import torch

import disyolo_oracle as O
import nms_modes_ref as R
from disyolo_amd import config as cfg
from disyolo_amd import lib as L
from disyolo_amd.net import YOLONet

pytestmark = pytest.mark.gpu

MAX_DET = cfg.MAX_DETECTION
ANCHORS = np.asarray(cfg.ANCHORS, np.float32).reshape(-1)
WIN2 = [[0.0, 0.0, 1.0, 1.0], [0.1, 0.05, 0.9, 0.95]]          # the second image has a window of its own


def n_cand(S):
    return 3 * ((S // 8) ** 2 + (S // 16) ** 2 + (S // 32) ** 2)


def decoded(ws, B, NC):
    """what decode_score_kernel left at the start of the workspace: boxes [B,NC,4], scores [B,NC], classes [B,NC]"""
    raw = ws.buf[:B * NC * 24].cpu().numpy()
    return (raw[:B * NC * 16].view(np.float32).reshape(B, NC, 4), raw[B * NC * 16:B * NC * 20].view(np.float32).reshape(B, NC),
            raw[B * NC * 20:B * NC * 24].view(np.int32).reshape(B, NC))


def restated(dec, thr, nms_thr, mode, max_det=MAX_DET):
    boxes, scores, classes = dec
    rows, cnt = np.zeros((len(boxes), max_det, 6), np.float32), []
    for b in range(len(boxes)):
        idx = R.select(boxes[b], scores[b], classes[b], thr, nms_thr, max_det, mode)
        rows[b] = R.rows_of(boxes[b], scores[b], classes[b], idx, max_det)
        cnt.append(len(idx))
    return rows, cnt


def run_detect(dev, ys, S, anchors, win, thr, nms_thr, mode=None, max_det=MAX_DET, ws=None):
    """L.detect on logits [B,g,g,3,8] x 3 -> detections, det_count, the decode results"""
    B = ys[0].shape[0]
    det = torch.full((B, max_det, 6), float("nan"), device=dev)
    cnt = torch.full((B,), -1, dtype=torch.int32, device=dev)
    logits = [y.reshape(B, y.shape[1], y.shape[2], 24).contiguous().to(dev) for y in ys]
    ws = ws or L.Workspace(dev)
    kw = {} if mode is None else {"nms": mode}
    L.detect(logits[0], logits[1], logits[2], B, S, 3, np.asarray(anchors, np.float32).reshape(-1),
             torch.as_tensor(win, device=dev).float(), float(thr), float(nms_thr), max_det, det, cnt, ws, **kw)
    torch.cuda.synchronize()
    return det.cpu().numpy(), cnt.cpu().numpy().tolist(), decoded(ws, B, n_cand(S))


def random_logits(case, S=576, B=2):
    """the inputs of tests/test_gpu_kat.py::test_detect_greedy_nms_on_thousands_of_candidates, and "dense": every candidate
    passes 0.25 (conf logits + 8: sigmoid > 0.95, times a softmax maximum >= 1/3 of three classes)"""
    g = torch.Generator().manual_seed({"balanced": 1, "one_class": 2, "sparse": 3, "ties": 4, "dense": 6}[case])
    ys = [torch.randn(B, S // d, S // d, 3, 8, generator=g) for d in (8, 16, 32)]
    for y in ys:
        y[..., 2:4] *= 0.5
        if case == "one_class":
            y[..., 4] += 3.0
            y[..., 5] += 4.0
        elif case == "sparse":
            y[..., 4] -= 3.0
        elif case == "ties":
            y[..., 4] = torch.round(y[..., 4])
            y[..., 5:] = torch.round(y[..., 5:]) * 40.0
        elif case == "dense":
            y[..., 4] += 8.0
        else:
            y[..., 4] += 1.5
    return ys


# ---- 1. mode 0 through the new entry point is the old filter
@pytest.mark.parametrize("case", ["balanced", "one_class", "sparse", "ties"])
def test_per_class_mode_is_bit_identical_to_detect_without_the_keyword(dev, case):
    ys = random_logits(case)
    thr = 0.25
    old, old_cnt, _ = run_detect(dev, ys, 576, ANCHORS, WIN2, thr, cfg.IOU_THRESHOLD)
    new, new_cnt, _ = run_detect(dev, ys, 576, ANCHORS, WIN2, thr, cfg.IOU_THRESHOLD, mode="per_class")
    assert min(old_cnt) > 0 and not np.isnan(old).any()
    assert old.tobytes() == new.tobytes() and old_cnt == new_cnt
    # ... and the unchanged C entry point, called directly
    B = 2
    det = torch.full((B, MAX_DET, 6), float("nan"), device=dev)
    cnt = torch.full((B,), -1, dtype=torch.int32, device=dev)
    logits = [y.reshape(B, y.shape[1], y.shape[2], 24).contiguous().to(dev) for y in ys]
    win = torch.tensor(WIN2, device=dev)
    lib = L.load()
    buf = L.Workspace(dev).get(lib.disyolo_detect_workspace_hw(B, 576, 576, 3))
    anc = (C.c_float * 18)(*[float(v) for v in ANCHORS])
    p = lambda t: C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    args = [p(logits[0]), p(logits[1]), p(logits[2]), B, 576, 576, 3, anc, p(win), thr, cfg.IOU_THRESHOLD, MAX_DET]
    tail = [p(det), p(cnt), p(buf), buf.numel(), stream]
    assert lib.disyolo_detect_hw(*args, *tail) == 0
    torch.cuda.synchronize()
    assert det.cpu().numpy().tobytes() == old.tobytes() and cnt.cpu().tolist() == old_cnt
    for bad in (-1, 3):
        assert lib.disyolo_detect_nms_hw(*args, bad, *tail) == -1          # DISYOLO_E_ARG
        assert b"nms_mode" in lib.disyolo_last_error()
    with pytest.raises(ValueError):
        run_detect(dev, ys, 576, ANCHORS, WIN2, thr, cfg.IOU_THRESHOLD, mode="soft")


# ---- 2. known answers at S = 64 (tests/test_gpu_kat.py's cases in the two image-wide modes)
def kat(dev, ys, win, thr, nms_thr, mode):
    got, cnt, dec = run_detect(dev, ys, R.KAT_S, R.KAT_ANCH, win, thr, nms_thr, mode=mode)
    want, want_cnt = restated(dec, thr, nms_thr, mode)
    np.testing.assert_array_equal(got, want)
    assert cnt == want_cnt
    # these inputs are exact in f32 on both sides: the oracle's own decode gives the same rows
    np.testing.assert_array_equal(got, R.filter_logits(ys, win, thr, nms_thr, MAX_DET, mode, anchors=R.KAT_ANCH))
    return got, cnt


def test_kat_a_box_of_another_class_suppresses_only_in_agnostic_mode(dev):
    win = [[0, 0, 1, 1]]
    for classes, want in (((1, 0), {"per_class": 2, "agnostic": 1, "none": 2}), ((1, 1), {"per_class": 1, "agnostic": 1, "none": 2})):
        ys = R.pair_one_cell_apart(*classes)
        for mode, n in want.items():
            got, cnt = kat(dev, ys, win, 0.25, 0.1, mode)
            assert cnt == [n]
            assert got[0, 0, 5] > 0.88 and got[0, 0, 4] == 1           # the higher score first, with its own class
            if n == 2:
                assert 0.73 < got[0, 1, 5] < 0.74 and got[0, 1, 4] == classes[1]


def test_kat_iou_exactly_at_the_threshold_survives_across_classes(dev):
    ys = R.pair_one_cell_apart(2, 0)
    win = [[0, 0, 1, 1]]
    assert kat(dev, ys, win, 0.25, R.THIRD, "agnostic")[1] == [2]      # IoU > thr is false at equality
    below = float(np.nextafter(np.float32(R.THIRD), np.float32(0)))
    got, cnt = kat(dev, ys, win, 0.25, below, "agnostic")
    assert cnt == [1] and got[0, 0, 4] == 2
    assert kat(dev, ys, win, 0.25, below, "none")[1] == [2]


@pytest.mark.parametrize("mode", ["agnostic", "none"])
def test_kat_equal_scores_come_out_in_candidate_order(dev, mode):
    ys = R.blank_logits(2)
    R.put(ys[1], 0, 2, 1, 0, cls=0, conf=1.0)                          # image 0: two overlapping equal-score boxes, two classes
    R.put(ys[1], 0, 2, 2, 0, cls=1, conf=1.0)
    R.put(ys[2], 1, 0, 0, 0, cls=1, conf=1.0)                          # image 1: four far apart, three scales, two classes
    R.put(ys[0], 1, 6, 6, 0, cls=2, conf=1.0)
    R.put(ys[0], 1, 1, 6, 0, cls=1, conf=1.0)
    R.put(ys[1], 1, 3, 0, 0, cls=2, conf=1.0)
    got, cnt = kat(dev, ys, [[0, 0, 1, 1]] * 2, 0.25, 0.2, mode)
    assert cnt == [1 if mode == "agnostic" else 2, 4]
    assert got[0, 0, 3] == np.float32(0.625) and got[0, 0, 4] == 0      # the x = 1 cell's box is first (and alone, with NMS)
    np.testing.assert_array_equal(got[1, :4, 4], [1, 2, 2, 1])          # 8-grid (1,6), 8-grid (6,6), 4-grid, 2-grid


@pytest.mark.parametrize("mode", ["agnostic", "none"])
def test_kat_cap_at_max_detection_and_clipping_before_the_iou(dev, mode):
    anch = R.KAT_ANCH.copy()
    anch[0] = [8, 8]                                                  # 8-grid boxes that tile the image: disjoint
    ys = R.blank_logits(2)
    for cy in range(8):                                               # image 0: 64 disjoint boxes, five distinct scores
        for cx in range(8):
            R.put(ys[0], 0, cy, cx, 0, cls=(cy + cx) % 3, conf=float((cy * 8 + cx) % 5))
    # image 1: two 0.5 x 0.5 boxes of different classes one cell apart, IoU 1/3 as decoded; the window cuts them to strips
    # [.25,.25,.375,.625] and [.25,.375,.375,.75] with IoU 1/2 -- at a threshold of 0.4 only the clipped boxes suppress
    R.put(ys[1], 1, 0, 1, 0, cls=0, conf=2.0)
    R.put(ys[1], 1, 0, 2, 0, cls=1, conf=1.0)
    R.put(ys[2], 1, 1, 1, 1, cls=2, conf=3.0)                          # 64 x 32 anchor: wider than the image
    win = [[0, 0, 1, 1], [0.25, 0.25, 0.75, 0.75]]
    got, cnt, dec = run_detect(dev, ys, R.KAT_S, anch, win, 0.25, 0.4, mode=mode)
    want, want_cnt = restated(dec, 0.25, 0.4, mode)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got, R.filter_logits(ys, win, 0.25, 0.4, MAX_DET, mode, anchors=anch))
    assert cnt == want_cnt and cnt[0] == 30
    # 12 candidates of conf 4, 13 of conf 3, and the first 5 of the 13 of conf 2: the cap cuts through a run of ties, by index
    assert (np.diff(got[0, :, 5]) <= 0).all() and got[0, 29, 5] == got[0, 25, 5] < got[0, 24, 5]
    np.testing.assert_array_equal(got[0, 25:30, 0] * 8 * 8 + got[0, 25:30, 1] * 8, [2, 7, 12, 17, 22])    # cells 2, 7, 12, 17, 22
    assert cnt[1] == (2 if mode == "agnostic" else 3)
    assert got[1, :cnt[1], :4].min() >= 0.25 and got[1, :cnt[1], :4].max() <= 0.75
    np.testing.assert_array_equal(got[1, 1, :4], np.float32([0.25, 0.25, 0.375, 0.625]))
    if mode == "none":
        np.testing.assert_array_equal(got[1, 2, :4], np.float32([0.25, 0.375, 0.375, 0.75]))


@pytest.mark.parametrize("mode", ["agnostic", "none"])
def test_kat_score_exactly_at_the_threshold_is_dropped(dev, mode):
    ys = R.blank_logits(1)
    R.put(ys[1], 0, 1, 1, 0, cls=2)                                    # score = 0.5 exactly
    win = [[0, 0, 1, 1]]
    got, cnt = kat(dev, ys, win, 0.5, 0.3, mode)
    assert cnt == [0] and (got == 0).all()                             # strict '>' (:558)
    got, cnt = kat(dev, ys, win, float(np.nextafter(np.float32(0.5), np.float32(0))), 0.3, mode)
    assert cnt == [1] and got[0, 0, 5] == 0.5 and got[0, 0, 4] == 2


# ---- 3. many candidates: the image-wide list in registers (up to detect_list_capacity()) and in global memory (beyond)
@pytest.mark.parametrize("S,case,modes", [(576, "dense", ("agnostic", "none")), (576, "balanced", ("agnostic",)),
                                          (576, "sparse", ("agnostic",)), (576, "ties", ("agnostic",)),
                                          (None, "dense", ("agnostic", "none"))])
def test_image_wide_filter_on_many_candidates(dev, S, case, modes):
    cap = L.detect_list_capacity()
    assert cap >= n_cand(576), "the register form must hold a whole 576^2 image"
    if S is None:                                   # the smallest net whose candidates do not fit: 608 for 20,480
        S = next(s for s in range(32, 4096, 32) if n_cand(s) > cap)
        assert n_cand(S - 32) <= cap
    ys = random_logits(case, S)
    thr, nms_thr = 0.25, cfg.IOU_THRESHOLD
    ws = L.Workspace(dev)
    per_class, _, dec = run_detect(dev, ys, S, ANCHORS, WIN2, thr, nms_thr, mode="per_class", ws=ws)
    above = (dec[1] > np.float32(thr)).sum(axis=1)
    if case == "dense":
        assert above.tolist() == [n_cand(S)] * 2
        assert (above > cap).all() if S > 576 else (above <= cap).all()
    elif case == "sparse":
        assert (0 < above).all() and (above < 1024).all()
    else:
        assert (above > 8192).all() and (above <= cap).all()      # more than a per-class register list holds
    for mode in modes:
        got, cnt, dec2 = run_detect(dev, ys, S, ANCHORS, WIN2, thr, nms_thr, mode=mode, ws=ws)
        assert all(np.array_equal(a, b) for a, b in zip(dec, dec2))
        want, want_cnt = restated(dec, thr, nms_thr, mode)
        np.testing.assert_array_equal(got, want)
        assert cnt == want_cnt and min(cnt) > 0
        if mode == "agnostic":
            assert not np.array_equal(got, per_class), "the case does not tell the two methods apart"
            np.testing.assert_array_equal(per_class, restated(dec, thr, nms_thr, "per_class")[0])
        else:
            assert cnt == [MAX_DET] * 2 and not np.array_equal(got, restated(dec, thr, nms_thr, "agnostic")[0])


# ---- 4. through the net
def make_net(dev, training, nms, B=2, S=96, seed=0):
    net = YOLONet(training=training, device=dev, image_size=S, batch_size=B, stage=1, seed=seed, nms=nms)
    g = torch.Generator().manual_seed(7919 + seed)
    with torch.no_grad():
        for i in (59, 67, 75, 82):
            net.params["yolo/convolutional%d/weights" % i].mul_(6.0)
            b = net.params["yolo/convolutional%d/biases" % i]
            b.copy_((torch.randn(b.shape, generator=g) * 0.5).to(b.device))
    net.refresh_weights()
    return net


@pytest.mark.parametrize("mode", R.MODES)
def test_inference_net_follows_its_mode(dev, mode):
    B, S, thr = 2, 96, 0.05
    net = make_net(dev, False, mode)
    assert net.nms == mode
    b = O.synthetic_batch(B, S, seed=5)
    b["clip_window"][1] = [0.1, 0.05, 0.9, 0.8]
    _, det, _ = net.forward(b["images"], b["clip_window"], [thr], is_training=False)
    torch.cuda.synchronize()
    got = det.cpu().numpy()
    dec = decoded(net.ws_det, B, n_cand(S))
    want, want_cnt = restated(dec, thr, cfg.IOU_THRESHOLD, mode)
    np.testing.assert_array_equal(got, want)
    assert net.det_count.cpu().tolist() == want_cnt and sum(want_cnt) >= 20
    others = [restated(dec, thr, cfg.IOU_THRESHOLD, m)[0] for m in R.MODES if m != mode]
    assert not any(np.array_equal(want, o) for o in others), "the batch does not tell the modes apart"
    # evaluation: boxes and masks of the net's own detections
    det_box, det_mask = net.evaluation(b["images"], b["clip_window"], [thr])
    torch.cuda.synchronize()
    np.testing.assert_array_equal(net.detections.cpu().numpy(), want)
    wb, wm = O.val_test(want, net.by_idx[82].act.cpu())
    for i in range(B):
        np.testing.assert_array_equal(det_box[i], wb[i])
        np.testing.assert_allclose(det_mask[i], wm[i], rtol=1e-5, atol=1e-6)
    # the recorded inference program runs the same filter
    keep, masks = net.keep.clone(), net.masks.clone()
    net.build_infer_program(det_thresh=thr, graph=False)
    net.detections.fill_(float("nan"))
    net.det_count.fill_(-1)
    d2, c2, m2, k2 = net.infer(b["images"], b["clip_window"])
    torch.cuda.synchronize()
    np.testing.assert_array_equal(d2.cpu().numpy(), want)
    assert c2.cpu().tolist() == want_cnt and torch.equal(k2, keep) and torch.equal(m2, masks)


# ---- 5. training: the mode picks the mask-loss RoIs
def test_training_net_takes_its_mask_rois_from_the_agnostic_filter(dev):
    B, S, thr = 2, 64, 0.1
    # (batch 33 with net seed 1: of 60 batch / net seeds tried, the one where the two filters' detections differ among the seven
    #  the mask loss draws AND one of those is a positive RoI -- 4 RoIs on the second image per class, 3 agnostic)
    b = O.synthetic_batch(B, S, seed=33)
    rng = np.random.RandomState(0)
    perm_det = np.stack([rng.permutation(cfg.MAX_DETECTION) for _ in range(B)]).astype(np.int32)
    perm_gt = np.stack([rng.permutation(cfg.MAX_BOX_PER_IMAGE) for _ in range(B)]).astype(np.int32)
    b["perm_det"], b["perm_gt"] = perm_det, perm_gt
    perms = [(perm_det[i], perm_gt[i]) for i in range(B)]
    net = make_net(dev, True, "agnostic", B=B, S=S, seed=1)
    ref = make_net(dev, True, "per_class", B=B, S=S, seed=1)
    ref.load_state_dict(net.state_dict())
    for n in (net, ref):
        n.set_batch(b)
        n.compute_losses(thr)
    torch.cuda.synchronize()
    det = net.detections.cpu().numpy()
    want, want_cnt = restated(decoded(net.ws_det, B, n_cand(S)), thr, cfg.IOU_THRESHOLD, "agnostic")
    np.testing.assert_array_equal(det, want)
    assert net.det_count.cpu().tolist() == want_cnt
    # ... which are the restatement's on the net's own logits, up to the device's expf (tests/test_gpu_net.py's tolerance)
    yolos = [net.by_idx[i].act.cpu().view(B, net.by_idx[i].Ho, net.by_idx[i].Wo, 3, 8) for i in (75, 67, 59)]
    np.testing.assert_allclose(det, R.filter_logits(yolos, b["clip_window"], thr, O.IOU_THRESHOLD, MAX_DET, "agnostic"),
                               rtol=1e-5, atol=1e-6)
    mp = net.by_idx[82].act.cpu().clone().requires_grad_(True)
    lm = O.loss_mask(det, mp, b["true_boxes"].numpy(), b["true_masks"], perms)
    assert int(net.roi_count.sum()) > 0, "test needs at least one positive RoI"
    lm.backward()
    np.testing.assert_allclose(float(net.mask_loss.cpu()[0]), float(lm), rtol=2e-4)
    ds = net.by_idx[82].dx.float().cpu()
    assert float(ds[..., 9:].abs().max()) == 0.0
    r = float((ds[..., :9].double() - mp.grad.double()).norm() / mp.grad.double().norm())
    assert r < 6e-3, "dscore rel err %.3g" % r
    # the per-class net, same batch, same weights: other detections, other RoIs, another mask loss
    assert torch.equal(ref.by_idx[75].act, net.by_idx[75].act)
    assert not torch.equal(ref.detections, net.detections)
    assert not (torch.equal(ref.rois, net.rois) and torch.equal(ref.roi_count, net.roi_count))
    assert float(ref.mask_loss.cpu()[0]) != float(net.mask_loss.cpu()[0])


def test_recorded_agnostic_step_is_bitwise_identical_to_eager(dev):
    B, S = 2, 64
    b = O.synthetic_batch(B, S, seed=21)
    nets = [make_net(dev, True, "agnostic", B=B, S=S, seed=4) for _ in range(2)]
    nets[1].load_state_dict(nets[0].state_dict())
    for n in nets:
        n.set_batch(b)
    nets[1].build_program(det_thresh=0.1)
    l0 = float(nets[0].train_step(None, det_thresh=0.1).cpu())
    l1 = float(nets[1].train_step(None).cpu())
    torch.cuda.synchronize()
    assert np.isfinite(l0) and l0 == l1
    assert torch.equal(nets[0].detections, nets[1].detections) and int(nets[0].det_count.sum()) > 0
    assert torch.equal(nets[0].arena, nets[1].arena) and torch.equal(nets[0].adam_v, nets[1].adam_v)
    for name in nets[0].params:
        assert torch.equal(nets[0].params[name], nets[1].params[name]), name

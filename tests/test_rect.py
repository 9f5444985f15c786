"""Rectangular nets, image_size = (H, W), on the CPU: the test-side reference (tests/rect_ref.py) against the oracle at H = W,
``synth`` and ``postprocess`` against golden files written by the reference's own code at net_h != net_w, the plan of a
rectangular net, and the oracle on every row of tests/test_gpu_rect.py."""
import json
import os

import numpy as np
import pytest
import torch

import disyolo_oracle as O
import mask_stride_ref as MR
import rect_ref as R
from disyolo_amd import postprocess as P
from disyolo_amd import synth
from disyolo_amd.net import YOLONet, check_image_size
from net_setup import perturb_variables

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


# ------------------------------------------------------------------------------------------------ rect_ref at H = W
def _same_batch(a, b):
    assert set(a) == set(b)
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y), k


@pytest.mark.parametrize("S,C,seed", [(64, 3, 11), (96, 6, 5)])
def test_square_synthetic_batch_and_targets_are_the_oracles(S, C, seed):
    _same_batch(R.synthetic_batch(2, S, S, seed=seed, num_class=C), O.synthetic_batch(2, S, seed=seed, num_class=C))
    rng = np.random.RandomState(seed)
    boxes = np.stack([rng.uniform(0, S, 12), rng.uniform(0, S, 12), rng.uniform(2, S, 12), rng.uniform(2, S, 12)], 1).astype(np.float32)
    cls = rng.randint(0, C, 12)
    for a, b in zip(R.assign_targets(boxes, cls, S, S, num_class=C), O.assign_targets(boxes, cls, S, num_class=C)):
        assert np.array_equal(a, b)


def _square_case(k, m, S=64, B=2, seed=11):
    """detections with boxes of positive area, score maps and a batch at S x S (computed on the CPU, no net)"""
    b = O.synthetic_batch(B, S, seed=seed)
    g = torch.Generator().manual_seed(seed)
    mask_pos = torch.randn(B, S // m, S // m, k * k, generator=g)
    det = np.zeros((B, O.MAX_DETECTION, 6), np.float32)
    tb = b["true_boxes"].numpy()[:, 0, 0, 0]
    for i in range(B):
        rows = np.where(np.abs(tb[i, :, :4]).sum(1) != 0)[0]
        for r, j in enumerate(rows):
            xc, yc, w, h = tb[i, j, :4]
            det[i, r] = [yc - 0.45 * h, xc - 0.45 * w, yc + 0.55 * h, xc + 0.5 * w, tb[i, j, 4], 0.9 - 0.1 * r]
    rng = np.random.RandomState(0)
    perms = [(rng.permutation(O.MAX_DETECTION), rng.permutation(O.MAX_BOX_PER_IMAGE)) for _ in range(B)]
    return b, mask_pos, det, perms


@pytest.mark.parametrize("k,m", [(3, 2), (5, 4), (7, 1)])
def test_square_mask_term_and_assembly_are_the_oracles(k, m):
    b, mask_pos, det, perms = _square_case(k, m)
    want = MR.loss_mask(det, mask_pos, b["true_boxes"].numpy(), b["true_masks"], perms, k)
    got = R.loss_mask(det, mask_pos, b["true_boxes"].numpy(), b["true_masks"], perms, k)
    assert np.isfinite(float(want)) and float(want) > 0
    assert float(got) == float(want)
    if k == 3:
        wb, wm = O.val_test(det, mask_pos)
        gb, gm = R.val_test(det, mask_pos, k)
        assert any(np.ndim(w) for w in wm)
        for a, c in zip(gb + gm, wb + wm):
            assert np.array_equal(a, c)
        for i in range(2):
            px = np.round(det[i, 0, :4] * np.float32(mask_pos.shape[1]))
            assert np.array_equal(R.channel_index_map(px, mask_pos.shape[1], mask_pos.shape[2], k),
                                  O.channel_index_map(px, mask_pos.shape[1], k))


def test_square_total_loss_is_the_oracles():
    """the whole composition at H = W on a small net (B = 1, 64^2, m = 1/4: the shortest forward), bit for bit"""
    net = YOLONet(training=True, plan_only=True, seed=1, image_size=64, batch_size=1, mask_stride=4, k_map=5)
    perturb_variables(net, 1)
    p = {k: v.detach().float().clone() for k, v in net.params.items()}
    b = O.synthetic_batch(1, 64, seed=11)
    lock = MR.default_lock(1, 4)
    with torch.no_grad():
        want = MR.total_loss(p, b, lock, 4, 5, None, {}, obj_thresh=0.1, quant=O.bf16_ste)
        got = R.total_loss(p, b, lock, 4, 5, None, {}, obj_thresh=0.1, quant=O.bf16_ste)
    for n in want[0]:
        assert float(got[0][n]) == float(want[0][n]) or (np.isnan(float(got[0][n])) and np.isnan(float(want[0][n]))), n
    assert np.array_equal(got[1], want[1])


def test_square_letterbox_and_paste_are_the_oracles():
    rng = np.random.RandomState(2)
    for (h, w) in [(348, 620), (600, 800), (450, 386)]:
        for S in (64, 96):
            assert np.array_equal(R.letterbox_window(h, w, S, S), O.letterbox_window(h, w, S))
            assert np.array_equal(P.letterbox_window(h, w, S), O.letterbox_window(h, w, S))
            assert np.array_equal(P.letterbox_window(h, w, (S, S)), O.letterbox_window(h, w, S))
    rgb = rng.randint(0, 256, size=(35, 62, 3)).astype(np.uint8)
    a, wa = R.image_read(rgb, 64, 64)
    c, wc = O.image_read(rgb, 64)
    assert np.array_equal(a, c) and np.array_equal(wa, wc)
    box = np.array([[0.3, 0.1, 0.7, 0.8, 1, 0.9], [0.25, 0.4, 0.6, 0.9, 0, 0.8], [0.5, 0.5, 0.5, 0.5, 2, 0.7]], np.float32)
    masks = rng.rand(3, 32, 32).astype(np.float32)
    ea, ma = R.paste_detections(box, masks, 35, 62, 64, 64)
    ec, mc = O.paste_detections(box, masks, 35, 62, 64)
    assert np.array_equal(ma, mc) and len(ea) == len(ec) == 2
    for x, y in zip(ea, ec):
        assert x["index"] == y["index"] and x["classid"] == y["classid"] and np.array_equal(x["mask"], y["mask"])
    rects, ok = P.paste_rects(box, 35, 62, 64, 32)
    rects2, ok2 = P.paste_rects(box, 35, 62, (64, 64), (32, 32))
    assert np.array_equal(rects, rects2) and np.array_equal(ok, ok2)


# ------------------------------------------------------------------------------------------------ the reference's own code at net_h != net_w
def test_target_assignment_matches_the_reference_at_rectangular_sizes():
    cases = json.load(open(os.path.join(GOLDEN, "assign_targets_rect.json")))["cases"]
    assert len(cases) >= 16 and {tuple(c["net_hw"]) for c in cases} >= {(64, 128), (128, 64)}
    seen_objects = 0
    for c in cases:
        H, W = c["net_hw"]
        boxes = np.array(c["true_box_xcycwh"], np.float32)
        cls = np.array([r[4] for r in c["boxes_x1y1x2y2c"]]).astype(int)
        for ys in (R.assign_targets(boxes, cls, H, W), synth.assign_targets(boxes, cls, (H, W), 3)):
            assert [y.shape[:2] for y in ys] == [(H // d, W // d) for d in (8, 16, 32)]
            got = [{"grid": gi, "idx": [int(v) for v in idx], "row": ys[gi][tuple(idx)].tolist()}
                   for gi in range(3) for idx in np.argwhere(ys[gi][..., 4] == 1)]
            assert got == c["objects"], c["net_hw"]
        seen_objects += len(c["objects"])
    assert seen_objects >= 40


def test_correct_yolo_boxes_and_paste_rects_match_the_reference_at_rectangular_sizes():
    cases = json.load(open(os.path.join(GOLDEN, "correct_yolo_boxes_rect.json")))["cases"]
    assert len(cases) >= 100 and {tuple(c["net_hw"]) for c in cases} >= {(64, 128), (128, 64)}
    for c in cases:
        x1, y1, x2, y2 = c["box"]
        (h, w), (nh, nw) = c["image_hw"], c["net_hw"]
        assert list(O.correct_yolo_boxes(x1, y1, x2, y2, h, w, nh, nw)) == c["out"]
        got = P.correct_yolo_boxes(np.array([[y1, x1, y2, x2]], np.float32), h, w, nh, nw)[0]
        assert [int(v) for v in got] == c["out"]
        rects, _ = P.paste_rects(np.array([[y1, x1, y2, x2, 0, 1]], np.float32), h, w, (nh, nw), (nh // 2, nw // 2))
        dst = [int(rects[0, 5]), int(rects[0, 4]), int(rects[0, 7]), int(rects[0, 6])]
        assert dst == c["out"] or not rects.any()
        assert np.array_equal(P.letterbox_window(h, w, (nh, nw)), R.letterbox_window(h, w, nh, nw))


def test_paste_rects_scale_each_axis_by_its_own_side():
    box = np.array([[2.5 / 32, 3.5 / 64, 20.5 / 32, 40.5 / 64, 1, 0.9]], np.float32)
    rects, ok = P.paste_rects(box, 64, 128, (64, 128), (32, 64))
    assert ok[0] and list(rects[0, :4]) == [2, 4, 20, 40]        # half to even: 2.5 -> 2, 3.5 -> 4, 20.5 -> 20, 40.5 -> 40


@pytest.mark.parametrize("H,W", [(64, 128), (128, 64), (96, 160)])
def test_synthetic_batch_matches_the_reference_side(H, W):
    a = synth.synthetic_batch(2, (H, W), seed=11, num_class=6)
    b = R.synthetic_batch(2, H, W, seed=11, num_class=6)
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
    assert a["images"].shape == (2, H, W, 3) and a["true_masks"].shape == (2, 20, H, W)
    assert a["yolo1"].shape == (2, H // 32, W // 32, 3, 11)
    tb = a["true_boxes"][:, 0, 0, 0]
    live = np.abs(tb[..., :4]).sum(-1) != 0
    assert live.any() and (tb[live][:, :4] <= 1).all() and (tb[live][:, :4] >= 0).all()


# ------------------------------------------------------------------------------------------------ the plan
def test_plan_of_a_rectangular_net():
    net = YOLONet(image_size=(64, 96), plan_only=True)
    sq = YOLONet(image_size=64, plan_only=True)
    assert (net.H, net.W, net.S, net.image_size) == (64, 96, None, (64, 96))
    assert (sq.H, sq.W, sq.S, sq.image_size) == (64, 64, 64, 64) and isinstance(sq.image_size, int)
    eq = YOLONet(image_size=(64, 64), plan_only=True)
    assert (eq.H, eq.W, eq.S, eq.image_size) == (64, 64, 64, 64)
    assert {n: tuple(v.shape) for n, v in net.params.items()} == {n: tuple(v.shape) for n, v in sq.params.items()}
    assert net.arena_slices == sq.arena_slices
    assert net.mask_map_size() == (32, 48)


def test_layer_sizes_of_a_rectangular_plan():
    """per-layer H, W of the plan: rows halve with rows, columns with columns, the up-sampled joins meet their skips"""
    net = YOLONet(image_size=(64, 96), plan_only=True)
    size = {l.idx: (l.Ho, l.Wo) for l in net.layers}
    assert (net.by_idx[1].H, net.by_idx[1].W) == (64, 96)
    assert size[1] == (64, 96) and size[2] == (32, 48) and size[5] == (16, 24) and size[10] == (8, 12)
    assert size[59] == (2, 3) and size[67] == (4, 6) and size[75] == (8, 12) and size[net.score_layer] == (32, 48)
    for l in net.layers:
        assert (l.H, l.W) == ((64, 96) if l.src == 0 else size[l.src]), l.idx
        assert (l.Ho, l.Wo) == (-(-l.H // l.stride), -(-l.W // l.stride)), l.idx
        if l.src_up is not None:
            hu, wu = size[l.src_up]
            assert size[l.src] == (2 * hu, 2 * wu), l.idx
    for m, want in ((4, (16, 24)), (1, (64, 96))):
        n2 = YOLONet(image_size=(64, 96), plan_only=True, mask_stride=m)
        assert (n2.by_idx[n2.score_layer].Ho, n2.by_idx[n2.score_layer].Wo) == want == n2.mask_map_size()


def test_square_state_dict_loads_into_a_rectangular_net():
    sq = YOLONet(image_size=64, plan_only=True, seed=3)
    perturb_variables(sq, 3)
    net = YOLONet(image_size=(96, 32), plan_only=True, seed=9)
    net.load_state_dict(sq.state_dict())
    for n, v in sq.params.items():
        assert torch.equal(net.params[n], v), n


@pytest.mark.parametrize("bad", [48, 0, -32, (64, 48), (0, 64), (64, 0), (64, 64, 3), (64,), (64.0, 96), "64", (True, 64)])
def test_bad_sizes_raise(bad):
    with pytest.raises(ValueError):
        YOLONet(image_size=bad, plan_only=True)
    with pytest.raises(ValueError):
        check_image_size(bad)


# ------------------------------------------------------------------------------------------------ the rows of the GPU tests
@pytest.mark.parametrize("row", R.VALUE_ROWS, ids=R.ids(R.VALUE_ROWS))
def test_oracle_is_finite_with_a_positive_roi_on_every_row(row):
    what = R.describe(row)
    net = YOLONet(training=True, plan_only=True, seed=1, **R.net_kwargs(row))
    perturb_variables(net, 1)
    assert set(net.trainable_names()) == set(R.trainable_names(row)), what
    b, perms = R.row_batch(row)
    p = {k: v.detach().float().clone() for k, v in net.params.items()}
    with torch.no_grad():
        parts, det, yolos, mask_pos = R.oracle_total_loss(row, p, b, perms, updates={})
    assert [tuple(y.shape[1:]) for y in yolos] == [(row.H // d, row.W // d, 3, 5 + row.C) for d in (8, 16, 32)], what
    assert tuple(mask_pos.shape) == (row.B, row.H // row.m, row.W // row.m, row.k ** 2), what
    bad = [n for n, v in parts.items() if not np.isfinite(float(v))]
    assert not bad, "%s: oracle loss parts not finite: %s" % (what, bad)
    nroi = [len(O.select_mask_rois(det[i], b["true_boxes"].numpy()[i, 0, 0, 0], *perms[i])[0]) for i in range(row.B)]
    assert sum(nroi) > 0 and float(parts["mask"]) > 0, "%s: the oracle has no positive RoI (RoIs per image %s)" % (what, nroi)


def test_square_loader_pixels_are_the_oracles():
    """the placement and blur restatements at net_h = net_w against the oracle's, bit for bit: pad, crop and overhang on each
    side, the three flips"""
    rng = np.random.RandomState(4)
    img = rng.randint(0, 256, (40, 50, 3)).astype(np.uint8)
    mask = (rng.rand(40, 50) < 0.4).astype(np.uint8)
    for (nw, nh, dx, dy) in [(64, 51, 0, 6), (48, 38, 9, 20), (90, 141, -13, -40), (95, 95, -31, -16)]:
        for flip in (1, 2, 3):
            assert np.array_equal(R.place_image(img, 64, 64, nw, nh, dx, dy, flip), O.place_image(img, 64, nw, nh, dx, dy, flip))
            assert np.array_equal(R.place_mask(mask, 64, 64, nw, nh, dx, dy, flip), O.place_mask(mask, 64, nw, nh, dx, dy, flip))
    sq = rng.randint(0, 256, (48, 48, 3)).astype(np.uint8)
    for angle in (0, 45, 90, 135):
        for lt in (0, 1, 2):
            assert np.array_equal(R.motion_blur3(sq, angle, lt), O.motion_blur3(sq, angle, lt))


def test_loader_restatement_fits_by_the_binding_side():
    """rect_ref.loader_sample without augmentation draws (scale_crop forced to 1 by a RandomState stub): a 100 x 300 image in a
    64 x 128 net is bound by the width (new_w = 128, new_h = 42, dy = 11), a 300 x 100 image by the height (new_h = 64,
    new_w = 21, dx = 53); at a square net the test is the reference's ``new_ar < 1``"""
    class Ones:
        def randint(self, low=None, high=None, size=None):
            return 1
    for (h, w, nh, nw, want) in [(100, 300, 64, 128, (128, 42, 0, 11)), (300, 100, 64, 128, (21, 64, 53, 0)),
                                 (100, 150, 64, 128, (96, 64, 16, 0)), (100, 300, 64, 64, (64, 21, 0, 21)),
                                 (300, 100, 64, 64, (21, 64, 21, 0))]:
        dec, boxes, ys = R.loader_sample(Ones(), h, w, np.array([[10, 10, 60, 50]], np.float32), [1], nh, nw)
        assert (dec["new_w"], dec["new_h"], dec["dx"], dec["dy"]) == want, (h, w, nh, nw, dec)
        assert dec["flip"] == 1 and dec["bnl"] == 1 and boxes.shape == (1, 4) and (boxes >= 0).all() and (boxes <= 1).all()
        assert sum(int((y[..., 4] == 1).sum()) for y in ys) == 1

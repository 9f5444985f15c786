"""Tiled evaluation on the GPU: disyolo_tile_group_counts, ``MAP.collect_tiled`` and ``evaluate(tiled=...)`` against the numpy
definition (tests/tiles_eval_ref.py).  Counts are integers and IoUs f32 quotients of integers: equality throughout."""
import numpy as np
import pytest
import torch

import net_setup as NS
import option_matrix as OM
import tiles_eval_ref as ER
import tiles_ref as TR
from disyolo_amd import evaluate as EV
from disyolo_amd import lib as L
from disyolo_amd import tiles as TL
from disyolo_amd.net import YOLONet

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ the kernel
HW = (70, 150)
# group boxes: x origins at 20 mod 32
GROUP_BOXES = [(10, 20, 50, 80),      # 40 x 60 = 2400 px: two blocks add into one count
               (3, 52, 30, 147),      # 27 x 95 = 2565 px, no multiple of 16
               (40, 84, 70, 150),     # on the right and the bottom border, 1980 px
               (0, 20, 7, 23),        # 3 columns wide, 21 px: 11 padding bytes behind it
               (33, 116, 34, 150)]    # one row
# ground-truth boxes: x origins at 5 mod 32, but for the last two real ones (the same origin as a group / a multiple of 32 off)
GT_BOXES = [(5, 5, 45, 75),           # left of group 0 (negative shift), 70 columns: wider than 64
            (12, 37, 60, 40),         # right of group 0's origin, 3 columns: the intersection is 3 wide
            (20, 69, 21, 140),        # one row; across group 1 it spans three words
            (50, 101, 70, 150),       # on the right and the bottom border
            (30, 20, 65, 140),        # group 0's own x origin; 64 and 96 left of group 2's and 4's (multiples of 32)
            (2, 52, 29, 84)]          # group 1's own x origin, ends on a word's edge


def kernel_case(dev):
    rng = np.random.default_rng(12)
    boxes = np.array(GROUP_BOXES, np.int32)
    groups, arena_bytes = L.tile_compose_plan(boxes, np.arange(len(boxes) + 1))
    arena = np.ones(arena_bytes, np.uint8)                                  # the padding stays 1: it must not be counted
    for g in groups:
        n = int((g[4] - g[2]) * (g[5] - g[3]))
        arena[16 * g[7]:16 * g[7] + n] = rng.random(n) < 0.5
    gt_masks = []
    for y1, x1, y2, x2 in GT_BOXES:
        m = np.zeros(HW, bool)
        m[y1:y2, x1:x2] = rng.random((y2 - y1, x2 - x1)) < 0.5
        m[y1, x1] = m[y2 - 1, x2 - 1] = True                                # the tight box is the box
        gt_masks.append(m)
    gt_masks.append(np.zeros(HW, bool))                                     # an instance without pixels
    gt, words = ER.pack_gt(gt_masks)
    assert gt[:6, :4].tolist() == [list(b) for b in GT_BOXES]
    pairs2 = [(g, -1) for g in range(len(boxes))] + [(g, j) for g in range(len(boxes)) for j in range(len(gt_masks))]
    return groups, arena, gt_masks, gt, words, pairs2


def test_group_counts_kernel(dev):
    groups, arena, gt_masks, gt, words, pairs2 = kernel_case(dev)
    assert sorted({int(g[3]) % 32 for g in groups}) == [20] and sorted({int(t[1]) % 32 for t in gt[:4]}) == [5]
    assert any(int(g[4] - g[2]) * int(g[5] - g[3]) % 16 for g in groups)
    want = ER.group_counts(groups, arena, gt_masks, pairs2)
    pairs, blocks = L.tile_group_counts_plan(groups, gt, pairs2)
    assert blocks > len(pairs2)                                             # some pair takes more than one block
    arena_d = torch.from_numpy(arena).to(dev)
    bits_d = torch.from_numpy(words.view(np.int32)).to(dev)
    got = L.tile_group_counts(groups, arena_d, gt, bits_d, pairs, HW)
    assert got.dtype == torch.int32 and tuple(got.shape) == (len(pairs2),)
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    again = L.tile_group_counts(groups, arena_d, gt, bits_d, pairs, HW)
    assert torch.equal(got, again)
    # the cases are what they claim to be
    by_pair = dict(zip(pairs2, want.tolist()))
    assert all(by_pair[(g, -1)] > 0 for g in range(5))
    for g, j in [(0, 0), (0, 1), (1, 2), (2, 3), (0, 4), (2, 4), (1, 5), (1, 0), (4, 4)]:
        assert by_pair[(g, j)] > 0, (g, j)
    for g, j in [(3, 3), (0, 3), (4, 0), (0, 6), (2, 6)]:                   # empty intersections, and the empty instance
        assert by_pair[(g, j)] == 0, (g, j)
    assert by_pair[(0, 1)] <= 3 * 38 and by_pair[(1, 2)] <= 71
    # device copies passed in go the same way
    got = L.tile_group_counts(groups, arena_d, gt, bits_d, pairs, HW, groups_dev=torch.from_numpy(groups).to(dev),
                              gt_dev=torch.from_numpy(gt).to(dev), pairs_dev=torch.from_numpy(pairs).to(dev))
    np.testing.assert_array_equal(got.cpu().numpy(), want)


def test_group_counts_strides_over_a_large_rectangle(dev):
    """more than 1024 chunks of 2048 pixels: the pair's 1024 blocks each take several chunks, the last one partly"""
    hw = (1450, 1500)
    rng = np.random.default_rng(13)
    groups, arena_bytes = L.tile_compose_plan(np.array([[1, 20, 1450, 1500], [7, 52, 9, 61]], np.int32), [0, 1, 2])
    assert 1449 * 1480 > 1024 * 2048 and (1449 * 1480) % 2048
    arena = (rng.random(arena_bytes) < 0.5).astype(np.uint8)
    gt_mask = np.zeros(hw, bool)
    gt_mask[0:1440, 5:1490] = rng.random((1440, 1485)) < 0.5
    gt_mask[0, 5] = gt_mask[1439, 1489] = True
    gt, words = EV.gt_bit_planes([gt_mask])                                 # (pack_gt's layout: tests/test_tiles_eval.py)
    pairs2 = [(0, -1), (0, 0), (1, -1), (1, 0)]
    pairs, blocks = L.tile_group_counts_plan(groups, gt, pairs2)
    assert pairs[:, 2].tolist() == [0, 1024, 2048, 2049] and blocks == 2050
    got = L.tile_group_counts(groups, torch.from_numpy(arena).to(dev), gt, torch.from_numpy(words.view(np.int32)).to(dev), pairs, hw)
    np.testing.assert_array_equal(got.cpu().numpy(), ER.group_counts(groups, arena, [gt_mask], pairs2))


def test_group_counts_of_nothing(dev):
    groups, arena, gt_masks, gt, words, _ = kernel_case(dev)
    arena_d = torch.from_numpy(arena).to(dev)
    bits_d = torch.from_numpy(words.view(np.int32)).to(dev)
    pairs, blocks = L.tile_group_counts_plan(groups, gt, np.zeros((0, 2), np.int32))
    assert tuple(L.tile_group_counts(groups, arena_d, gt, bits_d, pairs, HW).shape) == (0,) and blocks == 0              # P = 0
    none = np.zeros((0, 8), np.int32)
    assert tuple(L.tile_group_counts(none, arena_d, gt, bits_d, pairs, HW).shape) == (0,)                                 # G = 0
    # without ground truth the groups' own counts are still taken
    pairs, _ = L.tile_group_counts_plan(groups, none, [(g, -1) for g in range(5)])
    got = L.tile_group_counts(groups, arena_d, none, torch.zeros(0, dtype=torch.int32, device=dev), pairs, HW)
    np.testing.assert_array_equal(got.cpu().numpy(), ER.group_counts(groups, arena, [], [(g, -1) for g in range(5)]))
    with pytest.raises(L.DisyoloError):
        L.tile_group_counts(groups, arena_d, gt, bits_d, np.array([[5, -1, 0]], np.int32), HW)


# ------------------------------------------------------------------------------------------------ collect_tiled on the scene
COLLECT_CASES = {"o16": dict(net_size=(64, 96), overlap=16), "o32": dict(net_size=(64, 96), overlap=32),
                 "m4": dict(net_size=(64, 96), overlap=16, mask_stride=4)}
KNOWN = {0.5: [(1.0, 1.0, 1.0)] * 3, 1.0: [(1 / 2, 1 / 7, 1 / 14), (1, 2 / 3, 5 / 6), (1, 1, 1)]}


def scene_map(sc, classes=None):
    recs = {"scene": ER.records(sc.objects)}
    true_map = ER.class_map(sc.objects, sc.image_hw)
    return EV.MAP(recs, {"scene": list(sc.image_hw)}, ["scene"], merged={"scene": true_map}, net_size=sc.net_size,
                  classes=classes), recs, true_map


@pytest.mark.parametrize("name", sorted(COLLECT_CASES))
def test_collect_tiled_on_the_scene(dev, name, monkeypatch):
    monkeypatch.delenv("DISYOLO_EVAL_GPU_IOU", raising=False)
    sc = TR.scene(**COLLECT_CASES[name])
    masks_d = torch.from_numpy(sc.masks).to(dev)
    for mo in (0.5, 1.0) if name == "o16" else (0.5,):
        want = TR.merge_tiles(sc.tiles, sc.image_hw, sc.net_size, sc.detections, sc.keep, sc.masks, mo)
        res = TL.merge_tiles(sc.tiles, sc.image_hw, sc.net_size, sc.detections, sc.keep, masks_d, mo)
        m, recs, true_map = scene_map(sc)
        detfile = {str(c): [] for c in m.classid}
        conf = torch.zeros(16, dtype=torch.int64, device=dev)
        merged = m.collect_tiled("scene", res, detfile, true_map=true_map, conf=conf)
        assert merged is res.merged
        ref = ER.collect_tiled(want, recs, "scene", sc.image_hw, m.classid, ov=True)
        for c in m.classid:
            assert len(detfile[str(c)]) == len(ref[str(c)]) > 0
            for e, r in zip(detfile[str(c)], ref[str(c)]):
                assert set(e) == {"imageid", "score", "ov"} and e["imageid"] == "scene" and e["score"] == r["score"]
                assert e["ov"].dtype == np.float32
                np.testing.assert_array_equal(e["ov"], r["ov"])
        got_table = ER.ap_table(detfile, recs, ["scene"], m.classid)
        assert got_table == ER.ap_table(ER.collect_tiled(want, recs, "scene", sc.image_hw, m.classid), recs, ["scene"], m.classid)
        assert all(g == pytest.approx(w, abs=1e-12) for a, b in zip(got_table, KNOWN[mo]) for g, w in zip(a, b)), got_table
        assert m._ap_table(detfile)[0]["AP"] == [t[2] for t in got_table]
        np.testing.assert_array_equal(conf.cpu().numpy(), ER.confusion(true_map, want.merged, 4))
        # the ground truth was uploaded once: a second sweep finds it cached and appends the same entries again
        cached = m._gt_cache[("planes", "scene")]
        m.collect_tiled("scene", res, detfile)
        assert m._gt_cache[("planes", "scene")] is cached and len(detfile["0"]) == 2 * len(ref["0"])
        # a class list of six names: the same rows, and the confusion through confusion_n
        m6, _, _ = scene_map(sc, classes=OM.names(6))
        detfile6 = {str(c): [] for c in m6.classid}
        conf6 = torch.zeros(49, dtype=torch.int64, device=dev)
        m6.collect_tiled("scene", res, detfile6, true_map=true_map, conf=conf6)
        np.testing.assert_array_equal(conf6.cpu().numpy(), ER.confusion(true_map, want.merged, 7))
        assert [len(detfile6[str(c)]) for c in m6.classid] == [len(ref[str(c)]) for c in range(3)] + [0, 0, 0]
        # the host path is the comparator: full-size masks to voc_eval
        monkeypatch.setenv("DISYOLO_EVAL_GPU_IOU", "0")
        mh, _, _ = scene_map(sc)
        host = {str(c): [] for c in mh.classid}
        mh.collect_tiled("scene", res, host)
        assert all("mask" in e and "ov" not in e for c in mh.classid for e in host[str(c)])
        assert ER.ap_table(host, recs, ["scene"], mh.classid) == got_table
        monkeypatch.delenv("DISYOLO_EVAL_GPU_IOU")


def test_collect_tiled_without_groups_or_ground_truth(dev):
    sc = TR.scene()
    masks_d = torch.from_numpy(sc.masks).to(dev)
    m, recs, true_map = scene_map(sc)
    res = TL.merge_tiles(sc.tiles, sc.image_hw, sc.net_size, sc.detections, np.zeros_like(sc.keep), masks_d)
    detfile = {str(c): [] for c in m.classid}
    conf = torch.zeros(16, dtype=torch.int64, device=dev)
    m.collect_tiled("scene", res, detfile, true_map=true_map, conf=conf)
    assert not any(detfile.values())
    np.testing.assert_array_equal(conf.cpu().numpy(), ER.confusion(true_map, np.zeros(sc.image_hw, np.uint8), 4))
    # an image without class 1 and 2 in its ground truth: those classes get empty rows, as in collect
    res = TL.merge_tiles(sc.tiles, sc.image_hw, sc.net_size, sc.detections, sc.keep, masks_d)
    only0 = EV.MAP({"scene": [r for r in recs["scene"] if r["classid"] == 0]}, {"scene": list(sc.image_hw)}, ["scene"])
    only0.collect_tiled("scene", res, detfile)
    assert [e["ov"].shape for e in detfile["1"] + detfile["2"]] == [(0,)] * 3 and all(e["ov"].shape == (2,) for e in detfile["0"])


# ------------------------------------------------------------------------------------------------ evaluate(tiled=...)
NETS = {"A: k3 m2": dict(k_map=3, mask_stride=2),
        "B: k5 m4 C6 agnostic": dict(k_map=5, mask_stride=4, classes=OM.names(6), nms="agnostic")}
THR = 0.05
IMAGE_SIZES = {"big": (150, 200), "net": (64, 96), "small": (50, 70)}


def make_net(dev, kw, seed=0, batch_size=2):
    net = YOLONet(training=False, device=dev, image_size=(64, 96), batch_size=batch_size, stage=1, seed=seed, **kw)
    NS.perturb_variables(net, seed)
    net.refresh_weights()
    return net


def dataset(sizes, num_class, seed):
    """random images of the given sizes with the scene's objects, cropped to each image, as their ground truth; with six
    classes the objects are relabelled 1, 3, 3, 5, 1"""
    rng = np.random.default_rng(seed)
    objects = TR.scene_objects()
    images, recs, merged = {}, {}, {}
    for name, (h, w) in sizes.items():
        images[name] = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
        objs = [((2 * c + 1) if num_class == 6 else c, m[:h, :w]) for c, m in objects]
        recs[name] = ER.records(objs, name)
        merged[name] = ER.class_map(objs, (h, w))
    return images, recs, merged


@pytest.mark.parametrize("name", sorted(NETS))
def test_evaluate_tiled_is_the_reference_loop(dev, name, monkeypatch):
    monkeypatch.delenv("DISYOLO_EVAL_GPU_IOU", raising=False)
    net = make_net(dev, NETS[name])
    C = net.num_class
    images, recs, merged = dataset(IMAGE_SIZES, C, seed=21)
    index = list(IMAGE_SIZES)
    m = EV.MAP(recs, {k: list(v) for k, v in IMAGE_SIZES.items()}, index, merged=merged, net_size=(64, 96),
               classes=NETS[name].get("classes"))
    thresh_out, mask_acc, timing = EV.evaluate(net, images, m, det_thresh=THR, tiled={"overlap": 16})
    assert set(timing) == {"prediction_s", "crop_assemble_s", "per_image_s"}
    assert timing["prediction_s"] > 0 and timing["crop_assemble_s"] > 0
    # the reference loop, by hand: the net's own per-tile outputs through the numpy merge and voc_eval
    classids = list(range(C))
    detfile = {str(c): [] for c in classids}
    conf = np.zeros((C + 1) ** 2, np.int64)
    groups = []
    for k in index:
        res = TL.detect_tiled(net, images[k], overlap=16, det_thresh=THR, merge_overlap=0.5, keep_tiles=True)
        det, keep, masks = (t.cpu().numpy() for t in res.tile_outputs)
        want = TR.merge_tiles(res.tiles, IMAGE_SIZES[k], (64, 96), det, keep, masks, 0.5)
        ER.extend(detfile, ER.collect_tiled(want, recs, k, IMAGE_SIZES[k], classids))
        conf += ER.confusion(merged[k], want.merged, C + 1)
        groups.append(len(want.boxes))
    table = ER.ap_table(detfile, recs, index, classids)
    print("%s: %s groups in the %d images; AP %s" % (name, groups, len(index), [t[2] for t in table]))
    assert min(groups) > 0, "the threshold leaves images without detections"
    # (assert_array_equal: a class without ground truth has recall 0 / 0 on both sides)
    np.testing.assert_array_equal(np.array(thresh_out[0]["AP"]), np.array([t[2] for t in table]))
    np.testing.assert_array_equal(np.array(thresh_out[0]["mAP"]), np.array([float(np.mean([t[i] for t in table])) for i in range(3)]))
    np.testing.assert_array_equal(np.array(mask_acc), np.array(ER.mask_acc(conf, C + 1)))
    # merge_overlap reaches the merge; unknown keys and a training net do not get as far as the device
    out2 = EV.evaluate(net, images, m, det_thresh=THR, tiled={"overlap": (16, 16), "merge_overlap": 1.0})
    assert len(out2[0][0]["AP"]) == C
    with pytest.raises(ValueError, match="stride"):
        EV.evaluate(net, images, m, det_thresh=THR, tiled={"overlap": 16, "stride": 3})


@pytest.mark.parametrize("name,B", [("A: k3 m2", 2), ("B: k5 m4 C6 agnostic", 1)])
def test_evaluate_tiled_of_net_sized_images_is_the_plain_path(dev, name, B, monkeypatch):
    monkeypatch.delenv("DISYOLO_EVAL_GPU_IOU", raising=False)
    net = make_net(dev, NETS[name], seed=1, batch_size=B)
    sizes = {"a": (64, 96), "b": (64, 96), "c": (64, 96)}
    images, recs, merged = dataset(sizes, net.num_class, seed=22)
    m = EV.MAP(recs, {k: list(v) for k, v in sizes.items()}, list(sizes), merged=merged, net_size=(64, 96),
               classes=NETS[name].get("classes"))
    plain = EV.evaluate(net, images, m, det_thresh=THR)
    tiled = EV.evaluate(net, images, m, det_thresh=THR, tiled={"overlap": 0})
    assert len(tiled[0]) == len(plain[0]) == 1 and tiled[0][0]["thresh"] == plain[0][0]["thresh"]
    for key in ("AP", "mAP"):
        np.testing.assert_array_equal(np.array(tiled[0][0][key]), np.array(plain[0][0][key]))
    np.testing.assert_array_equal(np.array(tiled[1]), np.array(plain[1]))
    assert np.isfinite(plain[1][0]) and plain[1][0] < 1.0                   # detections were pasted: the background IoU is below 1

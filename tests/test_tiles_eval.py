"""Tiled evaluation without a GPU: the numpy definition's known answers on the scene (the metric sees the merge), the
ground-truth bit planes, the launch plan of disyolo_tile_group_counts and the argument errors of the new entry points."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

import tiles_eval_ref as ER
import tiles_ref as TR
from disyolo_amd import evaluate as EV
from disyolo_amd import lib as L

CLASSIDS = [0, 1, 2]
ALL_ONE = [(1.0, 1.0, 1.0)] * 3


def scene_tables(merge_overlap, **kw):
    """the AP table of the scene through the host-mask path and through the ov-row path, and the group count"""
    sc = TR.scene(**kw)
    res = TR.merge_tiles(sc.tiles, sc.image_hw, sc.net_size, sc.detections, sc.keep, sc.masks, merge_overlap)
    recs = {"scene": ER.records(sc.objects)}
    by_mask = ER.ap_table(ER.collect_tiled(res, recs, "scene", sc.image_hw, CLASSIDS), recs, ["scene"], CLASSIDS)
    by_ov = ER.ap_table(ER.collect_tiled(res, recs, "scene", sc.image_hw, CLASSIDS, ov=True), recs, ["scene"], CLASSIDS)
    return by_mask, by_ov, len(res.boxes)


def same_fractions(got, want):
    return all(g == pytest.approx(w, abs=1e-12) for row_g, row_w in zip(got, want) for g, w in zip(row_g, row_w))


# ------------------------------------------------------------------------------------------------ known answers
@pytest.mark.parametrize("kw", [dict(), dict(overlap=32), dict(net_size=(64, 64)), dict(mask_stride=4)],
                         ids=["o16", "o32", "sq64", "m4"])
@pytest.mark.parametrize("merge_overlap", [0.3, 0.5, 0.7])
def test_merged_scene_scores_one(kw, merge_overlap):
    by_mask, by_ov, G = scene_tables(merge_overlap, **kw)
    assert G == 5
    assert by_mask == ALL_ONE and by_ov == ALL_ONE


def test_the_metric_sees_the_merge():
    """merge_overlap = 1 leaves 11 groups, a threshold nothing reaches the 17 instances: the duplicates of an object are false
    positives and the crack's pieces each miss IoU 0.5"""
    by_mask, by_ov, G = scene_tables(1.0)
    assert G == 11
    want = [(1 / 2, 1 / 7, 1 / 14), (1, 2 / 3, 5 / 6), (1, 1, 1)]
    assert same_fractions(by_mask, want), by_mask
    assert by_ov == by_mask
    by_mask, by_ov, G = scene_tables(2.0)                  # ni >= 2 min(na, nb) never holds: nothing is merged
    assert G == 17
    assert same_fractions(by_mask[:1], [(1 / 2, 1 / 8, 1 / 16)]), by_mask
    assert by_ov == by_mask


# ------------------------------------------------------------------------------------------------ ground truth as bit planes
def gt_cases():
    h, w = 9, 140
    rng = np.random.default_rng(4)
    masks = []
    for x1, bw in [(5, 1), (37, 31), (5, 32), (69, 33), (20, 65)]:
        m = np.zeros((h, w), bool)
        m[2:7, x1:x1 + bw] = rng.random((5, bw)) < 0.6
        m[2, x1] = m[6, x1 + bw - 1] = True                   # the box is exactly bw wide
        masks.append(m)
    masks.append(np.zeros((h, w), bool))                      # empty
    m = np.zeros((h, w), bool)
    m[0:9, 100:140] = rng.random((9, 40)) < 0.5
    m[0, 100] = m[8, 139] = True                              # touches the right and the bottom border
    masks.append(m)
    return masks, (h, w)


def test_pack_gt_round_trip():
    masks, hw = gt_cases()
    gt, words = ER.pack_gt(masks)
    assert [int(r[3] - r[1]) for r in gt] == [1, 31, 32, 33, 65, 0, 40]
    assert gt[:, 5].tolist() == [1, 1, 1, 2, 3, 0, 2] and gt[5].tolist()[:4] == [0, 0, 0, 0] and gt[5, 7] == 0
    assert gt[:, 7].tolist() == [int(m.sum()) for m in masks]
    for m, back in zip(masks, ER.unpack_gt(gt, words, hw)):
        np.testing.assert_array_equal(back, m)
    # bits past a box's last column are zero: the words hold exactly the masks' pixels
    assert sum(bin(int(v)).count("1") for v in words) == sum(int(m.sum()) for m in masks)


def test_gt_bit_planes_is_pack_gt():
    masks, _ = gt_cases()
    want_gt, want_words = ER.pack_gt(masks)
    gt, words = EV.gt_bit_planes(masks)
    np.testing.assert_array_equal(gt, want_gt)
    np.testing.assert_array_equal(words, want_words)
    assert gt.dtype == np.int32 and words.dtype == np.uint32
    gt, words = EV.gt_bit_planes([])
    assert gt.shape == (0, 8) and words.shape == (0,)


# ------------------------------------------------------------------------------------------------ the launch plan
def test_group_counts_plan_is_the_helpers_prefix():
    lib = L.load()
    assert [lib.disyolo_tile_group_counts_blocks(a) for a in (-3, 0, 1, 2048, 2049, 4096, 4097)] == [1, 1, 1, 1, 2, 2, 3]
    # a pair gets at most 1024 blocks, which stride over the chunks of a larger rectangle
    assert [lib.disyolo_tile_group_counts_blocks(a) for a in (2048 * 1024, 2048 * 1024 + 1, 3000 * 4000)] == [1024] * 3
    boxes = np.array([[10, 20, 50, 80], [0, 0, 150, 200], [5, 5, 5, 9]], np.int32)            # 40 x 60, the image, empty
    groups, _ = L.tile_compose_plan(boxes, [0, 1, 2, 3])
    gt = np.array([[0, 0, 30, 40, 0, 2, 0, 7], [60, 100, 70, 103, 1, 1, 60, 5], [0, 0, 0, 0, 2, 0, 70, 0]], np.int32)
    pairs2 = [(0, -1), (1, -1), (2, -1), (0, 0), (1, 0), (1, 1), (0, 1), (1, 2), (2, 0)]
    rects = [40 * 60, 150 * 200, 0, 20 * 20, 30 * 40, 10 * 3, 0, 0, 0]
    pairs, blocks = L.tile_group_counts_plan(groups, gt, pairs2)
    assert pairs.dtype == np.int32 and pairs[:, :2].tolist() == [list(p) for p in pairs2]
    each = [lib.disyolo_tile_group_counts_blocks(a) for a in rects]
    assert each == [2, 15, 1, 1, 1, 1, 1, 1, 1]
    assert pairs[:, 2].tolist() == np.concatenate([[0], np.cumsum(each)[:-1]]).tolist() and blocks == sum(each)
    pairs, blocks = L.tile_group_counts_plan(groups, gt, np.zeros((0, 2), np.int32))
    assert pairs.shape == (0, 3) and blocks == 0
    for bad in ([(3, -1)], [(0, 3)], [(0, -2)], [(-1, 0)]):
        with pytest.raises(L.DisyoloError):
            L.tile_group_counts_plan(groups, gt, bad)


# ------------------------------------------------------------------------------------------------ argument errors
def test_group_counts_refuses_bad_arguments_before_any_launch():
    """in the style of test_tiles.py: the device pointers are host buffers a launch would fault on, so a code that comes back
    proves the check ran first"""
    lib = L.load()
    buf = ctypes.create_string_buffer(1 << 16)
    p = ctypes.cast(buf, ctypes.c_void_p)

    def i32(*v):
        return np.array(v, np.int32)

    ok_groups = i32(0, 1, 10, 20, 50, 80, 0, 0, 1, 2, 0, 0, 150, 200, 3, 150)        # 40 x 60 at 0, the image at 16 * 150
    ok_gt = i32(0, 0, 30, 40, 0, 2, 0, 7, 60, 100, 70, 103, 1, 1, 60, 5)
    ok_pairs = i32(0, -1, 0, 1, -1, 2, 0, 0, 17, 1, 1, 18)
    arena_ok = 16 * 150 + 150 * 200

    def run(groups=ok_groups, gt=ok_gt, pairs=ok_pairs, arena_bytes=arena_ok, gt_words=70, hw=(150, 200), dev=p, cnt=p):
        return lib.disyolo_tile_group_counts(groups.ctypes.data, dev, len(groups) // 8, dev, arena_bytes, gt.ctypes.data, dev,
                                             len(gt) // 8, dev, gt_words, pairs.ctypes.data, dev, len(pairs) // 3, hw[0], hw[1],
                                             cnt, None)

    def err():
        return lib.disyolo_last_error()

    assert run(pairs=i32(2, -1, 0)) == -1 and b"out of range" in err()
    assert run(pairs=i32(0, 2, 0)) == -1 and b"out of range" in err()
    assert run(pairs=i32(0, -2, 0)) == -1 and b"out of range" in err()
    assert run(pairs=i32(-1, 0, 0)) == -1 and b"out of range" in err()
    assert run(pairs=i32(0, -1, 0, 1, -1, 1)) == -1 and b"block0" in err()                   # the 40 x 60 box takes two blocks
    assert run(pairs=i32(0, -1, 1)) == -1 and b"block0" in err()
    assert run(groups=i32(0, 1, 10, 20, 50, 201, 0, 0)) == -1 and b"leaves" in err()
    assert run(groups=i32(0, 1, 50, 20, 10, 80, 0, 0)) == -1 and b"leaves" in err()           # inverted
    assert run(groups=i32(0, 1, -1, 20, 10, 80, 0, 0)) == -1 and b"leaves" in err()
    assert run(arena_bytes=arena_ok - 1) == -1 and b"arena" in err()
    assert run(groups=i32(0, 1, 10, 20, 50, 80, 0, -1)) == -1 and b"arena" in err()
    assert run(gt=i32(0, 0, 30, 201, 0, 7, 0, 7)) == -1 and b"leaves" in err()
    assert run(gt=i32(30, 0, 0, 40, 0, 2, 0, 7)) == -1 and b"leaves" in err()                 # inverted
    assert run(gt=i32(0, 0, 30, 40, 0, 1, 0, 7)) == -1 and b"pitch" in err()                  # 40 columns need two words
    assert run(gt_words=69) == -1 and b"pitch" in err()                                       # the second plane ends at 70
    assert run(gt=i32(0, 0, 30, 40, 0, 2, -1, 7)) == -1 and b"pitch" in err()
    assert run(hw=(0, 200)) == -1 and run(hw=(1 << 16, 1 << 15)) == -1 and b"too large" in err()
    assert run(dev=None) == -1 and b"null" in err()
    assert run(cnt=None) == -1 and b"null" in err()
    # more than 2^31 blocks cannot be asked for inside an image below 2^31 pixels with int32 tables of this size; the plan
    # refuses them on its own side (lib.tile_group_counts_plan)
    assert run(pairs=i32()) == 0                                                               # P = 0
    assert lib.disyolo_tile_group_counts(None, None, 0, None, 0, None, None, 0, None, 0, ok_pairs.ctypes.data, None, 4, 150,
                                         200, None, None) == 0                                 # G = 0


# ------------------------------------------------------------------------------------------------ the Python layers refuse
def test_evaluate_refuses_unknown_tiled_keys_and_a_training_net():
    with pytest.raises(ValueError, match="stride"):
        EV.evaluate(None, {}, None, tiled={"stride": 3})
    with pytest.raises(ValueError, match="inference"):
        EV.evaluate(SimpleNamespace(training=True), {}, None, tiled={"overlap": 16})


def test_collect_tiled_refuses_a_result_of_another_size():
    recs = {"a": []}
    m = EV.MAP(recs, {"a": [150, 200]}, ["a"])
    res = SimpleNamespace(image_hw=(150, 201))
    with pytest.raises(ValueError, match="150, 201"):
        m.collect_tiled("a", res, {"0": [], "1": [], "2": []})

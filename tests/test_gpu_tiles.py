"""Tiled detection on the GPU: the four kernels of csrc/tiles.hip, ``merge_tiles`` and ``detect_tiled`` against the numpy
definition (tests/tiles_ref.py).  Everything compared is an integer or a bit: equality throughout."""
import numpy as np
import pytest
import torch

import net_setup as NS
import option_matrix as OM
import tiles_ref as TR
from disyolo_amd import evaluate as EV
from disyolo_amd import lib as L
from disyolo_amd import postprocess as PP
from disyolo_amd import tiles as TL
from disyolo_amd.net import YOLONet

pytestmark = pytest.mark.gpu


def unpack(planes: torch.Tensor) -> np.ndarray:
    """int32 [N,H,W/32] bit planes -> bool [N,H,W]"""
    p = planes.cpu().numpy().view(np.uint32)
    return ((p[..., None] >> np.arange(32, dtype=np.uint32)) & 1).astype(bool).reshape(p.shape[0], p.shape[1], -1)


def pack(bits: np.ndarray) -> np.ndarray:
    """bool [N,H,W] -> int32 [N,H,W/32]"""
    b = bits.reshape(bits.shape[0], bits.shape[1], -1, 32).astype(np.uint64)
    return (b << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32).view(np.int32)


# ------------------------------------------------------------------------------------------------ gather
@pytest.mark.parametrize("hw,t0,t1", [((150, 200), 0, 9), ((150, 200), 3, 5), ((50, 130), 0, 2), ((150, 200), 8, 10),
                                      ((150, 200), 9, 11)], ids=["all", "mid", "short", "last+pad", "pad"])
def test_tile_gather(dev, hw, t0, t1):
    H, W = 64, 96
    img = np.random.default_rng(hw[0] + t0).integers(0, 256, size=hw + (3,), dtype=np.uint8)
    tiles = TL.plan_tiles(hw[0], hw[1], (H, W), 16)
    out = torch.full((t1 - t0, H, W, 3), float("nan"), device=dev)
    L.tile_gather(torch.from_numpy(img).to(dev), torch.from_numpy(tiles).to(dev), t0, t1, out, (H, W))
    want = TR.tile_gather(img, tiles, t0, t1, (H, W))
    np.testing.assert_array_equal(out.cpu().numpy(), want)
    if hw[0] < H:
        assert (want[:, hw[0]:] == np.float32(127.0 / 255.0)).all()
    if t1 > len(tiles):
        assert (want[-1] == np.float32(127.0 / 255.0)).all()


def test_tile_gather_of_a_net_sized_image_is_image_read(dev):
    H, W = 64, 96
    img = np.random.default_rng(5).integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    want, window = EV.image_read(img, (H, W), device=dev)
    out = torch.empty(1, H, W, 3, device=dev)
    L.tile_gather(torch.from_numpy(img).to(dev), torch.zeros(1, 2, dtype=torch.int32, device=dev), 0, 1, out, (H, W))
    assert torch.equal(out[0], want)
    np.testing.assert_array_equal(window, TL.tile_windows(np.zeros((1, 2), np.int32), (H, W), (H, W))[0])


# ------------------------------------------------------------------------------------------------ paste into bit planes
def paste_case(dev, H, W, Hm, Wm, seed):
    rng = np.random.default_rng(seed)
    box = rng.uniform(0, 1, size=(12, 6)).astype(np.float32)
    box[:, :2], box[:, 2:4] = np.minimum(box[:, :2], box[:, 2:4]), np.maximum(box[:, :2], box[:, 2:4])
    rects, _ = PP.paste_rects(box, H, W, (H, W), (Hm, Wm))
    c1, c3 = [Hm // 8, Wm // 8, Hm - Hm // 4, Wm - Wm // 4], [1, 1, Hm // 2, Wm - 1]
    hand = np.array([[0, 0, Hm, Wm, 0, 0, H, W],                      # the whole tile
                     c1 + [7, 5, 50, 64],                             # starts inside a word, ends on a word's edge
                     [0, 1, Hm, Wm - 2, 0, 32, H, 70],                # starts on a word's edge, ends inside a word
                     c3 + [10, 37, 33, 59],                           # inside one word
                     [0, 0, 0, 0, 0, 0, 0, 0],                        # empty
                     c1 + [20, 20, 20, 40]], np.int32)                # empty destination
    rects = np.concatenate([rects, hand]).astype(np.int32)
    masks = rng.uniform(0, 1, size=(len(rects), Hm, Wm)).astype(np.float32)
    return torch.from_numpy(masks).to(dev), torch.from_numpy(rects).to(dev)


@pytest.mark.parametrize("H,W,m", [(64, 96, 2), (64, 96, 4), (96, 128, 1)])
def test_tile_paste_bits_is_mask_paste(dev, H, W, m):
    masks, rects = paste_case(dev, H, W, H // m, W // m, seed=H + m)
    n = int(rects.shape[0])
    planes = torch.full((n, H, W // 32), -1, dtype=torch.int32, device=dev)
    L.tile_paste_bits(masks, rects, (H, W), planes)
    full = torch.empty(n, H, W, dtype=torch.uint8, device=dev)
    merged = torch.empty(H, W, dtype=torch.uint8, device=dev)
    L.mask_paste(masks, rects, torch.zeros(n, dtype=torch.int32, device=dev), H, W, full, merged)
    got, want = unpack(planes), full.cpu().numpy().astype(bool)
    np.testing.assert_array_equal(got, want)
    assert want[:-2].any(axis=(1, 2)).sum() >= n // 2 and want[12:16].any(axis=(1, 2)).all() and not want[-2:].any()      # the cases are not all empty
    np.testing.assert_array_equal(pack(got), planes.cpu().numpy())                # (and the test's own packing is consistent)


def test_tile_paste_bits_takes_no_rows_and_refuses_a_crop_outside_the_map(dev):
    H, W = 64, 96
    L.tile_paste_bits(torch.empty(0, 32, 48, device=dev), torch.empty(0, 8, dtype=torch.int32, device=dev), (H, W),
                      torch.empty(0, H, W // 32, dtype=torch.int32, device=dev))
    masks = torch.ones(2, 32, 48, device=dev)
    rects = torch.tensor([[0, 0, 32, 49, 0, 0, H, W], [-1, 0, 32, 48, 0, 0, H, W]], dtype=torch.int32, device=dev)
    planes = torch.full((2, H, W // 32), -1, dtype=torch.int32, device=dev)
    L.tile_paste_bits(masks, rects, (H, W), planes)
    assert not planes.any()
    with pytest.raises(L.DisyoloError):
        L.tile_paste_bits(masks, rects, (H, 80), torch.empty(2, H, 2, dtype=torch.int32, device=dev))


# ------------------------------------------------------------------------------------------------ seam counts
SCENE_TILES = [[y, x] for y in (0, 43, 86) for x in (0, 52, 104)]
SEAM_CASES = {
    # name: (image (h, w), net (H, W), origins, pairs of tile numbers)
    "20 mod 32": ((150, 200), (64, 96), SCENE_TILES, [(0, 1), (1, 2), (4, 5)]),
    "negative": ((150, 200), (64, 96), SCENE_TILES, [(1, 3), (2, 4), (1, 0), (5, 4)]),
    "multiple of 32": ((100, 200), (64, 96), [[0, 0], [0, 64], [20, 32]], [(0, 1), (1, 0), (0, 2), (2, 1)]),
    "vertical only": ((150, 200), (64, 96), SCENE_TILES, [(0, 3), (3, 6), (7, 4)]),
    "3 columns": ((64, 189), (64, 96), [[0, 0], [0, 93]], [(0, 1), (1, 0)]),
    "border": ((150, 190), (64, 96), SCENE_TILES, [(2, 5), (1, 2), (5, 8), (4, 2)]),
    "three deep": ((100, 100), (64, 64), [[y, x] for y in (0, 18, 36) for x in (0, 18, 36)], [(0, 2), (0, 8), (2, 6), (8, 0), (0, 6)]),
    "disjoint": ((150, 200), (64, 96), SCENE_TILES, [(0, 2), (0, 8)]),
}


@pytest.mark.parametrize("name", sorted(SEAM_CASES))
def test_tile_seam_counts(dev, name):
    hw, (H, W), origins, tpairs = SEAM_CASES[name]
    origins = np.array(origins, np.int32)
    rng = np.random.default_rng(len(name))
    # two instances per tile, so that a pair's planes are not each other's neighbours in memory
    inst_tile = np.repeat(np.arange(len(origins), dtype=np.int32), 2)
    bits = rng.random((len(inst_tile), H, W)) < 0.5
    planes = torch.from_numpy(pack(bits)).to(dev)
    pairs = np.array([(2 * a + i, 2 * b + j) for a, b in tpairs for i in (0, 1) for j in (0, 1)], np.int32)
    got = L.tile_seam_counts(pairs, inst_tile, origins, hw, planes, (H, W)).cpu().numpy()
    want = np.array([TR.seam_counts(bits[a], origins[inst_tile[a]], bits[b], origins[inst_tile[b]], hw, (H, W)) for a, b in pairs])
    np.testing.assert_array_equal(got, want)
    if name == "disjoint":
        assert not want.any()
    else:
        assert (want > 0).all()
    if name == "3 columns":
        assert (want[:, :2] <= 3 * 64).all()


def test_tile_seam_counts_refuses_an_index_out_of_range(dev):
    planes = torch.zeros(2, 64, 3, dtype=torch.int32, device=dev)
    origins = np.array([[0, 0], [0, 52]], np.int32)
    for pairs, inst_tile in (([[0, 2]], [0, 1]), ([[-1, 0]], [0, 1]), ([[0, 1]], [0, 2])):
        with pytest.raises(L.DisyoloError):
            L.tile_seam_counts(np.array(pairs, np.int32), np.array(inst_tile, np.int32), origins, (64, 148), planes, (64, 96))
    assert L.tile_seam_counts(np.zeros((0, 2), np.int32), np.array([0, 1], np.int32), origins, (64, 148), planes,
                              (64, 96)).shape == (0, 3)


# ------------------------------------------------------------------------------------------------ the merge
def assert_same(res, want, image_hw):
    np.testing.assert_array_equal(res.boxes, want.boxes)
    np.testing.assert_array_equal(res.classid, want.classid)
    np.testing.assert_array_equal(res.score, want.score)
    assert res.members == want.members
    assert res.boxes.dtype == np.int32 and res.score.dtype == np.float32
    for g in range(len(want.boxes)):
        m = res.mask(g)
        assert m.dtype == torch.bool and m.is_cuda
        np.testing.assert_array_equal(m.cpu().numpy(), want.masks[g])
        np.testing.assert_array_equal(res.full_mask(g).cpu().numpy(), TR.full_mask(want, g, image_hw))
    assert res.owner.dtype == torch.int32 and res.merged.dtype == torch.uint8
    np.testing.assert_array_equal(res.owner.cpu().numpy(), want.owner)
    np.testing.assert_array_equal(res.merged.cpu().numpy(), want.merged)


MERGE_CASES = {"o16": (dict(net_size=(64, 96), overlap=16), None), "o32": (dict(net_size=(64, 96), overlap=32), None),
               "sq64": (dict(net_size=(64, 64), overlap=16), None), "m4": (dict(net_size=(64, 96), overlap=16, mask_stride=4), None),
               "tile 4 dropped": (dict(net_size=(64, 96), overlap=16), 4)}


@pytest.mark.parametrize("name", sorted(MERGE_CASES))
def test_merge_tiles_on_the_scene(dev, name):
    kw, dropped = MERGE_CASES[name]
    sc = TR.scene(**kw)
    keep = sc.keep.copy()
    if dropped is not None:
        keep[dropped] = 0
    for mo in (0.5, 0.95):                                 # (0.95 is above some seam ratios: objects fall apart, in both)
        want = TR.merge_tiles(sc.tiles, sc.image_hw, sc.net_size, sc.detections, keep, sc.masks, mo)
        res = TL.merge_tiles(sc.tiles, sc.image_hw, sc.net_size, sc.detections, keep, torch.from_numpy(sc.masks).to(dev), mo)
        assert_same(res, want, sc.image_hw)
        if mo == 0.5 and dropped is None and name != "m4":
            assert len(res) == 5 and sorted(res.classid.tolist()) == [0, 0, 1, 1, 2]
    # tensors on the device go the same way
    res = TL.merge_tiles(sc.tiles, sc.image_hw, sc.net_size, torch.from_numpy(sc.detections).to(dev),
                         torch.from_numpy(keep).to(dev), torch.from_numpy(sc.masks).to(dev), 0.95)
    assert_same(res, want, sc.image_hw)


def test_merge_tiles_with_nothing_kept(dev):
    sc = TR.scene()
    res = TL.merge_tiles(sc.tiles, sc.image_hw, sc.net_size, sc.detections, np.zeros_like(sc.keep), torch.from_numpy(sc.masks).to(dev))
    assert len(res) == 0 and res.boxes.shape == (0, 4) and res.members == []
    assert not res.owner.any() and not res.merged.any() and tuple(res.merged.shape) == sc.image_hw


# ------------------------------------------------------------------------------------------------ through the net
NETS = {"k3 m2": dict(k_map=3, mask_stride=2), "k5 m4 C6 agnostic": dict(k_map=5, mask_stride=4, classes=OM.names(6), nms="agnostic")}
THR = 0.05


def make_net(dev, kw, seed=0):
    net = YOLONet(training=False, device=dev, image_size=(64, 96), batch_size=2, stage=1, seed=seed, **kw)
    NS.perturb_variables(net, seed)
    net.refresh_weights()
    return net


def tiled_want(res, image_hw, net_size):
    det, keep, masks = (t.cpu().numpy() for t in res.tile_outputs)
    return TR.merge_tiles(res.tiles, image_hw, net_size, det, keep, masks, 0.5), keep


@pytest.mark.parametrize("name", sorted(NETS))
def test_detect_tiled_end_to_end(dev, name):
    net = make_net(dev, NETS[name])
    H, W = net.H, net.W
    img = np.random.default_rng(11).integers(0, 256, size=(150, 200, 3), dtype=np.uint8)
    res = TL.detect_tiled(net, img, overlap=16, det_thresh=THR, keep_tiles=True)
    assert res.tiles.shape == (9, 2)                                     # T = 9 with B = 2: the last chunk is padded
    np.testing.assert_array_equal(res.inputs.cpu().numpy(), TR.tile_gather(img, res.tiles, 0, 9, (H, W)))
    want, keep = tiled_want(res, (150, 200), (H, W))
    print("%s: %d kept rows, %d instances, %d pairs, %d groups, %d of them merged" % (
        name, int(keep.sum()), len(want.instances), len(want.pairs), len(want.boxes), sum(len(m) > 1 for m in want.members)))
    assert (keep.sum(axis=1) > 0).all() and len(want.pairs) > 0, "the threshold leaves tiles without detections"
    assert_same(res, want, (150, 200))
    # the net's own outputs for the tiles are what a plain call gives for the same inputs
    win = TL.tile_windows(res.tiles, (150, 200), (H, W))
    det, kp, masks = net.evaluation_device(res.inputs[2:4], win[2:4], THR)
    assert torch.equal(det, res.tile_outputs[0][2:4]) and torch.equal(kp, res.tile_outputs[1][2:4])
    assert torch.equal(masks, res.tile_outputs[2][2:4])
    # the recorded inference program gives the same result as the eager path
    net.build_infer_program(det_thresh=THR, graph=False)
    res2 = TL.detect_tiled(net, torch.from_numpy(img).to(dev), overlap=16, det_thresh=THR)
    assert res2.inputs is None
    assert_same(res2, want, (150, 200))


@pytest.mark.parametrize("name", sorted(NETS))
def test_detect_tiled_of_a_net_sized_image_is_the_plain_path(dev, name):
    net = make_net(dev, NETS[name], seed=1)
    H, W = net.H, net.W
    img = np.random.default_rng(3).integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    res = TL.detect_tiled(net, img, overlap=16, det_thresh=THR)
    image, window = EV.image_read(img, (H, W), device=dev)
    det_box, det_mask = net.evaluation(torch.stack([image, image]), np.stack([window, window]), THR, masks_on_device=True)
    entries, merged = PP.paste_detections(det_box[0], det_mask[0], H, W, (H, W))
    assert len(entries) == len(res) >= 3
    for g, e in enumerate(entries):
        y1, x1, y2, x2 = res.boxes[g]
        assert res.classid[g] == e["classid"] and float(res.score[g]) == np.float32(e["score"])
        assert torch.equal(res.mask(g), e["mask"][y1:y2, x1:x2])
        assert int(e["mask"].sum()) == int(res.mask(g).sum())             # nothing of the mask lies outside the box
    assert torch.equal(res.merged, merged)


def test_detect_tiled_refuses_bad_arguments(dev):
    net = make_net(dev, NETS["k3 m2"])
    img = np.zeros((150, 200, 3), np.uint8)
    for overlap in (-1, 33, (16, 49)):
        with pytest.raises(ValueError):
            TL.detect_tiled(net, img, overlap=overlap)
    with pytest.raises(ValueError):
        TL.detect_tiled(net, img.astype(np.float32), overlap=16)
    with pytest.raises(ValueError):
        TL.detect_tiled(net, img[:, :, 0], overlap=16)

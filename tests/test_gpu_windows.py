"""Window training on the GPU: the three kernels of csrc/augment.hip (window_visible, window_targets, window_place_masks), the
image job through the existing placement launch and ``defect_train(placement="window")`` against the numpy definition
(tests/window_ref.py).  Everything compared is an integer, a byte or an f32 computed operation by operation: equality
throughout."""
import numpy as np
import pytest
import torch

import disyolo_oracle as O
import rect_ref as RR
import window_ref as WR
from disyolo_amd import config as cfg
from disyolo_amd import lib as L
from disyolo_amd import tiles as TL
from disyolo_amd import train_data as TD
from test_gpu_train_data import RecordingRandom, _labels

pytestmark = pytest.mark.gpu
H, W = WR.NET
NAMED = [(15, 0), (93, 15), (41, 34)]


def upload_jobs(dev, specs):
    """specs: (crop tensor uint8 CUDA [h,w], crop_x, crop_y, x0, y0, image_h, image_w, b, cls, flip) -> uint8 CUDA job bytes"""
    jobs = np.zeros(max(len(specs), 1), L.WINDOW_JOB)
    for k, (crop, cx, cy, x0, y0, ih, iw, b, c, flip) in enumerate(specs):
        jobs[k] = (crop.data_ptr(), crop.shape[0], crop.shape[1], cx, cy, x0, y0, ih, iw, b, c, flip, 0)
    return torch.from_numpy(jobs.view(np.uint8).copy()).to(dev)


def vis_numpy(crop, cx, cy, x0, y0, ih, iw, net=(H, W)):
    full = np.zeros((ih, iw), bool)
    full[cy:cy + crop.shape[0], cx:cx + crop.shape[1]] = crop[:max(ih - cy, 0), :max(iw - cx, 0)] > 0
    return WR.vis_row(WR.visible(full, x0, y0, net))


@pytest.fixture(scope="module")
def scene(dev):
    """the scene, its crops rasterised on the device (the loader's record cache) and the numpy record"""
    lab = WR.scene()
    image, masks, boxes, names = WR.record(lab)
    crops = [TD.rasterize_instance(p, y2 - y1, x2 - x1, dev, origin=(x1, y1)) for p, (x1, y1, x2, y2) in zip(lab["polygons"], boxes)]
    torch.cuda.synchronize()
    return lab, crops, masks, boxes, names


def test_crop_raster_on_the_device_equals_the_crop_of_the_full_raster(scene):
    lab, crops, masks, boxes, names = scene
    for crop, m, (x1, y1, x2, y2) in zip(crops, masks, boxes):
        np.testing.assert_array_equal(crop.cpu().numpy().astype(bool), m[y1:y2, x1:x2])


# ------------------------------------------------------------------------------------------------ window_visible
def test_window_visible_against_numpy(dev):
    rng = np.random.RandomState(1)
    ih, iw = 300, 400
    x0, y0 = 100, 90                                                  # the window: x 100 .. 196, y 90 .. 154
    one = np.zeros((9, 13), np.uint8)
    one[8, 12] = 1
    shapes = [((20, 37), 130, 100),                                   # inside
              ((30, 41), 85, 100), ((30, 41), 180, 100), ((31, 22), 130, 75), ((31, 22), 130, 140),   # cut left, right, top, bottom
              ((90, 150), 70, 80),                                    # larger than the window: cut on all four sides
              ((20, 37), 10, 10), ((20, 37), 196, 100), ((20, 37), 130, 154),                        # disjoint (two of them touching)
              ((9, 13), 88, 82),                                      # one visible pixel, the window's first
              ((17, 5), 195, 150)]                                    # the last column / the last rows
    specs, want = [], []
    for (h, w), cx, cy in shapes:
        crop = one if (h, w) == (9, 13) else (rng.rand(h, w) < 0.3).astype(np.uint8)
        if (h, w) == (17, 5):
            crop[:] = 1
        specs.append((torch.from_numpy(crop).to(dev), cx, cy, x0, y0, ih, iw, 0, 0, 1))
        want.append(vis_numpy(crop, cx, cy, x0, y0, ih, iw))
    # a window overhanging a small image (50 x 70 in a 64 x 96 net, origin 0): the image's edge cuts, not the window's
    small = (rng.rand(30, 40) < 0.5).astype(np.uint8)
    small[-1, -1] = 1
    specs.append((torch.from_numpy(small).to(dev), 30, 20, 0, 0, 50, 70, 0, 0, 1))
    want.append(vis_numpy(small, 30, 20, 0, 0, 50, 70))
    # a crop of 3000 x 40 (a crack's box as tall as the photograph): read inside the window only, its 64 rows over 4 blocks
    tall = (rng.rand(3000, 40) < 0.02).astype(np.uint8)
    specs.append((torch.from_numpy(tall).to(dev), 150, 0, 120, 1000, 3000, 400, 0, 0, 1))
    want.append(vis_numpy(tall, 150, 0, 120, 1000, 3000, 400))
    want = np.asarray(want, np.int32)
    assert want[0, 0] > 0 and (want[6:9] == 0).all() and want[9].tolist() == [1, 0, 0, 1, 1] and want[-1, 0] > 0
    assert want[10].tolist() == [4, 95, 60, 96, 64]
    assert want[-1, 4] - want[-1, 2] > 3 * 16                       # the tall crop's visible rows span several blocks
    jobs = upload_jobs(dev, specs)
    vis = torch.full((len(specs) + 1, 5), -7, dtype=torch.int32, device=dev)
    L.window_visible(jobs, len(specs), (H, W), vis)
    first = vis.cpu().numpy()
    np.testing.assert_array_equal(first[:-1], want)
    assert (first[-1] == -7).all()                                    # nothing written past njobs
    vis2 = torch.zeros_like(vis)
    L.window_visible(jobs, len(specs), (H, W), vis2)
    np.testing.assert_array_equal(vis2.cpu().numpy()[:-1], first[:-1])    # two runs equal
    L.window_visible(jobs, 0, (H, W), vis2)                           # njobs = 0: nothing happens
    np.testing.assert_array_equal(vis2.cpu().numpy()[:-1], first[:-1])


# ------------------------------------------------------------------------------------------------ window_targets
def scene_jobs(dev, scene, origins, flips, classes):
    """one batch image per (origin, flip): its jobs in record order, like the loader builds them"""
    lab, crops, masks, boxes, names = scene
    specs, images = [], []
    for (x0, y0) in origins:
        for flip in flips:
            b = len(images)
            images.append((x0, y0, flip))
            for i in TD.window_candidates(boxes, x0, y0, H, W):
                x1, y1, x2, y2 = boxes[i]
                specs.append((crops[i], x1, y1, x0, y0, 150, 200, b, list(classes).index(names[i]), flip))
    return upload_jobs(dev, specs), len(specs), images


def run_targets(dev, jobs, njobs, B, G, C, anchors, min_visible):
    vis = torch.zeros(max(njobs, 1), 5, dtype=torch.int32, device=dev)
    rows = torch.full((max(njobs, 1),), -5, dtype=torch.int32, device=dev)
    out = [torch.full((B, 1, 1, 1, G, 5), 3.0, device=dev)] + [torch.full((B, H // d, W // d, 3, 5 + C), 3.0, device=dev) for d in (8, 16, 32)]
    L.window_visible(jobs, njobs, (H, W), vis)
    L.window_targets(jobs, njobs, vis, torch.from_numpy(np.ascontiguousarray(anchors, np.float32)).to(dev), (H, W), min_visible,
                     out[0], out[1], out[2], out[3], rows)
    return vis, rows, out


SWEEP = [(x0, y0) for y0 in range(0, 87, 7) for x0 in range(0, 105, 7)] + NAMED


@pytest.mark.parametrize("G,C", [(20, 3), (2, 3), (20, 6), (2, 6)])
@pytest.mark.parametrize("scale", [1.0, 0.11], ids=["cfg", "x0.11"])
@pytest.mark.parametrize("min_visible", [1, 8])
def test_window_targets_against_the_definition(dev, scene, min_visible, scale, G, C):
    lab = scene[0]
    classes = cfg.CLASSES if C == 3 else ["stain", "crack", "joint", "spall", "rebar", "void"]
    anchors = (cfg.ANCHORS * np.float32(scale)).astype(np.float32)
    jobs, njobs, images = scene_jobs(dev, scene, SWEEP, (1, 2, 3), classes)
    B = len(images)
    assert B == 3 * (13 * 15 + 3) and njobs > 2 * B
    vis, rows, out = run_targets(dev, jobs, njobs, B, G, C, anchors, min_visible)
    vis, rows = vis.cpu().numpy(), rows.cpu().numpy()
    out = [t.cpu().numpy() for t in out]
    want = {"vis": [], "rows": [], "true_boxes": [], "yolo3": [], "yolo2": [], "yolo1": []}
    cells = dropped = 0
    for (x0, y0, flip) in images:
        r = WR.window_ref(lab, x0, y0, flip, (H, W), min_visible, G, classes, anchors, want_masks=False)
        for key in want:
            want[key].append(r[key])
        cells += r["cells"]
        dropped += int((r["rows"] < 0).sum())
    assert cells > B and dropped > 0
    np.testing.assert_array_equal(vis[:njobs], np.concatenate(want["vis"]))
    np.testing.assert_array_equal(rows[:njobs], np.concatenate(want["rows"]))
    np.testing.assert_array_equal(out[0][:, 0, 0, 0], np.stack(want["true_boxes"]))
    for got, key in zip(out[1:], ("yolo3", "yolo2", "yolo1")):
        np.testing.assert_array_equal(got, np.stack(want[key]))


def test_window_targets_without_jobs_zeroes_its_outputs(dev):
    jobs = torch.zeros(L.WINDOW_JOB.itemsize, dtype=torch.uint8, device=dev)
    vis, rows, out = run_targets(dev, jobs, 0, 2, 7, 3, cfg.ANCHORS, 8)
    assert all(not t.any() for t in out)


# ------------------------------------------------------------------------------------------------ window_place_masks
@pytest.mark.parametrize("G", [20, 2])
def test_window_place_masks_against_the_definition(dev, scene, G):
    lab = scene[0]
    origins = NAMED + [(0, 0), (104, 86), (60, 20), (37, 51)]
    jobs, njobs, images = scene_jobs(dev, scene, origins, (1, 2, 3), cfg.CLASSES)
    B = len(images)
    vis, rows, out = run_targets(dev, jobs, njobs, B, G, 3, cfg.ANCHORS, 8)
    planes = torch.zeros(B, G, H, W, dtype=torch.uint8, device=dev)
    L.window_place_masks(jobs, njobs, rows, planes, (H, W))
    got = planes.cpu().numpy()
    compact = False
    for b, (x0, y0, flip) in enumerate(images):
        r = WR.window_ref(lab, x0, y0, flip, (H, W), 8, G)
        np.testing.assert_array_equal(got[b].astype(bool), r["true_masks"], err_msg=str((x0, y0, flip)))
        kept = np.nonzero(r["rows"] >= 0)[0]
        compact |= len(kept) >= 2 and bool((r["rows"][kept[0]:kept[-1]] < 0).any())
    assert got.max() == 1 and (compact or G == 2)                      # a dropped instance between two kept ones
    L.window_place_masks(jobs, 0, rows, planes, (H, W))               # njobs = 0: nothing happens
    np.testing.assert_array_equal(planes.cpu().numpy(), got)


# ------------------------------------------------------------------------------------------------ the image
def place_windows(dev, image, windows, net=(H, W)):
    """the loader's image job -- new_w = image_w, new_h = image_h, dx = -x0, dy = -y0 -- through the existing placement launch"""
    src = torch.from_numpy(image).to(dev)
    frames = torch.zeros(len(windows), net[0], net[1], 3, dtype=torch.uint8, device=dev)
    jobs = np.zeros(len(windows), L.PLACE_JOB)
    for k, (x0, y0, flip) in enumerate(windows):
        jobs[k] = (src.data_ptr(), frames[k].data_ptr(), 0, image.shape[0], image.shape[1], image.shape[1], image.shape[0], -x0, -y0, flip)
    L.aug_place_batch(torch.from_numpy(jobs.view(np.uint8).copy()).to(dev), len(windows), net)
    torch.cuda.synchronize()
    return frames


def test_image_job_through_the_place_launch_is_the_numpy_window(dev):
    rng = np.random.RandomState(4)
    for shape, windows in (((150, 200), [(0, 0, 1), (104, 86, 1), (41, 34, 2), (93, 15, 3), (7, 80, 2)]),
                           ((50, 70), [(0, 0, 1), (0, 0, 2), (0, 0, 3)]), ((64, 300), [(204, 0, 1), (100, 0, 3)])):
        image = rng.randint(0, 256, shape + (3,)).astype(np.uint8)
        frames = place_windows(dev, image, windows).cpu().numpy()
        for k, (x0, y0, flip) in enumerate(windows):
            np.testing.assert_array_equal(frames[k], WR.window_image(image, x0, y0, flip, (H, W)), err_msg=str((shape, x0, y0, flip)))


class ScriptedRandom(np.random.RandomState):
    """randint answers from a script while it lasts"""

    def __init__(self, seed, script):
        super().__init__(seed)
        self.script = list(script)

    def randint(self, *a, **k):
        if self.script:
            return self.script.pop(0)
        return super().randint(*a, **k)


def test_a_training_window_at_a_tile_origin_is_the_tile_detect_tiled_sees(dev):
    """flip 1, no photometric step: ``images[b]`` of the loader equals ``tile_gather``'s tile bit for bit (the two /255 forms,
    f32 division and f64 division rounded to f32, agree on all 256 byte values)"""
    lab = dict(WR.scene())
    lab["image"] = lab["image"].copy()
    lab["image"][0, :86] = (np.arange(258) % 256).astype(np.uint8).reshape(86, 3)   # every byte value
    tiles = TL.plan_tiles(150, 200, (H, W), 16)
    T = len(tiles)
    script = [int(v) for (y0, x0) in tiles for v in (x0, y0)]
    data = TD.defect_train([lab], batch_size=T, image_size=(H, W), device=dev, rng=ScriptedRandom(0, script), flipped=False,
                           blur_noise_light=False, placement="window", positive_fraction=0.0)
    batch = data.get_device()
    assert [(d["y0"], d["x0"]) for d in data.last_decisions] == [tuple(t) for t in tiles.tolist()]
    out = torch.empty(T, H, W, 3, device=dev)
    L.tile_gather(torch.from_numpy(lab["image"]).to(dev), torch.from_numpy(tiles).to(dev), 0, T, out, (H, W))
    assert torch.equal(batch["images"], out)
    ramp = torch.arange(256, dtype=torch.uint8, device=dev)
    f = torch.empty(256, dtype=torch.float32, device=dev)
    L.aug_to_float(ramp, f)
    np.testing.assert_array_equal(f.cpu().numpy(), (np.arange(256, dtype=np.float64) / 255.0).astype(np.float32))


# ------------------------------------------------------------------------------------------------ the loader
def window_labels():
    """the scene, three random records larger than the net, one smaller than it (padded) and one without instances"""
    rng = np.random.RandomState(2)
    labels = [WR.scene()] + _labels(rng, 3)
    labels.append({"image": rng.randint(0, 256, (50, 70, 3)).astype(np.uint8), "class_names": ["rebar"],
                   "polygons": [[WR.polygon12(55, 37, 14, 12)]]})
    labels.append({"image": rng.randint(0, 256, (90, 130, 3)).astype(np.uint8), "class_names": [], "polygons": []})
    return labels


def expected_calls(data, cursor, n):
    """the draws of one batch in order, from its decisions: per image u, the window's draws, flip, bnl, the bnl's own"""
    calls = []
    for dec in data.last_decisions:
        calls += ["uniform"] + ["randint"] * (5 if dec["instance"] is not None else 2) + ["randint", "randint"]
        calls += {1: [], 2: ["randint"] * 6, 3: ["uniform"], 4: ["randint"] * 3}[dec["bnl"]]
        cursor += 1
        if cursor >= n:
            calls.append("shuffle")
            cursor = 0
    return calls


def test_window_loader_replayed_by_the_definition(dev):
    B, G = 4, 20
    labels = window_labels()
    rng = RecordingRandom(123)
    data = TD.defect_train(labels, batch_size=B, image_size=(H, W), device=dev, rng=rng, placement="window", positive_fraction=0.7)
    seen = {"flip": set(), "bnl": set(), "positive": set()}
    empty_images = 0
    for it in range(6):
        rng.calls.clear()
        order, cursor = list(data.random_labels), data.cursor
        images, masks, tboxes, y3, y2, y1, window = data.get()
        torch.cuda.synchronize()
        assert rng.calls == expected_calls(data, cursor, len(labels))
        assert images.shape == (B, H, W, 3) and masks.shape == (B, G, H, W) and masks.dtype == torch.bool
        assert tboxes.shape == (B, 1, 1, 1, G, 5) and y3.shape == (B, H // 8, W // 8, 3, 8) and y1.shape == (B, H // 32, W // 32, 3, 8)
        assert (window == [0, 0, 1, 1]).all()
        for b in range(B):
            dec = data.last_decisions[b]
            assert dec["placement"] == "window"
            seen["flip"].add(dec["flip"]); seen["bnl"].add(dec["bnl"]); seen["positive"].add(dec["instance"] is not None)
            if cursor + b >= len(order):
                continue                                       # the epoch wrapped inside this batch: order reshuffled
            lab = order[cursor + b]
            h, w = lab["image"].shape[:2]
            assert 0 <= dec["x0"] <= max(w - W, 0) and 0 <= dec["y0"] <= max(h - H, 0)
            r = WR.window_ref(lab, dec["x0"], dec["y0"], dec["flip"], (H, W), 8, G)
            img = r["image"]
            if dec["bnl"] == 2:
                rows = np.concatenate([dec["salt"][0], dec["pepper"][0]]); cols = np.concatenate([dec["salt"][1], dec["pepper"][1]])
                img = O.salt_pepper(img, rows, cols, len(dec["salt"][0]))
            elif dec["bnl"] == 3:
                img = O.change_light(img, dec["coeff"])
            elif dec["bnl"] == 4:
                img = RR.motion_blur3(img, dec["angle"], {"right": 1, "left": 2, "full": 0}[dec["line_type"]])
            np.testing.assert_array_equal(images[b].cpu().numpy(), img.astype(np.float32) / 255.0)
            np.testing.assert_array_equal(masks[b].cpu().numpy(), r["true_masks"])
            np.testing.assert_array_equal(tboxes[b, 0, 0, 0], r["true_boxes"])
            for got, key in ((y3, "yolo3"), (y2, "yolo2"), (y1, "yolo1")):
                np.testing.assert_array_equal(got[b], r[key])
            if dec["instance"] is not None:
                px, py = dec["point"]
                assert dec["x0"] <= px < dec["x0"] + W and dec["y0"] <= py < dec["y0"] + H
            empty_images += not (r["rows"] >= 0).any()
    assert seen["flip"] == {1, 2, 3} and seen["bnl"] == {1, 2, 3, 4} and seen["positive"] == {True, False}
    assert data.epoch >= 4 and empty_images >= 1
    # same seed -> same batches
    kw = dict(batch_size=B, image_size=(H, W), device=dev, placement="window", positive_fraction=0.7)
    a = TD.defect_train(labels, rng=np.random.RandomState(9), **kw).get()
    b_ = TD.defect_train(labels, rng=np.random.RandomState(9), **kw).get()
    assert torch.equal(a[0], b_[0]) and torch.equal(a[1], b_[1]) and all(np.array_equal(x, y) for x, y in zip(a[2:], b_[2:]))


def test_window_loader_record_cache_and_buffer_sets(dev):
    """the record cache changes nothing (cache_bytes=0: every crop rasterised again per visit), get_device() hands out the same
    arrays as get(), and a batch stays intact through the next get()"""
    B = 2
    labels = window_labels()
    kw = dict(batch_size=B, image_size=(H, W), device=dev, placement="window", positive_fraction=0.7)
    a = TD.defect_train(labels, rng=np.random.RandomState(3), **kw)
    b = TD.defect_train(labels, rng=np.random.RandomState(3), cache_bytes=0, **kw)
    prev = None
    for it in range(12):
        ga = a.get()
        gb = b.get_device()
        assert not b._cache and len(a._cache) >= 1
        assert torch.equal(ga[0], gb["images"]) and torch.equal(ga[1], gb["true_masks"])
        for x, key in zip(ga[2:], ("true_boxes", "yolo3", "yolo2", "yolo1", "clip_window")):
            assert np.array_equal(x, gb[key].cpu().numpy()), key
        if prev is not None:
            assert all(torch.equal(x, y) for x, y in zip(prev[0], prev[1]))               # the batch before this one: untouched
        keep = [gb[k] for k in ("images", "true_masks", "true_boxes", "yolo3", "yolo2", "yolo1")]
        prev = (keep, [t.clone() for t in keep])
    assert a.epoch == b.epoch and a.epoch >= 4
    # nothing full-size per instance is cached: the image and the crops of the static boxes
    lab = WR.scene()
    c = TD.defect_train([lab], rng=np.random.RandomState(0), **kw)
    c.get_device()
    assert c._cached == 150 * 200 * 3 + sum((x2 - x1) * (y2 - y1) for x1, y1, x2, y2 in
                                            (TD.static_box(p, 150, 200) for p in lab["polygons"]))


def test_window_loader_feeds_the_solver(dev, tmp_path):
    """end to end: window batches -> Solver.train -> finite losses, one record without any instance among them"""
    from disyolo_amd.net import YOLONet
    from disyolo_amd.solver import Solver
    B = 2
    labels = window_labels()
    data = TD.defect_train(labels, batch_size=B, image_size=(H, W), device=dev, rng=np.random.RandomState(1), placement="window")
    net = YOLONet(training=True, device=dev, image_size=(H, W), batch_size=B, stage=1, seed=0)
    net.shuffle_seed = 1
    hist = Solver(net, data, output_dir=str(tmp_path), max_iter=6, summary_iter=3, save_iter=6, log=lambda s: None).train()
    assert data.epoch >= 2                                              # twelve images of six records: the empty one was among them
    assert len(hist) == 6 and np.isfinite(hist).sum() >= 4

"""Window training on the CPU: the numpy definition (tests/window_ref.py) on its scene -- the counts of the sweep over every
window origin, the named windows --, the loader's window draws and their order, the crop raster, and the argument errors of
the three entry points and of the constructor.  Every figure here comes from the oracle's rasteriser and the loader's host
arithmetic alone; tests/test_gpu_windows.py holds the kernels to the same definition."""
import ctypes

import numpy as np
import pytest

import disyolo_oracle as O
import window_ref as WR
from disyolo_amd import config as cfg
from disyolo_amd import lib as L
from disyolo_amd import train_data as TD
from test_gpu_train_data import RecordingRandom

H, W = WR.NET


@pytest.fixture(scope="module")
def sweep():
    """window_ref at every origin of the scene (net 64 x 96, min_visible 8), once"""
    lab = WR.scene()
    return lab, {o: WR.window_ref(lab, o[0], o[1], want_masks=False) for o in WR.origins(lab)}


def test_scene_areas_and_static_boxes():
    lab = WR.scene()
    image, masks, boxes, names = WR.record(lab)
    assert image.shape == (150, 200, 3) and names == ["crack", "spall", "rebar", "rebar", "spall"]
    assert masks.reshape(5, -1).sum(1).tolist() == [580, 1959, 775, 106, 34]
    for m, (x1, y1, x2, y2) in zip(masks, boxes):
        assert WR.vis_row(m)[1:] == [x1, y1, x2, y2]                # integer vertices: the static box is the tight box


def test_sweep_counts(sweep):
    lab, refs = sweep
    full = WR.record(lab)[1].reshape(5, -1).sum(1)
    assert len(refs) == 9135
    empty = cut = small = compete = fewer = zero = 0
    first_small = first_compete = None
    for o, r in refs.items():
        vis, rows, cand = r["vis"], r["rows"], np.asarray(r["cand"])
        empty += not (vis[:, 0] > 0).any()
        cut += bool(((rows >= 0) & (vis[:, 0] < full[cand])).any())
        s = (vis[:, 0] >= 1) & (vis[:, 0] <= 7)
        if s.any():
            small += 1
            assert (rows[s] == -1).all()                            # 1 .. 7 visible pixels: dropped
            first_small = first_small or (o, (cand[s] + 1).tolist())
        # a window in which fewer cells were written than boxes kept: two kept instances fell into one (cell, anchor)
        kept = int((rows >= 0).sum())
        if r["cells"] < kept:
            compete += 1
            first_compete = first_compete or (o, (cand[rows >= 0] + 1).tolist())
        box_lost = (vis[:, 0] >= 8) & (rows < 0)                    # enough pixels, but a zero-size clamped box
        zero += bool(box_lost.any())
        fewer += r["cells"] < int((vis[:, 0] >= 8).sum())
    assert empty == 0 and cut == 8757 and small == 1067
    assert first_small == ((15, 0), [2])
    # 109 windows hold two kept instances that compete for one (cell, anchor); with window (41, 34), whose instance 3 has its
    # 8 pixels but a zero-size clamped box, 110 windows write fewer cells than they hold instances of min_visible pixels
    assert compete == 109 and zero == 1 and fewer == 110
    assert first_compete == ((93, 15), [1, 2, 4, 5])


def test_named_windows(sweep):
    lab, refs = sweep
    # (15, 0): the spall's left end, 1 .. 7 pixels: dropped; the crack is kept
    r = refs[(15, 0)]
    k = r["cand"].index(1)
    assert 1 <= r["vis"][k, 0] <= 7 and r["rows"][k] == -1 and r["rows"][r["cand"].index(0)] == 0
    # (93, 15): four kept, the later one of a competing pair has its row of true_boxes and no cell
    r = refs[(93, 15)]
    assert (np.asarray(r["cand"])[r["rows"] >= 0] + 1).tolist() == [1, 2, 4, 5] and r["cells"] == 3
    assert (r["true_boxes"][:4, 2] > 0).all() and (r["true_boxes"][4:] == 0).all()
    assert r["true_boxes"][:4, 4].tolist() == [0, 1, 2, 1]
    # (41, 34): the rebar shows one row of 8 pixels on the window's last row: y1 = 63, y2 = 64 -> clamped to 63: h = 0
    r = refs[(41, 34)]
    k = r["cand"].index(2)
    assert r["vis"][k].tolist() == [8, 0, 63, 8, 64] and r["rows"][k] == -1
    assert r["rows"].tolist() == [0, 1, -1, 2]                      # the rows compact over the dropped one


def test_the_cap_bites_and_a_large_min_visible_empties_the_window():
    lab = WR.scene()
    r = WR.window_ref(lab, 93, 15, G=2)
    assert r["rows"].tolist()[:2] == [0, 1] and (r["rows"][2:] == -1).all() and r["true_boxes"].shape == (2, 5)
    assert r["true_masks"].shape == (2, H, W) and r["true_masks"][1].any()
    for flip in (1, 2, 3):
        e = WR.window_ref(lab, 93, 15, flip=flip, min_visible=4000)
        assert (e["rows"] == -1).all() and not e["true_boxes"].any() and not e["true_masks"].any()
        assert not any(e[k].any() for k in ("yolo3", "yolo2", "yolo1"))


def test_flips_reflect_boxes_cells_and_masks():
    lab = WR.scene()
    a = WR.window_ref(lab, 60, 20, flip=1)
    for flip, axis in ((2, 1), (3, 0)):
        f = WR.window_ref(lab, 60, 20, flip=flip)
        np.testing.assert_array_equal(f["rows"], a["rows"])
        np.testing.assert_array_equal(f["true_masks"], np.flip(a["true_masks"], axis=axis + 1))
        np.testing.assert_array_equal(f["image"], np.flip(a["image"], axis=axis))
        n = int((a["rows"] >= 0).sum())
        side, c = (W, 0) if flip == 2 else (H, 1)
        np.testing.assert_allclose(f["true_boxes"][:n, c] * side, side - 1 - a["true_boxes"][:n, c] * side, atol=1e-4)
        np.testing.assert_array_equal(np.delete(f["true_boxes"], c, axis=1), np.delete(a["true_boxes"], c, axis=1))
        for k in ("yolo3", "yolo2", "yolo1"):
            assert (np.flip(f[k][..., 4], axis=axis) == a[k][..., 4]).all()


def test_a_record_smaller_than_the_net_is_padded_at_origin_zero():
    rng = np.random.RandomState(3)
    lab = {"image": rng.randint(0, 256, (50, 70, 3)).astype(np.uint8), "class_names": ["rebar"],
           "polygons": [[WR.polygon12(55, 37, 14, 12)]]}                # reaches the image's last column and last row
    assert WR.origins(lab) == [(0, 0)]
    for pf in (0.0, 1.0):
        d = TD.draw_window(np.random.RandomState(1), [TD.static_box(lab["polygons"][0], 50, 70)], 50, 70, H, W, pf)
        assert (d["x0"], d["y0"]) == (0, 0)
    r = WR.window_ref(lab, 0, 0)
    assert (r["image"][50:] == 127).all() and (r["image"][:, 70:] == 127).all()
    np.testing.assert_array_equal(r["image"][:50, :70], lab["image"])
    assert r["rows"].tolist() == [0] and not r["true_masks"][0, 50:].any() and not r["true_masks"][0, :, 70:].any()
    assert r["vis"][0, 3] == 70 and r["vis"][0, 4] == 50               # the box ends where the image does


def test_window_draw_order_and_the_point_stays_inside():
    lab = WR.scene()
    boxes = WR.record(lab)[2]
    rng = RecordingRandom(5)
    for _ in range(200):
        rng.calls.clear()
        d = TD.draw_window(rng, boxes, 150, 200, H, W, 1.0)
        assert rng.calls == ["uniform"] + ["randint"] * 5              # u; j, px, py, ox, oy
        (px, py), (x1, y1, x2, y2) = d["point"], boxes[d["instance"]]
        assert x1 <= px < x2 and y1 <= py < y2
        assert d["x0"] <= px < d["x0"] + W and d["y0"] <= py < d["y0"] + H
        assert 0 <= d["x0"] <= 200 - W and 0 <= d["y0"] <= 150 - H
    seen = set()
    for _ in range(200):
        rng.calls.clear()
        d = TD.draw_window(rng, boxes, 150, 200, H, W, 0.0)
        assert rng.calls == ["uniform", "randint", "randint"] and d["instance"] is None          # u; x0, y0
        assert 0 <= d["x0"] <= 200 - W and 0 <= d["y0"] <= 150 - H
        seen.add((d["x0"] in (0, 200 - W), d["y0"] in (0, 150 - H)))
    assert len(seen) > 1
    rng.calls.clear()
    d = TD.draw_window(rng, [], 150, 200, H, W, 1.0)                   # no instances: the uniform branch
    assert rng.calls == ["uniform", "randint", "randint"] and d["instance"] is None
    # the draws themselves: u, then randint(0, n), randint(bx1, bx2), randint(by1, by2), randint(0, net_w), randint(0, net_h)
    a, b = np.random.RandomState(9), np.random.RandomState(9)
    d = TD.draw_window(a, boxes, 150, 200, H, W, 1.0)
    b.uniform()
    j = int(b.randint(0, 5))
    px, py = int(b.randint(boxes[j][0], boxes[j][2])), int(b.randint(boxes[j][1], boxes[j][3]))
    ox, oy = int(b.randint(0, W)), int(b.randint(0, H))
    assert (d["instance"], d["point"]) == (j, (px, py))
    assert (d["x0"], d["y0"]) == (min(max(px - ox, 0), 200 - W), min(max(py - oy, 0), 150 - H))


def test_crop_raster_equals_the_crop_of_the_full_raster():
    """the record cache of window mode keeps each instance rasterised on its static box only, with the vertices shifted by the
    box's origin: with the oracle's rasteriser, 0 differing pixels for all five instances"""
    lab = WR.scene()
    image, masks, boxes, names = WR.record(lab)
    for polys, m, (x1, y1, x2, y2) in zip(lab["polygons"], masks, boxes):
        shifted = [{"type": p["type"], "all_points_x": [x - x1 for x in p["all_points_x"]],
                    "all_points_y": [y - y1 for y in p["all_points_y"]]} for p in polys]
        np.testing.assert_array_equal(O.instance_mask(shifted, y2 - y1, x2 - x1), m[y1:y2, x1:x2])
        assert not m[:y1].any() and not m[y2:].any() and not m[:, :x1].any() and not m[:, x2:].any()


def test_static_box_and_candidates():
    assert TD.static_box([], 10, 10) == (0, 0, 0, 0)
    tri = [{"type": "out", "all_points_x": [-4, 30, 8], "all_points_y": [3, 5, 40]}]
    assert TD.static_box(tri, 20, 25) == (0, 3, 25, 20)               # clipped to the image
    boxes = [(0, 0, 10, 10), (96, 0, 100, 10), (95, 63, 99, 70), (0, 64, 10, 70)]
    assert TD.window_candidates(boxes, 0, 0, H, W) == [0, 2]          # touching the window's edge from outside: not met
    many = [(0, 0, 4, 4)] * 300
    assert TD.window_candidates(many, 0, 0, H, W) == list(range(256))


def test_entry_points_reject_bad_arguments_before_any_launch():
    """host buffers stand in for device arrays: a launch would fault on them, so every error must come back as a code"""
    lib = L.load()
    assert lib.disyolo_window_job_size() == L.WINDOW_JOB.itemsize == 56
    buf = ctypes.create_string_buffer(1 << 12)
    p = ctypes.cast(buf, ctypes.c_void_p)

    def visible(njobs=1, nh=H, nw=W, jobs=p, vis=p):
        return lib.disyolo_window_visible(jobs, njobs, nh, nw, vis, None)

    for bad in (dict(njobs=-1), dict(njobs=65536), dict(nh=0), dict(nw=-32), dict(jobs=None), dict(vis=None)):
        assert visible(**bad) == -1 and b"window_visible" in lib.disyolo_last_error(), bad

    def targets(njobs=1, B=2, G=20, C=3, nh=H, nw=W, mv=8, jobs=p, vis=p, anchors=p, out=p, rows=p):
        return lib.disyolo_window_targets(jobs, njobs, vis, anchors, B, G, C, nh, nw, mv, out, out, out, out, rows, None)

    for bad in (dict(njobs=-1), dict(B=0), dict(G=0), dict(G=257), dict(C=0), dict(C=81), dict(nh=48), dict(nw=100), dict(mv=0),
                dict(jobs=None), dict(vis=None), dict(anchors=None), dict(out=None), dict(rows=None),
                dict(njobs=0, anchors=None), dict(njobs=0, out=None)):
        assert targets(**bad) == -1 and b"window_targets" in lib.disyolo_last_error(), bad

    def place(njobs=1, G=20, nh=H, nw=W, jobs=p, rows=p, masks=p):
        return lib.disyolo_window_place_masks(jobs, njobs, rows, masks, G, nh, nw, None)

    for bad in (dict(njobs=-1), dict(njobs=65536), dict(G=0), dict(G=257), dict(nh=0), dict(nw=0), dict(jobs=None), dict(rows=None),
                dict(masks=None)):
        assert place(**bad) == -1 and b"window_place_masks" in lib.disyolo_last_error(), bad


def test_constructor_rejects_bad_window_options():
    lab = [WR.scene()]
    kw = dict(batch_size=2, image_size=(H, W), device="cpu")
    for bad in (dict(placement="tile"), dict(placement=None), dict(min_visible=0), dict(min_visible=2.5), dict(min_visible=True),
                dict(positive_fraction=-0.1), dict(positive_fraction=1.5), dict(positive_fraction=float("nan")),
                dict(positive_fraction="1")):
        with pytest.raises(ValueError):
            TD.defect_train(lab, placement="window", **{**kw, **bad}) if "placement" not in bad else TD.defect_train(lab, **kw, **bad)
    d = TD.defect_train(lab, placement="window", min_visible=1, positive_fraction=0, **kw)
    assert (d.placement, d.min_visible, d.positive_fraction) == ("window", 1, 0.0)
    assert TD.defect_train(lab, **kw).placement == "letterbox"

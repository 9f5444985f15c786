"""Host side of the batched test loop (no GPU): the factored rect arithmetic of the paste, the job record's layout and the
argument checks of ``disyolo_mask_paste_iou_batch``, which come back as error codes before anything touches a device."""
import ctypes

import numpy as np

from disyolo_amd import lib as L
from disyolo_amd.postprocess import correct_yolo_boxes, paste_rects


def rects_before_the_refactor(box, image_h, image_w, net_size, size):
    """the body of paste_detections as it was before paste_rects was factored out of it"""
    dst = correct_yolo_boxes(box[:, :4], image_h, image_w, net_size, net_size)
    crop = np.around(box[:, :4] * np.float32(size)).astype(np.int32)
    rects = np.concatenate([crop, dst[:, [1, 0, 3, 2]]], axis=1).astype(np.int32)
    ok = ((dst[:, 3] - dst[:, 1]) * (dst[:, 2] - dst[:, 0]) > 0) & (crop[:, 2] > crop[:, 0]) & (crop[:, 3] > crop[:, 1])
    rects[~ok] = 0
    return rects, ok


BOXES = np.array([
    [0.10, 0.20, 0.60, 0.70, 1, 0.9],          # an ordinary box
    [0.00, 0.00, 1.00, 1.00, 0, 0.8],          # the whole frame
    [0.25, 0.25, 0.25, 0.75, 2, 0.7],          # no height
    [0.40, 0.50, 0.90, 0.50, 2, 0.6],          # no width
    [0.3125, 0.4375, 0.328125, 0.453125, 1, 0.5],      # corners on .5 of a map pixel: half-to-even rounding
    [0.499, 0.499, 0.501, 0.501, 0, 0.4],      # rounds to an empty crop on a small map
    [0.02, 0.02, 0.04, 0.98, 1, 0.3],          # inside the letter-box padding of a wide image: empty destination
    [0.0, 0.0, 0.0, 0.0, 0, 0.0],              # a zero-padded row of the fixed-shape output
], np.float32)


def test_paste_rects_equals_the_formula_it_was_factored_from():
    seen_ok, seen_empty = 0, 0
    for image_h, image_w, net_size, size in [(348, 620, 576, 288), (754, 1008, 576, 288), (450, 386, 576, 288), (96, 64, 96, 48),
                                             (1, 70, 96, 32), (131, 57, 96, 96)]:
        want_rects, want_ok = rects_before_the_refactor(BOXES, image_h, image_w, net_size, size)
        rects, ok = paste_rects(BOXES, image_h, image_w, net_size, size)
        assert rects.dtype == np.int32 and rects.shape == (len(BOXES), 8) and ok.dtype == bool
        np.testing.assert_array_equal(rects, want_rects)
        np.testing.assert_array_equal(ok, want_ok)
        assert (rects[~ok] == 0).all()
        seen_ok += int(ok.sum())
        seen_empty += int((~ok).sum())
    assert seen_ok >= 10 and seen_empty >= 10
    r, ok = paste_rects(np.zeros((0, 6), np.float32), 10, 10, 96, 48)
    assert r.shape == (0, 8) and ok.shape == (0,)


def test_paste_job_mirror_has_the_size_the_library_was_built_with():
    assert L.PASTE_JOB.itemsize == L.load().disyolo_paste_job_size() == 88
    assert L.PASTE_JOB.fields["n"][1] == 64 and L.PASTE_JOB.fields["block0"][1] == 80


def _job(buf, n=5, ng=2, h=37, w=53):
    p = ctypes.addressof(buf)
    j = np.zeros(1, L.PASTE_JOB)
    for f in ("masks", "rects", "classids", "gt", "gt_class", "merged", "true_map", "counts"):
        j[f] = p
    j["n"], j["ng"], j["image_h"], j["image_w"] = n, ng, h, w
    return j


def test_batch_paste_rejects_bad_arguments_before_any_launch():
    """the pointers are host buffers a launch would fault on: every call must come back with a code"""
    lib = L.load()
    buf = ctypes.create_string_buffer(1 << 12)
    p = ctypes.cast(buf, ctypes.c_void_p)
    conf = ctypes.cast(ctypes.create_string_buffer(128), ctypes.c_void_p)

    def call(j, njobs=1, size=32, table=True, dev=p, conf=conf):
        return lib.disyolo_mask_paste_iou_batch(j.ctypes.data if table else None, dev, njobs, size, conf, None)

    good = _job(buf)
    assert lib.disyolo_paste_job_plan(good.ctypes.data, 1) == 2 and good["block0"][0] == 0      # 1,961 pixels: two blocks
    too_many = _job(buf, n=65)
    assert lib.disyolo_paste_job_plan(too_many.ctypes.data, 1) == -1 and b"0..64" in lib.disyolo_last_error()
    assert call(too_many) == -1 and b"0..64" in lib.disyolo_last_error()
    assert call(good, table=False) == -1 and b"null table" in lib.disyolo_last_error()
    assert call(good, dev=None) == -1 and b"null table" in lib.disyolo_last_error()
    assert call(good, njobs=0) == -1
    assert call(good, size=0) == -1 and b"size" in lib.disyolo_last_error()
    assert call(good, size=-3) == -1 and b"size" in lib.disyolo_last_error()
    assert call(good, conf=None) == -1 and b"conf" in lib.disyolo_last_error()
    assert call(_job(buf, n=-1)) == -1
    assert call(_job(buf, ng=-1)) == -1
    assert call(_job(buf, h=0)) == -1 and b"image size" in lib.disyolo_last_error()
    assert call(_job(buf, h=1 << 16, w=1 << 15)) == -1 and b"image size" in lib.disyolo_last_error()
    no_merged = _job(buf)
    no_merged["merged"] = 0
    assert call(no_merged) == -1 and b"merged" in lib.disyolo_last_error()
    no_rects = _job(buf)
    no_rects["rects"] = 0
    assert call(no_rects) == -1 and b"n > 0" in lib.disyolo_last_error()
    no_gt = _job(buf)
    no_gt["gt"] = 0
    assert call(no_gt) == -1 and b"ng > 0" in lib.disyolo_last_error()
    two = np.concatenate([_job(buf), _job(buf)])
    assert lib.disyolo_paste_job_plan(two.ctypes.data, 2) == 4 and list(two["block0"]) == [0, 2]
    two["block0"][1] = 1                                       # a table that was not planned (or was changed afterwards)
    assert call(two, njobs=2) == -1 and b"not planned" in lib.disyolo_last_error()
    # the Python wrapper raises on the same codes
    import pytest
    with pytest.raises(L.DisyoloError, match="0..64"):
        L.paste_job_plan(too_many)

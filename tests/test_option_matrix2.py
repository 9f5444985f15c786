"""The second option matrix on the CPU: the table of tests/option_matrix2.py covers every pair of option values and the
crossings of three it names, every row gives the composed oracle finite losses and enough positive RoIs and detections for the
GPU comparison of that row to be well-posed, and every non-default option of a row changes what the oracle computes on the
row's batch.  These are conditions on the fixture, met by the reference alone."""
import itertools

import numpy as np
import pytest
import torch

import nms_modes_ref as NR
import option_matrix2 as OM
from disyolo_amd import config as cfg
from disyolo_amd.net import YOLONet
from net_setup import perturb_variables


def missing_pairs(rows):
    rows = [OM.factors(r) for r in rows]
    missing = []
    for fa, fb in itertools.combinations(OM.VALUES, 2):
        for va in OM.VALUES[fa]:
            for vb in OM.VALUES[fb]:
                if (fa, va, fb, vb) in OM.PAIRS_LEFT_OUT:
                    continue
                if not any(r[fa] == va and r[fb] == vb for r in rows):
                    missing.append("%s=%s with %s=%s" % (fa, va, fb, vb))
    return missing


def missing_triples(rows):
    return [what for what, holds in OM.TRIPLES if not any(holds(r) for r in rows)]


def test_every_pair_of_option_values_occurs_in_a_row():
    missing = missing_pairs(OM.ROWS)
    assert not missing, "pairs without a row: %s" % "; ".join(missing)
    for fa, va, fb, vb in OM.PAIRS_LEFT_OUT:       # (the pairs left out are left out: B = 1 keeps the stage-1 map)
        assert not any(OM.factors(r)[fa] == va and OM.factors(r)[fb] == vb for r in OM.ROWS), (fa, va, fb, vb)


def test_the_named_crossings_of_three_values_occur():
    missing = missing_triples(OM.ROWS)
    assert not missing, "crossings without a row: %s" % "; ".join(missing)


def test_the_extra_conditions_of_the_table():
    rows = OM.ROWS
    assert len(rows) <= 30 and len({r.name for r in rows}) == len(rows)
    for r in rows:
        for f, v in OM.factors(r).items():
            assert v in OM.VALUES[f], "%s: %s=%s is no value of the table" % (r.name, f, v)
        # every holed row's map has a hole, every map is one of its row's mask stride (lock_of_row asserts it)
        assert bool(OM.expected_pass_through(r)) == (OM.lock_kind(r) == "holed"), r.name
    maps = [r for r in rows if "map" in r.extras]
    assert len(maps) == 2 and all(r.lock == "stage1" for r in maps)
    assert any(r.H != r.W and r.D > 64 and r.k != 3 for r in maps), "a rectangular map row with wide paste jobs"
    tiled = [r for r in rows if "tiled" in r.extras]
    assert len(tiled) == 2 and any(r.D >= 100 for r in tiled)
    assert any((r.C > 16 and r.nms == "none") or r.m == 1 for r in tiled)
    loader = [r for r in rows if "loader" in r.extras]
    assert len(loader) == 1 and loader[0].H != loader[0].W


def plan_net(row, training=True, seed=1):
    net = YOLONet(training=training, plan_only=True, seed=seed, **OM.net_kwargs(row))
    perturb_variables(net, seed)
    return net


_CASES = {}


def case_of(row):
    """the row through the oracle alone, once: a plan-only net with the perturbation of the GPU tests, the training-mode
    forward, the row's batch (planted from the oracle's own detections where the row plants), the loss parts"""
    if row.name in _CASES:
        return _CASES[row.name]
    net = plan_net(row)
    p = {k: v.detach().float().clone() for k, v in net.params.items()}
    fwd = {}

    def det_of(b):
        with torch.no_grad():
            fwd["out"] = OM.oracle_forward(row, p, b["images"], True, {})
        return OM.oracle_detections(row, fwd["out"][0], b["clip_window"], OM.DET_THRESH)

    b, perms, planted = OM.row_batch(row, det_of)
    with torch.no_grad():
        yolos, mask_pos = fwd["out"] if fwd else OM.oracle_forward(row, p, b["images"], True, {})
        parts, det = OM.oracle_losses(row, p, yolos, mask_pos, b, perms)
    _CASES[row.name] = dict(net=net, p=p, b=b, perms=perms, planted=planted, yolos=yolos, mask_pos=mask_pos, parts=parts, det=det)
    return _CASES[row.name]


def kept(det):
    return [int(v) for v in (np.abs(det[..., :4]).sum(-1) != 0).sum(1)]


@pytest.mark.parametrize("row", OM.ROWS, ids=OM.ids(OM.ROWS))
def test_oracle_is_finite_with_positive_rois_on_every_row(row):
    what = OM.describe(row)
    c = case_of(row)
    net, b, parts, det = c["net"], c["b"], c["parts"], c["det"]
    assert net.pass_through_layers() == OM.expected_pass_through(row), what
    assert set(net.trainable_names()) == set(OM.trainable_names(row)), what
    assert [tuple(y.shape) for y in c["yolos"]] == [(row.B, row.H // g, row.W // g, 3, 5 + row.C) for g in (8, 16, 32)], what
    assert tuple(c["mask_pos"].shape) == (row.B, row.H // row.m, row.W // row.m, row.k ** 2), what
    assert tuple(b["true_boxes"].shape) == (row.B, 1, 1, 1, row.G, 5) and tuple(det.shape) == (row.B, row.D, 6), what
    assert b["perm_det"].shape == (row.B, row.D) and b["perm_gt"].shape == (row.B, row.G), what
    bad = [n for n, v in parts.items() if not np.isfinite(float(v))]
    assert not bad, "%s: oracle loss parts not finite: %s" % (what, bad)
    npos = OM.positives(row, det, b, c["perms"])
    rows_used = [r for r in range(row.G) if np.abs(b["true_boxes"].numpy()[0, 0, 0, 0, r, :4]).sum() != 0]
    print("%s: oracle %s, positive RoIs per image %s, detections per image %s" % (
        row.name, " ".join("%s %.5f" % (n, float(v)) for n, v in parts.items()), npos, kept(det)))
    assert len(rows_used) >= 20 and max(rows_used) == row.G - 1, "%s: twenty instances spread over the %d rows" % (what, row.G)
    assert min(npos) >= 1 and float(parts["mask"]) > 0, "%s: every image needs a positive RoI (per image %s)" % (what, npos)
    if row.rois[0] + row.rois[1] > 16:
        assert min(npos) > 16, "%s: the wide table needs more than 16 positives per image (got %s)" % (what, npos)
    if row.G > 64 and row.rois[1] > 0:
        r, _ = OM.RR.rows(det, b["true_boxes"].numpy()[:, 0, 0, 0], c["perms"], row.H // row.m, row.W // row.m, row.k, *row.rois)
        assert max(q[2 * row.k + 2] for x in r for q in x) >= 64, "%s: a ground-truth row >= 64 is assigned" % what
    if c["planted"] is not None:
        want = 17 if row.rois[1] == 0 else 1
        assert min(len(x) for x in c["planted"]) >= want, "%s: planted per image %s" % (what, [len(x) for x in c["planted"]])


_INFER = {}


def infer_case(row):
    """the inference net of the GPU test (d) through the oracle: its batch, the oracle's logits and detections"""
    if row.name not in _INFER:
        net = plan_net(row, training=False, seed=0)
        p = {k: v.detach().float().clone() for k, v in net.params.items()}
        b = OM.infer_batch(row)
        with torch.no_grad():
            yolos, mask_pos = OM.oracle_forward(row, p, b["images"], False)
        _INFER[row.name] = (b, yolos, OM.oracle_detections(row, yolos, b["clip_window"], OM.INFER_THRESH))
    return _INFER[row.name]


WIDE_D = [r for r in OM.ROWS if r.D > 64]


@pytest.mark.parametrize("row", WIDE_D, ids=OM.ids(WIDE_D))
def test_rows_past_64_detections_keep_more_than_64(row):
    """where D > 64 the oracle's filter at the inference threshold of the GPU test keeps more than 64 rows per image"""
    b, _, det = infer_case(row)
    print("%s: detections per image at %.2f: %s" % (row.name, OM.INFER_THRESH, kept(det)))
    assert min(kept(det)) > 64, "%s: kept rows per image %s" % (OM.describe(row), kept(det))
    assert not np.array_equal(b["clip_window"][-1], [0.0, 0.0, 1.0, 1.0])


@pytest.mark.parametrize("row", OM.ROWS, ids=OM.ids(OM.ROWS))
def test_every_non_default_option_bites_on_its_row(row):
    """each non-default option of the row reset to its default, one at a time, on the same forward pass: the total loss moves
    by more than 1e-4 relative, or the detections differ.  (max_box_per_image sizes the batch itself and has no reset; the RoI
    counts and the IoU threshold are held to ``roi_option_bites``.)  The row's NMS mode gives other detections than the two other modes: a cross-class suppression for agnostic, an overlapping
    pair kept for none"""
    what = OM.describe(row)
    c = case_of(row)
    total = float(c["parts"]["total"])

    def differs(**kw):
        with torch.no_grad():
            parts, det = OM.oracle_losses(row, c["p"], c["yolos"], c["mask_pos"], c["b"], c["perms"], **kw)
        if det.shape != c["det"].shape:
            n = min(det.shape[1], c["det"].shape[1])
            same = np.array_equal(det[:, :n], c["det"][:, :n]) and kept(det) == kept(c["det"])
        else:
            same = np.array_equal(det, c["det"])
        return abs(float(parts["total"]) - total) > 1e-4 * abs(total) or not same

    for mode in NR.MODES:
        if mode != row.nms:
            other = OM.oracle_detections(row, c["yolos"], c["b"]["clip_window"], OM.DET_THRESH, nms=mode)
            assert not np.array_equal(other, c["det"]), "%s: nms=%s gives the same detections" % (what, mode)
    if row.D != cfg.MAX_DETECTION:
        perms = [(p[0][p[0] < cfg.MAX_DETECTION], p[1]) for p in c["perms"]]      # (a permutation of the default's entries)
        with torch.no_grad():
            parts, det = OM.oracle_losses(row, c["p"], c["yolos"], c["mask_pos"], c["b"], perms, D=cfg.MAX_DETECTION)
        assert kept(det) != kept(c["det"]) or abs(float(parts["total"]) - total) > 1e-4 * abs(total), "%s: D does not bite" % what
    if row.anchors != "cfg":
        assert differs(anchors=np.asarray(cfg.ANCHORS, np.float32)), "%s: the anchors do not bite" % what
    n_det, n_gt, iou = row.rois
    for name, other in (("the RoI counts", (cfg.MASK_ROI_DET, cfg.MASK_ROI_GT, iou)), ("the IoU threshold", (n_det, n_gt, cfg.MASK_ROI_IOU))):
        if other != row.rois:
            roi_option_bites(row, c, other, name)


def roi_option_bites(row, c, other, name):
    """The RoI options act on the mask term alone, which is 0.2 to 0.4 % of the total loss of these untrained nets (the wh term
    of the perturbed heads is 2000 to 5000): with the configured counts it moves by 0.04 to 3 %, 1e-6 to 7e-5 of the total.  So
    the condition is held where the option acts: the mask term moves by more than 1e-4 relative (the condition of
    tests/test_gpu_mask_rois.py), and the selection itself differs -- another number of positives per image -- which is what the
    GPU test compares bit for bit.  The total's relative move is printed"""
    what = OM.describe(row)
    total, mask = float(c["parts"]["total"]), float(c["parts"]["mask"])
    with torch.no_grad():
        parts, _ = OM.oracle_losses(row, c["p"], c["yolos"], c["mask_pos"], c["b"], c["perms"], rois=other)
    pos, pos_other = OM.positives(row, c["det"], c["b"], c["perms"]), OM.positives(row, c["det"], c["b"], c["perms"], rois=other)
    print("%s: %s %s -> %s: mask term %.6f -> %.6f, total moves by %.2e relative, positives %s -> %s" % (
        row.name, name, row.rois, other, mask, float(parts["mask"]), abs(float(parts["total"]) - total) / abs(total), pos, pos_other))
    assert abs(float(parts["mask"]) - mask) > 1e-4 * abs(mask), "%s: %s do not move the mask term" % (what, name)
    assert pos != pos_other, "%s: %s leave the selection as it was" % (what, name)

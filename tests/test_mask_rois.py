"""The mask loss's RoI counts as options of the net (``mask_roi_det``, ``mask_roi_gt``, ``mask_roi_iou``), without a GPU: the
reference of tests/mask_roi_ref.py against the oracle at (7, 3, 0.5), the options and their errors on a plan-only net, the
argument errors of the three _x entry points, and every case of tests/test_gpu_mask_rois.py held to the condition it exists for."""
import ctypes
import math

import numpy as np
import pytest
import torch

import disyolo_oracle as O
import mask_roi_ref as MR
from disyolo_amd import config as cfg
from disyolo_amd import lib as L
from disyolo_amd.net import YOLONet


# ------------------------------------------------------------------------------------------------ 1. the reference
def random_case(seed, B=3, D=30, G=20, S=32):
    """random boxes and masks at S x S (score maps S/2 x S/2): zero rows between the filled ones, jittered detections"""
    rng = np.random.RandomState(seed)
    det = np.zeros((B, D, 6), np.float32)
    tb = np.zeros((B, G, 5), np.float32)
    tm = rng.rand(B, G, S, S) < 0.5
    for b in range(B):
        for r in sorted(rng.choice(G, 9, replace=False)):
            w, h = rng.uniform(0.15, 0.6, size=2)
            tb[b, r] = [rng.uniform(w / 2, 1 - w / 2), rng.uniform(h / 2, 1 - h / 2), w, h, rng.randint(0, 3)]
        filled = np.where(tb[b, :, 2] > 0)[0]
        for q in sorted(rng.choice(D, 19, replace=False)):
            xc, yc, w, h = tb[b, filled[rng.randint(len(filled))], :4]
            e = rng.uniform(-1, 1, 4) * rng.choice([0.02, 0.1, 0.3]) * np.array([h, w, h, w])
            det[b, q] = [yc - h / 2 + e[0], xc - w / 2 + e[1], yc + h / 2 + e[2], xc + w / 2 + e[3], 0, 0.9]
    perms = [(rng.permutation(D).astype(np.int32), rng.permutation(G).astype(np.int32)) for _ in range(B)]
    return det, tb, tm, perms


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_reference_at_7_3_half_equals_the_oracle(seed):
    det, tb, tm, perms = random_case(seed)
    B, sm = det.shape[0], 16
    some_negative = False
    for i in range(B):
        for pd, pg in ((None, None), perms[i]):
            want = O.select_mask_rois(det[i], tb[i], pd, pg)
            got = MR.select(det[i], tb[i], 7, 3, 0.5, pd, pg)
            for w, g in zip(want, got[:3]):
                np.testing.assert_array_equal(w, g)
            some_negative |= len(got[3]) < got[4]
            assert list(got[3]) == sorted(got[3]) and got[4] <= 10
    assert some_negative, "the cases need a negative RoI"
    assert any((np.abs(tb[i, :r, :4]).sum(1) == 0).any() for i in range(B) for r in np.where(tb[i, :, 2] > 0)[0])
    score = torch.randn(B, sm, sm, 9, generator=torch.Generator().manual_seed(seed)).double()
    for p in (None, perms):
        want = O.loss_mask(det, score, tb.reshape(B, 1, 1, 1, -1, 5), tm, p)
        got = MR.loss_mask(det, score, tb, tm, 7, 3, 0.5, p)
        assert float(want) > 0 and float(got) == float(want)


def test_reference_counts_take_what_is_there_and_zero_leaves_a_kind_out():
    det, tb, tm, perms = random_case(7)
    for i in range(det.shape[0]):
        nd, ng = int((np.abs(det[i, :, :4]).sum(1) != 0).sum()), int((np.abs(tb[i, :, :4]).sum(1) != 0).sum())
        assert MR.select(det[i], tb[i], 256, 256, 0.5, *perms[i])[4] == nd + ng
        assert MR.select(det[i], tb[i], 0, 256, 0.5, *perms[i])[4] == ng
        assert MR.select(det[i], tb[i], 256, 0, 0.5, *perms[i])[4] == nd
        pos, assign, gt_rows, idx, nr = MR.select(det[i], tb[i], 0, 256, 0.5, *perms[i])
        assert len(pos) == ng, "every ground-truth box is positive by itself"
        assert len(MR.select(det[i], tb[i], 256, 256, 1.0, *perms[i])[0]) >= ng      # the threshold is inclusive
        assert len(MR.select(det[i], tb[i], 256, 0, 0.95, *perms[i])[0]) < len(MR.select(det[i], tb[i], 256, 0, 0.3, *perms[i])[0])


# ------------------------------------------------------------------------------------------------ 2. the options
def plan(**kw):
    return YOLONet(training=True, plan_only=True, image_size=64, batch_size=2, **kw)


def test_options_default_to_cfg_and_are_kept_per_net(monkeypatch):
    a = plan()
    assert (a.mask_roi_det, a.mask_roi_gt, a.mask_roi_iou) == (cfg.MASK_ROI_DET, cfg.MASK_ROI_GT, cfg.MASK_ROI_IOU) == (7, 3, 0.5)
    b = plan(mask_roi_det=7, mask_roi_gt=3, mask_roi_iou=0.5)
    assert (b.mask_roi_det, b.mask_roi_gt, b.mask_roi_iou, b.mask_roi_rows) == (7, 3, 0.5, 16) and a.mask_roi_rows == 16
    c = plan(mask_roi_det=256, mask_roi_gt=256, mask_roi_iou=1)
    assert (c.mask_roi_det, c.mask_roi_gt, c.mask_roi_iou, c.mask_roi_rows) == (256, 256, 1.0, 512)
    assert isinstance(c.mask_roi_iou, float) and isinstance(c.mask_roi_det, int)
    assert plan(mask_roi_det=0).mask_roi_det == 0 and plan(mask_roi_gt=0).mask_roi_gt == 0
    assert plan(mask_roi_det=10, mask_roi_gt=6).mask_roi_rows == 16 and plan(mask_roi_det=9, mask_roi_gt=8).mask_roi_rows == 17
    assert plan(mask_roi_det=np.int64(12)).mask_roi_det == 12 and plan(mask_roi_iou=np.float32(0.25)).mask_roi_iou == 0.25
    # the cfg values are read at construction only: two nets in one process can differ
    monkeypatch.setattr(cfg, "MASK_ROI_DET", 30)
    monkeypatch.setattr(cfg, "MASK_ROI_GT", 20)
    monkeypatch.setattr(cfg, "MASK_ROI_IOU", 0.6)
    d = plan()
    assert (d.mask_roi_det, d.mask_roi_gt, d.mask_roi_iou, d.mask_roi_rows) == (30, 20, 0.6, 50)
    assert (a.mask_roi_det, a.mask_roi_gt, a.mask_roi_iou) == (7, 3, 0.5)


@pytest.mark.parametrize("name", ["mask_roi_det", "mask_roi_gt"])
@pytest.mark.parametrize("bad", [-1, 257, True, False, 7.0, "7", (7,), float("nan")])
def test_counts_are_ints_in_0_to_256(name, bad):
    with pytest.raises(ValueError, match=name + " must be .*0..256"):
        plan(**{name: bad})


def test_counts_must_leave_an_roi():
    with pytest.raises(ValueError, match="at least 1"):
        plan(mask_roi_det=0, mask_roi_gt=0)


@pytest.mark.parametrize("bad", [0, 0.0, -0.5, 1.0001, 2, float("nan"), float("inf"), True, "0.5", (0.5,)])
def test_iou_threshold_is_a_finite_float_in_0_1(bad):
    with pytest.raises(ValueError, match=r"mask_roi_iou must be .*\(0, 1\]"):
        plan(mask_roi_iou=bad)


# ------------------------------------------------------------------------------------------------ 3. the entry points
def _host():
    buf = ctypes.create_string_buffer(1 << 20)
    return buf, ctypes.cast(buf, ctypes.c_void_p)


def test_constants_and_the_old_limit():
    assert L.ROI_MAX == MR.ROI_MAX == 16 and L.ROI_CAP == MR.ROI_CAP == 512
    lib = L.load()
    buf, p = _host()
    assert lib.disyolo_mask_rois_hw(p, 30, p, 20, p, p, 2, 24, 40, 3, 9, 8, 0.5, p, p, None) == -1
    assert b"n_det + n_gt > 16" in lib.disyolo_last_error()
    assert lib.disyolo_mask_rois(p, 30, p, 20, p, p, 2, 32, 9, 8, 0.5, p, p, None) == -1
    assert b"n_det + n_gt > 16" in lib.disyolo_last_error()


def test_mask_rois_x_refuses_before_any_launch():
    lib = L.load()
    buf, p = _host()

    def rois(max_det=256, G=256, det=p, tb=p, out=p, cnt=p, n_det=9, n_gt=8, cap=17, k=3, B=2, Hm=24, Wm=40):
        return lib.disyolo_mask_rois_x(det, max_det, tb, G, p, p, B, Hm, Wm, k, n_det, n_gt, 0.5, cap, out, cnt, None)

    for kw in (dict(max_det=0), dict(max_det=257), dict(G=0), dict(G=257)):
        assert rois(**kw) == -1 and b"1..256" in lib.disyolo_last_error(), kw
    for kw in (dict(det=None), dict(tb=None), dict(out=None), dict(cnt=None)):
        assert rois(**kw) == -1 and b"null pointer" in lib.disyolo_last_error(), kw
    for kw in (dict(cap=0), dict(cap=513), dict(cap=-1)):
        assert rois(**kw) == -1 and b"roi_cap must be in 1..512" in lib.disyolo_last_error(), kw
    for kw in (dict(cap=16), dict(n_det=256, n_gt=256, cap=511), dict(n_det=-1), dict(n_gt=-1), dict(n_det=513, n_gt=0, cap=512)):
        assert rois(**kw) == -1 and b"n_det + n_gt" in lib.disyolo_last_error(), kw
    for k in (2, 4, 9):
        assert rois(k=k) == -1 and b"k = 3" in lib.disyolo_last_error()
    for kw in (dict(B=0), dict(Hm=0), dict(Wm=-1)):
        assert rois(**kw) == -1 and b"bad sizes" in lib.disyolo_last_error(), kw
    rois_t = torch.zeros(2, 17, 12, dtype=torch.int32)
    with pytest.raises(L.DisyoloError, match="rois must be"):
        L.mask_rois_x(None, 30, None, 20, None, None, 2, (24, 40), 9, 8, 0.5, rois_t, None, k=5)


def test_psroi_loss_x_refuses_before_any_launch_and_its_workspace():
    lib = L.load()
    buf, p = _host()
    B, Hm, Wm = 2, 24, 40
    nblk = math.ceil(Hm * Wm / 256)
    for cap in (1, 16, 17, 512):
        assert lib.disyolo_psroi_loss_workspace_x(B, Hm, Wm, cap) == (B * nblk * cap + B) * 4
    assert lib.disyolo_psroi_loss_workspace_x(B, Hm, Wm, 16) == lib.disyolo_psroi_loss_workspace_hw(B, Hm, Wm)
    for args in ((0, Hm, Wm, 17), (B, 0, Wm, 17), (B, Hm, 0, 17), (B, Hm, Wm, 0), (B, Hm, Wm, 513)):
        assert lib.disyolo_psroi_loss_workspace_x(*args) == 0
    assert L.psroi_loss_workspace_x(B, (Hm, Wm), 512) == (B * nblk * 512 + B) * 4
    # the cost at the headline shape: B = 8, 288 x 288 maps, 512 rows
    assert L.psroi_loss_workspace_x(8, 288, 512) == (8 * 324 * 512 + 8) * 4

    def loss(score=p, tm=p, G=20, rois=p, cnt=p, cap=17, B=B, Hm=Hm, Wm=Wm, st=2, k=3, ds=p, out=p, ws=p, ws_bytes=len(buf)):
        return lib.disyolo_psroi_loss_x(score, tm, G, rois, cnt, cap, B, Hm, Wm, st, k, 5.0, ds, out, ws, ws_bytes, None)

    for kw in (dict(score=None), dict(tm=None), dict(rois=None), dict(cnt=None), dict(ds=None), dict(out=None)):
        assert loss(**kw) == -1 and b"null pointer" in lib.disyolo_last_error(), kw
    for kw in (dict(B=0), dict(Hm=0), dict(Wm=0), dict(G=0)):
        assert loss(**kw) == -1 and b"bad sizes" in lib.disyolo_last_error(), kw
    for kw in (dict(cap=0), dict(cap=513)):
        assert loss(**kw) == -1 and b"roi_cap must be in 1..512" in lib.disyolo_last_error(), kw
    for k in (2, 4, 9):
        assert loss(k=k) == -1 and b"k = 3" in lib.disyolo_last_error()
    for st in (0, 3, 8):
        assert loss(st=st) == -1 and b"mask_stride" in lib.disyolo_last_error()
    need = lib.disyolo_psroi_loss_workspace_x(B, Hm, Wm, 17)
    assert loss(ws_bytes=need - 1) == -2 and b"workspace" in lib.disyolo_last_error()
    assert loss(ws=None) == -2


# ------------------------------------------------------------------------------------------------ 4. the GPU cases
def _sel_rows(n_det, n_gt, D, G, k=3):
    det, tb, perms = MR.sel_case(D, G)
    Hm, Wm = MR.SEL_MAP
    return (det, tb) + MR.rows(det, tb, perms, Hm, Wm, k, n_det, n_gt, 0.5)


@pytest.mark.parametrize("n_det,n_gt,D,G", MR.SEL_CASES)
def test_selection_cases_hold_their_conditions(n_det, n_gt, D, G):
    det, tb, rows, info = _sel_rows(n_det, n_gt, D, G)
    Hm, Wm = MR.SEL_MAP
    nz_det = [(np.abs(det[i, :, :4]).sum(1) != 0).sum() for i in range(3)]
    nz_gt = [(np.abs(tb[i, :, :4]).sum(1) != 0).sum() for i in range(3)]
    assert [nr for _, nr in info] == [min(n_det, nz_det[i]) + min(n_gt, nz_gt[i]) for i in range(3)]
    assert n_det + n_gt > 16
    assert len(rows[2]) == 0 and info[2][1] == min(n_det, nz_det[2]), "image 2 has RoIs and no positive"
    if n_det:
        assert nz_det[1] == 5 < n_det, "image 1 has fewer non-zero detections than n_det"
        assert nz_det[0] < D and (np.abs(det[0, :nz_det[0], :4]).sum(1) == 0).any(), "zero rows between the filled ones"
    if n_gt:
        assert len(rows[0]) >= min(n_gt, nz_gt[0]), "every picked box is positive by itself"
    if n_det + n_gt >= 50:
        assert len(rows[0]) > 16, "an image with more than 16 positives"
        idx = info[0][0]
        assert any(r >= 16 and idx[r] != r for r in range(len(idx))), "a positive at row >= 16 behind a negative"
    # the IoUs are far from the threshold, so that f32 and f64 decide alike: positives >= 225/287, negatives <= 9/256
    for i in range(2):
        pos, assign, gt_rows, idx, nr = MR.select(det[i], tb[i], n_det, n_gt, 0.1, *MR.sel_case(D, G)[2][i])
        assert list(idx) == list(info[i][0]), "no IoU between 0.1 and 0.5"
        assert list(MR.select(det[i], tb[i], n_det, n_gt, 0.78, *MR.sel_case(D, G)[2][i])[3]) == list(idx)
    for r in rows[0] + rows[1]:
        assert 0 <= r[0] < r[3] <= Hm + 1 and 0 <= r[4] < r[7] <= Wm + 1 and r[9] > 0 and 0 <= r[8] < G


def test_selection_at_7_3_and_10_6_fits_the_old_table():
    for D, G in MR.OLD_SIZES:
        for n_det, n_gt in MR.OLD_CASES:
            det, tb, rows, info = _sel_rows(n_det, n_gt, D, G)
            assert max(len(r) for r in rows) <= 16 and len(rows[0]) > 0
            assert any(len(idx) < nr for idx, nr in info), "a negative among the RoIs"


@pytest.mark.parametrize("Hm,Wm", MR.LOSS_MAPS + ((8, 300),))
@pytest.mark.parametrize("nrow", MR.LOSS_ROWS)
def test_loss_tables_hold_their_conditions(nrow, Hm, Wm):
    assert (Hm * Wm) % 256 != 0, "a map whose pixel count is not a multiple of 256"
    for k in (3, 7):
        table, cnt = MR.loss_table(nrow, Hm, Wm, k)
        assert list(cnt) == [nrow, min(nrow, 9), 0] and table.shape == (3, nrow, MR.roi_w(k))
        assert (table[0, :, 2 * k + 3] > 0).all() and (table[:, :, 2 * k + 2] < MR.LOSS_G).all()
        cover = MR.cover_of(table, cnt, Hm, Wm, k)
        assert cover[0].max() >= 17, "a pixel covered by at least 17 RoIs"
        assert cover[2].max() == 0 and (cover[1] == 0).any() and (cover[0] == 0).sum() >= 0
        lists = MR.block_lists(table, cnt, Hm, Wm, k)
        assert any(len(l) == 0 for l in lists[1]), "a block whose culled list is empty"
        assert all(l == sorted(l) for per in lists for l in per)
        if nrow >= 64:
            gy0, gyk, gx0, gxk = table[0, :, 0], table[0, :, k], table[0, :, k + 1], table[0, :, 2 * k + 1]
            assert (gy0 < 0).any() and (gyk > Hm).any() and (gx0 < 0).any() and (gxk > Wm).any(), "RoIs across the four borders"
            assert max(len(l) for l in lists[0]) > 16, "a block with more than 16 RoIs in its list"
            assert any(len(l) < nrow for l in lists[0]), "a block that culls"
        if (Hm, Wm) != (24, 40) and nrow >= 64:
            # a block within one row of the map drops an RoI of that row by its columns
            npx = Hm * Wm
            found = False
            for j, i0 in enumerate(range(0, npx, 256)):
                i1 = min(i0 + 255, npx - 1)
                if i0 // Wm == i1 // Wm:
                    y = i0 // Wm
                    in_row = [r for r in range(nrow) if table[0, r, 0] <= y < table[0, r, k]]
                    found |= any(r not in lists[0][j] for r in in_row)
            assert found


def test_zero_area_row_gives_nan_in_the_reference():
    k, Hm, Wm = 3, 24, 40
    row = MR.row_of(5, Wm + 2, 9, Wm + 6, 0, Hm, Wm, k)             # wholly right of the map
    assert row[2 * k + 3] == 0
    table, cnt = MR.table_of([[MR.row_of(2, 2, 9, 9, 1, Hm, Wm, k), row]], 17, k)
    score, tm = MR.loss_inputs(Hm, Wm, k, 2, B=1)
    want, grad = MR.loss_want(table, cnt, score, tm, 2, k)
    assert np.isnan(want)


def test_planted_detections_are_positive_by_themselves():
    import limits_ref as LR
    b = LR.net_batch(11, B=MR.NET_B, S=MR.NET_S, G=MR.NET_G, rows=MR.NET_ROWS)
    rng = np.random.RandomState(3)
    det = np.zeros((2, 40, 6), np.float32)
    for i in range(2):
        for q in range(12):
            y1, x1 = rng.uniform(0, 0.6, 2)
            h, w = rng.uniform(0.02, 0.3, 2) if q % 2 else rng.uniform(0.13, 0.3, 2)
            det[i, q] = [y1, x1, y1 + h, x1 + w, 0, 0.9]
    g, rows = MR.plant_detections(b, det, LR.NET_ANCH)
    tb = g["true_boxes"].numpy()[:, 0, 0, 0]
    assert [len(r) for r in rows] == [3, 3] and ((np.abs(tb[..., :4]).sum(-1) != 0).sum(1) == 20).all()
    assert not np.array_equal(tb, b["true_boxes"].numpy()[:, 0, 0, 0]) and any(not torch.equal(g[k], b[k]) for k in ("yolo1", "yolo2", "yolo3"))
    for i in range(2):
        pos, assign, gt_rows, idx, nr = MR.select(det[i], tb[i], 40, 0, 0.5)
        assert nr == 12 and set(q for q, _ in rows[i]) <= set(idx.tolist())
        for q, r in rows[i]:
            assert gt_rows[assign[list(idx).index(q)]] == r and g["true_masks"][i, r].sum() >= 64
        before = MR.select(det[i], b["true_boxes"].numpy()[i, 0, 0, 0], 40, 0, 0.5)[3]
        assert not set(q for q, _ in rows[i]) <= set(before.tolist())


def test_net_batch_has_twenty_boxes_per_image():
    import limits_ref as LR
    b = LR.net_batch(11, B=MR.NET_B, S=MR.NET_S, G=MR.NET_G, rows=MR.NET_ROWS)
    tb = b["true_boxes"].numpy()[:, 0, 0, 0]
    assert tb.shape == (2, 40, 5) and ((np.abs(tb[..., :4]).sum(-1) != 0).sum(1) == 20).all()
    for i in range(2):
        pos, assign, gt_rows, idx, nr = MR.select(np.zeros((40, 6), np.float32), tb[i], 40, 40, 0.5)
        assert nr == 20 and len(pos) == 20 > MR.ROI_MAX, "the boxes alone give more than 16 positives"

"""Anchors and per-image limits per net on the GPU: the detection filter at 65 / 100 / 256 detections in its three NMS modes,
``shuffle_perm`` and ``mask_rois`` at up to 256 rows, the YOLO loss with 65 / 256 ground-truth boxes, the batched paste with
100 / 256 detections, and whole nets built with ``anchors=``, ``max_box_per_image=`` and ``max_detection=``.

The cases and their CPU references are in tests/limits_ref.py (tests/test_limits.py holds each to the condition that makes it
a case).  The filter, the RoI selection, the permutations and the paste are compared exactly: a difference is another
decision, not rounding.  The loss keeps the bounds of tests/test_gpu_loss.py and the whole step those of
tests/test_gpu_lock_map.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import disyolo_oracle as O
import limits_ref as LR
import nms_modes_ref as R
from disyolo_amd import config as cfg
from disyolo_amd import evaluate as E
from disyolo_amd import lib as L
from disyolo_amd import train_data as TD
from disyolo_amd.net import YOLONet
from disyolo_amd.postprocess import SegmentationAccuracy
from net_setup import perturb_variables
from test_gpu_eval_batch import guard_intact, guarded, same_detfiles
from test_gpu_lock_map import _same_state, oracle_params, rel_err
from test_gpu_loss import bits, check_yolo_outputs
from test_gpu_nms_modes import decoded, random_logits

pytestmark = pytest.mark.gpu

ANCH = np.asarray(cfg.ANCHORS, np.float32)


# ------------------------------------------------------------------------------------------------ 1. the filter
def run_detect(dev, ys, S, Cn, anchors, win, thr, nms_thr, mode, max_det, ws=None, entry=None):
    """L.detect (or, ``entry``: that C entry point called directly) on logits [B,g,g,3,5+C] x 3 -> rows, counts, decode results"""
    B = ys[0].shape[0]
    det = torch.full((B, max_det, 6), float("nan"), device=dev)
    cnt = torch.full((B,), -1, dtype=torch.int32, device=dev)
    logits = [y.reshape(B, y.shape[1], y.shape[2], 3 * (5 + Cn)).contiguous().to(dev) for y in ys]
    ws = ws or L.Workspace(dev)
    anc = np.asarray(anchors, np.float32).reshape(-1)
    wint = torch.as_tensor(win, device=dev).float()
    if entry is None:
        L.detect(logits[0], logits[1], logits[2], B, S, Cn, anc, wint, float(thr), float(nms_thr), max_det, det, cnt, ws, nms=mode)
    else:
        lib = L.load()
        need = lib.disyolo_detect_workspace_x(B, S, S, Cn, max_det) if entry == "disyolo_detect_x" else \
            lib.disyolo_detect_workspace_hw(B, S, S, Cn)
        buf = ws.get(need)
        p = lambda t: C.c_void_p(t.data_ptr())
        rc = getattr(lib, entry)(p(logits[0]), p(logits[1]), p(logits[2]), B, S, S, Cn, (C.c_float * 18)(*[float(v) for v in anc]),
                                 p(wint), float(thr), float(nms_thr), max_det, L.nms_mode(mode), p(det), p(cnt), p(buf),
                                 buf.numel(), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, lib.disyolo_last_error()
    torch.cuda.synchronize()
    return det.cpu().numpy(), cnt.cpu().numpy().tolist(), decoded(ws, B, LR.n_cand(S))


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("D", LR.FILTER_D)
@pytest.mark.parametrize("Cn", LR.FILTER_C)
def test_filter_keeps_up_to_256_rows(dev, Cn, D, mode):
    """S = 96, B = 2, the second image with its own window; C = 3 crosses C * D = 512 between D = 100 and 256 (LDS rank merge
    -> k-way merge), C = 80 runs the bucketed path"""
    ys = LR.filter_logits(Cn)
    got, cnt, dec = run_detect(dev, ys, LR.FILTER_S, Cn, LR.FILTER_ANCH, LR.FILTER_WIN, LR.FILTER_THR, LR.FILTER_NMS, mode, D)
    want, want_cnt = LR.restated(dec, LR.FILTER_THR, LR.FILTER_NMS, mode, D)
    assert min(want_cnt) > 64, "the case must keep more than 64 rows in every image: %s" % want_cnt
    np.testing.assert_array_equal(got, want)
    assert cnt == want_cnt
    # (the oracle's own decode of these logits keeps as many rows: tests/test_limits.py)
    assert cnt == LR.filter_want(ys, D, mode)[1]


@pytest.mark.parametrize("mode", R.MODES)
def test_filter_256_rows_of_a_dense_576_image(dev, mode):
    """20,412 candidates above the threshold: the register form of the image-wide loop with 256 winners, and the per-class
    lists past 8,192 in global memory"""
    S, D = 576, 256
    ys = random_logits("dense", S)
    thr, nms_thr = 0.25, cfg.IOU_THRESHOLD
    got, cnt, dec = run_detect(dev, ys, S, 3, ANCH, LR.FILTER_WIN, thr, nms_thr, mode, D)
    assert (dec[1] > np.float32(thr)).sum(axis=1).tolist() == [LR.n_cand(S)] * 2
    want, want_cnt = LR.restated(dec, thr, nms_thr, mode, D)
    np.testing.assert_array_equal(got, want)
    assert cnt == want_cnt and min(cnt) > 64


@pytest.mark.parametrize("D", [30, 64])
@pytest.mark.parametrize("Cn", [3, 80])
def test_new_entry_point_at_the_old_sizes_is_bit_identical(dev, Cn, D):
    ys = LR.filter_logits(Cn)
    for mode in R.MODES:
        old = run_detect(dev, ys, LR.FILTER_S, Cn, LR.FILTER_ANCH, LR.FILTER_WIN, LR.FILTER_THR, LR.FILTER_NMS, mode, D,
                         entry="disyolo_detect_nms_hw")
        new = run_detect(dev, ys, LR.FILTER_S, Cn, LR.FILTER_ANCH, LR.FILTER_WIN, LR.FILTER_THR, LR.FILTER_NMS, mode, D,
                         entry="disyolo_detect_x")
        assert min(old[1]) > 0 and not np.isnan(old[0]).any()
        assert old[0].tobytes() == new[0].tobytes() and old[1] == new[1]


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("Cn,D", [(16, 64), (10, 64), (16, 40), (9, 57)])
def test_up_to_16_classes_past_512_kept_rows_take_the_new_entry_point(dev, Cn, D, mode):
    """C <= 16 with C * D > 512 and D <= 64: more survivors than the LDS rank merge of the old entry point holds, which it
    refuses (in every mode) -- L.detect sends these sizes to disyolo_detect_x, whose per-class form merges k-way"""
    assert L.detect_takes_x(Cn, D) and Cn * D > 512 and D <= 64
    ys = LR.filter_logits(Cn)
    args = (dev, ys, LR.FILTER_S, Cn, LR.FILTER_ANCH, LR.FILTER_WIN, LR.FILTER_THR, LR.FILTER_NMS, mode, D)
    got, cnt, dec = run_detect(*args)
    want, want_cnt = LR.restated(dec, LR.FILTER_THR, LR.FILTER_NMS, mode, D)
    np.testing.assert_array_equal(got, want)
    assert cnt == want_cnt and min(cnt) > 30
    direct = run_detect(*args, entry="disyolo_detect_x")
    assert direct[0].tobytes() == got.tobytes() and direct[1] == cnt
    # the entry point of before still refuses, with its message
    lib = L.load()
    buf = L.Workspace(dev).get(lib.disyolo_detect_workspace_hw(2, LR.FILTER_S, LR.FILTER_S, Cn))
    p = C.c_void_p(buf.data_ptr())
    anc = (C.c_float * 18)(*[float(v) for v in LR.FILTER_ANCH.reshape(-1)])
    assert lib.disyolo_detect_nms_hw(p, p, p, 2, LR.FILTER_S, LR.FILTER_S, Cn, anc, p, 0.25, 0.3, D, L.nms_mode(mode), p, p, p,
                                     buf.numel(), None) == -1
    assert b"max_det must be <= 64" in lib.disyolo_last_error()


def test_net_of_16_classes_and_40_detections_detects(dev):
    """YOLONet(classes=<16 names>, max_detection=40): 640 kept rows at most, past the old merge; the net's filter runs and
    equals the oracle's on the kernel's logits"""
    Cn, D, S, B = 16, 40, 64, 2
    net = YOLONet(training=False, device=dev, image_size=S, batch_size=B, stage=1, seed=3, classes=["c%02d" % i for i in range(Cn)],
                  max_detection=D)
    perturb_variables(net, 3, "scale")
    net.refresh_weights()
    b = O.synthetic_batch(B, S, seed=5)
    preds, det, _ = net.forward(b["images"], b["clip_window"], [0.02], is_training=False)
    torch.cuda.synchronize()
    assert tuple(det.shape) == (B, D, 6)
    pred = O.interpret_output([t.cpu() for t in preds])
    want = O.filter_detections(pred[2], pred[3], pred[5], np.asarray(b["clip_window"]), 0.02, max_detection=D)
    assert ((np.abs(want[..., :4]).sum(-1) > 0).sum(1) > 10).all()
    np.testing.assert_allclose(det.cpu().numpy(), want, rtol=1e-5, atol=1e-6)


# ------------------------------------------------------------------------------------------------ 2. shuffle_perm
def run_shuffle(dev, nd, ng, B, seed, step):
    pd = torch.full((B, nd), -1, dtype=torch.int32, device=dev)
    pg = torch.full((B, ng), -1, dtype=torch.int32, device=dev)
    st = torch.tensor([step], dtype=torch.int64, device=dev)
    L.shuffle_perm(pd, pg, B, seed, st)
    torch.cuda.synchronize()
    return pd.cpu().numpy(), pg.cpu().numpy()


@pytest.mark.parametrize("nd,ng", [(30, 20), (64, 64), (256, 100), (65, 20), (30, 256)])
def test_shuffle_perm_up_to_256(dev, nd, ng):
    B, seed = 3, 20190530
    pd, pg = run_shuffle(dev, nd, ng, B, seed, 7)
    for p, n in ((pd, nd), (pg, ng)):
        assert all(sorted(r.tolist()) == list(range(n)) for r in p), "every row is a permutation"
        assert not np.array_equal(p[0], p[1]), "rows differ between images"
    # the keys and the rank rule, restated: the same permutation whichever block size ranked it (at 30 / 20 and 64 / 64 this
    # is the kernel from before)
    np.testing.assert_array_equal(pd, LR.shuffle_perm_want(nd, B, 0, seed, 7))
    np.testing.assert_array_equal(pg, LR.shuffle_perm_want(ng, B, 1, seed, 7))
    again = run_shuffle(dev, nd, ng, B, seed, 7)
    assert np.array_equal(pd, again[0]) and np.array_equal(pg, again[1]), "equal for the same (seed, step)"
    other = run_shuffle(dev, nd, ng, B, seed, 8)
    assert not np.array_equal(pd, other[0]) and not np.array_equal(pg, other[1]), "rows differ between steps"
    if nd > 64:     # the first 64 keys do not depend on n: an n <= 64 call ranks the same keys
        small = run_shuffle(dev, 64, 20, B, seed, 7)[0]
        for b in range(B):
            assert [v for v in pd[b].tolist() if v < 64] == small[b].tolist()


# ------------------------------------------------------------------------------------------------ 3. mask_rois
def run_rois(dev, det, tb, perms, Hm, Wm, k):
    B, D, G = det.shape[0], det.shape[1], tb.shape[4]
    rois = torch.full((B, L.ROI_MAX, L.roi_w(k)), -1, dtype=torch.int32, device=dev)
    cnt = torch.full((B,), -1, dtype=torch.int32, device=dev)
    pd = torch.as_tensor(np.stack([p[0] for p in perms]), device=dev).int().contiguous()
    pg = torch.as_tensor(np.stack([p[1] for p in perms]), device=dev).int().contiguous()
    L.mask_rois(torch.as_tensor(det, device=dev), D, torch.as_tensor(tb.reshape(B, G, 5), device=dev), G, pd, pg, B, (Hm, Wm),
                cfg.MASK_ROI_DET, cfg.MASK_ROI_GT, cfg.MASK_ROI_IOU, rois, cnt, k=k)
    torch.cuda.synchronize()
    return rois.cpu().numpy(), cnt.cpu().numpy()


@pytest.mark.parametrize("k", [3, 7])
@pytest.mark.parametrize("D,G", LR.ROI_CASES)
def test_mask_rois_up_to_256_rows(dev, D, G, k):
    det, tb, perms = LR.roi_case(D, G)
    Hm, Wm = LR.ROI_MAP
    want, _ = LR.roi_rows(det, tb, perms, Hm, Wm, k)
    rois, cnt = run_rois(dev, det, tb, perms, Hm, Wm, k)
    assert list(cnt) == [len(w) for w in want] and min(cnt) >= 6
    for b in range(det.shape[0]):
        np.testing.assert_array_equal(rois[b, :cnt[b]], np.array(want[b], np.int32).reshape(cnt[b], L.roi_w(k)))
        assert (rois[b, cnt[b]:] == 0).all()
        assert (rois[b, :cnt[b], 2 * k + 2] >= 64).any()


def test_mask_rois_wide_form_equals_the_narrow_one_on_padded_tables(dev):
    """the 20 / 30-row case of the narrow kernel, zero-padded to 100 / 65 rows (the wave form): the same RoI rows, the
    permutations' extra entries pointing past the trimmed lists"""
    rng = np.random.RandomState(5)
    B, G, D = 3, 20, 30
    b = O.synthetic_batch(B, 64, seed=17)
    tb = b["true_boxes"].numpy()
    det = np.zeros((B, D, 6), np.float32)
    for i in range(B):
        rows = [r for r in range(G) if np.abs(tb[i, 0, 0, 0, r, :4]).sum() > 0]
        for q in range(12):
            xc, yc, w, h = tb[i, 0, 0, 0, rows[q % len(rows)], :4]
            j = (rng.rand(4) - 0.5) * 0.08
            det[i, 2 * q] = [yc - h / 2 + j[0], xc - w / 2 + j[1], yc + h / 2 + j[2], xc + w / 2 + j[3], q % 3, 0.9 - 0.01 * q]
    perms = [(rng.permutation(D).astype(np.int32), rng.permutation(G).astype(np.int32)) for _ in range(B)]
    narrow, ncnt = run_rois(dev, det, tb, perms, 32, 32, 3)
    det2 = np.zeros((B, 100, 6), np.float32)
    det2[:, :D] = det
    tb2 = np.zeros((B, 1, 1, 1, 65, 5), np.float32)
    tb2[:, :, :, :, :G] = tb
    perms2 = [(np.concatenate([p[0], np.arange(D, 100)]).astype(np.int32), np.concatenate([p[1], np.arange(G, 65)]).astype(np.int32))
              for p in perms]
    wide, wcnt = run_rois(dev, det2, tb2, perms2, 32, 32, 3)
    assert ncnt.sum() >= 6 and np.array_equal(ncnt, wcnt)
    np.testing.assert_array_equal(narrow, wide)


# ------------------------------------------------------------------------------------------------ 4. the YOLO loss
def run_loss(dev, heads, labels, tb, S, Cn, ld):
    B, G = tb.shape[0], tb.shape[1]
    lg = [torch.from_numpy(h).to(dev).contiguous() for h in heads]
    lb = [torch.from_numpy(l).to(dev).contiguous() for l in labels]
    dl = [torch.full((B, h.shape[1], h.shape[2], ld or L.GRAD_LD), float("nan"), dtype=torch.bfloat16, device=dev) for h in heads]
    losses = torch.full((8,), float("nan"), device=dev)
    scales = (O.OBJECT_SCALE, O.NOOBJECT_SCALE, O.CLASS_SCALE, O.COORD_SCALE)
    tbd = torch.from_numpy(tb).to(dev).contiguous()
    if ld:
        L.yolo_loss_wide(lg, lb, tbd, G, B, S, Cn, ld, ANCH.reshape(-1), cfg.IGNORE_THRESH, scales, dl, losses, L.Workspace(dev))
    else:
        L.yolo_loss(lg, lb, tbd, G, B, S, Cn, ANCH.reshape(-1), cfg.IGNORE_THRESH, scales, dl, losses, L.Workspace(dev))
    torch.cuda.synchronize()
    return losses.cpu(), [d.cpu() for d in dl]


@pytest.mark.parametrize("G", LR.LOSS_G)
@pytest.mark.parametrize("Cn,ld", [(3, 0), (80, 256)])
def test_yolo_loss_with_up_to_256_boxes(dev, Cn, ld, G):
    """B = 2, 64^2; the boxes that push a cell over IGNORE_THRESH sit in rows >= 64.  Bounds: tests/test_gpu_loss.py's (loss
    terms rtol 2e-5, gradients 2^-8 |want| + 1e-6 max|want|), unchanged."""
    heads, labels, tb = LR.loss_case(Cn, G)
    losses, dl = run_loss(dev, heads, labels, tb, LR.LOSS_S, Cn, ld)
    want = check_yolo_outputs(losses, dl, heads, labels, tb, "C=%d G=%d" % (Cn, G))
    cut = tb.copy()
    cut[:, 64:] = 0
    short = LR.loss_terms(heads, labels, cut)
    assert abs(want[1] - short[1]) > 1e-3 * want[1], "rows >= 64 must decide the noobj term"
    assert abs(float(losses[1]) - short[1]) > 0.5 * abs(want[1] - short[1]), "the kernel saw the rows past 64"
    losses2, dl2 = run_loss(dev, heads, labels, tb, LR.LOSS_S, Cn, ld)
    assert torch.equal(bits(losses), bits(losses2))
    for d, d2 in zip(dl, dl2):
        assert torch.equal(bits(d), bits(d2))
    # the same boxes in a 64-row table (the instance of before): rows of zeros add nothing, bit for bit
    if G == 65:
        tb64 = np.zeros((tb.shape[0], 64, 5), np.float32)
        tb64[:, 63] = tb[:, 64]
        l64, d64 = run_loss(dev, heads, labels, tb64, LR.LOSS_S, Cn, ld)
        assert torch.equal(bits(losses), bits(l64)) and all(torch.equal(bits(a), bits(b)) for a, b in zip(dl, d64))


# ------------------------------------------------------------------------------------------------ 5. the batched paste
def test_paste_and_iou_with_up_to_256_detections(dev):
    """jobs of 100 and 256 detections (37 x 53 and 130 x 257: more than one block's chunk), 5 and 33 ground-truth instances,
    against the per-image paste with full masks and integer sums, as tests/test_gpu_eval_batch.py does at n <= 64"""
    size = 32
    shapes, ndet, ngt = [(37, 53), (130, 257), (40, 41)], [100, 256, 64], [5, 33, 2]
    jobs = np.zeros(3, L.PASTE_JOB)
    keep, want_counts, want_merged, merged_bufs, counts_bufs = [], [], [], [], []
    want_conf = torch.zeros(16, dtype=torch.int64, device=dev)
    conf_buf = guarded(128, dev)
    for b, ((h, w), n, ng) in enumerate(zip(shapes, ndet, ngt)):
        m, r, cls, gt, gt_cls, tm = LR.paste_case(max(n, 72), h, w, ng, size, seed=n)
        m, r, cls = m[:n], r[:n], cls[:n]
        masks_d, rects_d, cls_d = torch.from_numpy(m).to(dev), torch.from_numpy(r).to(dev), torch.from_numpy(cls).to(dev)
        gt_d, gt_cls_d, tm_d = torch.from_numpy(gt).to(dev), torch.from_numpy(gt_cls).to(dev), torch.from_numpy(tm).to(dev)
        full = torch.empty(n, h, w, dtype=torch.uint8, device=dev)
        merged = torch.empty(h, w, dtype=torch.uint8, device=dev)
        L.mask_paste(masks_d.contiguous(), rects_d, cls_d, h, w, full, merged)
        want = torch.zeros(n, 1 + ng, dtype=torch.int64, device=dev)
        want[:, 0] = full.to(torch.int64).sum((1, 2))
        for g in range(ng):
            want[:, 1 + g] = (full & gt_d[g][None]).to(torch.int64).sum((1, 2)) * (cls_d == int(gt_cls[g]))
        L.confusion16(tm_d, merged, want_conf)
        if n > 70:
            # detections 3 and 70 overlap with different classes: 70 owns the overlap (and 64 over 63, the last over its twin)
            fm = full.cpu().numpy().astype(bool)
            mg = merged.cpu().numpy()
            both = fm[3] & fm[70] & ~fm[71:].any(axis=0)
            assert both.sum() > 20 and (mg[both] == cls[70] + 1).all() and cls[3] != cls[70]
            assert (fm[63] & fm[64]).sum() > 20 and (fm[n - 2] & fm[n - 1]).sum() > 20
            assert (mg[fm[n - 1]] == cls[n - 1] + 1).all()
        want_counts.append(want.to(torch.int32))
        want_merged.append(merged)
        mb, cb = guarded(h * w, dev), guarded(n * (1 + ng) * 4, dev)
        merged_bufs.append(mb)
        counts_bufs.append(cb)
        j = jobs[b]
        j["masks"], j["rects"], j["classids"] = masks_d.data_ptr(), rects_d.data_ptr(), cls_d.data_ptr()
        j["gt"], j["gt_class"] = gt_d.data_ptr(), gt_cls_d.data_ptr()
        j["merged"], j["counts"], j["true_map"] = mb.data_ptr(), cb.data_ptr(), tm_d.data_ptr()
        j["n"], j["ng"], j["image_h"], j["image_w"] = n, ng, h, w
        keep += [masks_d, rects_d, cls_d, gt_d, gt_cls_d, tm_d]
    with pytest.raises(L.DisyoloError, match="0..64"):
        L.paste_job_plan(jobs.copy())
    blocks = L.paste_job_plan(jobs, wide=True)
    assert blocks > 3 and jobs["block0"][0] == 0 and blocks - jobs["block0"][1] > 1
    assert all(int(c[:, 0].sum()) > 1000 and int(c[:, 1:].sum()) > 100 for c in want_counts), "vacuous fixture"
    jobs_d = torch.from_numpy(jobs.view(np.uint8).copy()).to(dev)
    runs = []
    for _ in range(2):
        conf_buf[:128] = 0
        for n, ng, cb in zip(ndet, ngt, counts_bufs):
            cb[:n * (1 + ng) * 4] = 0
        L.mask_paste_iou_batch(jobs, jobs_d, size, conf_buf[:128].view(torch.int64), wide=True)
        torch.cuda.synchronize()
        runs.append(([cb[:n * (1 + ng) * 4].view(torch.int32).reshape(n, 1 + ng).clone() for n, ng, cb in zip(ndet, ngt, counts_bufs)],
                     [mb[:h * w].reshape(h, w).clone() for (h, w), mb in zip(shapes, merged_bufs)],
                     conf_buf[:128].view(torch.int64).clone()))
    for got_counts, got_merged, got_conf in runs:
        for b in range(3):
            assert torch.equal(got_merged[b], want_merged[b]), "merged map of job %d" % b
            assert torch.equal(got_counts[b], want_counts[b]), "counts of job %d" % b
        assert torch.equal(got_conf, want_conf)
    for (h, w), n, ng, mb, cb in zip(shapes, ndet, ngt, merged_bufs, counts_bufs):
        assert guard_intact(mb, h * w) and guard_intact(cb, n * (1 + ng) * 4)
    assert guard_intact(conf_buf, 128)


def test_collect_batch_with_100_detections_gives_the_per_image_table(dev):
    """MAP.collect_batch at D = 100 against MAP.collect on the same detections and masks: the same entries, merged maps,
    confusion counts and AP table (voc_eval's)"""
    rng = np.random.RandomState(3)
    B, D, size = 2, 100, 32
    shapes = [(70, 120), (131, 57)]
    index = ["img0", "img1"]
    recs, sizes, merged = {}, {}, {}
    det = np.zeros((B, D, 6), np.float32)
    for b, (n, (h, w)) in enumerate(zip(index, shapes)):
        sizes[n] = [h, w]
        objs, mm = [], np.zeros((h, w), np.uint8)
        for j in range(6):
            y1, x1 = rng.randint(0, h - 20), rng.randint(0, w - 20)
            m = np.zeros((h, w), bool)
            m[y1:y1 + rng.randint(8, 20), x1:x1 + rng.randint(8, 20)] = True
            c = int(rng.randint(0, 3))
            objs.append({"imageid": n, "classid": c, "difficult": 0, "mask": m})
            mm[m] = c + 1
        recs[n], merged[n] = objs, mm
        for q in range(D - 4 * b):                         # image 1 ends with zero rows
            y1, x1 = rng.uniform(0.05, 0.7, size=2)
            det[b, q] = [y1, x1, y1 + rng.uniform(0.05, 0.25), x1 + rng.uniform(0.05, 0.25), rng.randint(0, 3), 1.0 - q / 128.0]
    dets = torch.from_numpy(det).to(dev)
    masks = torch.from_numpy(rng.rand(B, D, size, size).astype(np.float32)).to(dev)
    keep = torch.from_numpy((np.abs(det[..., :4]).sum(-1) > 0).astype(np.int32)).to(dev)
    keep[0, 5] = 0
    kp = keep.cpu().numpy().astype(bool)
    emap_b = E.MAP(recs, sizes, index, merged, net_size=64)
    file_b = {str(c): [] for c in emap_b.classid}
    seg_b = SegmentationAccuracy(dev)
    merged_b = emap_b.collect_batch(index, dets, keep, masks, file_b, true_maps=[merged[n] for n in index], conf=seg_b.conf)
    emap_a = E.MAP(recs, sizes, index, merged, net_size=64)
    file_a = {str(c): [] for c in emap_a.classid}
    seg_a = SegmentationAccuracy(dev)
    for b, n in enumerate(index):
        m = emap_a.collect(n, det[b][kp[b]], masks[b][torch.from_numpy(kp[b]).to(dev)], file_a)
        seg_a.add(merged[n], m)
        assert torch.equal(m, merged_b[b]), "merged map of %s" % n
    assert sum(len(v) for v in file_a.values()) >= 150
    assert any(e["ov"].size and np.nanmax(e["ov"]) > 0 for v in file_a.values() for e in v), "no detection meets a ground truth"
    same_detfiles(file_a, file_b)
    assert torch.equal(seg_a.conf, seg_b.conf)
    assert repr(emap_a._ap_table(file_a)) == repr(emap_b._ap_table(file_b))


# ------------------------------------------------------------------------------------------------ 6. whole nets
KW = dict(anchors=LR.NET_ANCH, max_box_per_image=LR.NET_G, max_detection=LR.NET_D)


def make_net(dev, training=True, seed=1, **kw):
    net = YOLONet(training=training, device=dev, image_size=LR.NET_S, batch_size=LR.NET_B, stage=1, seed=seed, **kw)
    perturb_variables(net, seed, "scale")
    net.refresh_weights()
    return net


def test_train_step_with_options_matches_the_composed_oracle(dev):
    """the recipe and the bounds of tests/test_gpu_lock_map.py::test_train_step_with_a_holed_map_matches_oracle, on a stage-1 net
    with G = 100, D = 100 and anchors x 0.11: the oracle's total loss composed from its parts with the same values"""
    net = make_net(dev, **KW)
    assert tuple(net.true_boxes.shape) == (2, 100, 5) and tuple(net.detections.shape) == (2, 100, 6)
    assert tuple(net.true_masks.shape) == (2, 100, 64, 64) and tuple(net.perm_det.shape) == (2, 100)
    net.fuse_first_two = net.fuse_blocks = False
    lock = O.default_lock(1)
    b, perms = LR.with_perms(LR.net_batch(11))
    p0 = oracle_params(net)
    net.set_batch(b)
    net.compute_losses(0.1)
    torch.cuda.synchronize()
    assert int(net.roi_count.sum()) > 0, "test needs at least one positive RoI"
    rois = net.rois.cpu().numpy()
    cnt = net.roi_count.cpu().numpy()
    assert max(int(rois[i, :cnt[i], 2 * net.k + 2].max()) for i in range(2) if cnt[i]) >= 64, "a ground-truth row >= 64 is assigned"
    want_names = O.trainable_names(lock)
    tr = {n: p0[n].clone().requires_grad_(True) for n in want_names}
    pp = dict(p0)
    pp.update(tr)
    upd, taps = {}, {}
    force = {"act%d" % l.idx: l.act.float().cpu() for l in net.layers}
    parts, _, _, _ = LR.total_loss(pp, b, lock, LR.NET_ANCH, LR.NET_D, perms, upd, obj_thresh=0.1, quant=O.bf16_ste, taps=taps,
                                   force=force)
    fails = []
    for l in net.layers:
        r, _, _ = rel_err(l.act, taps["act%d" % l.idx])
        if not r < 1.5e-2:
            fails.append("layer %d forward (teacher-forced inputs): rel l2 err %.3g" % (l.idx, r))
    parts["total"].backward()
    total = float(net.total_loss().cpu())
    print("total loss %.6f (oracle %.6f)" % (total, float(parts["total"].detach())))
    assert abs(total - float(parts["total"])) < 1e-3 * abs(float(parts["total"]))
    # ... and not with the configured anchors: the loss terms depend on them
    with torch.no_grad():
        other, _, _, _ = LR.total_loss(p0, b, lock, ANCH, LR.NET_D, perms, {}, obj_thresh=0.1, quant=O.bf16_ste, force=force)
    assert abs(float(other["total"]) - float(parts["total"])) > 1e-2 * abs(float(parts["total"]))
    net.backward()
    torch.cuda.synchronize()
    assert set(net.trainable_names()) == set(want_names)
    for nm, (o, n) in net.arena_slices.items():
        g = net.grad_arena[o:o + n].cpu()
        want_g = tr[nm].grad.flatten()
        if nm.endswith("weights") or nm.endswith("biases"):
            want_g = want_g - O.L2_WEIGHT * tr[nm].detach().flatten()
        r, amax, wmax = rel_err(g, want_g)
        if not (r < 0.03 or amax < 1e-3 * max(wmax, 1e-6)):
            fails.append("grad %s: rel l2 err %.3g (max abs %.3g of %.3g)" % (nm, r, amax, wmax))
    assert not fails, "%d checks failed:\n%s" % (len(fails), "\n".join(fails[:40]))


def test_two_steps_eager_recorded_and_pipelined_are_bit_identical(dev):
    batches = [LR.net_batch(500 + t) for t in range(3)]
    eager, rec, piped = (make_net(dev, seed=4, **KW) for _ in range(3))
    for n in (eager, rec, piped):
        n.shuffle_seed = 77                     # the device shuffle at 100 / 100 entries (the 256-thread block)
        n.set_batch(batches[0])
    rec.build_program(det_thresh=0.1)
    piped.build_program(det_thresh=0.1, pipeline_backbone=True)
    piped._set_inputs(batches[0]["images"], batches[0]["clip_window"])
    piped.prime_pipeline()
    le, lr, lp = [], [], []
    for t in range(2):
        le.append(float(eager.train_step(batches[t], det_thresh=0.1).cpu()))
        lr.append(float(rec.train_step(batches[t]).cpu()))
        mixed = dict(batches[t])
        mixed["images"] = batches[t + 1]["images"]            # labels of batch t, images of batch t + 1
        piped.set_batch(mixed)
        lp.append(float(piped.train_step(None).cpu()))
    torch.cuda.synchronize()
    assert np.isfinite(le).all()
    assert le == lr == lp
    _same_state(eager, rec)
    _same_state(rec, piped)
    assert sorted(eager.perm_det[0].cpu().tolist()) == list(range(100)) and torch.equal(eager.perm_det, rec.perm_det)


def test_inference_net_with_options_detects_and_assembles_like_the_oracle(dev):
    B, S, thr = LR.NET_B, LR.NET_S, 0.05
    net = make_net(dev, training=False, seed=3, **KW)
    b = LR.net_batch(5)
    b["clip_window"][1] = torch.tensor([0.1, 0.05, 0.9, 0.8])
    preds, det, mask_pos = net.forward(b["images"], b["clip_window"], [thr], is_training=False)
    torch.cuda.synchronize()
    assert tuple(det.shape) == (B, 100, 6)
    p = {k: v.detach().cpu() for k, v in net.params.items()}
    yq, mq = O.build_network(p, b["images"], False, O.default_lock(1), quant=O.bf16_ste)
    for got, want in list(zip(preds, yq)) + [(mask_pos, mq)]:
        err = float((got.cpu().double() - want.double()).norm() / want.double().norm())
        assert err < 2e-2, "forward differs from the oracle (rel l2 %.3g)" % err
    # detections and assembled masks: the oracle on the kernel's own logits, with the net's anchors and D
    ys = [t.cpu() for t in preds]
    pred = O.interpret_output(ys, anchors=LR.NET_ANCH)
    want_det = O.filter_detections(pred[2], pred[3], pred[5], b["clip_window"].numpy(), thr, max_detection=100)
    got = det.cpu().numpy()
    kept = (np.abs(want_det[..., :4]).sum(-1) > 0).sum(1)
    print("detections per image:", kept)
    assert (kept > 64).all(), "the case must yield more than 64 detections: %s" % kept
    np.testing.assert_allclose(got, want_det, rtol=1e-5, atol=1e-6)
    with_cfg = O.filter_detections(*[O.interpret_output(ys)[i] for i in (2, 3, 5)], b["clip_window"].numpy(), thr, max_detection=100)
    assert not np.allclose(with_cfg, want_det, atol=1e-3), "the anchors must matter"
    dets, keep, masks = net.evaluation_device(b["images"], b["clip_window"], [thr])
    torch.cuda.synchronize()
    assert tuple(masks.shape) == (B, 100, S // 2, S // 2) and tuple(keep.shape) == (B, 100)
    wb, wm = O.val_test(dets.cpu().numpy(), mask_pos.cpu())
    kp = keep.cpu().numpy().astype(bool)
    for i in range(B):
        assert kp[i].sum() == len(wb[i]) and kp[i].sum() > 30 and kp[i, 64:].any()
        np.testing.assert_allclose(masks[i].cpu().numpy()[kp[i]], wm[i], rtol=0, atol=1e-6)


def test_loader_with_options_places_30_instances_and_assigns_with_the_anchors(dev):
    S, B, G = 128, 2, 100
    classes = list(cfg.CLASSES)
    rng = np.random.RandomState(8)
    labels = [LR.rectangle_record(rng, 300, 260, 30, classes), LR.rectangle_record(rng, 240, 320, 30, classes)]
    data = TD.defect_train(labels, batch_size=B, image_size=S, device=dev, rng=np.random.RandomState(2), flipped=False,
                           blur_noise_light=False, anchors=LR.NET_ANCH, max_box_per_image=G)
    order = list(data.random_labels)
    images, masks, tboxes, y3, y2, y1, window = data.get()
    torch.cuda.synchronize()
    assert masks.shape == (B, G, S, S) and tboxes.shape == (B, 1, 1, 1, G, 5)
    differs = 0
    for b in range(B):
        lab, dec = order[b], data.last_decisions[b]
        assert (np.abs(tboxes[b, 0, 0, 0, :30, :4]).sum(axis=1) > 0).all() and not tboxes[b, 0, 0, 0, 30:].any(), "all 30 arrive"
        assert masks[b, :30].flatten(1).any(dim=1).all() and not masks[b, 30:].any()
        image_h, image_w, _, _, boxes, cls = data._record(lab)
        assert len(boxes) == 30 and tboxes[b, 0, 0, 0, :30, 4].tolist() == [float(c) for c in cls]
        # the boxes in the net frame, as the loader transforms them (utils/train_data.py:136-147)
        sx, sy = float(dec["new_w"]) / image_w, float(dec["new_h"]) / image_h
        bx = np.zeros((30, 4), np.float32)
        for j, (x1, y1_, x2, y2_) in enumerate(boxes):
            x1 = max(min(float(x1) * sx + dec["dx"], S - 1), 0)
            y1_ = max(min(float(y1_) * sy + dec["dy"], S - 1), 0)
            x2 = max(min(float(x2) * sx + dec["dx"], S - 1), 0)
            y2_ = max(min(float(y2_) * sy + dec["dy"], S - 1), 0)
            bx[j] = [(x2 + x1) / 2.0, (y2_ + y1_) / 2.0, x2 - x1, y2_ - y1_]
        np.testing.assert_array_equal(tboxes[b, 0, 0, 0, :30, :4], bx / np.float32(S))
        want = O.assign_targets(bx, np.asarray(cls), S, anchors=LR.NET_ANCH, num_class=3)
        other = O.assign_targets(bx, np.asarray(cls), S, num_class=3)
        for got, w, o in zip((y3, y2, y1), want, other):
            w[..., 0:4] /= np.float32(S)
            np.testing.assert_array_equal(got[b], w)
            differs += int(not np.array_equal(w[..., 4], o[..., 4]))
    assert differs, "the anchors must decide where a target lands"


# ------------------------------------------------------------------------------------------------ 7. the defaults
def _counts(prog):
    return {"%s/%d" % (what, lane): prog.count(what, lane) for what in ("launches", "records", "waits") for lane in range(4)}


def test_defaults_given_explicitly_record_the_same_step(dev):
    B, S = 2, 64
    b = O.synthetic_batch(B, S, seed=3)
    nets, counts = [], []
    for kw in ({}, dict(anchors=cfg.ANCHORS, max_box_per_image=20, max_detection=30)):
        net = YOLONet(training=True, device=dev, image_size=S, batch_size=B, stage=1, seed=2, **kw)
        net.shuffle_seed = 5
        net.set_batch(b)
        net.build_program(det_thresh=0.1, overlap_tail=True)
        counts.append(_counts(net._prog))
        nets.append(net)
    assert counts[0] == counts[1] and nets[0]._prog.size() == nets[1]._prog.size()
    for _ in range(2):
        for net in nets:
            net.train_step(None, want_loss=False)
    la, lb = float(nets[0].total_loss().cpu()), float(nets[1].total_loss().cpu())
    torch.cuda.synchronize()
    assert la == lb or (np.isnan(la) and np.isnan(lb))
    assert torch.equal(nets[0].arena, nets[1].arena) and torch.equal(nets[0].adam_v, nets[1].adam_v)
    assert torch.equal(nets[0].adam_m, nets[1].adam_m) and torch.equal(nets[0].detections, nets[1].detections)
    # a net with larger limits records the same number of commands (the wide forms are one launch each, too)
    big = YOLONet(training=True, device=dev, image_size=S, batch_size=B, stage=1, seed=2, max_box_per_image=100, max_detection=100)
    big.shuffle_seed = 5
    big.set_batch(LR.net_batch(3, anchors=ANCH))
    big.build_program(det_thresh=0.1, overlap_tail=True)
    assert _counts(big._prog) == counts[0]

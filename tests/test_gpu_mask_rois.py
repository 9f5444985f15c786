"""The mask loss on more than 16 RoIs per image (``mask_roi_det`` / ``mask_roi_gt`` / ``mask_roi_iou``; disyolo_mask_rois_x,
disyolo_psroi_loss_x) on the GPU: the selection against the old entry point and against the reference of
tests/mask_roi_ref.py (exact), the loss against the float64 reference with the bounds of tests/test_gpu_loss.py and against the
narrow kernel (bit for bit), and whole nets at 64^2.  tests/test_mask_rois.py holds every case to its condition without a GPU."""
import numpy as np
import pytest
import torch

import disyolo_oracle as O
import limits_ref as LR
import mask_roi_ref as MR
from disyolo_amd import config as cfg
from disyolo_amd import lib as L
from disyolo_amd.net import YOLONet
from net_setup import perturb_variables
from test_gpu_lock_map import _same_state, oracle_params, rel_err
from test_gpu_loss import assert_grad_close, bits

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ 1. the selection
def run_rois(dev, det, tb, perms, Hm, Wm, k, n_det, n_gt, thr=0.5, cap=None):
    """cap=None: the old entry point on its table of 16 rows"""
    B, D, G = det.shape[0], det.shape[1], tb.shape[1]
    rois = torch.full((B, L.ROI_MAX if cap is None else cap, L.roi_w(k)), -1, dtype=torch.int32, device=dev)
    cnt = torch.full((B,), -1, dtype=torch.int32, device=dev)
    pd = torch.as_tensor(np.stack([p[0] for p in perms]), device=dev).int().contiguous()
    pg = torch.as_tensor(np.stack([p[1] for p in perms]), device=dev).int().contiguous()
    (L.mask_rois if cap is None else L.mask_rois_x)(torch.as_tensor(det, device=dev), D, torch.as_tensor(tb, device=dev), G, pd, pg,
                                                    B, (Hm, Wm), n_det, n_gt, thr, rois, cnt, k=k)
    torch.cuda.synchronize()
    return rois.cpu().numpy(), cnt.cpu().numpy()


@pytest.mark.parametrize("k", [3, 7])
@pytest.mark.parametrize("D,G", MR.OLD_SIZES)
@pytest.mark.parametrize("n_det,n_gt", MR.OLD_CASES)
def test_selection_x_equals_the_old_entry_point(dev, n_det, n_gt, D, G, k):
    """(D, G) = (30, 20) is the single-lane kernel's range, (100, 65) the wave kernel's"""
    det, tb, perms = MR.sel_case(D, G)
    Hm, Wm = MR.SEL_MAP
    old, ocnt = run_rois(dev, det, tb, perms, Hm, Wm, k, n_det, n_gt)
    new, ncnt = run_rois(dev, det, tb, perms, Hm, Wm, k, n_det, n_gt, cap=16)
    assert ocnt.sum() > 0 and np.array_equal(ocnt, ncnt)
    np.testing.assert_array_equal(old, new)


@pytest.mark.parametrize("k", [3, 7])
@pytest.mark.parametrize("n_det,n_gt,D,G", MR.SEL_CASES)
def test_selection_x_equals_the_reference(dev, n_det, n_gt, D, G, k):
    det, tb, perms = MR.sel_case(D, G)
    Hm, Wm = MR.SEL_MAP
    want, _ = MR.rows(det, tb, perms, Hm, Wm, k, n_det, n_gt, 0.5)
    for cap in sorted({n_det + n_gt, MR.ROI_CAP}):
        rois, cnt = run_rois(dev, det, tb, perms, Hm, Wm, k, n_det, n_gt, cap=cap)
        assert list(cnt) == [len(w) for w in want], (cap, list(cnt))
        for b in range(det.shape[0]):
            np.testing.assert_array_equal(rois[b, :cnt[b]], np.array(want[b], np.int32).reshape(cnt[b], L.roi_w(k)))
            assert (rois[b, cnt[b]:] == 0).all()


def test_selection_x_threshold_is_an_argument(dev):
    """IoU 225/287 = 0.784: positive at 0.78, negative at 0.79; a box is positive by itself up to 1.0"""
    det, tb, perms = MR.sel_case(30, 20)
    Hm, Wm = MR.SEL_MAP
    for thr in (0.1, 0.79, 1.0):
        want, _ = MR.rows(det, tb, perms, Hm, Wm, 3, 30, 20, thr)
        rois, cnt = run_rois(dev, det, tb, perms, Hm, Wm, 3, 30, 20, thr=thr, cap=50)
        assert list(cnt) == [len(w) for w in want]
        for b in range(3):
            np.testing.assert_array_equal(rois[b, :cnt[b]], np.array(want[b], np.int32).reshape(cnt[b], 12))
    assert cnt[0] == 10 and cnt[1] == 10 and cnt[2] == 0            # at 1.0 the ten boxes alone


# ------------------------------------------------------------------------------------------------ 2. the loss
def run_loss(dev, table, cnt, score, tm, st, k, wide=True, fill=float("nan")):
    B, Hm, Wm = score.shape[0], score.shape[1], score.shape[2]
    ld = (k * k + 31) // 32 * 32
    dscore = torch.full((B, Hm, Wm, ld), fill, dtype=torch.bfloat16, device=dev)
    loss = torch.full((1,), fill, device=dev)
    ws = L.Workspace(dev)
    ws.buf.fill_(0xff)
    (L.psroi_loss_x if wide else L.psroi_loss)(score.to(dev), tm.to(dev), tm.shape[1], torch.as_tensor(table, device=dev).contiguous(),
                                               torch.as_tensor(cnt, device=dev), B, (Hm, Wm), k, cfg.MASK_SCALE, dscore, loss, ws,
                                               mask_stride=st)
    torch.cuda.synchronize()
    return float(loss.cpu()[0]), dscore.cpu()


_WANT = {}


def want_of(nrow, Hm, Wm, k, st):
    key = (nrow, Hm, Wm, k, st)
    if key not in _WANT:
        table, cnt = MR.loss_table(nrow, Hm, Wm, k)
        score, tm = MR.loss_inputs(Hm, Wm, k, st)
        _WANT[key] = (table, cnt, score, tm) + MR.loss_want(table, cnt, score, tm, st, k)
    return _WANT[key]


def check_loss(dev, nrow, Hm, Wm, k, st):
    table, cnt, score, tm, want, grad = want_of(nrow, Hm, Wm, k, st)
    loss, dscore = run_loss(dev, table, cnt, score, tm, st, k)
    what = "%d rows, map %d x %d, k = %d, stride %d" % (nrow, Hm, Wm, k, st)
    print("%s: loss %.9g, reference %.9g" % (what, loss, want))
    assert np.isfinite(loss) and np.isfinite(want) and want > 0
    np.testing.assert_allclose(loss, want, rtol=2e-5, err_msg=what + ": mask loss")
    assert not torch.isnan(dscore).any(), what + ": dscore not fully written"
    assert float(dscore[..., k * k:].abs().max()) == 0.0, what + ": pad channels"
    assert_grad_close(dscore[..., :k * k], grad, what + ": dscore")
    cover = MR.cover_of(table, cnt, Hm, Wm, k)
    assert float(dscore[torch.from_numpy(cover == 0)].abs().max()) == 0.0, what + ": gradient where no RoI covers"
    assert float(dscore[2].abs().max()) == 0.0                      # the image without rows
    loss2, dscore2 = run_loss(dev, table, cnt, score, tm, st, k, fill=0.0)
    assert np.float32(loss).view(np.int32) == np.float32(loss2).view(np.int32), what + ": second launch"
    assert torch.equal(bits(dscore), bits(dscore2)), what + ": second launch"


@pytest.mark.parametrize("st", [1, 2, 4])
@pytest.mark.parametrize("k", [3, 5, 7])
@pytest.mark.parametrize("Hm,Wm", MR.LOSS_MAPS)
@pytest.mark.parametrize("nrow", MR.LOSS_ROWS)
def test_loss_x_matches_the_f64_reference(dev, nrow, Hm, Wm, k, st):
    check_loss(dev, nrow, Hm, Wm, k, st)


@pytest.mark.parametrize("k", [3, 7])
def test_loss_x_on_a_map_wider_than_a_block(dev, k):
    """8 x 300: blocks that lie within one row of the map and cull by columns too"""
    check_loss(dev, 64, 8, 300, k, 2)


@pytest.mark.parametrize("st", [1, 2])
@pytest.mark.parametrize("k", [3, 5, 7])
@pytest.mark.parametrize("Hm,Wm", MR.LOSS_MAPS)
def test_loss_x_equals_the_narrow_kernel_on_its_table(dev, Hm, Wm, k, st):
    """the first 16 rows of the 17-row table (sixteen concentric boxes: the centre pixel adds sixteen terms) copied into tables
    of 17 and 512 rows: dscore bit for bit"""
    table, cnt = MR.loss_table(17, Hm, Wm, k)
    score, tm = MR.loss_inputs(Hm, Wm, k, st)
    narrow = np.ascontiguousarray(table[:, :16])
    ncnt = np.minimum(cnt, 16).astype(np.int32)
    want_loss, want = run_loss(dev, narrow, ncnt, score, tm, st, k, wide=False)
    assert np.isfinite(want_loss) and float(want.abs().max()) > 0
    for cap in (17, 512):
        wide = np.zeros((table.shape[0], cap, table.shape[2]), np.int32)
        wide[:, :16] = narrow
        loss, got = run_loss(dev, wide, ncnt, score, tm, st, k)
        assert torch.equal(bits(got), bits(want)), "cap %d" % cap
        np.testing.assert_allclose(loss, want_loss, rtol=2e-5)


def test_loss_x_special_rows(dev):
    """a zero-area positive row gives a NaN loss, as the narrow kernel does; images without positives give 0 and no gradient"""
    k, Hm, Wm, st = 3, 24, 40, 2
    score, tm = MR.loss_inputs(Hm, Wm, k, st, B=2)
    gone = MR.row_of(5, Wm + 2, 9, Wm + 6, 0, Hm, Wm, k)             # wholly right of the map: area 0
    rows = [[MR.row_of(2, 2, 9, 9, 1, Hm, Wm, k), gone], []]
    for cap, wide in ((16, False), (17, True), (512, True)):
        table, cnt = MR.table_of(rows, cap, k)
        loss, dscore = run_loss(dev, table, cnt, score, tm, st, k, wide=wide)
        assert np.isnan(loss), cap
        assert not torch.isnan(dscore).any() and float(dscore[1].abs().max()) == 0.0 and float(dscore[0].abs().max()) > 0
    table, cnt = MR.table_of([[], []], 40, k)
    table[:] = 7                                                      # rows behind the count are not read
    loss, dscore = run_loss(dev, table, cnt, score, tm, st, k)
    assert loss == 0.0 and float(dscore.abs().max()) == 0.0 and not torch.isnan(dscore).any()


# ------------------------------------------------------------------------------------------------ 3. whole nets
NET_KW = dict(anchors=LR.NET_ANCH, max_box_per_image=MR.NET_G, max_detection=MR.NET_D)
COUNTS = [(40, 40), (0, 40), (40, 0)]


def make_net(dev, seed=1, **kw):
    net = YOLONet(training=True, device=dev, image_size=MR.NET_S, batch_size=MR.NET_B, stage=1, seed=seed, **NET_KW, **kw)
    perturb_variables(net, seed, "scale")
    net.refresh_weights()
    return net


def net_batch(seed):
    return LR.net_batch(seed, B=MR.NET_B, S=MR.NET_S, G=MR.NET_G, rows=MR.NET_ROWS)


def planted(scratch, batch):
    """``MR.plant_detections`` with the detections a net of the same variables yields on the batch's images"""
    scratch.set_batch(batch)
    scratch.compute_losses(0.1)
    torch.cuda.synchronize()
    out, rows = MR.plant_detections(batch, scratch.detections.cpu().numpy(), LR.NET_ANCH)
    assert all(len(r) >= 1 for r in rows), "every image needs a detection of 8 pixels: %s" % rows
    return out, rows


def composed_loss(params, batch, lock, n_det, n_gt, thr, perms, updates, taps=None, force=None):
    """``limits_ref.total_loss`` with the mask loss of tests/mask_roi_ref.py"""
    yolos, mask_pos = O.build_network(params, batch["images"], True, lock, updates, taps, O.bf16_ste, force)
    pred = O.interpret_output(yolos, anchors=LR.NET_ANCH)
    with torch.no_grad():
        det = O.filter_detections(pred[2], pred[3], pred[5], batch["clip_window"], 0.1, max_detection=MR.NET_D)
    ly = O.loss_yolo(pred, batch["true_boxes"], [batch["yolo3"], batch["yolo2"], batch["yolo1"]])
    lm = MR.loss_mask(det, mask_pos, batch["true_boxes"].numpy()[:, 0, 0, 0], batch["true_masks"], n_det, n_gt, thr, perms)
    return ly["conf"] + ly["class"] + ly["coord"] + lm + O.l2_regularization(params, lock), lm, det


@pytest.mark.parametrize("n_det,n_gt", COUNTS)
def test_train_step_matches_the_composed_oracle(dev, n_det, n_gt):
    """the recipe and the bounds of tests/test_gpu_lock_map.py::test_train_step_with_a_holed_map_matches_oracle on a stage-1 net
    with G = D = 40, anchors x 0.11 and the two counts"""
    net = make_net(dev, mask_roi_det=n_det, mask_roi_gt=n_gt)
    assert tuple(net.rois.shape) == (2, n_det + n_gt, 12)
    net.fuse_first_two = net.fuse_blocks = False
    lock = O.default_lock(1)
    b, rows = planted(net, net_batch(11))            # (a first pass of the same net, with the same kernels: the same detections)
    b, perms = LR.with_perms(b, D=MR.NET_D)
    p0 = oracle_params(net)
    net.set_batch(b)
    net.compute_losses(0.1)
    torch.cuda.synchronize()
    cnt = net.roi_count.cpu().numpy()
    ndet = (net.detections[..., :4].abs().sum(-1) != 0).sum(1).cpu().numpy()
    print("positives per image %s, detections per image %s" % (cnt, ndet))
    want_cnt = [(20 if n_gt else 0) + (len(r) if n_det else 0) for r in rows]
    assert (cnt >= want_cnt).all(), "the twenty boxes and the planted detections are positive by themselves: %s" % want_cnt
    assert n_det + n_gt < 80 or (cnt > 20).all()
    want_names = O.trainable_names(lock)
    tr = {n: p0[n].clone().requires_grad_(True) for n in want_names}
    pp = dict(p0)
    pp.update(tr)
    taps = {}
    force = {"act%d" % l.idx: l.act.float().cpu() for l in net.layers}
    total, lm, det = composed_loss(pp, b, lock, n_det, n_gt, 0.5, perms, {}, taps, force)
    fails = []
    for l in net.layers:
        r, _, _ = rel_err(l.act, taps["act%d" % l.idx])
        if not r < 1.5e-2:
            fails.append("layer %d forward (teacher-forced inputs): rel l2 err %.3g" % (l.idx, r))
    total.backward()
    got = float(net.total_loss().cpu())
    print("total loss %.6f (oracle %.6f), mask loss %.6f (oracle %.6f)" % (got, float(total.detach()), float(net.mask_loss.cpu()[0]),
                                                                           float(lm.detach())))
    assert abs(got - float(total.detach())) < 1e-3 * abs(float(total.detach()))
    # ... and not with the counts of the reference: the mask loss depends on them
    with torch.no_grad():
        _, other, _ = composed_loss(p0, b, lock, 7, 3, 0.5, perms, {}, None, force)
    assert abs(float(other) - float(lm.detach())) > 1e-4 * abs(float(lm.detach()))
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


@pytest.mark.parametrize("shuffle", ["injected", "device"])
@pytest.mark.parametrize("n_det,n_gt", COUNTS)
def test_two_steps_eager_recorded_overlapped_and_pipelined_are_bit_identical(dev, n_det, n_gt, shuffle):
    scratch = make_net(dev, seed=4)
    batches = [planted(scratch, net_batch(500 + t))[0] for t in range(3)]
    if shuffle == "injected":
        batches = [LR.with_perms(b, D=MR.NET_D, seed=t)[0] for t, b in enumerate(batches)]
    eager, rec, over, piped = (make_net(dev, seed=4, mask_roi_det=n_det, mask_roi_gt=n_gt) for _ in range(4))
    for n in (eager, rec, over, piped):
        if shuffle == "device":
            n.shuffle_seed = 77
        n.set_batch(batches[0])
    rec.build_program(det_thresh=0.1)
    over.build_program(det_thresh=0.1, overlap_tail=True)
    piped.build_program(det_thresh=0.1, pipeline_backbone=True)
    piped._set_inputs(batches[0]["images"], batches[0]["clip_window"])
    piped.prime_pipeline()
    le, lr, lo, lp = [], [], [], []
    first = None
    for t in range(2):
        le.append(float(eager.train_step(batches[t], det_thresh=0.1).cpu()))
        first = eager.roi_count.cpu().tolist() if first is None else first
        lr.append(float(rec.train_step(batches[t]).cpu()))
        lo.append(float(over.train_step(batches[t]).cpu()))
        mixed = dict(batches[t])
        mixed["images"] = batches[t + 1]["images"]            # labels of batch t, images of batch t + 1
        piped.set_batch(mixed)
        lp.append(float(piped.train_step(None).cpu()))
    torch.cuda.synchronize()
    assert np.isfinite(le).all()
    assert le == lr == lo == lp
    _same_state(eager, rec)
    _same_state(rec, over)
    _same_state(over, piped)
    assert torch.equal(eager.rois, rec.rois) and torch.equal(eager.roi_count, rec.roi_count)
    print("positives per image: first step %s, second step %s" % (first, eager.roi_count.cpu().tolist()))
    assert min(first) >= (21 if n_det and n_gt else 20 if n_gt else 1)


# ------------------------------------------------------------------------------------------------ 4. the defaults
def _counts(prog):
    return {"%s/%d" % (what, lane): prog.count(what, lane) for what in ("launches", "records", "waits") for lane in range(4)}


def test_defaults_given_explicitly_record_the_same_step(dev):
    B, S = 2, 64
    b = O.synthetic_batch(B, S, seed=3)
    nets, counts = [], []
    for kw in ({}, dict(mask_roi_det=7, mask_roi_gt=3, mask_roi_iou=0.5), dict(mask_roi_det=10, mask_roi_gt=6)):
        net = YOLONet(training=True, device=dev, image_size=S, batch_size=B, stage=1, seed=2, **kw)
        assert tuple(net.rois.shape) == (B, L.ROI_MAX, L.ROI_W)
        net.shuffle_seed = 5
        net.set_batch(b)
        net.build_program(det_thresh=0.1, overlap_tail=True)
        counts.append(_counts(net._prog))
        nets.append(net)
    assert counts[0] == counts[1] == counts[2] and nets[0]._prog.size() == nets[1]._prog.size() == nets[2]._prog.size()
    for _ in range(2):
        for net in nets[:2]:
            net.train_step(None, want_loss=False)
    la, lb = float(nets[0].total_loss().cpu()), float(nets[1].total_loss().cpu())
    torch.cuda.synchronize()
    assert la == lb or (np.isnan(la) and np.isnan(lb))
    assert torch.equal(nets[0].arena, nets[1].arena) and torch.equal(nets[0].adam_v, nets[1].adam_v)
    assert torch.equal(nets[0].adam_m, nets[1].adam_m) and torch.equal(nets[0].rois, nets[1].rois)
    # a net past 16 RoIs records the same number of commands: the _x forms are one and three launches, too
    big = YOLONet(training=True, device=dev, image_size=S, batch_size=B, stage=1, seed=2, mask_roi_det=30, mask_roi_gt=20)
    big.shuffle_seed = 5
    big.set_batch(b)
    big.build_program(det_thresh=0.1, overlap_tail=True)
    assert _counts(big._prog) == counts[0]

"""The batched test loop: ``disyolo_mask_paste_iou_batch`` against the launches it replaces, ``MAP.collect_batch`` against
``MAP.collect``, ``evaluate()`` at a batch size above 1 against the per-image loop, and ``Solver.validate`` through the batch
collector.  Every comparison is exact: both sides take the same rounded > 0.5 decisions and count integers."""
import numpy as np
import pytest
import torch

from disyolo_amd import evaluate as E
from disyolo_amd import lib as L
from disyolo_amd.net import YOLONet
from disyolo_amd.postprocess import SegmentationAccuracy
from disyolo_amd.solver import Solver
from disyolo_amd.synth import synthetic_batch

pytestmark = pytest.mark.gpu

GUARD = 256


def guarded(nbytes, dev):
    """a device buffer of nbytes + 256 guard bytes, all 0xAB"""
    return torch.full((nbytes + GUARD,), 0xAB, dtype=torch.uint8, device=dev)


def guard_intact(buf, nbytes):
    return bool((buf[nbytes:] == 0xAB).all())


def _rects(rng, n, h, w, size):
    """n rect rows (cy1,cx1,cy2,cx2, y1,x1,y2,x2) and class ids: the first five are the hand-made cases, the rest random
    crops and destinations (some of them empty by chance)"""
    r = np.zeros((n, 8), np.int32)
    cls = rng.randint(0, 3, size=n).astype(np.int32)
    for k in range(n):
        cy1, cx1 = rng.randint(0, size, size=2)
        cy2, cx2 = rng.randint(cy1, size + 1), rng.randint(cx1, size + 1)
        y1, x1 = rng.randint(0, h), rng.randint(0, w)
        y2, x2 = rng.randint(y1, h + 1), rng.randint(x1, w + 1)
        r[k] = [cy1, cx1, cy2, cx2, y1, x1, y2, x2]
    if n >= 5:
        r[0] = [7, 3, 7, 20, 0, 0, h, w]                     # empty crop
        r[1] = [2, 2, 30, 30, 0, w // 2, h, w // 2]          # empty destination
        r[2] = [0, 0, size, size, 0, 0, h, w]                # the whole mask over the whole image: all four borders
        r[3] = [11, 13, 12, 14, 0, 0, h, max(w // 2, 1)]     # 1-pixel crop
        r[4] = [5, 1, 29, 31, 0, 0, h, w]                    # over row 2 with another class: the last one wins in merged
        cls[2], cls[4] = 0, 2
    return r, cls


def test_batch_kernel_matches_the_launches_it_replaces(dev):
    rng = np.random.RandomState(11)
    size = 32
    shapes = [(37, 53), (96, 64), (1, 70), (130, 257)]
    ndet = [0, 30, 5, 64]
    ngt = [1, 0, 20, 33]
    with_true_map = [True, False, True, True]
    jobs = np.zeros(4, L.PASTE_JOB)
    keep, want_counts, want_merged = [], [], []
    want_conf = torch.zeros(16, dtype=torch.int64, device=dev)
    merged_bufs, counts_bufs = [], []
    conf_buf = guarded(128, dev)
    for b, ((h, w), n, ng) in enumerate(zip(shapes, ndet, ngt)):
        m = rng.rand(max(n, 1), size, size).astype(np.float32)
        flat = m.reshape(-1)
        at = rng.choice(flat.size, size=min(200, flat.size), replace=False)
        flat[at[::2]] = np.float32(0.5)
        flat[at[1::2]] = np.nextafter(np.float32(0.5), np.float32(1.0))
        m[:, 16:, :16] = np.float32(0.5)                    # (a flat region at exactly the threshold)
        r, cls = _rects(rng, n, h, w, size)
        gt = (rng.rand(ng, h, w) < 0.4).astype(np.uint8)
        gt_cls = rng.randint(0, 3, size=ng).astype(np.int32)
        tm = rng.randint(0, 6, size=(h, w)).astype(np.uint8)      # values 4 and 5 are ignored
        masks_d, rects_d, cls_d = torch.from_numpy(m).to(dev), torch.from_numpy(r).to(dev), torch.from_numpy(cls).to(dev)
        gt_d, gt_cls_d, tm_d = torch.from_numpy(gt).to(dev), torch.from_numpy(gt_cls).to(dev), torch.from_numpy(tm).to(dev)
        # ---- expected: the per-image paste with full masks, torch integer sums, the per-image confusion launch
        full = torch.empty(n, h, w, dtype=torch.uint8, device=dev)
        merged = torch.empty(h, w, dtype=torch.uint8, device=dev)
        L.mask_paste(masks_d[:n].contiguous(), rects_d, cls_d, h, w, full, merged)
        want = torch.zeros(n, 1 + ng, dtype=torch.int64, device=dev)
        if n:
            want[:, 0] = full.to(torch.int64).sum((1, 2))
            for g in range(ng):
                same = cls_d == int(gt_cls[g])
                want[:, 1 + g] = (full & gt_d[g][None]).to(torch.int64).sum((1, 2)) * same
        if with_true_map[b]:
            L.confusion16(tm_d, merged, want_conf)
        want_counts.append(want.to(torch.int32))
        want_merged.append(merged)
        # ---- the job
        mb, cb = guarded(h * w, dev), guarded(n * (1 + ng) * 4, dev)
        merged_bufs.append(mb)
        counts_bufs.append(cb)
        j = jobs[b]
        j["masks"], j["rects"], j["classids"] = (masks_d.data_ptr(), rects_d.data_ptr(), cls_d.data_ptr()) if n else (0, 0, 0)
        j["gt"], j["gt_class"] = (gt_d.data_ptr(), gt_cls_d.data_ptr()) if ng else (0, 0)
        j["merged"], j["counts"] = mb.data_ptr(), cb.data_ptr()
        j["true_map"] = tm_d.data_ptr() if with_true_map[b] else 0
        j["n"], j["ng"], j["image_h"], j["image_w"] = n, ng, h, w
        keep += [masks_d, rects_d, cls_d, gt_d, gt_cls_d, tm_d]
    blocks = L.paste_job_plan(jobs)
    assert blocks > 4 and list(jobs["block0"]) == sorted(jobs["block0"]) and jobs["block0"][0] == 0
    assert blocks - jobs["block0"][3] > 1, "the last image must span more than one block"
    assert sum(int(c[:, 0].sum()) for c in want_counts) > 1000 and int(want_counts[3][:, 1:].sum()) > 1000, "vacuous fixture"
    assert (want_merged[3] == 3).any() and (want_merged[3] == 1).any()
    jobs_d = torch.from_numpy(jobs.view(np.uint8).copy()).to(dev)
    runs = []
    for _ in range(2):
        conf_buf[:128] = 0
        for (h, w), n, ng, cb in zip(shapes, ndet, ngt, counts_bufs):
            cb[:n * (1 + ng) * 4] = 0
        L.mask_paste_iou_batch(jobs, jobs_d, size, conf_buf[:128].view(torch.int64))
        torch.cuda.synchronize()
        got_counts = [cb[:n * (1 + ng) * 4].view(torch.int32).reshape(n, 1 + ng).clone()
                      for n, ng, cb in zip(ndet, ngt, counts_bufs)]
        got_merged = [mb[:h * w].reshape(h, w).clone() for (h, w), mb in zip(shapes, merged_bufs)]
        runs.append((got_counts, got_merged, conf_buf[:128].view(torch.int64).clone()))
    for got_counts, got_merged, got_conf in runs:
        for b in range(4):
            assert torch.equal(got_merged[b], want_merged[b]), "merged map of job %d" % b
            assert torch.equal(got_counts[b], want_counts[b]), "counts of job %d" % b
        assert torch.equal(got_conf, want_conf)
    for b in range(4):
        assert torch.equal(runs[0][0][b], runs[1][0][b]) and torch.equal(runs[0][1][b], runs[1][1][b])
    assert torch.equal(runs[0][2], runs[1][2])
    for (h, w), n, ng, mb, cb in zip(shapes, ndet, ngt, merged_bufs, counts_bufs):
        assert guard_intact(mb, h * w) and guard_intact(cb, n * (1 + ng) * 4)
    assert guard_intact(conf_buf, 128)


def randomize_heads(net, seed, gain=6.0, bias_std=0.5):
    """detection and mask heads with enough spread that every image keeps detections of several classes at a low threshold
    (the initial heads give near-zero logits: one class, tied scores)"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for i in (59, 67, 75, net.score_layer):
            net.params["yolo/convolutional%d/weights" % i].mul_(gain)
            b = net.params["yolo/convolutional%d/biases" % i]
            b.copy_((torch.randn(b.shape, generator=g) * bias_std).to(b.device))
    net.refresh_weights()


def synth_ground_truth(shapes, seed):
    """images of the given sizes with the instances of ``synth.synthetic_batch`` cut to each size: (images, MAP arguments)"""
    rng = np.random.RandomState(seed)
    images, recs, sizes, merged, index = {}, {}, {}, {}, []
    for k, (h, w) in enumerate(shapes):
        name = "img%03d" % k
        index.append(name)
        images[name] = rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
        sizes[name] = [h, w]
        batch = synthetic_batch(1, (max(h, w) + 31) // 32 * 32, seed=seed + k)      # (the target grids need a multiple of 32)
        objs, mm = [], np.zeros((h, w), np.uint8)
        for j in range(batch["true_masks"].shape[1]):
            m = batch["true_masks"][0, j][:h, :w]
            if m.any():
                c = int(batch["true_boxes"][0, 0, 0, 0, j, 4])
                objs.append({"imageid": name, "classid": c, "difficult": 0, "mask": m.copy()})
                mm[m] = c + 1
        recs[name], merged[name] = objs, mm
    return images, recs, sizes, merged, index


def same_detfiles(a, b):
    assert sorted(a) == sorted(b)
    for c in a:
        assert len(a[c]) == len(b[c]), "class %s: %d vs %d entries" % (c, len(a[c]), len(b[c]))
        for x, y in zip(a[c], b[c]):
            assert x["imageid"] == y["imageid"] and x["score"] == y["score"]
            assert x["ov"].dtype == y["ov"].dtype == np.float32 and x["ov"].tobytes() == y["ov"].tobytes()


def test_collect_batch_appends_what_collect_appends(dev):
    S, B = 96, 3
    net = YOLONet(training=False, device=dev, image_size=S, batch_size=B, stage=1, seed=0)
    randomize_heads(net, 5)
    images, recs, sizes, merged, index = synth_ground_truth([(70, 120), (96, 96), (131, 57)], 21)
    assert all(len(recs[n]) >= 1 for n in index)
    frame = torch.empty(B, S, S, 3, dtype=torch.float32, device=dev)
    windows = np.stack([E.image_read(images[n], S, dev, out=frame[i])[1] for i, n in enumerate(index)])
    dets, keep, masks = net.evaluation_device(frame, windows, [np.float32(0.05)])
    kp = keep.cpu().numpy().astype(bool)
    det = dets.cpu().numpy()
    print("kept rows per image:", kp.sum(1))
    assert (kp.sum(1) >= 10).all(), "every image must keep at least 10 detections: %s" % kp.sum(1)
    # the batch path
    emap_b = E.MAP(recs, sizes, index, merged, net_size=S)
    file_b = {str(c): [] for c in emap_b.classid}
    seg_b = SegmentationAccuracy(dev)
    merged_b = emap_b.collect_batch(index, dets, keep, masks, file_b, true_maps=[merged[n] for n in index], conf=seg_b.conf)
    # the per-image path on the SAME outputs
    emap_a = E.MAP(recs, sizes, index, merged, net_size=S)
    file_a = {str(c): [] for c in emap_a.classid}
    seg_a = SegmentationAccuracy(dev)
    for b, n in enumerate(index):
        m = emap_a.collect(n, det[b][kp[b]], masks[b][torch.from_numpy(kp[b]).to(dev)], file_a)
        seg_a.add(merged[n], m)
        assert torch.equal(m, merged_b[b]), "merged map of %s" % n
    assert sum(len(v) for v in file_a.values()) >= 30
    assert any(e["ov"].size and np.nanmax(e["ov"]) > 0 for v in file_a.values() for e in v), "no detection meets a ground truth"
    same_detfiles(file_a, file_b)
    assert torch.equal(seg_a.conf, seg_b.conf)


def test_collect_batch_falls_back_to_collect_with_the_switch_off(dev, monkeypatch):
    """DISYOLO_EVAL_GPU_IOU=0: per-image ``collect`` with host-side masks, the same order and merged maps"""
    S, B = 64, 2
    net = YOLONet(training=False, device=dev, image_size=S, batch_size=B, stage=1, seed=0)
    randomize_heads(net, 5)
    images, recs, sizes, merged, index = synth_ground_truth([(40, 64), (64, 50)], 4)
    frame = torch.empty(B, S, S, 3, dtype=torch.float32, device=dev)
    windows = np.stack([E.image_read(images[n], S, dev, out=frame[i])[1] for i, n in enumerate(index)])
    dets, keep, masks = net.evaluation_device(frame, windows, [np.float32(0.05)])
    emap = E.MAP(recs, sizes, index, merged, net_size=S)
    file_on, file_off = ({str(c): [] for c in emap.classid} for _ in range(2))
    merged_on = emap.collect_batch(index, dets, keep, masks, file_on)
    monkeypatch.setenv("DISYOLO_EVAL_GPU_IOU", "0")
    merged_off = emap.collect_batch(index, dets, keep, masks, file_off)
    assert sum(len(v) for v in file_on.values()) > 0
    for c in file_on:
        assert [(e["imageid"], e["score"]) for e in file_on[c]] == [(e["imageid"], e["score"]) for e in file_off[c]]
        assert all("mask" in e for e in file_off[c])
    for a, b in zip(merged_on, merged_off):
        assert torch.equal(a, b)


def test_evaluate_at_batch_3_matches_the_per_image_loop(dev):
    S, B, thr = 96, 3, 0.05
    net = YOLONet(training=False, device=dev, image_size=S, batch_size=B, stage=1, seed=0)
    randomize_heads(net, 7)
    shapes = [(70, 120), (96, 96), (131, 57), (64, 64), (50, 140), (111, 83), (90, 31)]
    images, recs, sizes, merged, index = synth_ground_truth(shapes, 33)
    thresh_out, mask_acc, timing = E.evaluate(net, images, E.MAP(recs, sizes, index, merged, net_size=S), det_thresh=thr)
    assert set(timing) == {"prediction_s", "crop_assemble_s", "per_image_s"} and timing["per_image_s"] > 0
    # the per-image loop over the same net: one pass per batch (a last batch of one image, the stale frames left in place)
    emap = E.MAP(recs, sizes, index, merged, net_size=S)
    detfile = {str(c): [] for c in emap.classid}
    seg = SegmentationAccuracy(dev)
    frame = torch.zeros(B, S, S, 3, dtype=torch.float32, device=dev)
    windows = np.tile(np.array([0.0, 0.0, 1.0, 1.0], np.float32), (B, 1))
    ndet = 0
    for a in range(0, len(index), B):
        ids = index[a:a + B]
        for i, n in enumerate(ids):
            _, windows[i] = E.image_read(images[n], S, dev, out=frame[i])
        det_box, det_mask = net.evaluation(frame, windows, [np.float32(thr)], masks_on_device=True)
        for i, n in enumerate(ids):
            if torch.is_tensor(det_mask[i]):
                m = emap.collect(n, det_box[i], det_mask[i], detfile)
                ndet += len(det_box[i])
            else:
                m = torch.zeros(*sizes[n], dtype=torch.uint8, device=dev)
            seg.add(merged[n], m)
    assert ndet >= 30, "fixture needs detections"
    want = emap._ap_table(detfile)
    assert repr(thresh_out) == repr(want)
    assert repr(mask_acc) == repr(seg.result())


class _TrainData:
    def __init__(self, B, S):
        self.batch_size, self.image_size, self.epoch = B, S, 1

    def get(self):
        b = synthetic_batch(self.batch_size, self.image_size, seed=500)
        return b["images"], b["true_masks"], b["true_boxes"], b["yolo3"], b["yolo2"], b["yolo1"], b["clip_window"]


class _ValData:
    def __init__(self, images, index, S, dev):
        self.items = [(n,) + tuple(E.image_read(images[n], S, dev)) for n in index]

    def get(self):
        return (torch.stack([it[1] for it in self.items]), [it[0] for it in self.items], np.stack([it[2] for it in self.items]))


class _PerImageOnly:
    """an evaluator of the user's own: ``do_python_eval`` and nothing else"""

    def __init__(self, emap):
        self._emap = emap

    def do_python_eval(self, detdata):
        self.entries = sum(len(d["boxes"]) for d in detdata)
        return self._emap.do_python_eval(detdata)


def test_solver_validate_through_collect_batch_returns_the_per_image_table(dev, tmp_path, monkeypatch):
    from disyolo_amd import config as cfg
    B, S = 2, 64
    monkeypatch.setattr(cfg, "OBJ_THRESHOLD", 0.05)
    images, recs, sizes, merged, index = synth_ground_truth([(40, 64), (64, 50), (64, 64), (33, 60)], 4)
    net = YOLONet(training=True, device=dev, image_size=S, batch_size=B, stage=1, seed=4)
    randomize_heads(net, 8)
    emap = E.MAP(recs, sizes, index, merged, net_size=S)
    assert hasattr(emap, "collect_batch")
    solver = Solver(net, _TrainData(B, S), emap, _ValData(images, index, S, dev), output_dir=str(tmp_path / "out"), max_iter=0,
                    log=lambda s: None)
    got = solver.validate()
    plain = _PerImageOnly(E.MAP(recs, sizes, index, merged, net_size=S))
    solver.eval = plain
    want = solver.validate()
    assert plain.entries >= 10, "fixture needs detections"
    assert set(got) == {"thresh", "AP", "mAP"} and repr(got) == repr(want)

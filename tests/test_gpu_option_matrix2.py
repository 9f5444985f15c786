"""The second option matrix on the GPU (tests/option_matrix2.py): image_size=(H, W) x nms x anchors / limits x mask-loss RoI
counts x tiled detection, crossed with the class list, k_map, mask_stride and the lock map, one row at a time -- the training
step against the composed CPU oracle, the same step with the fused launches on, its recorded / overlapped / pipelined forms bit
for bit against the eager step, inference and evaluation against the oracle's filter and mask assembly, evaluate() end to end,
detect_tiled and the loader on the rows marked for them.

The recipes and bounds are those of the per-option files (test_gpu_limits, test_gpu_mask_rois, test_gpu_nms_modes,
test_gpu_rect, test_gpu_tiles) and of test_gpu_option_matrix; nothing here is looser for any row.  Each row files its ratios to
the bounds in test_reports/option_matrix2_<row>.json.

Measured on an MI355X when the file was written: every case passes; over the 29 rows the worst teacher-forced forward is 0.21 of
its bound (the rows with pass-through layers; 0.03 elsewhere), the worst gradient 0.81 (the frozen_heads_m4 row; the stage-2
rows 0.59 to 0.79, the rows with a locked prefix 0.36 to 0.50), the total loss below 0.001 of its bound on every row; the file
takes about as long as test_gpu_option_matrix.py (156 s against 138 s)."""
import json
import os

import numpy as np
import pytest
import torch

import disyolo_oracle as O
import limits_ref as LR
import mask_roi_ref as RR
import option_matrix2 as OM
import rect_ref as R
import tiles_ref as TR
from disyolo_amd import evaluate as E
from disyolo_amd import tiles as TL
from disyolo_amd import train_data as TD
from disyolo_amd.net import YOLONet
from disyolo_amd.postprocess import SegmentationAccuracy
from disyolo_amd.solver import Solver
from disyolo_amd.voc_eval import voc_eval
from net_setup import perturb_variables
from test_gpu_eval_batch import randomize_heads, same_detfiles
from test_gpu_lock_map import REPORTS, _same_state, oracle_params, rel_err
from test_gpu_option_matrix import FUSED_PREFIX_BOUND
from test_gpu_rect import _ground_truth
from test_gpu_tiles import assert_same

pytestmark = pytest.mark.gpu

ROWS = OM.ROWS
DET_THRESH = OM.DET_THRESH


def make_net(dev, row, training=True, seed=1, **kw):
    """the row's net with the perturbation the CPU test ran through the oracle (tests/net_setup.py)"""
    net = YOLONet(training=training, device=dev, seed=seed, **dict(OM.net_kwargs(row), **kw))
    perturb_variables(net, seed)
    net.refresh_weights()
    return net


def file_report(row, **entries):
    """merge ``entries`` into the row's report (the tests of one row run in any order, or alone)"""
    os.makedirs(REPORTS, exist_ok=True)
    path = os.path.join(REPORTS, "option_matrix2_%s.json" % row.name)
    report = {}
    if os.path.exists(path):
        with open(path) as f:
            report = json.load(f)
    if report.get("options") != OM.describe(row):
        report = {"options": OM.describe(row)}
    report.update(entries)
    with open(path, "w") as f:
        json.dump(report, f, indent=1)


def det_of_net(net):
    """``row_batch``'s det_of: a first pass of the same net, with the same kernels, yields the detections that are planted"""
    def det_of(b):
        net.set_batch(LR.with_perms(b, D=net.max_detection)[0])
        net.compute_losses(DET_THRESH)
        torch.cuda.synchronize()
        return net.detections.cpu().numpy()
    return det_of


def kept(det):
    return [int(v) for v in (np.abs(np.asarray(det)[..., :4]).sum(-1) != 0).sum(1)]


# ------------------------------------------------------------------------------------------------ a. the step against the oracle
def check_shapes(net, row, what):
    B, G, D, k = row.B, row.G, row.D, row.k
    assert (net.H, net.W) == (row.H, row.W) and net.num_class == row.C and net.k == k and net.mask_stride == row.m, what
    assert tuple(net.true_boxes.shape) == (B, G, 5) and tuple(net.detections.shape) == (B, D, 6), what
    assert tuple(net.true_masks.shape) == (B, G, row.H, row.W), what
    assert tuple(net.rois.shape) == (B, max(row.rois[0] + row.rois[1], 16), 2 * (k + 1) + 4), what
    assert tuple(net.perm_det.shape) == (B, D) and tuple(net.perm_gt.shape) == (B, G), what
    assert [tuple(t.shape) for t in net.labels] == [(B, row.H // d, row.W // d, 3, 5 + row.C) for d in (8, 16, 32)], what


def own_logits(net, row):
    """the net's head logits [B, gh, gw, 3, 5 + C] x 3, as ``YOLONet.forward`` returns them"""
    return [net.by_idx[i].act.float().cpu().view(row.B, net.by_idx[i].Ho, net.by_idx[i].Wo, 3, 5 + row.C) for i in (75, 67, 59)]


def check_detections_and_rois(net, row, b, perms, what):
    """exact, on the same step: net.detections == nms_modes_ref on the net's own training-mode logits with the row's anchors,
    D and mode; net.rois / roi_count == mask_roi_ref.rows on the net's own detections, bit for bit"""
    det = net.detections.cpu().numpy()
    want_det = OM.oracle_detections(row, own_logits(net, row), b["clip_window"], DET_THRESH)
    np.testing.assert_allclose(det, want_det, rtol=1e-5, atol=1e-6, err_msg=what)
    Hm, Wm = row.H // row.m, row.W // row.m
    want_rows, _ = RR.rows(det, b["true_boxes"].numpy()[:, 0, 0, 0], perms, Hm, Wm, row.k, *row.rois)
    table, cnt = RR.table_of(want_rows, net.rois.shape[1], row.k)
    got_cnt = net.roi_count.cpu().numpy()
    assert got_cnt.tolist() == cnt.tolist(), "%s: positives per image %s, reference %s" % (what, got_cnt.tolist(), cnt.tolist())
    got = net.rois.cpu().numpy()
    for i in range(row.B):
        np.testing.assert_array_equal(got[i, :cnt[i]], table[i, :cnt[i]], err_msg="%s: RoI table of image %d" % (what, i))
    return cnt


@pytest.mark.parametrize("row", ROWS, ids=OM.ids(ROWS))
def test_train_step_matches_the_composed_oracle(dev, row):
    """the recipe of tests/test_gpu_option_matrix.py::test_train_step_matches_oracle, bounds unchanged: teacher-forced per-layer
    forward within 1.5e-2 relative l2, total loss within 1e-3, the trainable set, every arena gradient within 3 % relative l2 (or
    1e-3 of its largest element), moving statistics of trainable layers only, locked variables bit-unchanged by the optimizer;
    and, exact, the detections and the RoI table of the same step"""
    what = OM.describe(row)
    lock = OM.lock_of_row(row)
    net = make_net(dev, row)
    net.fuse_first_two = net.fuse_blocks = False      # (the per-layer comparison reads every layer's output)
    check_shapes(net, row, what)
    assert net.pass_through_layers() == OM.expected_pass_through(row), what
    b, perms, planted = OM.row_batch(row, det_of_net(net))
    p0 = oracle_params(net)
    net.set_batch(b)
    net.compute_losses(DET_THRESH)
    torch.cuda.synchronize()
    cnt = check_detections_and_rois(net, row, b, perms, what)
    print("%s: positives per image %s, detections per image %s" % (row.name, cnt.tolist(), kept(net.detections.cpu().numpy())))
    assert min(cnt) >= 1, "%s: every image needs a positive RoI" % what
    if row.rois[0] + row.rois[1] > 16:
        assert min(cnt) > 16, "%s: the wide table needs more than 16 positives per image" % what
    want_names = OM.trainable_names(row)
    tr = {n: p0[n].clone().requires_grad_(True) for n in want_names}
    pp = dict(p0)
    pp.update(tr)
    upd, taps = {}, {}
    force = {"act%d" % l.idx: l.act.float().cpu() for l in net.layers}
    parts, _, _, _ = OM.oracle_total_loss(row, pp, b, perms, upd, taps, force)
    report = {"forward": {}, "grad": {}}
    fails = []
    for l in net.layers:
        assert tuple(l.act.shape[1:3]) == tuple(taps["act%d" % l.idx].shape[1:3]), "%s: layer %d" % (what, l.idx)
        r, _, _ = rel_err(l.act, taps["act%d" % l.idx])
        report["forward"][l.idx] = r / 1.5e-2
        if not r < 1.5e-2:
            fails.append("layer %d forward (teacher-forced inputs): rel l2 err %.3g" % (l.idx, r))
    parts["total"].backward()
    total = float(net.total_loss().cpu())
    want_total = float(parts["total"])
    print("%s: total loss %.6f (oracle %.6f), mask %.6f (oracle %.6f)" % (row.name, total, want_total, float(net.mask_loss.cpu()[0]),
                                                                        float(parts["mask"])))
    report["total_loss"] = abs(total - want_total) / (1e-3 * abs(want_total))
    net.backward()
    torch.cuda.synchronize()
    got_names = set(net.trainable_names())
    for nm, (o, n) in net.arena_slices.items():
        g = net.grad_arena[o:o + n].cpu()
        assert nm in tr and tr[nm].grad is not None, "%s: %s" % (what, nm)
        want_g = tr[nm].grad.flatten()
        if nm.endswith("weights") or nm.endswith("biases"):
            want_g = want_g - O.L2_WEIGHT * tr[nm].detach().flatten()   # (the kernel adds l2*w inside Adam)
        r, amax, wmax = rel_err(g, want_g)
        report["grad"][nm] = min(r / 0.03, amax / (1e-3 * max(wmax, 1e-6)))
        if not (r < 0.03 or amax < 1e-3 * max(wmax, 1e-6)):
            fails.append("grad %s: rel l2 err %.3g (max abs %.3g of %.3g)" % (nm, r, amax, wmax))
    worst_f, worst_g = max(report["forward"].values()), max(report["grad"].values())
    print("%s: worst forward ratio %.3f, worst gradient ratio %.3f, loss ratio %.3f" % (row.name, worst_f, worst_g, report["total_loss"]))
    file_report(row, worst_forward=worst_f, worst_grad=worst_g, total_loss=report["total_loss"], forward=report["forward"],
                grad=report["grad"], positives=cnt.tolist())
    assert abs(total - want_total) < 1e-3 * abs(want_total), "%s: total loss %.6f, oracle %.6f" % (what, total, want_total)
    assert got_names == set(want_names), "%s: trainable set differs: %s" % (what, sorted(got_names ^ set(want_names)))
    assert not fails, "%s: %d checks failed:\n%s" % (what, len(fails), "\n".join(fails[:40]))
    # only trainable layers update their moving statistics
    assert {int(n.split("convolutional")[1].split("/")[0]) for n in upd} == {l.idx for l in net.layers if not l.lock and l.kind != "lin"}, what
    for nm, val in upd.items():
        r, amax, _ = rel_err(net.params[nm], val)
        assert r < 2e-2 or amax < 1e-4, "%s: moving stat %s: rel err %.3g" % (what, nm, r)
    # a locked layer: variables and moving statistics bit-unchanged by the step
    before = {n: p0[n] for n in p0 if lock[int(n.split("convolutional")[1].split("/")[0])]}
    w_before = net.arena.clone()
    net.optimizer_step()
    torch.cuda.synchronize()
    assert bool(before) == any(lock.values()), what
    for n, v in before.items():
        assert torch.equal(net.params[n].cpu(), v), "%s: locked variable %s changed" % (what, n)
    assert not torch.equal(net.arena, w_before), what


# ------------------------------------------------------------------------------------------------ b. the fused launches
def expected_plan(row):
    """the fused launches of a training step in front of conv10, from the lock map, m and the two sides: conv1+2 where both are
    in the locked prefix and nothing else reads act1 (m = 1's conv83 does), conv3+4 behind a prefix of 4, and the two 64-channel
    blocks behind a prefix of 9 where the quarter-size map divides into patches of 8 x 16 (tests/test_gpu_rect.py)"""
    P = OM.locked_prefix(row)
    blocks = (row.H // 4) % 8 == 0 and (row.W // 4) % 16 == 0
    return ([1, 2] if P >= 2 and row.m != 1 else []) + ([3, 4] if P >= 4 else []) + ([6, 7, 8, 9] if P >= 9 and blocks else [])


@pytest.mark.parametrize("row", ROWS, ids=OM.ids(ROWS))
def test_fused_step_agrees_with_the_layer_by_layer_step(dev, row):
    """the plan and the locked-prefix check of tests/test_gpu_option_matrix.py::test_fused_step_agrees_with_the_layer_by_layer_step:
    the fused launches in front of conv10 are those the row's lock map, m and sides allow, no more, no fewer, and every output of
    the locked prefix is within FUSED_PREFIX_BOUND relative l2 of the layer-by-layer one; the detections of the two steps are
    those of the oracle's filter on each step's own logits"""
    what = OM.describe(row)
    u, f = make_net(dev, row), make_net(dev, row)
    u.fuse_first_two = u.fuse_blocks = False
    plan = sorted(f._fusion_plan(True, 1, f.score_layer))
    assert sorted(u._fusion_plan(True, 1, u.score_layer)) == [], what
    assert [i for i in plan if i < 10] == expected_plan(row), "%s: fused launches %s, expected %s" % (what, plan, expected_plan(row))
    b, perms, _ = OM.row_batch(row, det_of_net(u))
    for n in (u, f):
        n.set_batch(b)
        n.compute_losses(DET_THRESH)
    torch.cuda.synchronize()
    P = f._backbone_prefix()
    assert P == OM.locked_prefix(row), what
    inner = {1, 3, 6, 8} & set(plan)          # (the first layer of a fused pair: its output is never written)
    prefix = {l.idx: rel_err(f.by_idx[l.idx].act, l.act)[0] for l in u.layers if 2 <= l.idx <= P and l.idx not in inner}
    print("%s: plan %s, worst prefix distance %.3g" % (row.name, plan, max(prefix.values()) if prefix else 0.0))
    file_report(row, fused_plan=plan, fused_prefix={str(i): v / FUSED_PREFIX_BOUND for i, v in prefix.items()})
    bad = {i: v for i, v in prefix.items() if not v < FUSED_PREFIX_BOUND}
    assert not bad, "%s: locked-prefix outputs of the fused step beyond %.1e relative l2 of the layer-by-layer ones: %s" % (
        what, FUSED_PREFIX_BOUND, bad)
    assert np.isfinite(float(f.total_loss().cpu())), what
    check_detections_and_rois(f, row, b, perms, what)


# ------------------------------------------------------------------------------------------------ c. recorded forms
@pytest.mark.parametrize("row", ROWS, ids=OM.ids(ROWS))
def test_recorded_overlapped_and_pipelined_steps_equal_eager(dev, row):
    """two steps on two batches with the device shuffle: eager == build_program() == build_program(overlap_tail=True), and ==
    the pipelined step behind a locked prefix; losses and every variable, Adam moment, rois, roi_count and perm_* bit for bit"""
    what = OM.describe(row)
    piped = OM.locked_prefix(row) >= 2
    scratch = make_net(dev, row, seed=4)
    batches = [OM.row_batch(row, det_of_net(scratch), seed=500 + t)[0] for t in range(3)]
    nets = [make_net(dev, row, seed=4) for _ in range(4 if piped else 3)]
    eager, rec, over = nets[:3]
    for n in nets:
        n.shuffle_seed = 77
        n.set_batch(batches[0])
    rec.build_program(det_thresh=DET_THRESH)
    over.build_program(det_thresh=DET_THRESH, overlap_tail=True)
    assert over._overlap, what
    if piped:
        pipe = nets[3]
        assert pipe._backbone_prefix() == OM.locked_prefix(row), what
        pipe.build_program(det_thresh=DET_THRESH, pipeline_backbone=True)
        pipe._set_inputs(batches[0]["images"], batches[0]["clip_window"])
        pipe.prime_pipeline()
    losses = [[] for _ in nets]
    first = None
    for t in range(2):
        losses[0].append(float(eager.train_step(batches[t], det_thresh=DET_THRESH).cpu()))
        first = eager.roi_count.cpu().tolist() if first is None else first
        losses[1].append(float(rec.train_step(batches[t]).cpu()))
        if t == 0:
            over.train_step(batches[t], want_loss=False)        # (the tail stays open into the next call)
            assert over._tail_open, what
            losses[2].append(float(over.total_loss().cpu()))
        else:
            losses[2].append(float(over.train_step(batches[t]).cpu()))
        if piped:
            mixed = dict(batches[t])
            mixed["images"] = batches[t + 1]["images"]
            pipe.set_batch(mixed)
            losses[3].append(float(pipe.train_step(None).cpu()))
    torch.cuda.synchronize()
    print("%s: losses %s, positives per image %s then %s" % (row.name, losses, first, eager.roi_count.cpu().tolist()))
    # (a batch whose mask term meets an RoI of zero area is NaN, as in the reference -- SURVEY B14; the comparison holds then too)
    assert np.isfinite(losses[0]).any(), "%s: no finite loss: %s" % (what, losses[0])
    assert bool(torch.isfinite(eager.arena).all()) and min(first) >= 1, what
    assert sorted(eager.perm_det[0].cpu().tolist()) == list(range(row.D)), what
    assert sorted(eager.perm_gt[-1].cpu().tolist()) == list(range(row.G)), what
    for other, ls in zip(nets[1:], losses[1:]):
        assert np.array_equal(np.asarray(losses[0]), np.asarray(ls), equal_nan=True), "%s: losses %s" % (what, losses)
        try:
            _same_state(eager, other)
            for name in ("rois", "roi_count", "detections"):
                assert torch.equal(getattr(eager, name), getattr(other, name)), name
            for name in ("perm_det", "perm_gt"):
                # (the pipelined step keeps two sets of inputs: the permutations of the last step are in one of them)
                sets = [getattr(other, name)] if other._pipe_in is None else [s[name] for s in other._pipe_in]
                assert any(torch.equal(getattr(eager, name), s) for s in sets), name
        except AssertionError as e:
            raise AssertionError("%s: state of net %d differs from the eager net's: %s" % (what, nets.index(other), e))
    assert all(n.step_count == 2 for n in nets), what
    if piped:
        pipe.check_cluster_sync()
    rec.check_cluster_sync()


# ------------------------------------------------------------------------------------------------ d. inference
@pytest.mark.parametrize("row", ROWS, ids=OM.ids(ROWS))
def test_inference_returns_the_oracle_detections_and_masks(dev, row):
    """an inference net of the row, a clip window of its own on the last image: logits and score maps within 2e-2 relative l2
    of the oracle's forward, the detections == the oracle's filter on the kernel's own logits (the row's anchors, D and mode),
    the device-side masks == rect_ref.val_test at the row's k and m, rows past 64 kept where D > 64, and the recorded inference
    program == the eager call"""
    what = OM.describe(row)
    B, H, W, C, D = row.B, row.H, row.W, row.C, row.D
    thr = OM.INFER_THRESH
    net = make_net(dev, row, training=False, seed=0)
    assert net.pass_through_layers() == [], what
    batch = OM.infer_batch(row)
    preds, det, mask_pos = net.forward(batch["images"], batch["clip_window"], [thr], is_training=False)
    torch.cuda.synchronize()
    assert [tuple(p.shape) for p in preds] == [(B, H // d, W // d, 3, 5 + C) for d in (8, 16, 32)], what
    assert tuple(mask_pos.shape) == (B, H // row.m, W // row.m, row.k ** 2) and tuple(det.shape) == (B, D, 6), what
    yq, mq = OM.oracle_forward(row, oracle_params(net), batch["images"], False)
    ratios = [rel_err(got, want)[0] / 2e-2 for got, want in list(zip(preds, yq)) + [(mask_pos, mq)]]
    want = OM.oracle_detections(row, [t.cpu() for t in preds], batch["clip_window"], thr)
    got = det.cpu().numpy()
    print("%s: inference forward ratios %s, detections per image %s" % (row.name, ["%.3f" % r for r in ratios], kept(want)))
    file_report(row, inference_forward=max(ratios), inference_detections=kept(want))
    assert max(ratios) < 1.0, "%s: forward differs from the oracle, ratios to 2e-2: %s" % (what, ratios)
    assert min(kept(want)) >= 1, "%s: fixture needs detections" % what
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-6, err_msg=what)
    dets, keep, masks = net.evaluation_device(batch["images"], batch["clip_window"], [thr])
    torch.cuda.synchronize()
    assert tuple(masks.shape) == (B, D, H // row.m, W // row.m) and tuple(keep.shape) == (B, D), what
    score = net.by_idx[net.score_layer].act.cpu()
    assert torch.equal(score, mask_pos.cpu()) and torch.equal(dets, det), what
    wb, wm = R.val_test(dets.cpu().numpy(), score, row.k)
    kp = keep.cpu().numpy().astype(bool)
    assert any(np.ndim(w) for w in wm), "%s: test needs detections with a box of positive area" % what
    for i in range(B):
        assert kp[i].sum() == len(wb[i]), what
        np.testing.assert_array_equal(dets[i].cpu().numpy()[kp[i]], wb[i], err_msg=what)
        if len(wb[i]):
            np.testing.assert_allclose(masks[i].cpu().numpy()[kp[i]], wm[i], rtol=1e-5, atol=1e-6, err_msg=what)
        if D > 64:
            assert kept(want)[i] > 64 and kp[i, 64:].any(), "%s: rows past 64 must be kept (image %d keeps %d)" % (what, i, kp[i].sum())
    det_e, keep_e, masks_e = dets.clone(), keep.clone(), masks.clone()
    net.build_infer_program(det_thresh=thr, graph=False)
    net.detections.fill_(float("nan"))
    d2, c2, m2, k2 = net.infer(batch["images"], batch["clip_window"])
    torch.cuda.synchronize()
    assert torch.equal(d2, det_e) and torch.equal(k2, keep_e) and torch.equal(m2, masks_e), what
    assert c2.cpu().tolist() == kept(want), what


# ------------------------------------------------------------------------------------------------ e. evaluate() end to end
MAP_ROWS = [r for r in ROWS if "map" in r.extras]


@pytest.mark.parametrize("row", MAP_ROWS, ids=OM.ids(MAP_ROWS))
def test_evaluate_end_to_end_with_the_rows_options(dev, row):
    """the recipe of tests/test_gpu_rect.py::test_evaluate_end_to_end_on_a_rectangular_net with the row's options: the AP table
    and the mIoU of evaluate() equal the per-image loop of the reference side on the same detections; and the batched paste +
    IoU (MAP.collect_batch) equals the per-image path (MAP.collect) on them
    (tests/test_gpu_limits.py::test_collect_batch_with_100_detections_gives_the_per_image_table)"""
    what = OM.describe(row)
    C, thr, B = row.C, 0.05, row.B
    assert B > 1, "the batched test loop needs a batch"
    net = YOLONet(training=False, device=dev, stage=1, seed=0, **dict(OM.net_kwargs(row), lock=None))
    randomize_heads(net, 7)
    shapes = [(70, 120), (96, 96), (100, 60)][:B + 1]            # (a short last batch)
    images, recs, sizes, merged, index = _ground_truth(shapes, 33, C)
    emap = E.MAP(recs, sizes, index, merged, net_size=(row.H, row.W), classes=OM.names(C))
    thresh_out, mask_acc, _ = E.evaluate(net, images, emap, det_thresh=thr)
    assert len(thresh_out) == 1 and len(thresh_out[0]["AP"]) == C and len(mask_acc) == C + 2, what
    detfile = {str(c): [] for c in range(C)}
    conf = np.zeros((C + 1, C + 1), np.int64)
    ndet, past64 = 0, False
    for at in range(0, len(index), B):
        ids = index[at:at + B]
        frame = torch.zeros(B, row.H, row.W, 3, dtype=torch.float32, device=dev)
        windows = np.tile(np.array([[0.0, 0.0, 1.0, 1.0]], np.float32), (B, 1))
        for i, n in enumerate(ids):
            windows[i] = E.image_read(images[n], (row.H, row.W), dev, out=frame[i])[1]
            assert np.array_equal(windows[i], R.letterbox_window(sizes[n][0], sizes[n][1], row.H, row.W)), what
        dets, keep, masks = net.evaluation_device(frame, windows, [np.float32(thr)])
        torch.cuda.synchronize()
        dets, keep, masks = dets.clone(), keep.clone(), masks.clone()
        kp = keep.cpu().numpy().astype(bool)
        past64 = past64 or bool(kp[:len(ids), 64:].any())
        if len(ids) == B:
            # the batched paste + IoU against the per-image path, on this batch's detections
            emap_b = E.MAP(recs, sizes, index, merged, net_size=(row.H, row.W), classes=OM.names(C))
            emap_a = E.MAP(recs, sizes, index, merged, net_size=(row.H, row.W), classes=OM.names(C))
            file_b, file_a = {str(c): [] for c in emap_b.classid}, {str(c): [] for c in emap_a.classid}
            seg_b, seg_a = SegmentationAccuracy(dev, C), SegmentationAccuracy(dev, C)
            merged_b = emap_b.collect_batch(ids, dets, keep, masks, file_b, true_maps=[merged[n] for n in ids], conf=seg_b.conf)
            for i, n in enumerate(ids):
                sel = torch.from_numpy(kp[i]).to(dev)
                m = emap_a.collect(n, dets[i].cpu().numpy()[kp[i]], masks[i][sel], file_a)
                seg_a.add(merged[n], m)
                assert torch.equal(m, merged_b[i]), "%s: merged map of %s" % (what, n)
            same_detfiles(file_a, file_b)
            assert torch.equal(seg_a.conf, seg_b.conf), what
        det_box, det_mask = net.evaluation(frame, windows, [np.float32(thr)])
        for i, n in enumerate(ids):
            h, w = sizes[n]
            entries, mm = R.paste_detections(np.asarray(det_box[i]), det_mask[i], h, w, row.H, row.W)
            ndet += len(entries)
            for e in entries:
                detfile[str(e["classid"])].append({"imageid": n, "score": e["score"], "mask": e["mask"]})
            conf += np.bincount(merged[n].astype(np.int64).ravel() * (C + 1) + mm.astype(np.int64).ravel(),
                                minlength=(C + 1) ** 2).reshape(C + 1, C + 1)
    assert ndet >= 10 and len({c for c in detfile if detfile[c]}) >= 3, "%s: fixture needs detections of several classes" % what
    assert past64 == (row.D > 64), "%s: rows past 64 pasted: %s" % (what, past64)
    res, pres, aps = [], [], []
    for c in range(C):
        if not detfile[str(c)]:
            r, p, a = 0.0, 0.0, 0.0
        else:
            r, p, a = voc_eval(detfile[str(c)], recs, index, c, ovthresh=0.5, use_07_metric=False)
        res, pres, aps = res + [r], pres + [p], aps + [a]
    print("%s: evaluate: %d detections, AP %s" % (row.name, ndet, json.dumps(aps)))
    assert repr(thresh_out[0]["AP"]) == repr(aps), what
    assert repr(thresh_out[0]["mAP"]) == repr([float(np.mean(res)), float(np.mean(pres)), float(np.mean(aps))]), what
    cf = conf.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        ious = [cf[k, k] / (cf[k].sum() + cf[:, k].sum() - cf[k, k]) for k in range(C + 1)]
    np.testing.assert_array_equal(np.asarray(mask_acc[:-1]), np.asarray(ious))
    np.testing.assert_array_equal(mask_acc[-1], float(np.mean(ious)))


# ------------------------------------------------------------------------------------------------ f. tiled detection
TILED_ROWS = [r for r in ROWS if "tiled" in r.extras]
IMAGE_HW = (150, 200)


@pytest.mark.parametrize("row", TILED_ROWS, ids=OM.ids(TILED_ROWS))
def test_detect_tiled_with_the_rows_options(dev, row):
    """tests/test_gpu_tiles.py::test_detect_tiled_end_to_end with the row's inference net on a 150 x 200 image: the result ==
    tiles_ref.merge_tiles on the net's own tile outputs, eager and recorded; the case has seam pairs and a merged group, and on
    a row with D >= 100 more than 64 kept rows in some tile"""
    what = OM.describe(row)
    thr = 0.05
    net = make_net(dev, row, training=False, seed=0)
    img = np.random.default_rng(11).integers(0, 256, size=IMAGE_HW + (3,), dtype=np.uint8)
    res = TL.detect_tiled(net, img, overlap=16, det_thresh=thr, keep_tiles=True)
    np.testing.assert_array_equal(res.inputs.cpu().numpy(), TR.tile_gather(img, res.tiles, 0, len(res.tiles), (row.H, row.W)))
    det, keep, masks = (t.cpu().numpy() for t in res.tile_outputs)
    assert det.shape[1:] == (row.D, 6) and masks.shape[1:] == (row.D, row.H // row.m, row.W // row.m), what
    want = TR.merge_tiles(res.tiles, IMAGE_HW, (row.H, row.W), det, keep, masks, 0.5)
    merged_groups = sum(len(m) > 1 for m in want.members)
    print("%s: %d tiles, kept rows per tile %s, %d instances, %d pairs, %d groups, %d of them merged" % (
        row.name, len(res.tiles), keep.sum(axis=1).tolist(), len(want.instances), len(want.pairs), len(want.boxes), merged_groups))
    assert (keep.sum(axis=1) > 0).all() and len(want.pairs) > 0 and merged_groups >= 1, "%s: the case needs seam pairs and a merged group" % what
    if row.D >= 100:
        assert keep.sum(axis=1).max() > 64 and keep[:, 64:].any(), "%s: more than 64 kept rows in some tile" % what
    assert_same(res, want, IMAGE_HW)
    net.build_infer_program(det_thresh=thr, graph=False)
    res2 = TL.detect_tiled(net, torch.from_numpy(img).to(dev), overlap=16, det_thresh=thr)
    assert res2.inputs is None
    assert_same(res2, want, IMAGE_HW)


# ------------------------------------------------------------------------------------------------ g. the loader
LOADER_ROWS = [r for r in ROWS if "loader" in r.extras]


@pytest.mark.parametrize("row", LOADER_ROWS, ids=OM.ids(LOADER_ROWS))
def test_loader_on_the_rows_net_is_replayed_by_the_reference_side(dev, row, tmp_path):
    """defect_train with the row's sides, class list, anchors and G, for one epoch of 5 records of more than 20 rectangular
    instances each (limits_ref.rectangle_record): every decision, the boxes, the three target grids and the pixels of the images
    and the instance masks equal rect_ref.loader_sample / place_* on a RandomState of the same seed, bit for bit
    (tests/test_gpu_rect.py::test_defect_train_on_a_rectangular_net_replayed_by_the_reference_side); two Solver steps on it give
    finite losses"""
    what = OM.describe(row)
    NH, NW, B, G, C = row.H, row.W, row.B, row.G, row.C
    classes = OM.names(C)
    anchors = OM.anchors_of(row)
    rng = np.random.RandomState(8)
    n_inst = min(G, 24)
    assert n_inst > 20, "%s: the loader row needs room for more than 20 instances" % what
    # (records about as large as the net: the smallest instance, 6 pixels, stays more than a pixel of the score map after the
    #  loader's fit, so that no RoI of the two steps below rounds to zero area -- a NaN mask term, as in the reference)
    labels = [LR.rectangle_record(rng, h, w, n_inst, classes) for (h, w) in [(110, 80), (96, 64), (130, 70), (100, 90), (90, 60)]]
    data = TD.defect_train(labels, batch_size=B, image_size=(NH, NW), device=dev, rng=np.random.RandomState(123), classes=classes,
                           anchors=anchors, max_box_per_image=G)
    ref_rng = np.random.RandomState(123)
    ref_labels = list(labels)
    ref_rng.shuffle(ref_labels)
    cursor, served = 0, 0
    while served < len(labels):
        images, masks, tboxes, y3, y2, y1, window = data.get()
        torch.cuda.synchronize()
        assert images.shape == (B, NH, NW, 3) and masks.shape == (B, G, NH, NW) and tboxes.shape == (B, 1, 1, 1, G, 5), what
        assert y3.shape == (B, NH // 8, NW // 8, 3, 5 + C) and y1.shape == (B, NH // 32, NW // 32, 3, 5 + C), what
        for b in range(B):
            lab = ref_labels[cursor]
            h, w = lab["image"].shape[:2]
            inst = [O.instance_mask(p, h, w) for p in lab["polygons"]]
            boxes = []
            for m in inst:
                rr, cc = np.where(m)
                boxes.append([cc.min(), rr.min(), cc.max() + 1, rr.max() + 1])
            cls = [classes.index(n) for n in lab["class_names"]]
            dec, want_boxes, _ = R.loader_sample(ref_rng, h, w, np.asarray(boxes, np.float32), cls, NH, NW, num_class=C)
            got = data.last_decisions[b]
            for key in ("scale_crop", "new_w", "new_h", "dx", "dy", "flip", "bnl"):
                assert got[key] == dec[key], (what, served, key, got, dec)
            n = len(inst)
            assert n == n_inst
            np.testing.assert_array_equal(tboxes[b, 0, 0, 0, :n, :4], want_boxes)
            np.testing.assert_array_equal(tboxes[b, 0, 0, 0, :n, 4], np.asarray(cls, np.float32))
            assert (tboxes[b, 0, 0, 0, n:] == 0).all() and not masks[b, n:].any(), what
            # the targets with the row's anchors: rect_ref.assign_targets on the placed boxes, flipped as the loader flips
            want_ys = loader_targets(np.asarray(boxes, np.float32), h, w, cls, dec, NH, NW, anchors, C)
            for g_, w_ in zip((y3, y2, y1), want_ys):
                np.testing.assert_array_equal(g_[b], w_)
            img = R.place_image(lab["image"], NH, NW, dec["new_w"], dec["new_h"], dec["dx"], dec["dy"], dec["flip"])
            if dec["bnl"] == 2:
                rows_ = np.concatenate([dec["salt"][0], dec["pepper"][0]])
                cols_ = np.concatenate([dec["salt"][1], dec["pepper"][1]])
                img = O.salt_pepper(img, rows_, cols_, len(dec["salt"][0]))
            elif dec["bnl"] == 3:
                img = O.change_light(img, dec["coeff"])
            elif dec["bnl"] == 4:
                img = R.motion_blur3(img, dec["angle"], {"right": 1, "left": 2, "full": 0}[dec["line_type"]])
            np.testing.assert_array_equal(images[b].cpu().numpy(), img.astype(np.float32) / 255.0)
            for j in range(n):
                m = R.place_mask(inst[j].astype(np.float32), NH, NW, dec["new_w"], dec["new_h"], dec["dx"], dec["dy"], dec["flip"])
                np.testing.assert_array_equal(masks[b, j].cpu().numpy(), m)
            cursor += 1
            served += 1
            if cursor >= len(ref_labels):
                ref_rng.shuffle(ref_labels)
                cursor = 0
    net = make_net(dev, row)
    hist = Solver(net, data, output_dir=str(tmp_path), max_iter=2, summary_iter=2, save_iter=10 ** 6, log=lambda s: None).train()
    torch.cuda.synchronize()
    print("%s: two Solver steps: %s" % (row.name, hist))
    assert net.step_count == 2 and len(hist) == 2 and np.isfinite(hist).all(), "%s: losses %s" % (what, hist)


def loader_targets(boxes_xyxy, image_h, image_w, cls, dec, NH, NW, anchors, C):
    """the three target grids of rect_ref.loader_sample with ``anchors``: the boxes placed in the net frame by the sample's
    decisions (utils/train_data.py:136-147), assigned before the flip, the grids flipped as the loader flips them"""
    norm = np.asarray([NW, NH, NW, NH], np.float32)
    sx, sy = float(dec["new_w"]) / image_w, float(dec["new_h"]) / image_h
    flip = dec["flip"]
    bx = np.zeros((len(boxes_xyxy), 4), np.float32)
    for j, (x1, y1, x2, y2) in enumerate(boxes_xyxy):
        x1 = max(min(float(x1) * sx + dec["dx"], NW - 1), 0)
        y1 = max(min(float(y1) * sy + dec["dy"], NH - 1), 0)
        x2 = max(min(float(x2) * sx + dec["dx"], NW - 1), 0)
        y2 = max(min(float(y2) * sy + dec["dy"], NH - 1), 0)
        bx[j] = [(x2 + x1) / 2.0, (y2 + y1) / 2.0, x2 - x1, y2 - y1]
    ys = R.assign_targets(bx, cls, NH, NW, anchors=anchors, num_class=C)
    if flip == 2:
        for k in range(3):
            ys[k] = ys[k][:, ::-1].copy()
            on = ys[k][..., 4] == 1
            ys[k][on, 0] = np.float32(NW - 1) - ys[k][on, 0]
    elif flip == 3:
        for k in range(3):
            ys[k] = ys[k][::-1].copy()
            on = ys[k][..., 4] == 1
            ys[k][on, 1] = np.float32(NH - 1) - ys[k][on, 1]
    for k in range(3):
        ys[k][..., 0:4] = ys[k][..., 0:4] / norm
    return ys

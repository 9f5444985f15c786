"""Rectangular nets, image_size = (H, W), on the GPU: the rows of tests/rect_ref.py through the training step (against the
oracle, its recorded forms bit for bit, fused against layer by layer), inference, image_size=(64, 64) against 64, known
answers worked out by hand, and the letter box / paste / evaluate drivers with the net's two sides.

Recipes and bounds are those of tests/test_gpu_option_matrix.py (and, through it, of the per-option files); nothing is
looser here for any row."""
import json

import numpy as np
import pytest
import torch

import disyolo_oracle as O
import mask_stride_ref as MR
import rect_ref as R
from disyolo_amd import config as cfg
from disyolo_amd import evaluate as E
from disyolo_amd import lib as L
from disyolo_amd import train_data as TD
from disyolo_amd.net import YOLONet
from disyolo_amd.postprocess import paste_detections
from disyolo_amd.synth import synthetic_batch
from disyolo_amd.voc_eval import voc_eval
from net_setup import perturb_variables
from test_gpu_eval_batch import randomize_heads
from test_gpu_lock_map import _same_state, oracle_params, rel_err
from test_gpu_train_data import PLACE

pytestmark = pytest.mark.gpu

ROWS, VALUE_ROWS = R.ROWS, R.VALUE_ROWS
ANCHOR = [r for r in ROWS if "anchor" in r.extras][0]
DET_THRESH = 0.1
FUSED_PREFIX_BOUND = 1.5e-2     # tests/test_gpu_fullsize.py: fused launches against the layer-by-layer forward, relative l2


def make_net(dev, row, training=True, seed=1, **kw):
    net = YOLONet(training=training, device=dev, seed=seed, **dict(R.net_kwargs(row), **kw))
    perturb_variables(net, seed)
    net.refresh_weights()
    return net


# ------------------------------------------------------------------------------------------------ 1. the step against the oracle
def run_step(dev, row, fused):
    net = make_net(dev, row)
    if not fused:
        net.fuse_first_two = net.fuse_blocks = False      # (the per-layer comparison reads every layer's output)
    b, perms = R.row_batch(row)
    p0 = oracle_params(net)
    net.set_batch(b)
    net.compute_losses(DET_THRESH)
    torch.cuda.synchronize()
    return net, b, perms, p0


@pytest.mark.parametrize("row", VALUE_ROWS, ids=R.ids(VALUE_ROWS))
def test_train_step_matches_oracle(dev, row):
    """tests/test_gpu_option_matrix.py::test_train_step_matches_oracle on a rectangular row, bounds unchanged: teacher-forced
    per-layer forward within 1.5e-2 relative l2, total loss within 1e-3, every arena gradient within 3 % relative l2 (or 1e-3
    of its largest element), moving statistics of trainable layers only, locked variables bit-unchanged by the optimizer"""
    what = R.describe(row)
    lock = R.lock_of_row(row)
    net, b, perms, p0 = run_step(dev, row, fused=False)
    assert (net.H, net.W, net.S) == (row.H, row.W, None), what
    assert [tuple(t.shape) for t in net.labels] == [(row.B, row.H // d, row.W // d, 3, 5 + row.C) for d in (8, 16, 32)], what
    assert tuple(net.true_masks.shape) == (row.B, cfg.MAX_BOX_PER_IMAGE, row.H, row.W), what
    assert int(net.roi_count.sum()) > 0, "%s: test needs at least one positive RoI" % what
    want_names = R.trainable_names(row)
    tr = {n: p0[n].clone().requires_grad_(True) for n in want_names}
    pp = dict(p0)
    pp.update(tr)
    upd, taps = {}, {}
    force = {"act%d" % l.idx: l.act.float().cpu() for l in net.layers}
    parts, _, _, _ = R.oracle_total_loss(row, pp, b, perms, upd, taps, force)
    fails, worst_f, worst_g = [], 0.0, 0.0
    for l in net.layers:
        assert tuple(l.act.shape[1:3]) == tuple(taps["act%d" % l.idx].shape[1:3]), "%s: layer %d" % (what, l.idx)
        r, _, _ = rel_err(l.act, taps["act%d" % l.idx])
        worst_f = max(worst_f, r / 1.5e-2)
        if not r < 1.5e-2:
            fails.append("layer %d forward (teacher-forced inputs): rel l2 err %.3g" % (l.idx, r))
    parts["total"].backward()
    total = float(net.total_loss().cpu())
    want_total = float(parts["total"])
    print("%s: total loss %.6f (oracle %.6f), mask %.6f (oracle %.6f)" % (row.name, total, want_total, float(net.mask_loss.cpu()[0]),
                                                                        float(parts["mask"])))
    net.backward()
    torch.cuda.synchronize()
    got_names = set(net.trainable_names())
    for nm, (o, cnt) in net.arena_slices.items():
        g = net.grad_arena[o:o + cnt].cpu()
        assert nm in tr and tr[nm].grad is not None, "%s: %s" % (what, nm)
        want_g = tr[nm].grad.flatten()
        if nm.endswith("weights") or nm.endswith("biases"):
            want_g = want_g - O.L2_WEIGHT * tr[nm].detach().flatten()   # (the kernel adds l2*w inside Adam)
        r, amax, wmax = rel_err(g, want_g)
        worst_g = max(worst_g, min(r / 0.03, amax / (1e-3 * max(wmax, 1e-6))))
        if not (r < 0.03 or amax < 1e-3 * max(wmax, 1e-6)):
            fails.append("grad %s: rel l2 err %.3g (max abs %.3g of %.3g)" % (nm, r, amax, wmax))
    print("%s: worst forward ratio %.3f, worst gradient ratio %.3f, loss ratio %.3f" % (
        row.name, worst_f, worst_g, abs(total - want_total) / (1e-3 * abs(want_total))))
    assert abs(total - want_total) < 1e-3 * abs(want_total), "%s: total loss %.6f, oracle %.6f" % (what, total, want_total)
    assert got_names == set(want_names), "%s: trainable set differs: %s" % (what, sorted(got_names ^ set(want_names)))
    assert not fails, "%s: %d checks failed:\n%s" % (what, len(fails), "\n".join(fails[:40]))
    assert {int(n.split("convolutional")[1].split("/")[0]) for n in upd} == {l.idx for l in net.layers if not l.lock and l.kind != "lin"}, what
    for nm, val in upd.items():
        r, amax, _ = rel_err(net.params[nm], val)
        assert r < 2e-2 or amax < 1e-4, "%s: moving stat %s: rel err %.3g" % (what, nm, r)
    before = {n: p0[n] for n in p0 if lock[int(n.split("convolutional")[1].split("/")[0])]}
    w_before = net.arena.clone()
    net.optimizer_step()
    torch.cuda.synchronize()
    assert bool(before) == any(lock.values()), what
    for n, v in before.items():
        assert torch.equal(net.params[n].cpu(), v), "%s: locked variable %s changed" % (what, n)
    assert not torch.equal(net.arena, w_before), what


# ------------------------------------------------------------------------------------------------ 2. recorded forms
def _batches(row, n, first=500):
    return [R.synthetic_batch(row.B, row.H, row.W, seed=first + t, num_class=row.C) for t in range(n)]


@pytest.mark.parametrize("row", ROWS, ids=R.ids(ROWS))
def test_recorded_overlapped_pipelined_and_graph_steps_equal_eager(dev, row):
    """tests/test_gpu_option_matrix.py::test_recorded_overlapped_and_pipelined_steps_equal_eager plus the hipGraph of the
    recorded step: two steps on two batches, losses and every variable bit for bit"""
    what = R.describe(row)
    piped = R.locked_prefix(row) >= 2
    batches = _batches(row, 3)
    nets = [make_net(dev, row, seed=4) for _ in range(5 if piped else 4)]
    eager, rec, over, graph = nets[:4]
    for n in nets:
        n.set_batch(batches[0])
    rec.build_program(det_thresh=DET_THRESH)
    over.build_program(det_thresh=DET_THRESH, overlap_tail=True)
    graph.build_program(det_thresh=DET_THRESH, graph=True)
    assert over._overlap and graph._graph is not None, what
    if piped:
        pipe = nets[4]
        assert pipe._backbone_prefix() == R.locked_prefix(row), what
        pipe.build_program(det_thresh=DET_THRESH, pipeline_backbone=True)
        pipe._set_inputs(batches[0]["images"], batches[0]["clip_window"])
        pipe.prime_pipeline()
    losses = [[] for _ in nets]
    for t in range(2):
        losses[0].append(float(eager.train_step(batches[t], det_thresh=DET_THRESH).cpu()))
        losses[1].append(float(rec.train_step(batches[t]).cpu()))
        if t == 0:
            over.train_step(batches[t], want_loss=False)        # (the tail stays open into the next call)
            assert over._tail_open, what
            losses[2].append(float(over.total_loss().cpu()))
        else:
            losses[2].append(float(over.train_step(batches[t]).cpu()))
        losses[3].append(float(graph.train_step(batches[t]).cpu()))
        if piped:
            mixed = dict(batches[t])
            mixed["images"] = batches[t + 1]["images"]
            pipe.set_batch(mixed)
            losses[4].append(float(pipe.train_step(None).cpu()))
    torch.cuda.synchronize()
    print("%s: losses %s" % (row.name, losses))
    if row.values:
        assert np.isfinite(losses[0]).any(), "%s: no finite loss: %s" % (what, losses[0])
    assert bool(torch.isfinite(eager.arena).all()), what
    for other, ls in zip(nets[1:], losses[1:]):
        assert np.array_equal(np.asarray(losses[0]), np.asarray(ls), equal_nan=True), "%s: losses %s" % (what, losses)
        try:
            _same_state(eager, other)
        except AssertionError as e:
            raise AssertionError("%s: state of net %d differs from the eager net's: %s" % (what, nets.index(other), e))
    assert all(n.step_count == 2 for n in nets), what
    if piped:
        pipe.check_cluster_sync()
    rec.check_cluster_sync()


PAIR_ROWS = [r for r in VALUE_ROWS if "pair" in r.extras]
FP8_ROWS = [r for r in VALUE_ROWS if "fp8" in r.extras]


@pytest.mark.parametrize("row", PAIR_ROWS, ids=R.ids(PAIR_ROWS))
def test_backbone_pair_steps_like_the_plain_net(dev, row):
    """tests/test_gpu_option_matrix.py::test_backbone_pair_steps_like_the_plain_net (same bounds) on the wide anchor"""
    what = R.describe(row)
    batches = _batches(row, 5, first=70)
    plain = make_net(dev, row, seed=8)
    pair = YOLONet(training=True, device=dev, seed=8, backbone_pair=True, **R.net_kwargs(row))
    pair.load_state_dict(plain.state_dict())
    assert tuple(pair.images.shape) == (2 * row.B, row.H, row.W, 3), what
    lp, lq = [], []
    for t in range(4):
        lp.append(float(plain.train_step(batches[t], det_thresh=DET_THRESH).cpu()))
        lq.append(float(pair.train_step((batches[t], batches[t + 1]) if t % 2 == 0 else None, det_thresh=DET_THRESH).cpu()))
    torch.cuda.synchronize()
    print("%s: plain %s pair %s" % (row.name, lp, lq))
    np.testing.assert_allclose(lq, lp, rtol=2e-3, err_msg=what)
    for name in plain.params:
        a, b = plain.params[name], pair.params[name]
        assert float((a - b).abs().max()) <= 4.5e-4 + 1e-3 * float(a.abs().max()), "%s: %s" % (what, name)


@pytest.mark.parametrize("row", FP8_ROWS, ids=R.ids(FP8_ROWS))
def test_fp8_backbone_inference(dev, row):
    """tests/test_gpu_option_matrix.py::test_fp8_backbone_inference (same bound) on the wide anchor"""
    what = R.describe(row)
    b = R.synthetic_batch(row.B, row.H, row.W, seed=7, num_class=row.C)
    kw = dict(R.net_kwargs(row), lock=None)
    net = YOLONet(training=False, device=dev, stage=1, seed=0, dtype="fp8", **kw)
    ref = YOLONet(training=False, device=dev, stage=1, seed=0, **kw)
    net._set_inputs(b["images"], b["clip_window"])
    net.calibrate_fp8()
    preds, _, mask_pos = net.forward(b["images"], b["clip_window"], [0.1], is_training=False)
    preds = [p.clone() for p in preds]
    mask_pos = mask_pos.clone()
    preds_b, _, mask_b = ref.forward(b["images"], b["clip_window"], [0.1], is_training=False)
    torch.cuda.synchronize()
    assert mask_pos.shape == (row.B, row.H // row.m, row.W // row.m, row.k ** 2), what
    for a, c in list(zip(preds, preds_b)) + [(mask_pos, mask_b)]:
        r, _, _ = rel_err(a, c)
        print("%s: fp8 vs bf16 rel l2 %.4f" % (row.name, r))
        assert r < 0.35, "%s: %.3g" % (what, r)


# ------------------------------------------------------------------------------------------------ 3. fused against layer by layer
# the fused launches each row's training step takes in front of conv10 and in the mask head.  conv1+2 needs both locked and
# no other reader of act1 (m = 1's conv83 is one); conv3+4 a locked pair; the two 64-channel blocks patches of 8 x 16 at
# (H/4, W/4), i.e. W a multiple of 64; the mask head (conv80-82 in one launch) is inference-only, so no training step has it
EXPECTED_TRAIN_PLAN = {
    "b2_64x128_c3_k3_m2_stage1": [1, 2, 3, 4, 6, 7, 8, 9],
    "b2_128x64_c3_k3_m2_stage2": [],
    "b3_96x160_c6_k5_m4_stage1": [1, 2, 3, 4],
    "b1_160x96_c5_k7_m1_stage1": [3, 4],
}
# ... and of an inference net of the row (every layer in inference mode)
EXPECTED_INFER_PLAN = {
    "b2_64x128_c3_k3_m2_stage1": [1, 2, 3, 4, 6, 7, 8, 9, 80, 81, 82],
    "b2_128x64_c3_k3_m2_stage2": [1, 2, 3, 4, 6, 7, 8, 9, 80, 81, 82],
    "b3_96x160_c6_k5_m4_stage1": [1, 2, 3, 4],
    "b1_160x96_c5_k7_m1_stage1": [3, 4],
}


@pytest.mark.parametrize("row", VALUE_ROWS, ids=R.ids(VALUE_ROWS))
def test_fused_launches_agree_with_the_layer_by_layer_forward(dev, row):
    """the plan itself against the table above (so the comparison cannot pass by fusing nothing), then every output of an
    inference pass with the fused launches on within 1.5e-2 relative l2 of the layer-by-layer pass, and the same for the
    locked prefix of a training step"""
    what = R.describe(row)
    b = R.synthetic_batch(row.B, row.H, row.W, seed=3, num_class=row.C)
    inner = {1, 3, 6, 8, 80, 81}          # (the leading layers of a fused group: their outputs are never written)
    # inference
    u, f = make_net(dev, row, training=False, seed=0), make_net(dev, row, training=False, seed=0)
    u.fuse_first_two = u.fuse_blocks = False
    assert sorted(u._fusion_plan(False, 1, u.score_layer)) == [], what
    plan = sorted(f._fusion_plan(False, 1, f.score_layer))
    assert plan == EXPECTED_INFER_PLAN[row.name], "%s: inference plan %s" % (what, plan)
    for n in (u, f):
        n.forward(b["images"], b["clip_window"], [DET_THRESH], is_training=False)
    torch.cuda.synchronize()
    worst = {}
    for lu, lf in zip(u.layers, f.layers):
        if lu.idx in inner and lu.idx in plan:
            continue
        worst[lu.idx] = rel_err(lf.act, lu.act)[0]
    bad = {i: v for i, v in worst.items() if not v < FUSED_PREFIX_BOUND}
    print("%s: inference plan %s, worst fused vs unfused %.3g" % (row.name, plan, max(worst.values())))
    assert not bad, "%s: fused inference outputs beyond %.1e of the layer-by-layer ones: %s" % (what, FUSED_PREFIX_BOUND, bad)
    # the training step's locked prefix
    tu, tf = make_net(dev, row), make_net(dev, row)
    tu.fuse_first_two = tu.fuse_blocks = False
    tplan = sorted(tf._fusion_plan(True, 1, tf.score_layer))
    assert tplan == EXPECTED_TRAIN_PLAN[row.name], "%s: training plan %s" % (what, tplan)
    assert sorted(tu._fusion_plan(True, 1, tu.score_layer)) == [], what
    bt, _ = R.row_batch(row)
    for n in (tu, tf):
        n.set_batch(bt)
        n.compute_losses(DET_THRESH)
    torch.cuda.synchronize()
    P = tf._backbone_prefix()
    tw = {l.idx: rel_err(tf.by_idx[l.idx].act, l.act)[0] for l in tu.layers if 2 <= l.idx <= P and not (l.idx in inner and l.idx in tplan)}
    bad = {i: v for i, v in tw.items() if not v < FUSED_PREFIX_BOUND}
    assert not bad, "%s: locked-prefix outputs of the fused step beyond %.1e of the layer-by-layer ones: %s" % (what, FUSED_PREFIX_BOUND, bad)
    if row is ANCHOR:
        assert tplan and max(tw.values()) > 0, "the anchor fused nothing"


# ------------------------------------------------------------------------------------------------ 4. inference
@pytest.mark.parametrize("row", ROWS, ids=R.ids(ROWS))
def test_inference_returns_the_oracle_detections_and_masks(dev, row):
    """detections == the oracle's filter on the net's own logits, masks == rect_ref.val_test on the net's own score maps (rtol
    1e-5, atol 1e-6), logits and score maps within 2e-2 relative l2 of the oracle forward, the graph replay == the eager call"""
    what = R.describe(row)
    B, H, W, C = row.B, row.H, row.W, row.C
    net = make_net(dev, row, training=False, seed=0)
    batch = R.synthetic_batch(B, H, W, seed=3, num_class=C)
    thr = 0.02
    preds, det, mask_pos = net.forward(batch["images"], batch["clip_window"], [thr], is_training=False)
    torch.cuda.synchronize()
    assert [tuple(p.shape) for p in preds] == [(B, H // d, W // d, 3, 5 + C) for d in (8, 16, 32)], what
    assert tuple(mask_pos.shape) == (B, H // row.m, W // row.m, row.k ** 2), what
    yq, mq = MR.build_network(oracle_params(net), batch["images"], False, R.lock_of_row(row), row.m, row.k, quant=O.bf16_ste)
    ratios = [rel_err(got, want)[0] / 2e-2 for got, want in list(zip(preds, yq)) + [(mask_pos, mq)]]
    pred = O.interpret_output([t.cpu() for t in preds])
    want = O.filter_detections(pred[2], pred[3], pred[5], batch["clip_window"], thr)
    got = det.cpu().numpy()
    ndet = int((want[:, :, 5] > 0).sum())
    print("%s: inference forward ratios %s, %d detections" % (row.name, ["%.3f" % r for r in ratios], ndet))
    assert max(ratios) < 1.0, "%s: forward differs from the oracle, ratios to 2e-2: %s" % (what, ratios)
    assert ndet >= B, "%s: fixture needs detections (got %d)" % (what, ndet)
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-6, err_msg=what)
    det_box, det_mask = net.evaluation(batch["images"], batch["clip_window"], [thr])
    torch.cuda.synchronize()
    score = net.by_idx[net.score_layer].act.cpu()
    assert torch.equal(score, mask_pos.cpu()), what
    wb, wm = R.val_test(net.detections.cpu().numpy(), score, row.k)
    assert any(np.ndim(w) for w in wm), "%s: test needs detections with a box of positive area" % what
    for i in range(B):
        np.testing.assert_array_equal(det_box[i], wb[i], err_msg=what)
        np.testing.assert_allclose(det_mask[i], wm[i], rtol=1e-5, atol=1e-6, err_msg=what)
    det_e, keep_e, masks_e = net.detections.clone(), net.keep.clone(), net.masks.clone()
    assert tuple(masks_e.shape) == (B, cfg.MAX_DETECTION, H // row.m, W // row.m), what
    net.build_infer_program(det_thresh=thr, graph=True)
    assert net._infer_graph is not None
    for _ in range(2):
        d, cnt, masks, keep = net.infer(batch["images"], batch["clip_window"])
    torch.cuda.synchronize()
    assert torch.equal(d, det_e) and torch.equal(keep, keep_e) and torch.equal(masks, masks_e), what


# ------------------------------------------------------------------------------------------------ 5. (64, 64) against 64
def test_a_pair_of_equal_sides_is_the_square_net(dev):
    """image_size=(64, 64) and image_size=64: a training step's arena and losses, an inference's detections and masks, bit for
    bit"""
    b = O.synthetic_batch(2, 64, seed=11)
    outs = []
    for size in (64, (64, 64)):
        net = YOLONet(training=True, device=dev, image_size=size, batch_size=2, stage=1, seed=1)
        perturb_variables(net, 1)
        net.refresh_weights()
        assert net.S == 64 and net.image_size == 64 and (net.H, net.W) == (64, 64)
        loss = net.train_step(b, det_thresh=DET_THRESH)
        torch.cuda.synchronize()
        inf = YOLONet(training=False, device=dev, image_size=size, batch_size=2, stage=1, seed=1)
        perturb_variables(inf, 1)
        inf.refresh_weights()
        inf.evaluation_device(b["images"], b["clip_window"], [0.02])
        torch.cuda.synchronize()
        outs.append((float(loss.cpu()), net.losses.cpu().clone(), float(net.mask_loss.cpu()[0]), net.arena.cpu().clone(),
                     net.grad_arena.cpu().clone(), inf.detections.cpu().clone(), inf.keep.cpu().clone(), inf.masks.cpu().clone()))
    a, c = outs
    assert np.isfinite(a[0]) and a[0] == c[0] and a[2] == c[2] and int(a[6].sum()) > 0
    for x, y in zip(a, c):
        if torch.is_tensor(x):
            assert torch.equal(x, y)


# ------------------------------------------------------------------------------------------------ 6. known answers, by hand
ANCH = np.asarray(cfg.ANCHORS, np.float32)


def test_decoded_box_of_one_cell_on_a_wide_net(dev):
    """64 x 128 net: coarse grid 2 x 4, fine grid 8 x 16.  One cell of the fine grid (y = 3, x = 9, anchor 0 = 31 x 23 pixels)
    carries logits (0, 0, 0, 0, +8, class 2 = +8), everything else has objectness -20.  Its decoded box by hand: xc =
    (9 + 0.5) / gw = 9.5 / 16, yc = (3 + 0.5) / gh = 3.5 / 8, w = a_w / net_w = 31 / 128, h = a_h / net_h = 23 / 64 -- inside
    the window, nothing is clipped.  A swap of gw / gh or net_w / net_h anywhere moves it."""
    B, H, W, C = 1, 64, 128, 3
    D = 5 + C
    lg = [torch.zeros(B, H // d, W // d, 3, D) for d in (8, 16, 32)]
    for t in lg:
        t[..., 4] = -20.0
    lg[0][0, 3, 9, 0, 4] = 8.0
    lg[0][0, 3, 9, 0, 5 + 2] = 8.0
    lg = [t.to(dev).contiguous() for t in lg]
    window = torch.tensor([[0.0, 0.0, 1.0, 1.0]], device=dev)
    det = torch.zeros(B, cfg.MAX_DETECTION, 6, device=dev)
    cnt = torch.zeros(B, dtype=torch.int32, device=dev)
    L.detect(lg[0], lg[1], lg[2], B, (H, W), C, ANCH.reshape(-1), window, 0.25, cfg.IOU_THRESHOLD, cfg.MAX_DETECTION, det, cnt,
             L.Workspace(dev))
    torch.cuda.synchronize()
    assert int(cnt[0]) == 1
    assert tuple(ANCH[0]) == (31.0, 23.0)      # the fine scale's anchors are the first three
    xc, yc, w, h = 9.5 / 16, 3.5 / 8, 31.0 / 128.0, 23.0 / 64.0
    want = [yc - h / 2, xc - w / 2, yc + h / 2, xc + w / 2]
    assert 0 < min(want) and max(want) < 1
    got = det[0, 0].cpu().numpy()
    np.testing.assert_allclose(got[:4], want, rtol=1e-5, atol=1e-6)
    assert got[4] == 2.0 and 0.9 < got[5] <= 1.0
    # the oracle's decode agrees
    pred = O.interpret_output([t.cpu() for t in lg])
    ref = O.filter_detections(pred[2], pred[3], pred[5], window.cpu().numpy(), 0.25)
    np.testing.assert_allclose(det.cpu().numpy(), ref, rtol=1e-5, atol=1e-6)


def _rois_of(dev, box_yxyx, Hm, Wm, k=3):
    """mask_rois on one image whose single ground-truth box is ``box_yxyx`` itself (IoU 1): the RoI row"""
    y1, x1, y2, x2 = box_yxyx
    tb = torch.zeros(1, cfg.MAX_BOX_PER_IMAGE, 5)
    tb[0, 0] = torch.tensor([(x1 + x2) / 2, (y1 + y2) / 2, x2 - x1, y2 - y1, 0.0])
    det = torch.zeros(1, cfg.MAX_DETECTION, 6)
    det[0, 0] = torch.tensor([y1, x1, y2, x2, 0.0, 0.9])
    rois = torch.zeros(1, L.ROI_MAX, L.roi_w(k), dtype=torch.int32, device=dev)
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    L.mask_rois(det.to(dev), cfg.MAX_DETECTION, tb.to(dev), cfg.MAX_BOX_PER_IMAGE, None, None, 1, (Hm, Wm), 1, 0, 0.5, rois, cnt, k=k)
    torch.cuda.synchronize()
    assert int(cnt[0]) == 1
    return rois[0, 0].cpu().numpy(), det.to(dev)


def test_roi_rounding_uses_each_axis_own_side(dev):
    """Hm = 32, Wm = 64 (a 64 x 128 net at m = 2).  y1 = 2.5 / 32 -> 2.5 -> 2 (half to even), x1 = 3.5 / 64 -> 3.5 -> 4,
    y2 = 20 / 32 -> 20, x2 = 40 / 64 -> 40.  With the one `size` of the square code y would be scaled by 64 or x by 32.
    k = 3 edges: y [2, round(2 + 6) = 8, round(2 + 12) = 14, 20], x [4, 16, 28, 40]; area = 18 * 36."""
    row, det = _rois_of(dev, (2.5 / 32, 3.5 / 64, 20.0 / 32, 40.0 / 64), 32, 64)
    assert list(row[:4]) == [2, 8, 14, 20] and list(row[4:8]) == [4, 16, 28, 40]
    assert row[8] == 0 and row[9] == 18 * 36 and row[10] == 1
    # the assembly: 0.5 outside the box, sigmoid(channel by * 3 + bx) inside, on a map whose channel c holds the value c
    score = torch.arange(9, dtype=torch.float32).repeat(1, 32, 64, 1).contiguous().to(dev)
    masks = torch.zeros(1, cfg.MAX_DETECTION, 32, 64, device=dev)
    keep = torch.zeros(1, cfg.MAX_DETECTION, dtype=torch.int32, device=dev)
    L.psroi_assemble(score, det, 1, cfg.MAX_DETECTION, (32, 64), 3, masks, keep)
    torch.cuda.synchronize()
    m = masks[0, 0].cpu().numpy()
    assert keep[0].cpu().tolist() == [1] + [0] * (cfg.MAX_DETECTION - 1)
    want = np.full((32, 64), 0.5, np.float32)
    ye, xe = [2, 8, 14, 20], [4, 16, 28, 40]
    for by in range(3):
        for bx in range(3):
            want[ye[by]:ye[by + 1], xe[bx]:xe[bx + 1]] = 1.0 / (1.0 + np.exp(-np.float32(by * 3 + bx)))
    np.testing.assert_allclose(m, want, rtol=1e-5, atol=1e-6)
    assert (m[:2] == 0.5).all() and (m[20:] == 0.5).all() and (m[:, :4] == 0.5).all() and (m[:, 40:] == 0.5).all()
    assert (masks[0, 1:] == 0).all()


def test_boxes_touching_the_far_edges(dev):
    """a box that touches the right edge of a wide map (Hm = 32, Wm = 64: x2 = 1.0 -> 64, past column 31 where a square 32-map
    ends) and one that touches the bottom edge of a tall map (Hm = 64, Wm = 32: y2 = 1.0 -> 64).  Areas are the pixel counts
    clipped to the map: the last bin ends at the map's own side."""
    row, _ = _rois_of(dev, (8.0 / 32, 40.0 / 64, 20.0 / 32, 1.0), 32, 64)
    assert list(row[:4]) == [8, 12, 16, 20] and list(row[4:8]) == [40, 48, 56, 64] and row[9] == 12 * 24
    row, _ = _rois_of(dev, (40.0 / 64, 8.0 / 32, 1.0, 20.0 / 32), 64, 32)
    assert list(row[:4]) == [40, 48, 56, 64] and list(row[4:8]) == [8, 12, 16, 20] and row[9] == 24 * 12
    # the mask loss of the wide one by hand: score 0 everywhere -> BCE = ln 2 on every pixel of the box whatever the ground
    # truth, mean over the area = ln 2, one RoI, one image: loss = MASK_SCALE * ln 2; its gradient is +-0.5 / area * scale
    rois = torch.zeros(1, L.ROI_MAX, L.roi_w(3), dtype=torch.int32, device=dev)
    r0, _ = _rois_of(dev, (8.0 / 32, 40.0 / 64, 20.0 / 32, 1.0), 32, 64)
    rois[0, 0] = torch.from_numpy(r0).to(dev)
    cnt = torch.ones(1, dtype=torch.int32, device=dev)
    score = torch.zeros(1, 32, 64, 9, device=dev)
    tm = torch.zeros(1, cfg.MAX_BOX_PER_IMAGE, 64, 128, dtype=torch.uint8, device=dev)
    tm[0, 0, :, 96:] = 1                         # ground truth set on the right quarter: columns >= 48 of the map
    dscore = torch.full((1, 32, 64, 32), float("nan"), dtype=torch.bfloat16, device=dev)
    loss = torch.zeros(1, device=dev)
    L.psroi_loss(score, tm, cfg.MAX_BOX_PER_IMAGE, rois, cnt, 1, (32, 64), 3, cfg.MASK_SCALE, dscore, loss, L.Workspace(dev),
                 mask_stride=2)
    torch.cuda.synchronize()
    np.testing.assert_allclose(float(loss[0]), cfg.MASK_SCALE * np.log(2.0), rtol=1e-5)
    g = dscore.float().cpu().numpy()[0]
    coef = cfg.MASK_SCALE * 0.5 / (12 * 24)
    want = np.zeros((32, 64, 32), np.float32)
    ye, xe = [8, 12, 16, 20], [40, 48, 56, 64]
    for by in range(3):
        for bx in range(3):
            want[ye[by]:ye[by + 1], xe[bx]:xe[bx + 1], by * 3 + bx] = coef if xe[bx] < 48 else -coef
    np.testing.assert_allclose(g, want, rtol=2.0 ** -8, atol=0)


def test_yolo_loss_targets_use_each_axis_own_side(dev):
    """64 x 128 net, one object in coarse cell (y = 1, x = 3), anchor 0, label box (xc, yc, w, h) normalised.  All logits 0.
    By hand: true_cxy = (xc * gw - 3, yc * gh - 1); true_twh = (log(w * net_w / a_w), log(h * net_h / a_h)); with
    sigmoid(0) = 0.5 and t_wh = 0 the xy term is ((0.5 - tcx)^2 + (0.5 - tcy)^2) * whs^2 * COORD and the wh term
    (ttw^2 + tth^2) * whs^2 * COORD, whs = 2 - w h."""
    B, H, W, C = 1, 64, 128, 3
    D = 5 + C
    lg = [torch.zeros(B, H // d, W // d, 3, D, device=dev) for d in (8, 16, 32)]
    lb = [torch.zeros(B, H // d, W // d, 3, D) for d in (8, 16, 32)]
    xc, yc, w, h = 0.90, 0.70, 0.30, 0.50
    lb[2][0, 1, 3, 0, :5] = torch.tensor([xc, yc, w, h, 1.0])
    lb[2][0, 1, 3, 0, 5 + 1] = 1.0
    tb = torch.zeros(B, cfg.MAX_BOX_PER_IMAGE, 5)
    tb[0, 0] = torch.tensor([xc, yc, w, h, 1.0])
    dl = [torch.zeros(B, H // d, W // d, L.GRAD_LD, dtype=torch.bfloat16, device=dev) for d in (8, 16, 32)]
    losses = torch.zeros(8, device=dev)
    scales = (cfg.OBJECT_SCALE, cfg.NOOBJECT_SCALE, cfg.CLASS_SCALE, cfg.COORD_SCALE)
    L.yolo_loss(lg, [t.to(dev) for t in lb], tb.to(dev), cfg.MAX_BOX_PER_IMAGE, B, (H, W), C, ANCH.reshape(-1), cfg.IGNORE_THRESH,
                scales, dl, losses, L.Workspace(dev))
    torch.cuda.synchronize()
    aw, ah = ANCH[6]
    tcx, tcy = xc * 4 - 3, yc * 2 - 1
    ttw, tth = np.log(w * 128 / aw), np.log(h * 64 / ah)
    whs2 = (2 - w * h) ** 2 * cfg.COORD_SCALE
    got = losses.cpu().numpy()
    np.testing.assert_allclose(got[3], ((0.5 - tcx) ** 2 + (0.5 - tcy) ** 2) * whs2, rtol=2e-5)
    np.testing.assert_allclose(got[4], (ttw ** 2 + tth ** 2) * whs2, rtol=2e-5)
    # ... and the oracle on the same tensors
    pred = O.interpret_output([t.cpu().double() for t in lg])
    want = O.loss_yolo(pred, tb.double().view(B, 1, 1, 1, -1, 5), [t.double() for t in lb])
    for i, n in enumerate(("obj", "noobj", "class", "xy", "wh")):
        np.testing.assert_allclose(got[i], float(want[n]), rtol=2e-5, err_msg=n)


def test_argument_errors_of_the_rectangular_entry_points(dev):
    lib = L.load()
    assert lib.disyolo_detect_workspace_hw(2, 64, 100, 3) == 0 and lib.disyolo_detect_workspace_hw(2, 0, 64, 3) == 0
    assert lib.disyolo_detect_workspace_hw(2, 64, 64, 3) == lib.disyolo_detect_workspace(2, 64, 3)
    assert lib.disyolo_yolo_loss_workspace_hw(2, 96, 96, 3) == lib.disyolo_yolo_loss_workspace(2, 96, 3)
    assert lib.disyolo_psroi_loss_workspace_hw(2, 32, 32) == lib.disyolo_psroi_loss_workspace(2, 32)
    assert lib.disyolo_psroi_loss_workspace_hw(2, 0, 32) == 0
    t = torch.zeros(64, device=dev)
    with pytest.raises(L.DisyoloError, match="bad sizes"):
        L.detect(t, t, t, 1, (64, 80), 3, ANCH.reshape(-1), t, 0.1, 0.3, 30, t, t, L.Workspace(dev))


# ------------------------------------------------------------------------------------------------ 7. drivers
@pytest.mark.parametrize("net_hw", [(64, 128), (128, 64)])
@pytest.mark.parametrize("flip", [1, 2, 3])
def test_augmentation_kernels_on_a_rectangular_frame(dev, net_hw, flip):
    """tests/test_gpu_train_data.py's placement and photometric checks (bit for bit) on frames of 64 x 128 and 128 x 64:
    placements that pad, crop and overhang each side, the flips about the frame's own width / height, salt-and-pepper with
    rows up to net_h - 2 and columns up to net_w - 2, the light change, the 3 x 3 motion blur with its 255 border"""
    nh, nw = net_hw
    rng = np.random.RandomState(nh + flip)
    for (H, W, _, new_w, new_h, dx, dy) in PLACE + [(40, 50, 0, nw, nh, 0, 0), (30, 90, 0, nw + 20, nh // 2, -9, nh // 4)]:
        img = rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
        out = torch.zeros(nh, nw, 3, dtype=torch.uint8, device=dev)
        L.aug_place(torch.from_numpy(img).to(dev), False, out, (nh, nw), new_w, new_h, dx, dy, flip)
        mask = (rng.rand(H, W) < 0.4).astype(np.uint8)
        mout = torch.zeros(nh, nw, dtype=torch.uint8, device=dev)
        L.aug_place(torch.from_numpy(mask).to(dev), True, mout, (nh, nw), new_w, new_h, dx, dy, flip)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(out.cpu().numpy(), R.place_image(img, nh, nw, new_w, new_h, dx, dy, flip))
        np.testing.assert_array_equal(mout.cpu().numpy().astype(bool), R.place_mask(mask, nh, nw, new_w, new_h, dx, dy, flip))
    if flip != 1:
        return
    img = rng.randint(0, 256, (nh, nw, 3)).astype(np.uint8)
    d = torch.from_numpy(img).to(dev)
    for coeff in (0.5, 1.31):
        x = d.clone()
        L.aug_change_light(x, (nh, nw), coeff)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(x.cpu().numpy(), O.change_light(img, coeff))
    for angle in (0, 45, 90, 135):
        for lt in (0, 1, 2):
            y = torch.zeros_like(d)
            L.aug_motion_blur3(d, y, (nh, nw), angle, lt)
            torch.cuda.synchronize()
            np.testing.assert_array_equal(y.cpu().numpy(), R.motion_blur3(img, angle, lt), err_msg="%d %d" % (angle, lt))
    ns, npp = 40, 90
    rows, cols = rng.randint(0, nh - 1, ns + npp), rng.randint(0, nw - 1, ns + npp)
    rows[0], cols[0], rows[1], cols[1] = nh - 2, nw - 2, 0, nw - 2          # the far corner of the draw's range on both axes
    rows[ns], cols[ns] = rows[0], cols[0]                                   # a pepper on a salt: pepper wins
    x = d.clone()
    L.aug_salt_pepper(x, (nh, nw), torch.from_numpy(rows.astype(np.int32)).to(dev), torch.from_numpy(cols.astype(np.int32)).to(dev), ns, npp)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(x.cpu().numpy(), O.salt_pepper(img, rows, cols, ns))


def _sized_labels(rng, sizes):
    """tests/test_gpu_train_data.py::_labels with the image sizes given: ellipse-like polygons, the first with a hole"""
    out = []
    for (h, w) in sizes:
        image = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
        polys, names = [], []
        for j in range(rng.randint(1, 4)):
            cy, cx = rng.uniform(0.3, 0.7) * h, rng.uniform(0.3, 0.7) * w
            ry, rx = rng.uniform(0.08, 0.22) * h, rng.uniform(0.08, 0.22) * w
            t = np.sort(rng.uniform(0, 2 * np.pi, rng.randint(5, 9)))
            inst = [{"type": "out", "all_points_x": np.clip(cx + rx * np.cos(t), 0, w - 1).astype(int).tolist(),
                     "all_points_y": np.clip(cy + ry * np.sin(t), 0, h - 1).astype(int).tolist()}]
            if j == 0:
                inst.append({"type": "in", "all_points_x": [int(cx - 2), int(cx + 2), int(cx)], "all_points_y": [int(cy - 2), int(cy - 2), int(cy + 2)]})
            polys.append(inst)
            names.append(cfg.CLASSES[rng.randint(0, 3)])
        out.append({"image": image, "class_names": names, "polygons": polys})
    return out


def test_defect_train_on_a_rectangular_net_replayed_by_the_reference_side(dev):
    """defect_train(image_size=(64, 128)) against rect_ref.loader_sample on a RandomState of the same seed: every decision
    (fit, placement, flip, photometric draw), the boxes and the three target grids equal the restatement's, and the pixels
    equal the restatement's placement / photometric functions bit for bit, as
    tests/test_gpu_train_data.py::test_defect_train_get_replayed_by_the_oracle does at S = 96.  Every augmentation branch is
    drawn at least once; labels of both orientations make either side bind the fit."""
    NH, NW, B = 64, 128, 4
    labels = _sized_labels(np.random.RandomState(2), [(120, 130), (70, 220), (200, 90), (100, 260), (150, 150)])
    data = TD.defect_train(labels, batch_size=B, image_size=(NH, NW), device=dev, rng=np.random.RandomState(123))
    assert data.image_size == (NH, NW) and (data.net_h, data.net_w) == (NH, NW)
    ref_rng = np.random.RandomState(123)
    ref_labels = list(labels)
    ref_rng.shuffle(ref_labels)
    cursor = 0
    seen = {"scale": set(), "flip": set(), "bnl": set(), "bind": set()}
    for it in range(8):
        images, masks, tboxes, y3, y2, y1, window = data.get()
        torch.cuda.synchronize()
        assert images.shape == (B, NH, NW, 3) and masks.shape == (B, cfg.MAX_BOX_PER_IMAGE, NH, NW) and masks.dtype == torch.bool
        assert y3.shape == (B, NH // 8, NW // 8, 3, 8) and y1.shape == (B, NH // 32, NW // 32, 3, 8) and (window == [0, 0, 1, 1]).all()
        for b in range(B):
            lab = ref_labels[cursor]
            h, w = lab["image"].shape[:2]
            inst = [O.instance_mask(p, h, w) for p in lab["polygons"]]
            boxes = []
            for m in inst:
                rr, cc = np.where(m)
                boxes.append([cc.min(), rr.min(), cc.max() + 1, rr.max() + 1])
            cls = [cfg.CLASSES.index(n) for n in lab["class_names"]]
            dec, want_boxes, want_ys = R.loader_sample(ref_rng, h, w, np.asarray(boxes, np.float32), cls, NH, NW)
            got = data.last_decisions[b]
            for key in ("scale_crop", "new_w", "new_h", "dx", "dy", "flip", "bnl"):
                assert got[key] == dec[key], (it, b, key, got, dec)
            seen["scale"].add(dec["scale_crop"]); seen["flip"].add(dec["flip"]); seen["bnl"].add(dec["bnl"])
            seen["bind"].add("h" if w / h < NW / NH else "w")
            n = len(inst)
            np.testing.assert_array_equal(tboxes[b, 0, 0, 0, :n, :4], want_boxes)
            np.testing.assert_array_equal(tboxes[b, 0, 0, 0, :n, 4], np.asarray(cls, np.float32))
            assert (tboxes[b, 0, 0, 0, n:] == 0).all() and not masks[b, n:].any()
            for g_, w_ in zip((y3, y2, y1), want_ys):
                np.testing.assert_array_equal(g_[b], w_)
            assert sum(int((g_[b, ..., 4] == 1).sum()) for g_ in (y3, y2, y1)) >= 1
            img = R.place_image(lab["image"], NH, NW, dec["new_w"], dec["new_h"], dec["dx"], dec["dy"], dec["flip"])
            if dec["bnl"] == 2:
                for k in (0, 1):
                    np.testing.assert_array_equal(got["salt"][k], dec["salt"][k])
                    np.testing.assert_array_equal(got["pepper"][k], dec["pepper"][k])
                assert dec["salt"][0].max() <= NH - 2 and dec["salt"][1].max() <= NW - 2 and dec["pepper"][1].max() > NH
                rows = np.concatenate([dec["salt"][0], dec["pepper"][0]]); cols = np.concatenate([dec["salt"][1], dec["pepper"][1]])
                img = O.salt_pepper(img, rows, cols, len(dec["salt"][0]))
            elif dec["bnl"] == 3:
                assert got["coeff"] == dec["coeff"]
                img = O.change_light(img, dec["coeff"])
            elif dec["bnl"] == 4:
                assert (got["angle"], got["line_type"]) == (dec["angle"], dec["line_type"])
                img = R.motion_blur3(img, dec["angle"], {"right": 1, "left": 2, "full": 0}[dec["line_type"]])
            np.testing.assert_array_equal(images[b].cpu().numpy(), img.astype(np.float32) / 255.0)
            for j in range(n):
                m = R.place_mask(inst[j].astype(np.float32), NH, NW, dec["new_w"], dec["new_h"], dec["dx"], dec["dy"], dec["flip"])
                np.testing.assert_array_equal(masks[b, j].cpu().numpy(), m)
            cursor += 1
            if cursor >= len(ref_labels):
                ref_rng.shuffle(ref_labels)
                cursor = 0
    assert seen["scale"] == {1, 2} and seen["flip"] == {1, 2, 3} and seen["bnl"] == {1, 2, 3, 4} and seen["bind"] == {"h", "w"}
    # the batch feeds a rectangular net as it is
    net = YOLONet(training=True, device=dev, image_size=(NH, NW), batch_size=B, stage=1, seed=0)
    loss = net.train_step(data.get_device(), det_thresh=DET_THRESH)
    assert np.isfinite(float(loss.cpu())) or int(net.roi_count.sum()) == 0


@pytest.mark.parametrize("net_hw", [(64, 128), (128, 64), (96, 160)])
def test_rectangular_letterbox_matches_the_reference_side(dev, net_hw):
    """E.image_read into a rectangular net against rect_ref.image_read; images whose width binds, whose height binds, and one
    of the net's own aspect.  Bit for bit, like tests/test_gpu_drivers.py::test_image_read_matches_oracle_bit_for_bit"""
    nh, nw = net_hw
    rng = np.random.RandomState(5)
    for (h, w) in [(35, 62), (60, 80), (45, 39), (nh // 2, nw // 2), (nh * 2, nw * 2 + 2)]:
        rgb = rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
        got, win = E.image_read(rgb, (nh, nw), dev)
        torch.cuda.synchronize()
        want, wwin = R.image_read(rgb, nh, nw)
        assert tuple(got.shape) == (nh, nw, 3)
        assert np.array_equal(win, wwin), (h, w, win, wwin)
        np.testing.assert_array_equal(got.cpu().numpy(), want)


def _ground_truth(shapes, seed, C):
    """tests/test_gpu_class_list.py::class_ground_truth (instances from a synthetic batch, cut to the image)"""
    rng = np.random.RandomState(seed)
    images, recs, sizes, merged, index = {}, {}, {}, {}, []
    for k, (h, w) in enumerate(shapes):
        name = "img%03d" % k
        index.append(name)
        images[name] = rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
        sizes[name] = [h, w]
        batch = synthetic_batch(1, (max(h, w) + 31) // 32 * 32, seed=seed + k, num_class=C)
        objs, mm = [], np.zeros((h, w), np.uint8)
        for j in range(batch["true_masks"].shape[1]):
            m = batch["true_masks"][0, j][:h, :w]
            if m.any():
                c = int(batch["true_boxes"][0, 0, 0, 0, j, 4])
                objs.append({"imageid": name, "classid": c, "difficult": 0, "mask": m.copy()})
                mm[m] = c + 1
        recs[name], merged[name] = objs, mm
    return images, recs, sizes, merged, index


def test_paste_matches_the_reference_side_on_a_rectangular_net(dev):
    """postprocess.paste_detections with the net's two sides against rect_ref.paste_detections on the same detections"""
    row = [r for r in ROWS if "map" in r.extras][0]
    net = YOLONet(training=False, device=dev, stage=1, seed=0, **dict(R.net_kwargs(row), batch_size=1, lock=None))
    randomize_heads(net, 7)
    rng = np.random.RandomState(3)
    npasted = 0
    for (h, w) in [(70, 120), (100, 60)]:
        rgb = rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
        frame, window = E.image_read(rgb, (row.H, row.W), dev)
        det_box, det_mask = net.evaluation(frame[None], window[None], [np.float32(0.05)], masks_on_device=True)
        assert torch.is_tensor(det_mask[0]) and tuple(det_mask[0].shape[1:]) == (row.H // row.m, row.W // row.m)
        entries, merged = paste_detections(det_box[0], det_mask[0], h, w, (row.H, row.W))
        want_e, want_m = R.paste_detections(np.asarray(det_box[0]), det_mask[0].cpu().numpy(), h, w, row.H, row.W)
        assert [e["index"] for e in entries] == [e["index"] for e in want_e]
        np.testing.assert_array_equal(merged.cpu().numpy(), want_m)
        for e, we in zip(entries, want_e):
            np.testing.assert_array_equal(e["mask"].cpu().numpy(), we["mask"])
        npasted += len(entries)
    assert npasted >= 4, "fixture needs pasted detections"


def test_evaluate_end_to_end_on_a_rectangular_net(dev):
    """evaluate() on the C = 6 row (96 x 160, k = 5, m = 4, B = 3: the batched test loop) with non-square images: the AP table
    and the mIoU equal the per-image loop of the reference side (rect_ref.paste_detections + voc_eval + numpy confusion counts)
    on the same detections, as tests/test_gpu_class_list.py::check_evaluate_with_a_6_class_map does for a square net"""
    row = [r for r in ROWS if "map" in r.extras][0]
    C, thr, B = row.C, 0.05, row.B
    assert C == 6
    net = YOLONet(training=False, device=dev, stage=1, seed=0, **dict(R.net_kwargs(row), lock=None))
    randomize_heads(net, 7)
    images, recs, sizes, merged, index = _ground_truth([(70, 120), (96, 96), (100, 60)], 33, C)
    emap = E.MAP(recs, sizes, index, merged, net_size=(row.H, row.W), classes=R.names(C))
    thresh_out, mask_acc, _ = E.evaluate(net, images, emap, det_thresh=thr)
    assert len(thresh_out) == 1 and len(thresh_out[0]["AP"]) == C and len(mask_acc) == C + 2
    frame = torch.zeros(B, row.H, row.W, 3, dtype=torch.float32, device=dev)
    windows = np.stack([E.image_read(images[n], (row.H, row.W), dev, out=frame[i])[1] for i, n in enumerate(index)])
    for i, n in enumerate(index):
        assert np.array_equal(windows[i], R.letterbox_window(sizes[n][0], sizes[n][1], row.H, row.W))
    det_box, det_mask = net.evaluation(frame, windows, [np.float32(thr)])
    detfile = {str(c): [] for c in range(C)}
    conf = np.zeros((C + 1, C + 1), np.int64)
    ndet = 0
    for i, n in enumerate(index):
        h, w = sizes[n]
        entries, mm = R.paste_detections(np.asarray(det_box[i]), det_mask[i], h, w, row.H, row.W)
        ndet += len(entries)
        for e in entries:
            detfile[str(e["classid"])].append({"imageid": n, "score": e["score"], "mask": e["mask"]})
        conf += np.bincount(merged[n].astype(np.int64).ravel() * (C + 1) + mm.astype(np.int64).ravel(),
                            minlength=(C + 1) ** 2).reshape(C + 1, C + 1)
    assert ndet >= 10 and len({c for c in detfile if detfile[c]}) >= 3, "fixture needs detections of several classes"
    res, pres, aps = [], [], []
    for c in range(C):
        if not detfile[str(c)]:
            r, p, a = 0.0, 0.0, 0.0
        else:
            r, p, a = voc_eval(detfile[str(c)], recs, index, c, ovthresh=0.5, use_07_metric=False)
        res, pres, aps = res + [r], pres + [p], aps + [a]
    print("rect evaluate: %d detections, AP %s" % (ndet, json.dumps(aps)))
    assert repr(thresh_out[0]["AP"]) == repr(aps)
    assert repr(thresh_out[0]["mAP"]) == repr([float(np.mean(res)), float(np.mean(pres)), float(np.mean(aps))])
    cf = conf.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        ious = [cf[k, k] / (cf[k].sum() + cf[:, k].sum() - cf[k, k]) for k in range(C + 1)]
    np.testing.assert_array_equal(np.asarray(mask_acc[:-1]), np.asarray(ious))
    np.testing.assert_array_equal(mask_acc[-1], float(np.mean(ious)))

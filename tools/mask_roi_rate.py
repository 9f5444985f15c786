"""What the mask loss's RoI counts cost at B = 8, 576^2, m = 1/2, k = 3, by HIP events:

    python tools/mask_roi_rate.py [--batch 8] [--size 576] [--steps 0] [--json F] [--txt F]

* the RoI selection and the mask loss per call on dense tables -- every detection is a ground-truth box moved by a hair, so
  every RoI is positive -- at (mask_roi_det, mask_roi_gt) = (7, 3) and (8, 8) through the entry points of the 16-row table,
  (9, 8), (30, 20), (100, 100) and (256, 256) through the _x forms, and (8, 8) through the _x forms on a 16-row table beside
  the narrow ones.  The launches are replayed from a recorded command list back to back over rotating inputs (as in
  tools/limits_rate.py), so a figure includes the gap between two launches; the loss is three launches a call;
* with --steps N: the pipelined stage-1 training step (bench.py's step) over N steps, three regions, with the default counts,
  with (30, 20), and with (256, 256) on a net of 256 boxes and 256 detections."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import disyolo_amd  # noqa: E402,F401
from disyolo_amd import config as cfg  # noqa: E402
from disyolo_amd import lib as L  # noqa: E402

NB = 4          # rotating buffers


def replay_us(record, calls, repeats=7):
    prog = L.CmdList()
    with prog:
        record()
    prog.run()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        prog.run()
        e.record()
        torch.cuda.synchronize()
        ts.append(s.elapsed_time(e) * 1e3 / calls)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def dense_tables(dev, B, D, G, seed):
    """NB sets of (detections, true_boxes, perm_det, perm_gt): every row filled, every detection on a box"""
    rng = np.random.RandomState(seed)
    tabs = []
    for _ in range(NB):
        tb = np.zeros((B, G, 5), np.float32)
        wh = rng.uniform(0.05, 0.4, size=(B, G, 2))
        tb[..., 2:4] = wh
        tb[..., 0:2] = rng.uniform(wh / 2, 1 - wh / 2)
        det = np.zeros((B, D, 6), np.float32)
        src = tb[np.arange(B)[:, None], rng.randint(0, G, size=(B, D))]
        j = (rng.rand(B, D, 4) - 0.5) * 0.002
        det[..., 0], det[..., 1] = src[..., 1] - src[..., 3] / 2 + j[..., 0], src[..., 0] - src[..., 2] / 2 + j[..., 1]
        det[..., 2], det[..., 3] = src[..., 1] + src[..., 3] / 2 + j[..., 2], src[..., 0] + src[..., 2] / 2 + j[..., 3]
        det[..., 5] = 0.9
        pd = np.stack([rng.permutation(D) for _ in range(B)]).astype(np.int32)
        pg = np.stack([rng.permutation(G) for _ in range(B)]).astype(np.int32)
        tabs.append([torch.from_numpy(a).to(dev).contiguous() for a in (det, tb, pd, pg)])
    return tabs


def pair_rate(dev, B, S, n_det, n_gt, D, G, wide, k=3, st=2):
    Sm = S // st
    cap = (n_det + n_gt if n_det + n_gt > L.ROI_MAX else L.ROI_MAX)
    tabs = dense_tables(dev, B, D, G, 10 * n_det + n_gt)
    rois = [torch.zeros(B, cap, L.roi_w(k), dtype=torch.int32, device=dev) for _ in range(NB)]
    cnt = [torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(NB)]
    sel, loss_fn = (L.mask_rois_x, L.psroi_loss_x) if wide else (L.mask_rois, L.psroi_loss)
    reps = 10

    def record_sel():
        for _ in range(reps):
            for i, (det, tb, pd, pg) in enumerate(tabs):
                sel(det, D, tb, G, pd, pg, B, Sm, n_det, n_gt, cfg.MASK_ROI_IOU, rois[i], cnt[i], k=k)

    s_us, s_lo, s_hi = replay_us(record_sel, reps * NB)
    g = torch.Generator(device=dev).manual_seed(n_det + n_gt)
    score = [torch.randn(B, Sm, Sm, k * k, device=dev, generator=g) for _ in range(NB)]
    dscore = [torch.zeros(B, Sm, Sm, 32, dtype=torch.bfloat16, device=dev) for _ in range(NB)]
    tm = (torch.rand(B, G, S, S, device=dev, generator=g) < 0.5).to(torch.uint8)
    out = torch.zeros(1, device=dev)
    ws = L.Workspace(dev)
    ws.get(L.psroi_loss_workspace_x(B, Sm, cap))
    reps = 5

    def record_loss():
        for _ in range(reps):
            for i in range(NB):
                loss_fn(score[i], tm, G, rois[i], cnt[i], B, Sm, k, cfg.MASK_SCALE, dscore[i], out, ws, mask_stride=st)

    l_us, l_lo, l_hi = replay_us(record_loss, reps * NB)
    return {"n_det": n_det, "n_gt": n_gt, "max_det": D, "G": G, "form": "x" if wide else "narrow", "table_rows": cap,
            "positives_per_image": round(float(torch.stack(cnt).float().mean()), 1),
            "select_us": round(s_us, 2), "select_min_max": [round(s_lo, 2), round(s_hi, 2)],
            "loss_us": round(l_us, 2), "loss_min_max": [round(l_lo, 2), round(l_hi, 2)],
            "workspace_MB": round(L.psroi_loss_workspace_x(B, Sm, cap) / 1e6, 2), "loss": round(float(out), 4)}


def step_rate(dev, B, S, steps, label, **kw):
    """bench.py's pipelined stage-1 step: ms per step, median of three regions"""
    from disyolo_amd.net import YOLONet
    from disyolo_amd.synth import synthetic_batch
    net = YOLONet(training=True, device=dev, image_size=S, batch_size=B, stage=1, seed=0, **kw)
    net.set_batch(synthetic_batch(B, S, seed=1234, max_box_per_image=net.max_box_per_image))
    net.shuffle_seed = 1234
    net.build_program(pipeline_backbone=True)
    net.prime_pipeline()
    for _ in range(5):
        net.train_step(None, want_loss=False)
    torch.cuda.synchronize()
    regions = []
    for _ in range(3):
        t0 = time.perf_counter()
        for _ in range(steps):
            net.train_step(None, want_loss=False)
        torch.cuda.synchronize()
        regions.append((time.perf_counter() - t0) * 1e3 / steps)
    return {"step": label, "B": B, "S": S, "mask_roi_det": net.mask_roi_det, "mask_roi_gt": net.mask_roi_gt,
            "G": net.max_box_per_image, "max_det": net.max_detection, "ms_per_step": round(float(np.median(regions)), 3),
            "regions_ms": [round(r, 3) for r in regions], "img_per_s": round(B * 1e3 / float(np.median(regions)), 1),
            "positives_last_step": net.roi_count.cpu().tolist(), "loss": round(float(net.total_loss().cpu()), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=576)
    ap.add_argument("--steps", type=int, default=0, help="also time the training step over this many steps per region")
    ap.add_argument("--json", default=None)
    ap.add_argument("--txt", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, S = args.batch, args.size
    out = []
    for n_det, n_gt, D, G, wide in ((7, 3, 30, 20, False), (8, 8, 30, 20, False), (8, 8, 30, 20, True), (9, 8, 30, 20, True),
                                    (30, 20, 30, 20, True), (100, 100, 100, 100, True), (256, 256, 256, 256, True)):
        out.append(pair_rate(dev, B, S, n_det, n_gt, D, G, wide))
        print(json.dumps(out[-1]), flush=True)
    if args.steps > 0:
        for label, kw in (("defaults", {}), ("30+20", dict(mask_roi_det=30, mask_roi_gt=20)),
                          ("256+256, G = D = 256", dict(mask_roi_det=256, mask_roi_gt=256, max_box_per_image=256, max_detection=256))):
            out.append(step_rate(dev, B, S, args.steps, label, **kw))
            print(json.dumps(out[-1]), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    if args.txt:
        with open(args.txt, "w") as f:
            f.write("tools/mask_roi_rate.py --batch %d --size %d --steps %d (HIP events, replayed command lists, median of 7)\n"
                    % (B, S, args.steps))
            for r in out:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()

"""What the per-image limits cost at B = 8, 576^2, by HIP events:

    python tools/limits_rate.py [--batch 8] [--size 576] [--json F] [--txt F]

* the detection filter per call at max_detection = 30 / 100 / 256 for 3 and 80 classes, in the three NMS modes, on random
  logits (an untrained net: thousands of candidates above the threshold) over rotating logit buffers.  30 takes the entry
  point and the kernel instances of before, 100 and 256 disyolo_detect_x (256 winners per list; at 3 classes x 256 rows the
  k-way merge instead of the LDS rank merge);
* the mask-loss RoI selection at (max_detection, max_box_per_image) = (30, 20) -- one lane walks the rows -- and (256, 256)
  with every row filled -- ballots and a lane-parallel IoU arg-max -- on rotating tables.

The launches are replayed from a recorded command list back to back (as in tools/class_list_rate.py), so a figure includes
the gap between two launches."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import disyolo_amd  # noqa: E402,F401
from disyolo_amd import config as cfg  # noqa: E402
from disyolo_amd import lib as L  # noqa: E402

ANCH = np.asarray(cfg.ANCHORS, np.float32).reshape(-1)
NB = 4          # rotating buffers


def replay_us(record, launches, repeats=7):
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
        ts.append(s.elapsed_time(e) * 1e3 / launches)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def detect_rate(dev, B, S, C, D, mode):
    g = torch.Generator(device=dev).manual_seed(100 + C)
    grids = (S // 8, S // 16, S // 32)
    lg = [[torch.randn(B, gs, gs, 3 * (5 + C), device=dev, generator=g) for gs in grids] for _ in range(NB)]
    win = torch.tensor([[0.0, 0.0, 1.0, 1.0]] * B, device=dev)
    det = torch.zeros(B, D, 6, device=dev)
    cnt = torch.zeros(B, dtype=torch.int32, device=dev)
    ws = L.Workspace(dev)
    reps = 3

    def record():
        for _ in range(reps):
            for i in range(NB):
                L.detect(lg[i][0], lg[i][1], lg[i][2], B, S, C, ANCH, win, cfg.OBJ_THRESHOLD, cfg.IOU_THRESHOLD, D, det, cnt, ws,
                         nms=mode)

    us, lo, hi = replay_us(record, reps * NB)
    return {"kernel": "detect", "entry": "disyolo_detect_x" if D > 64 else "disyolo_detect_nms_hw", "nms": mode, "B": B, "S": S,
            "C": C, "max_det": D, "us_per_call": round(us, 1), "min": round(lo, 1), "max": round(hi, 1),
            "workspace_MB": round(L.detect_workspace(B, S, C, D) / 1e6, 1), "rows_last_call": int(cnt.sum())}


def rois_rate(dev, B, D, G, Sm, k=3):
    rng = np.random.RandomState(D + G)
    tabs = []
    for _ in range(NB):
        tb = np.zeros((B, G, 5), np.float32)
        wh = rng.uniform(0.05, 0.4, size=(B, G, 2))
        tb[..., 2:4] = wh
        tb[..., 0:2] = rng.uniform(wh / 2, 1 - wh / 2)
        det = np.zeros((B, D, 6), np.float32)
        src = tb[np.arange(B)[:, None], rng.randint(0, G, size=(B, D))]
        j = (rng.rand(B, D, 4) - 0.5) * 0.04
        det[..., 0], det[..., 1] = src[..., 1] - src[..., 3] / 2 + j[..., 0], src[..., 0] - src[..., 2] / 2 + j[..., 1]
        det[..., 2], det[..., 3] = src[..., 1] + src[..., 3] / 2 + j[..., 2], src[..., 0] + src[..., 2] / 2 + j[..., 3]
        det[..., 5] = 0.9
        pd = np.stack([rng.permutation(D) for _ in range(B)]).astype(np.int32)
        pg = np.stack([rng.permutation(G) for _ in range(B)]).astype(np.int32)
        tabs.append([torch.from_numpy(a).to(dev).contiguous() for a in (det, tb, pd, pg)])
    rois = torch.zeros(B, L.ROI_MAX, L.roi_w(k), dtype=torch.int32, device=dev)
    cnt = torch.zeros(B, dtype=torch.int32, device=dev)
    reps = 10

    def record():
        for _ in range(reps):
            for det, tb, pd, pg in tabs:
                L.mask_rois(det, D, tb, G, pd, pg, B, Sm, cfg.MASK_ROI_DET, cfg.MASK_ROI_GT, cfg.MASK_ROI_IOU, rois, cnt, k=k)

    us, lo, hi = replay_us(record, reps * NB)
    return {"kernel": "mask_rois", "form": "wave" if max(D, G) > 64 else "one lane", "B": B, "max_det": D, "G": G, "map": Sm,
            "us_per_call": round(us, 2), "min": round(lo, 2), "max": round(hi, 2), "rois_last_call": int(cnt.sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=576)
    ap.add_argument("--json", default=None)
    ap.add_argument("--txt", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, S = args.batch, args.size
    out = []
    for C in (3, 80):
        for mode in ("per_class", "agnostic", "none"):
            for D in (30, 100, 256):
                out.append(detect_rate(dev, B, S, C, D, mode))
                print(json.dumps(out[-1]), flush=True)
    for D, G in ((30, 20), (256, 256)):
        out.append(rois_rate(dev, B, D, G, S // cfg.MASK_STRIDE))
        print(json.dumps(out[-1]), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    if args.txt:
        with open(args.txt, "w") as f:
            f.write("tools/limits_rate.py --batch %d --size %d (HIP events, replayed command lists, median of 7)\n" % (B, S))
            for r in out:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()

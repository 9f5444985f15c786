"""What the kernels of wide class lists cost at B = 8, 576^2, by HIP events:

    python tools/class_list_rate.py [--batch 8] [--size 576] [--json F]

* disyolo_yolo_loss_wide at C = 80 (pitch 256) over rotating buffers, against its byte bound -- logits and labels read once
  (2 x 55.5 MB), the bf16 gradient rows written once (27.9 MB) -- and the 6.3 TB/s copy rate of the card; the 32-channel
  disyolo_yolo_loss at C = 3 beside it;
* disyolo_detect on random logits: the bucketed path at C = 80 and at C = 17, the block-per-(image, class) path at C = 16 on
  the same box, and what that path would need at C = 80 -- EXTRAPOLATED from its C = 16 and C = 8 times (its blocks each
  sweep all candidates of their image, so its time grows with the class count; it cannot run at C = 80).

The launches are replayed from a recorded command list back to back (as in tools/lock_map_rate.py), so a figure includes the
gap between two launches."""
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
from disyolo_amd.synth import synthetic_batch  # noqa: E402

COPY_RATE = 6.3e12
ANCH = np.asarray(cfg.ANCHORS, np.float32).reshape(-1)


def replay_us(record, launches, repeats=5):
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
    return float(np.median(ts)), prog


def loss_rate(dev, B, S, C, wide):
    NB = 6 if wide else 12                    # rotating buffers: more bytes than the last-level cache holds
    ld = (3 * (5 + C) + 31) // 32 * 32
    batch = synthetic_batch(B, S, seed=1234, num_class=C)
    g = torch.Generator(device=dev).manual_seed(C)
    grids = (S // 8, S // 16, S // 32)
    lg = [[torch.randn(B, gs, gs, 3, 5 + C, device=dev, generator=g) for gs in grids] for _ in range(NB)]
    lb = [[torch.as_tensor(batch[k]).to(dev).float().contiguous() for k in ("yolo3", "yolo2", "yolo1")] for _ in range(NB)]
    dl = [[torch.empty(B, gs, gs, ld, dtype=torch.bfloat16, device=dev) for gs in grids] for _ in range(NB)]
    tb = torch.as_tensor(batch["true_boxes"]).to(dev).float().reshape(B, -1, 5).contiguous()
    losses = torch.zeros(8, device=dev)
    ws = L.Workspace(dev)
    scales = (cfg.OBJECT_SCALE, cfg.NOOBJECT_SCALE, cfg.CLASS_SCALE, cfg.COORD_SCALE)
    reps = 4

    def record():
        for _ in range(reps):
            for i in range(NB):
                if wide:
                    L.yolo_loss_wide(lg[i], lb[i], tb, tb.shape[1], B, S, C, ld, ANCH, cfg.IGNORE_THRESH, scales, dl[i], losses, ws)
                else:
                    L.yolo_loss(lg[i], lb[i], tb, tb.shape[1], B, S, C, ANCH, cfg.IGNORE_THRESH, scales, dl[i], losses, ws)

    us, _prog = replay_us(record, reps * NB)
    rows = B * 3 * sum(gs * gs for gs in grids)
    nbytes = rows * (5 + C) * 4 * 2 + rows // 3 * ld * 2
    rate = nbytes / (us * 1e-6)
    return {"kernel": "yolo_loss_wide" if wide else "yolo_loss", "B": B, "S": S, "C": C, "dlogits_ld": ld,
            "us_per_call_2_launches": round(us, 2), "bytes": nbytes, "us_at_copy_rate": round(nbytes / COPY_RATE * 1e6, 2),
            "GB_per_s": round(rate / 1e9, 1), "of_copy_rate": round(rate / COPY_RATE, 3), "loss_finite": bool(torch.isfinite(losses).all())}


def detect_rate(dev, B, S, C):
    g = torch.Generator(device=dev).manual_seed(100 + C)
    grids = (S // 8, S // 16, S // 32)
    lg = [torch.randn(B, gs, gs, 3 * (5 + C), device=dev, generator=g) for gs in grids]
    win = torch.tensor([[0.0, 0.0, 1.0, 1.0]] * B, device=dev)
    det = torch.zeros(B, cfg.MAX_DETECTION, 6, device=dev)
    cnt = torch.zeros(B, dtype=torch.int32, device=dev)
    ws = L.Workspace(dev)
    reps = 10

    def record():
        for _ in range(reps):
            L.detect(lg[0], lg[1], lg[2], B, S, C, ANCH, win, cfg.OBJ_THRESHOLD, cfg.IOU_THRESHOLD, cfg.MAX_DETECTION, det, cnt, ws)

    us, _prog = replay_us(record, reps)
    return {"kernel": "detect", "path": "bucketed" if C > 16 else "block per (image, class)", "B": B, "S": S, "C": C,
            "us_per_call": round(us, 1), "workspace_MB": round(L.load().disyolo_detect_workspace(B, S, C) / 1e6, 1),
            "detections": int(cnt.sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=576)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, S = args.batch, args.size
    out = [loss_rate(dev, B, S, 80, True), loss_rate(dev, B, S, 3, False)]
    for rec in out:
        print(json.dumps(rec), flush=True)
    det = {C: detect_rate(dev, B, S, C) for C in (80, 17, 16, 8)}
    for rec in det.values():
        print(json.dumps(rec), flush=True)
    slope = (det[16]["us_per_call"] - det[8]["us_per_call"]) / 8.0
    extra = {"kernel": "detect", "path": "block per (image, class), EXTRAPOLATED to C = 80 (it cannot run there)", "B": B, "S": S,
             "C": 80, "us_per_call": round(det[16]["us_per_call"] + slope * 64, 1),
             "workspace_MB": round((B * 20412 * 24 + B * 80 * 20412 * 8) / 1e6, 1) if S == 576 else None,
             "how": "linear in C through the measured C = 8 and C = 16 times"}
    print(json.dumps(extra), flush=True)
    out += list(det.values()) + [extra]
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

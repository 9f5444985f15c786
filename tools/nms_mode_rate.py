"""What the detection filter costs in its three NMS modes (YOLONet(nms=...), lib.detect(nms=...)), by HIP events:

    python tools/nms_mode_rate.py [--json F] [--no-step]

* the filter call alone (decode + filter launches, replayed from a recorded command list back to back as in
  tools/class_list_rate.py, so a figure includes the gap between launches) on random logits of three classes:
  576^2 at B = 8 -- "dense" (conf logits + 8: all 20,412 candidates of an image pass the threshold, the image-wide list fills
  the register form), "random" (logits as drawn: what an untrained head gives), "sparse" (conf logits - 3: about a hundred pass) --
  and 832^2 at B = 4, dense (42,588 candidates per image: the image-wide list runs from global memory) and random.
  The modes alternate inside each repeat; the figure is the median of the repeats, the spread its min .. max.
* the cost of one round of the greedy loop: the same call at max_detection 30 and 2, difference / 28;
* the stage-1 pipelined training step at B = 8, 576^2 (bench.py's flagship, untrained net, resident batch) with nms="per_class" and
  nms="agnostic": two nets in this process, timed regions alternating, host clock around a device synchronise."""
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
from disyolo_amd.net import YOLONet  # noqa: E402
from disyolo_amd.synth import synthetic_batch  # noqa: E402

ANCH = np.asarray(cfg.ANCHORS, np.float32).reshape(-1)
MODES = ("per_class", "agnostic", "none")
REPS = 10          # calls per replay


def make_logits(dev, B, S, case, C=3):
    g = torch.Generator(device=dev).manual_seed(100 + S)
    lg = [torch.randn(B, S // d, S // d, 3, 5 + C, device=dev, generator=g) for d in (8, 16, 32)]
    for y in lg:
        y[..., 2:4] *= 0.5
        y[..., 4] += {"dense": 8.0, "random": 0.0, "sparse": -3.0}[case]
    return [y.reshape(B, y.shape[1], y.shape[2], 3 * (5 + C)).contiguous() for y in lg]


def filter_rates(dev, B, S, case, max_det=cfg.MAX_DETECTION, repeats=9):
    lg = make_logits(dev, B, S, case)
    win = torch.tensor([[0.0, 0.0, 1.0, 1.0]] * B, device=dev)
    det = torch.zeros(B, max_det, 6, device=dev)
    cnt = torch.zeros(B, dtype=torch.int32, device=dev)
    ws = L.Workspace(dev)
    progs, found = {}, {}
    for m in MODES:
        prog = L.CmdList()
        with prog:
            for _ in range(REPS):
                L.detect(lg[0], lg[1], lg[2], B, S, 3, ANCH, win, cfg.OBJ_THRESHOLD, cfg.IOU_THRESHOLD, max_det, det, cnt, ws, nms=m)
        for _ in range(3):                       # warm-up
            prog.run()
        torch.cuda.synchronize()
        progs[m], found[m] = prog, int(cnt.sum())
    ts = {m: [] for m in MODES}
    for _ in range(repeats):
        for m in MODES:
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            progs[m].run()
            e.record()
            torch.cuda.synchronize()
            ts[m].append(s.elapsed_time(e) * 1e3 / REPS)
    NC = 3 * 21 * (S // 32) ** 2
    raw = ws.buf[:B * NC * 24].cpu().numpy()
    above = (raw[B * NC * 16:B * NC * 20].view(np.float32).reshape(B, NC) > np.float32(cfg.OBJ_THRESHOLD)).sum(axis=1)
    rec = {"B": B, "S": S, "case": case, "max_det": max_det, "candidates_per_image": NC,
           "above_threshold_per_image": [int(above.min()), int(above.max())],
           "image_wide_list": "registers" if above.max() <= L.detect_list_capacity() else "global memory"}
    for m in MODES:
        rec[m] = {"us_per_call": round(float(np.median(ts[m])), 1), "min": round(min(ts[m]), 1), "max": round(max(ts[m]), 1),
                  "detections": found[m]}
    return rec


def step_rates(dev, B=8, S=576, steps=20, repeats=5, warmup=6):
    cache = os.path.join(ROOT, "profiles", "tune_train_B8_576_stage1.json")
    nets = {}
    for m in ("per_class", "agnostic"):
        net = YOLONet(training=True, device=dev, image_size=S, batch_size=B, stage=1, seed=0, nms=m)
        net.set_batch(synthetic_batch(B, S, seed=1234))
        if os.path.exists(cache):
            net.autotune(cache=cache)            # the committed tile table: loaded, nothing is timed
        net.shuffle_seed = 1234
        net.build_program(pipeline_backbone=True)
        net.prime_pipeline()
        for _ in range(warmup):
            net.train_step(None, want_loss=False)
        torch.cuda.synchronize()
        nets[m] = net
    ts = {m: [] for m in nets}
    for _ in range(repeats):
        for m, net in nets.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                net.train_step(None, want_loss=False)
            torch.cuda.synchronize()
            ts[m].append((time.perf_counter() - t0) / steps * 1e3)
    out = {"workload": "stage-1 pipelined step, B%d %dx%d, untrained net, resident batch" % (B, S, S), "steps_per_region": steps}
    for m, net in nets.items():
        out[m] = {"ms_per_step": round(float(np.median(ts[m])), 3), "min": round(min(ts[m]), 3), "max": round(max(ts[m]), 3),
                  "images_per_s": round(B / float(np.median(ts[m])) * 1e3, 1), "detections": int(net.det_count.sum()),
                  "loss_finite": bool(np.isfinite(float(net.total_loss().cpu())))}
    out["agnostic_over_per_class"] = round(out["agnostic"]["ms_per_step"] / out["per_class"]["ms_per_step"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--no-step", action="store_true", help="the filter call only")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"list_capacity": L.detect_list_capacity(), "filter": [], "rounds": []}
    for B, S, case in ((8, 576, "dense"), (8, 576, "random"), (8, 576, "sparse"), (4, 832, "dense"), (4, 832, "random")):
        rec = filter_rates(dev, B, S, case)
        out["filter"].append(rec)
        print(json.dumps(rec), flush=True)
    for B, S in ((8, 576), (4, 832)):
        full, two = filter_rates(dev, B, S, "dense"), filter_rates(dev, B, S, "dense", max_det=2)
        rec = {"B": B, "S": S, "case": "dense", "image_wide_list": full["image_wide_list"]}
        for m in MODES:
            rec[m] = {"us_at_30": full[m]["us_per_call"], "us_at_2": two[m]["us_per_call"],
                      "us_per_round": round((full[m]["us_per_call"] - two[m]["us_per_call"]) / 28.0, 2)}
        out["rounds"].append(rec)
        print(json.dumps(rec), flush=True)
    if not args.no_step:
        out["step"] = step_rates(dev)
        print(json.dumps(out["step"]), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

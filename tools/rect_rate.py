"""Training and inference rates of rectangular nets (YOLONet(image_size=(H, W))) against the square net, measured in ONE
process, alternating.

    python tools/rect_rate.py [--shapes 576x576,576x448,352x576] [--rounds 3] [--steps 20] [--warmup 5] [--json out.json]

Per shape (HxW): the pipelined stage-1 training step (B = 8, bf16; bench.py's default step) and the B = 32 hipGraph
inference (network + filter + mask assembly).  Every net is built first; then each round times every shape's step once, one
after the other, so that slow drifts of the box hit all shapes alike.  The committed tile tables are keyed to the square
shapes (profiles/tune_train_B8_576_stage1.json, profiles/tune_infer_B32_576.json): the square net loads them, the
rectangular nets run the launcher's default tiles.  ``--no-tables`` runs the square net on default tiles too, which is the
like-for-like comparison.  Prints one JSON line per workload and shape (median of the rounds) with the pixel ratio and the
time ratio to the first shape, and the time per pixel relative to it.

``--layers``: instead of the two workloads, the per-layer forward times of the inference nets (default tiles for every shape,
eager launches, events around every layer, median of 5 passes) and, per rectangular shape, the layers that take the most time
beyond (square time x pixel ratio) -- which kernel keeps a rectangular pass from being faster by its pixel count."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

import disyolo_amd  # noqa: E402,F401
from disyolo_amd.net import YOLONet  # noqa: E402
from disyolo_amd.synth import synthetic_batch  # noqa: E402


def timed(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def table(name):
    p = os.path.join(ROOT, "profiles", "tune_%s.json" % name)
    return p if os.path.exists(p) else None


def layer_times(shapes, B, dev, passes=5):
    """{shape: {layer: (us, launch tag)}}: a fused group is timed under its last layer, the others show 0"""
    from disyolo_amd import lib as L
    out = {}
    for (H, W) in shapes:
        net = YOLONet(training=False, device=dev, image_size=(H, W), batch_size=B, stage=1, seed=0)
        b = synthetic_batch(B, (H, W), seed=1234)
        net._set_inputs(b["images"], b["clip_window"])
        net.use_side_lane = False
        plan = net._fusion_plan(False, 1, net.score_layer)
        ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in net.layers] for _ in range(passes + 1)]
        for p in range(passes + 1):
            for i, l in enumerate(net.layers):
                ev[p][i][0].record()
                if l.idx in plan:
                    if plan[l.idx] is not None:
                        plan[l.idx]()
                else:
                    net._forward_layer(l, False)
                ev[p][i][1].record()
        torch.cuda.synchronize()
        res = {}
        for i, l in enumerate(net.layers):
            us = float(np.median([ev[p][i][0].elapsed_time(ev[p][i][1]) for p in range(1, passes + 1)])) * 1e3
            if l.idx in plan:
                tag = "fused" if plan[l.idx] is not None else "-"
            elif l.idx == 1:
                tag = "conv_first"
            else:
                tid, bm, bn, _, _ = L.conv2d_tile(l.desc)
                tag = "tile %d (%dx%d)" % (tid, bm, bn)
            res[l.idx] = (us, tag, "%d->%d %dx%d/%d @%dx%d" % (l.cin, l.cout, l.k, l.k, l.stride, l.Ho, l.Wo))
        out[(H, W)] = res
        del net
    return out


def report_layers(shapes, B, dev, json_path):
    t = layer_times(shapes, B, dev)
    base = shapes[0]
    recs = []
    for s in shapes:
        tot = sum(v[0] for v in t[s].values())
        px = (s[0] * s[1]) / float(base[0] * base[1])
        rec = {"shape": "%dx%d" % s, "batch": B, "layers_sum_us": round(tot, 1), "pixels_vs_base": round(px, 4),
               "sum_vs_base": round(tot / sum(v[0] for v in t[base].values()), 4)}
        if s != base:
            excess = sorted(((t[s][i][0] - t[base][i][0] * px, i) for i in t[s]), reverse=True)
            rec["excess_us_total"] = round(sum(e for e, _ in excess), 1)
            rec["top_excess"] = [{"layer": i, "shape": t[s][i][2], "launch": t[s][i][1], "base_launch": t[base][i][1],
                                  "us": round(t[s][i][0], 1), "base_us": round(t[base][i][0], 1), "excess_us": round(e, 1)}
                                 for e, i in excess[:10]]
        recs.append(rec)
        print(json.dumps(rec))
    if json_path:
        with open(json_path, "w") as f:
            json.dump(recs, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="576x576,576x448,352x576")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--train-batch", type=int, default=8)
    ap.add_argument("--infer-batch", type=int, default=32)
    ap.add_argument("--no-tables", action="store_true", help="default tiles for the square net too")
    ap.add_argument("--layers", action="store_true", help="per-layer inference times and the excess over the pixel ratio")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]
    dev = torch.device("cuda:0")
    if args.layers:
        report_layers(shapes, args.infer_batch, dev, args.json)
        return
    BT, BI = args.train_batch, args.infer_batch
    train, infer, tuned = {}, {}, {}
    for (H, W) in shapes:
        net = YOLONet(training=True, device=dev, image_size=(H, W), batch_size=BT, stage=1, seed=0)
        net.set_batch(synthetic_batch(BT, (H, W), seed=1234))
        cache = table("train_B%d_%d_stage1" % (BT, H)) if (H == W and not args.no_tables) else None
        if cache:
            net.autotune(cache=cache)
        net.shuffle_seed = 1234
        net.build_program(pipeline_backbone=True)
        net.prime_pipeline()
        train[(H, W)] = net
        inet = YOLONet(training=False, device=dev, image_size=(H, W), batch_size=BI, stage=1, seed=0)
        b = synthetic_batch(BI, (H, W), seed=1234)
        inet._set_inputs(b["images"], b["clip_window"])
        icache = table("infer_B%d_%d" % (BI, H)) if (H == W and not args.no_tables) else None
        if icache:
            inet.autotune(cache=icache)
        inet.build_infer_program(graph=True)
        infer[(H, W)] = inet
        tuned[(H, W)] = {"train": bool(cache), "infer": bool(icache)}
    step = {s: (lambda n=n: n.train_step(None, want_loss=False)) for s, n in train.items()}
    inf = {s: (lambda n=n: n.infer()) for s, n in infer.items()}
    for s in shapes:
        timed(step[s], args.warmup)
        timed(inf[s], args.warmup)
    ts = {(w, s): [] for w in ("train", "infer") for s in shapes}
    for _ in range(args.rounds):
        for s in shapes:
            ts[("train", s)].append(timed(step[s], args.steps) / args.steps)
        for s in shapes:
            ts[("infer", s)].append(timed(inf[s], args.steps) / args.steps)
    for s in shapes:
        assert np.isfinite(float(train[s].total_loss().cpu()))
    out = []
    base = shapes[0]
    for w in ("train", "infer"):
        ref = float(np.median(ts[(w, base)]))
        for s in shapes:
            B = BT if w == "train" else BI
            med = float(np.median(ts[(w, s)]))
            px = (s[0] * s[1]) / float(base[0] * base[1])
            rec = {"workload": "train_B%d_stage1_pipelined" % B if w == "train" else "infer_B%d_graph" % B,
                   "shape": "%dx%d" % s, "tuned_tiles": tuned[s][w], "fused_launches": sorted(
                       (train[s] if w == "train" else infer[s])._fusion_plan(w == "train", 1, train[s].score_layer)),
                   "ms_per_step": round(med * 1e3, 3), "images_per_s": round(B / med, 1),
                   "rounds_ms": [round(x * 1e3, 3) for x in ts[(w, s)]], "pixels_vs_%dx%d" % base: round(px, 4),
                   "time_vs_%dx%d" % base: round(med / ref, 4), "time_per_pixel_vs_%dx%d" % base: round(med / ref / px, 4)}
            out.append(rec)
            print(json.dumps(rec))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

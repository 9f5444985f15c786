"""Training and inference rates of the mask-subnet strides (YOLONet(mask_stride=...)), measured in ONE process, alternating.

    python tools/mask_stride_rate.py [--strides 4,2,1] [--rounds 3] [--steps 20] [--warmup 5] [--json out.json]

Per stride: the pipelined stage-1 training step (B = 8, 576^2, bf16; bench.py's default step) and the B = 32 hipGraph
inference (network + filter + mask assembly).  Every net is built first; then each round times every stride's step once,
one after the other, so that slow drifts of the box hit all strides alike.  The committed tile tables
(profiles/tune_train_B8_576_stage1.json, profiles/tune_infer_B32_576.json) are loaded where present; shapes they do not
list (the new layers of m != 1/2) run the launcher's pick.  Prints one JSON line per workload and stride (median of the
rounds) and the ratio to m = 1/2."""
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
from disyolo_amd import lib as L  # noqa: E402
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--strides", default="4,2,1")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--size", type=int, default=576)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    strides = [int(s) for s in args.strides.split(",")]
    dev = torch.device("cuda:0")
    S = args.size
    train, infer = {}, {}
    for m in strides:
        net = YOLONet(training=True, device=dev, image_size=S, batch_size=8, stage=1, seed=0, mask_stride=m)
        net.set_batch(synthetic_batch(8, S, seed=1234))
        cache = table("train_B8_%d_stage1" % S)
        if cache:
            net.autotune(cache=cache)
        net.shuffle_seed = 1234
        net.build_program(pipeline_backbone=True)
        net.prime_pipeline()
        train[m] = net
        inet = YOLONet(training=False, device=dev, image_size=S, batch_size=32, stage=1, seed=0, mask_stride=m)
        b = synthetic_batch(32, S, seed=1234)
        inet._set_inputs(b["images"], b["clip_window"])
        cache = table("infer_B32_%d" % S)
        if cache:
            inet.autotune(cache=cache)
        inet.build_infer_program(graph=True)
        infer[m] = inet
    step = {m: (lambda n=n: n.train_step(None, want_loss=False)) for m, n in train.items()}
    inf = {m: (lambda n=n: n.infer()) for m, n in infer.items()}
    for m in strides:
        timed(step[m], args.warmup)
        timed(inf[m], args.warmup)
    ts = {("train", m): [] for m in strides}
    ts.update({("infer", m): [] for m in strides})
    for _ in range(args.rounds):
        for m in strides:
            ts[("train", m)].append(timed(step[m], args.steps) / args.steps)
        for m in strides:
            ts[("infer", m)].append(timed(inf[m], args.steps) / args.steps)
    for m in strides:
        assert np.isfinite(float(train[m].total_loss().cpu()))
    out = []
    for (w, m), v in sorted(ts.items(), key=lambda kv: (kv[0][0], -kv[0][1])):
        B = 8 if w == "train" else 32
        med = float(np.median(v))
        ref = float(np.median(ts[(w, 2)])) if (w, 2) in ts else None
        rec = {"workload": "train_B8_%d_stage1_pipelined" % S if w == "train" else "infer_B32_%d_graph" % S,
               "mask_stride": m, "m": {4: "1/4", 2: "1/2", 1: "1"}[m], "ms_per_step": round(med * 1e3, 3),
               "images_per_s": round(B / med, 1), "rounds_ms": [round(x * 1e3, 3) for x in v],
               "vs_m_half": round(med / ref, 4) if ref else None}
        out.append(rec)
        print(json.dumps(rec))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

"""What a holed lock map costs: the recorded training step at B = 8, 576^2 for lock maps with locked layers downstream of
trainable ones, beside stage 2 (nothing locked) in ONE process, interleaved; and the frozen batch-norm backward kernel alone.

    python tools/lock_map_rate.py [--maps stage2,hole_5_9,frozen_heads] [--steps 10] [--warmup 4] [--repeats 10] [--json F]

Per map: YOLONet(stage=2, lock=<map>), build_program(overlap_tail=True) (the plain recorded two-lane step; a map with a
trainable first layer has no locked prefix to pipeline), bench.py's timing recipe -- a region of ``steps`` replays between two
device synchronisations, the median of ``repeats`` regions; the regions of the maps alternate so that slow drifts of the box
hit all of them alike.  A holed map computes strictly less than stage 2 (no weight gradient, batch statistics or optimizer
slice for its locked layers), so it should be no slower.  The kernel: disyolo_bn_frozen_bwd at 2,654,208 x 32 (conv1's shape
at B = 8, 576^2) and 20,736 x 1024 over rotating buffers, 6 B per element, against the 6.3 TB/s copy rate of the card; the
launches are replayed from a command list back to back, so a figure still includes the gap between two dependent-free
launches (a few us: visible at the small shape, whose launch moves 127 MB)."""
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
from disyolo_amd import lib as L  # noqa: E402
from disyolo_amd.net import YOLONet  # noqa: E402
from disyolo_amd.synth import synthetic_batch  # noqa: E402

MAPS = {
    "stage2": {},
    "hole_5_9": {i: True for i in range(5, 10)},
    "frozen_heads": {i: True for i in range(53, 76)},
    "odd": {i: True for i in range(1, 83, 2)},
}
COPY_RATE = 6.3e12


def timed(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def kernel_rates(dev):
    out = []
    for rows, C in ((2654208, 32), (20736, 1024)):
        NB = 4 if rows * C > (1 << 24) else 24          # (rotating buffers: more bytes than the 256 MB of last-level cache)
        g = torch.Generator(device=dev).manual_seed(rows + C)
        dy = [torch.randn(rows, C, device=dev, generator=g).to(torch.bfloat16) for _ in range(NB)]
        x = [torch.randn(rows, C, device=dev, generator=g).to(torch.bfloat16) for _ in range(NB)]
        dx = [torch.empty(rows, C, dtype=torch.bfloat16, device=dev) for _ in range(NB)]
        sc = torch.rand(C, device=dev, generator=g) + 0.5
        sh = torch.randn(C, device=dev, generator=g) * 0.5
        # the launches go through a recorded command list, as the step's do: one C call replays all of them, so the time
        # between two launches is the device's own launch gap, not the interpreter's
        reps = 5 if NB == 4 else 3
        prog = L.CmdList()
        with prog:
            for _ in range(reps):
                for i in range(NB):
                    L.bn_frozen_bwd(dy[i], x[i], sc, sh, dx[i], rows, C)
        prog.run()
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        prog.run()
        e.record()
        torch.cuda.synchronize()
        us = s.elapsed_time(e) * 1e3 / (reps * NB)
        rate = rows * C * 6 / (us * 1e-6)
        rec = {"kernel": "bn_frozen_bwd", "rows": rows, "C": C, "us": round(us, 2), "GB_per_s": round(rate / 1e9, 1),
               "of_copy_rate": round(rate / COPY_RATE, 3)}
        out.append(rec)
        print(json.dumps(rec), flush=True)
        del dy, x, dx
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", default="stage2,hole_5_9,frozen_heads")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--size", type=int, default=576)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--json", default=None)
    ap.add_argument("--no-kernel", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    out = [] if args.no_kernel else kernel_rates(dev)
    names = args.maps.split(",")
    nets = {}
    for name in names:
        net = YOLONet(training=True, device=dev, image_size=args.size, batch_size=args.batch, stage=2, lock=MAPS[name], seed=0)
        net.set_batch(synthetic_batch(args.batch, args.size, seed=1234))
        net.shuffle_seed = 1234
        net.build_program(overlap_tail=True)
        nets[name] = net
    step = {n: (lambda net=net: net.train_step(None, want_loss=False)) for n, net in nets.items()}
    for n in names:
        timed(step[n], args.warmup)
    ts = {n: [] for n in names}
    for _ in range(args.repeats):
        for n in names:
            ts[n].append(timed(step[n], args.steps) / args.steps)
    ref = float(np.median(ts["stage2"])) if "stage2" in ts else None
    for n in names:
        loss = float(nets[n].total_loss().cpu())
        nets[n].check_cluster_sync()
        med = float(np.median(ts[n]))
        rec = {"workload": "train_B%d_%d_recorded" % (args.batch, args.size), "map": n,
               "locked": len([i for i, v in nets[n].lock.items() if v]), "pass_through": len(nets[n].pass_through_layers()),
               "trainable_variables": nets[n].n_params, "ms_per_step": round(med * 1e3, 3),
               "ms_min_max": [round(min(ts[n]) * 1e3, 3), round(max(ts[n]) * 1e3, 3)],
               "images_per_s": round(args.batch / med, 1), "vs_stage2": round(med / ref, 4) if ref else None,
               "loss_finite": bool(np.isfinite(loss))}
        out.append(rec)
        print(json.dumps(rec), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

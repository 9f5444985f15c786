"""What a batch of training windows costs (``defect_train(placement="window")``), on synthetic photographs:

    python tools/window_rate.py [--record 3000x4000] [--size 576] [--batch 8] [--records 16] [--txt F]

One process measures
* ``get_device()`` per batch: the host's time in the call (median of 50, no synchronise) and the batch time with the device
  (50 calls, one synchronise at the end), after a warm-up that fills the record cache;
* whether ``get_device()`` waits for the device: 300 ms of matrix products are queued on its stream first; a call that
  synchronised would take that long on the host clock;
* each of the three new launches on the jobs of the last batch (HIP events, median of 20 calls) with the bytes it has to move
  against the 6.29 TB/s the project measured for a device copy;
* the record cache: bytes per record against what full-size instance masks would take."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "examples")):
    if p not in sys.path:
        sys.path.insert(0, p)

import disyolo_amd  # noqa: E402,F401
from disyolo_amd import lib as L  # noqa: E402
from disyolo_amd.train_data import defect_train  # noqa: E402
from train_synthetic import large_labels, parse_size  # noqa: E402

COPY_TBS = 6.29


def events_us(fn, repeats=20):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        ts.append(s.elapsed_time(e) * 1e3)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--record", type=parse_size, default=(3000, 4000))
    ap.add_argument("--size", type=parse_size, default=576)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--records", type=int, default=16)
    ap.add_argument("--txt", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    labels = large_labels(np.random.RandomState(0), args.records, args.record)
    data = defect_train(labels, batch_size=args.batch, image_size=args.size, device=dev, rng=np.random.RandomState(1),
                        placement="window")
    S, B, G = (data.net_h, data.net_w), args.batch, data.max_box_per_image
    for _ in range(3 * args.records // B + 5):
        data.get_device()
    torch.cuda.synchronize()
    host = []
    t0 = time.perf_counter()
    for _ in range(50):
        t = time.perf_counter()
        data.get_device()
        host.append(time.perf_counter() - t)
    torch.cuda.synchronize()
    per_batch = (time.perf_counter() - t0) / 50
    # does the call wait for the device?  (three batches each: a batch may draw no photometric step that uploads anything)
    x = torch.randn(8192, 8192, device=dev)

    def behind_queued_work(loader):
        worst, queued = 0.0, 0.0
        for _ in range(5):
            loader.get_device()
        for _ in range(3):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            s.record()
            for _ in range(24):
                x @ x
            e.record()
            t = time.perf_counter()
            loader.get_device()
            worst = max(worst, time.perf_counter() - t)
            torch.cuda.synchronize()
            queued = s.elapsed_time(e)
        return worst * 1e3, queued

    behind, queued_ms = behind_queued_work(data)
    kw = dict(batch_size=B, image_size=args.size, device=dev, rng=np.random.RandomState(1))
    plain, _ = behind_queued_work(defect_train(labels, placement="window", blur_noise_light=False, **kw))
    small = large_labels(np.random.RandomState(0), args.records, (300, 400), instances=3)
    box, _ = behind_queued_work(defect_train(small, **kw))
    box_plain, _ = behind_queued_work(defect_train(small, blur_noise_light=False, **kw))
    # the three launches on the last batch's jobs
    wj, nwin = data._last_window
    jobs = data._jobs_host[data._last].numpy()[B * L.PLACE_JOB.itemsize:].view(L.WINDOW_JOB)[:nwin]
    x1 = np.maximum(np.maximum(jobs["crop_x"], jobs["x0"]), 0)
    y1 = np.maximum(np.maximum(jobs["crop_y"], jobs["y0"]), 0)
    x2 = np.minimum(np.minimum(jobs["crop_x"] + jobs["crop_w"], jobs["x0"] + S[1]), jobs["image_w"])
    y2 = np.minimum(np.minimum(jobs["crop_y"] + jobs["crop_h"], jobs["y0"] + S[0]), jobs["image_h"])
    rect = int((np.maximum(x2 - x1, 0).astype(np.int64) * np.maximum(y2 - y1, 0)).sum())
    d = data._dev[data._last]
    out_bytes = 4 * (sum(t.numel() for t in d[:4]) + nwin)
    planes = torch.zeros_like(data.true_masks)
    t_vis = events_us(lambda: L.window_visible(wj, nwin, S, data._vis))
    t_tgt = events_us(lambda: L.window_targets(wj, nwin, data._vis, data._anchors_dev, S, data.min_visible, d[0], d[1], d[2], d[3], data._rows))
    t_msk = events_us(lambda: L.window_place_masks(wj, nwin, data._rows, planes, S))
    kept = int((data._rows[:nwin] >= 0).sum())
    n_inst = sum(len(l["polygons"]) for l in labels)
    full = n_inst * args.record[0] * args.record[1] + len(labels) * args.record[0] * args.record[1] * 3
    lines = [
        "window batches: %d records of %dx%d, net %dx%d, B = %d, %s" % (len(labels), args.record[0], args.record[1], S[0], S[1], B, torch.cuda.get_device_name(0)),
        "get_device(): host %.3f ms per call (median of 50), %.3f ms per batch with the device (50 calls, one synchronise)" % (
            float(np.median(host)) * 1e3, per_batch * 1e3),
        "behind %.0f ms of queued matrix products get_device() returned after (the slowest of 3 calls): window %.3f ms, window "
        "without blur / noise / light %.3f ms, letterbox %.3f ms, letterbox without blur / noise / light %.3f ms "
        "(a call that returns in a fraction of the queued time did not wait for the device)" % (queued_ms, behind, plain, box, box_plain),
        "last batch: %d jobs, %d kept, visible rects %d bytes" % (nwin, kept, rect),
        "window_visible      %7.1f us  reads %d bytes: %.4f of the copy rate" % (t_vis, rect, rect / (t_vis * 1e-6) / (COPY_TBS * 1e12)),
        "window_targets      %7.1f us  writes %d bytes (the zeroed arrays): %.4f of the copy rate" % (t_tgt, out_bytes, out_bytes / (t_tgt * 1e-6) / (COPY_TBS * 1e12)),
        "window_place_masks  %7.1f us  reads and writes %d bytes: %.4f of the copy rate" % (t_msk, 2 * rect, 2 * rect / (t_msk * 1e-6) / (COPY_TBS * 1e12)),
        "record cache: %d records, %.2f MB each (image + crops); full-size instance masks would make it %.1f MB each" % (
            len(data._cache), data._cached / max(len(data._cache), 1) / 1e6, full / len(labels) / 1e6),
    ]
    print("\n".join(lines))
    if args.txt:
        with open(args.txt, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

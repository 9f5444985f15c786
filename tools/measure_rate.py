"""What instance measurement costs, on the drawn defects of one synthetic photograph, by HIP events and a host clock:

    python tools/measure_rate.py [--image 3000x4000] [--defects 36] [--chunk 8] [--txt F]

The crops are the shapes ``tools/tiles_rate.py`` draws (long thin cracks at any angle, whose boxes are mostly background, and
elliptic blobs), packed by ``measure.pack_masks``.  One process measures
* ``measure.measure_arena`` per call (host clock around the call, which ends in its own copy to the host; median of 5);
* disyolo_measure_d2 (two launches), ONE thinning iteration of disyolo_measure_thin with every group live (two launches; the
  first iteration, the most expensive one), and disyolo_measure_counts (two launches and a memset), each by HIP events (median
  of 7 calls from Python, so a short launch is the host's call time);
* the bytes each of them has to move at least once, against the 6.29 TB/s the project measured for a device copy.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import disyolo_amd  # noqa: E402,F401
from disyolo_amd import lib as L  # noqa: E402
from disyolo_amd import measure as MZ  # noqa: E402
from tiles_rate import COPY_TBS, events_us, host_ms, synthetic_photo  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--image", default="3000x4000")
    ap.add_argument("--defects", type=int, default=36)
    ap.add_argument("--chunk", type=int, default=8)
    ap.add_argument("--txt", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("measure_rate: no GPU: nothing here can be measured without one")
    dev = torch.device("cuda:0")
    h, w = (int(v) for v in args.image.lower().split("x"))
    shapes = []
    synthetic_photo(h, w, defects=args.defects, shapes=shapes)
    crops = [np.ascontiguousarray(inside) for _, _, _, inside in shapes]
    groups, arena_np, nbytes = MZ.pack_masks(crops)
    arena = torch.from_numpy(arena_np).to(dev)
    groups_dev = torch.from_numpy(groups).to(dev)
    G = len(crops)
    rows = []

    def put(**kw):
        rows.append(kw)
        print(json.dumps(kw), flush=True)

    m = MZ.measure_arena(groups, arena, nbytes, groups_dev, chunk=args.chunk)
    ms, lo, hi = host_ms(lambda: MZ.measure_arena(groups, arena, nbytes, groups_dev, chunk=args.chunk))
    put(what="measure_arena per call", crops=G, arena_MB=round(nbytes / 1e6, 2), foreground_px=int(m.area_px.sum()),
        largest_box=[int(v) for v in max((c.shape for c in crops), key=lambda s: s[0] * s[1])], iterations=m.iterations,
        flag_reads=-(-m.iterations // args.chunk), chunk=args.chunk, ms=round(ms, 2), min=round(lo, 2), max=round(hi, 2))

    d2 = torch.empty(nbytes, dtype=torch.int32, device=dev)
    colg = torch.empty(nbytes, dtype=torch.int16, device=dev)
    skel, tmp = torch.empty(nbytes, dtype=torch.uint8, device=dev), torch.empty(nbytes, dtype=torch.uint8, device=dev)
    flags = torch.empty(2, G, dtype=torch.int32, device=dev)
    iters = torch.zeros(G, dtype=torch.int32, device=dev)

    def rate(name, fn, moved, **kw):
        us, lo, hi = events_us(fn)
        put(kernel=name, us=round(us, 1), min=round(lo, 1), max=round(hi, 1), MB=round(moved / 1e6, 2),
            TBps=round(moved / us / 1e6, 3), of_copy_rate=round(moved / us / 1e6 / COPY_TBS, 4),
            us_at_copy_rate=round(moved / COPY_TBS / 1e6, 1), **kw)

    # bytes per pixel moved at least once: d2 = mask 1 + g 2 written, read twice (the second column sweep, the row pass) + d2 4
    rate("measure_d2 (column pass + row pass)", lambda: L.measure_d2(groups, arena, colg, d2, groups_dev, nbytes), 11 * nbytes)
    # one iteration = two sub-steps, each a byte read and a byte written per pixel (the 3x3 neighbourhood comes from the cache)
    rate("measure_thin, the first iteration (2 launches, every group live)",
         lambda: L.measure_thin(groups, arena, skel, tmp, flags, iters, 0, 1, groups_dev, nbytes), 4 * nbytes)
    L.measure_d2(groups, arena, colg, d2, groups_dev, nbytes)
    rate("measure_counts (memset + 2 launches)", lambda: L.measure_counts(groups, arena, m.skeleton_arena, d2, groups_dev, nbytes),
         6 * nbytes, blocks=L.measure_blocks(groups))
    if args.txt:
        with open(args.txt, "w") as f:
            f.write("tools/measure_rate.py --image %s --defects %d --chunk %d\n" % (args.image, args.defects, args.chunk))
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()

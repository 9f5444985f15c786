"""What the shape of an instance costs, on the drawn defects of one synthetic photograph, by HIP events and a host clock:

    python tools/shape_rate.py [--image 3000x4000] [--defects 36] [--directions 180] [--disc 2000] [--noise 80x140] [--txt F]

The crops are those of ``tools/trace_rate.py`` (long thin cracks at any angle, whose boxes are mostly background, and elliptic
blobs: the same 29.1 MB arena).  A second arena adds the union-find's bad cases: one solid disc of --disc pixels across (long
chains: every pixel of it ends under one root) and one crop of random pixels at density 0.6 (--noise HxW: many parts).  A third
holds the disc alone, to say which part of the call its parts labelling takes.  One process measures, per arena,
* ``measure.shape_arena`` per call (host clock around the call, which ends in its own copy to the host; median of 5);
* the three entry points, each by HIP events (median of 7 calls from Python, so a short launch is the host's call time):
  disyolo_shape_sums (rows; one launch over the arena), disyolo_shape_parts (a memset; init, merge, flatten, count, roots) and
  disyolo_shape_extents (rows; one launch over the arena);
* the bytes each of them has to move at least once, against the 6.29 TB/s the project measured for a device copy.
No threshold is set: there is no parent to compare with.
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
    ap.add_argument("--directions", type=int, default=180)
    ap.add_argument("--disc", type=int, default=2000, help="the side of the solid disc's crop")
    ap.add_argument("--noise", default="80x140", metavar="HxW", help="the crop of random pixels (density 0.6)")
    ap.add_argument("--txt", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("shape_rate: no GPU: nothing here can be measured without one")
    dev = torch.device("cuda:0")
    h, w = (int(v) for v in args.image.lower().split("x"))
    shapes = []
    synthetic_photo(h, w, defects=args.defects, shapes=shapes)
    drawn = [np.ascontiguousarray(inside) for _, _, _, inside in shapes]
    yy, xx = np.mgrid[:args.disc, :args.disc]
    c = (args.disc - 1) / 2.0
    disc = (yy - c) ** 2 + (xx - c) ** 2 <= c * c
    nh, nw = (int(v) for v in args.noise.lower().split("x"))
    noise = np.random.default_rng(0).random((nh, nw)) < 0.6
    K = args.directions
    dirs = MZ.shape_directions(K)
    rows_out = []

    def put(**kw):
        rows_out.append(kw)
        print(json.dumps(kw), flush=True)

    for name, crops in (("the drawn defects", drawn), ("the drawn defects, the disc and the noise", drawn + [disc, noise]),
                        ("the disc alone", [disc])):
        groups, arena_np, nbytes = MZ.pack_masks(crops)
        arena = torch.from_numpy(arena_np).to(dev)
        groups_dev = torch.from_numpy(groups).to(dev)
        dirs_dev = torch.from_numpy(dirs).to(dev)
        G = len(crops)
        s = MZ.shape_arena(groups, arena, nbytes, groups_dev, K)
        ms, lo, hi = host_ms(lambda: MZ.shape_arena(groups, arena, nbytes, groups_dev, K))
        put(what="shape_arena per call", arena=name, crops=G, arena_MB=round(nbytes / 1e6, 2), directions=K,
            foreground_px=int(s.area_px.sum()), parts=int(s.n_parts.sum()), holes=int(s.n_holes.sum()), host_reads=1,
            ms=round(ms, 3), min=round(lo, 3), max=round(hi, 3))
        labels, px = (torch.empty(nbytes, dtype=torch.int32, device=dev) for _ in range(2))
        sums = torch.empty(G, L.SHAPE_COLS, dtype=torch.int64, device=dev)
        parts = torch.empty(G, 2, dtype=torch.int64, device=dev)
        pminmax = torch.empty(G, K, 2, dtype=torch.int32, device=dev)
        took = {}

        def rate(key, label, fn, moved):
            us, lo, hi = events_us(fn)
            took[key] = us
            put(kernel=label, arena=name, us=round(us, 1), min=round(lo, 1), max=round(hi, 1), MB=round(moved / 1e6, 2),
                TBps=round(moved / us / 1e6, 3), of_copy_rate=round(moved / us / 1e6 / COPY_TBS, 4),
                us_at_copy_rate=round(moved / COPY_TBS / 1e6, 1))

        # bytes per pixel moved at least once (neighbourhoods come from the cache): sums = the mask read (1); parts = init (the
        # mask 1 read, labels 4 + px 4 written), merge (the mask 1, labels 4), flatten (labels 4), count (labels 4), roots
        # (labels 4); extents = the mask read (1) -- the K multiply-adds per boundary pixel move nothing
        rate("sums", "shape_sums (rows + 1 launch over the arena)", lambda: L.shape_sums(groups, arena, sums, groups_dev, nbytes), nbytes)
        rate("parts", "shape_parts (memset + init + merge + flatten + count + roots)",
             lambda: L.shape_parts(groups, arena, labels, px, parts, groups_dev, nbytes), 26 * nbytes)
        rate("extents", "shape_extents (rows + 1 launch over the arena, K = %d)" % K,
             lambda: L.shape_extents(groups, arena, dirs, pminmax, groups_dev, dirs_dev, nbytes), nbytes)
        total = sum(took.values())
        put(what="the three entry points together", arena=name, us=round(total, 1),
            parts_share=round(took["parts"] / total, 3), sums_share=round(took["sums"] / total, 3),
            extents_share=round(took["extents"] / total, 3))
    if args.txt:
        with open(args.txt, "w") as f:
            f.write("tools/shape_rate.py --image %s --defects %d --directions %d --disc %d --noise %s\n" % (
                args.image, args.defects, K, args.disc, args.noise))
            for r in rows_out:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()

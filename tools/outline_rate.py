"""What the outlines of the instances cost, on the drawn defects of one synthetic photograph, by HIP events and a host clock:

    python tools/outline_rate.py [--image 3000x4000] [--defects 36] [--disc 2000] [--noise 80x140] [--txt F]

The three arenas are those of ``tools/shape_rate.py``: the drawn defects (long thin cracks and elliptic blobs), the same with one
solid disc of --disc pixels across and one crop of random pixels at density 0.6 (--noise HxW: many small loops and holes), and the
disc alone.  One process measures, per arena,
* ``measure.instance_outlines`` of an InstanceShapes per call (host clock around the call, which ends in its own copies to the host;
  median of 5), with and without the points;
* the three entry points, each by HIP events (median of 7 calls from Python, so a short launch is the host's call time):
  disyolo_outline_edges (a memset and two launches over the arena), disyolo_outline_loops (2 R + 2 launches over the list, R =
  bit_length(the most edges of a group - 1)) and disyolo_outline_gather (one launch over the list);
* beside them the only way a user had before: the same masks copied to the host in one transfer and
  ``pre_process.find_contours`` (the one-threaded tracer of csrc/contours.hip) run on each (host clock, median of 5).
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
from disyolo_amd import pre_process as PP  # noqa: E402
from tiles_rate import events_us, host_ms, synthetic_photo  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--image", default="3000x4000")
    ap.add_argument("--defects", type=int, default=36)
    ap.add_argument("--disc", type=int, default=2000, help="the side of the solid disc's crop")
    ap.add_argument("--noise", default="80x140", metavar="HxW", help="the crop of random pixels (density 0.6)")
    ap.add_argument("--txt", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("outline_rate: no GPU: nothing here can be measured without one")
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
    rows_out = []

    def put(**kw):
        rows_out.append(kw)
        print(json.dumps(kw), flush=True)

    for name, crops in (("the drawn defects", drawn), ("the drawn defects, the disc and the noise", drawn + [disc, noise]),
                        ("the disc alone", [disc])):
        groups, arena_np, nbytes = MZ.pack_masks(crops)
        arena = torch.from_numpy(arena_np).to(dev)
        groups_dev = torch.from_numpy(groups).to(dev)
        G = len(crops)
        s = MZ.shape_arena(groups, arena, nbytes, groups_dev, 2)
        o = MZ.instance_outlines(s)
        E, n_loops = int(s.edges.sum()), len(o.loops)
        rounds = max(int(s.edges.max()) - 1, 0).bit_length()
        common = dict(arena=name, crops=G, arena_MB=round(nbytes / 1e6, 2), edges=E, loops=n_loops, points=int(o.point_offsets[-1]),
                      corners=int(o.corner_offsets[-1]), rounds=rounds)
        ms, lo, hi = host_ms(lambda: MZ.instance_outlines(s))
        put(what="instance_outlines per call", host_reads=2, ms=round(ms, 3), min=round(lo, 3), max=round(hi, 3), **common)
        ms, lo, hi = host_ms(lambda: MZ.instance_outlines(s, points=False))
        put(what="instance_outlines(points=False) per call", arena=name, host_reads=1, ms=round(ms, 3), min=round(lo, 3), max=round(hi, 3))

        def baseline():
            host = arena.cpu().numpy()
            for gr in groups:
                bh, bw, off = int(gr[4] - gr[2]), int(gr[5] - gr[3]), int(gr[7]) * 16
                PP.find_contours(host[off:off + bh * bw].reshape(bh, bw))

        ms, lo, hi = host_ms(baseline)
        put(what="the masks copied to the host and pre_process.find_contours on each", arena=name, ms=round(ms, 3), min=round(lo, 3),
            max=round(hi, 3))
        i32 = lambda *sh: torch.empty(*sh, dtype=torch.int32, device=dev)
        first, sides = i32(nbytes), torch.empty(nbytes, dtype=torch.uint8, device=dev)
        ekey, nxt, aterm, flag, eidx, ctrl = i32(E), i32(E), i32(E), torch.empty(E, dtype=torch.uint8, device=dev), i32(E, 3), i32(4)
        work = torch.empty(L.OUTLINE_WORK * E, dtype=torch.int64, device=dev)
        rows = torch.empty(n_loops, L.OUTLINE_ROW, dtype=torch.int64, device=dev)
        took = {}

        def rate(key, label, fn):
            us, lo, hi = events_us(fn)
            took[key] = us
            put(kernel=label, arena=name, us=round(us, 1), min=round(lo, 1), max=round(hi, 1))

        edges = lambda: L.outline_edges(groups, arena, first, sides, ekey, nxt, flag, aterm, work, ctrl, groups_dev, nbytes)
        loops = lambda: L.outline_loops(groups, arena, s.labels_arena, first, sides, ekey, nxt, flag, aterm, rounds, work, eidx, rows, ctrl,
                                        groups_dev, nbytes)
        rate("edges", "outline_edges (memset + mark + next over the arena)", edges)

        def edges_then_loops():                                        # (the loops take their rows by a counter the edges zero)
            edges()
            loops()

        rate("both", "outline_edges + outline_loops (%d + %d rounds over the list)" % (rounds, rounds), edges_then_loops)
        took["loops"] = took["both"] - took["edges"]
        raw = rows.cpu().numpy()
        table, order = MZ.order_loops(raw)
        assert np.array_equal(table, o.loops)
        plan = torch.from_numpy(MZ.outline_plan(groups, o, raw, order)).to(dev)
        pts, cor = i32(int(o.point_offsets[-1]), 2), i32(int(o.corner_offsets[-1]), 2)
        rate("gather", "outline_gather (1 launch over the list)",
             lambda: L.outline_gather(groups, arena, ekey, flag, eidx, ctrl, plan, pts, cor, groups_dev, nbytes))
        assert np.array_equal(pts.cpu().numpy(), o._points) and np.array_equal(cor.cpu().numpy(), o._corners)
        put(what="the three entry points together", arena=name, us=round(took["edges"] + took["loops"] + took["gather"], 1),
            edges_us=round(took["edges"], 1), loops_us=round(took["loops"], 1), gather_us=round(took["gather"], 1))
    if args.txt:
        with open(args.txt, "w") as f:
            f.write("tools/outline_rate.py --image %s --defects %d --disc %d --noise %s\n" % (args.image, args.defects, args.disc, args.noise))
            for r in rows_out:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()

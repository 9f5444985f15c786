"""What the skeleton graph costs, on the drawn defects of one synthetic photograph, by HIP events and a host clock:

    python tools/skeleton_rate.py [--image 3000x4000] [--defects 36] [--min-branch 10] [--txt F]

The crops are those of ``tools/measure_rate.py`` (long thin cracks at any angle, whose boxes are mostly background, and elliptic
blobs), measured once by ``measure.measure_arena``.  One process measures
* ``measure.skeleton_graph`` per call at min_branch_px 0 and at --min-branch (host clock around the call, which ends in its own
  copy to the host; median of 5), with the analyses it took and the branches it found;
* the four launch groups of one analysis, each by HIP events (median of 7 calls from Python, so a short launch is the host's
  call time): disyolo_skeleton_classify (one launch), disyolo_skeleton_label (init, merge, flatten), disyolo_skeleton_rows (two
  memsets; alloc, accumulate, finish) and disyolo_skeleton_prune (one launch);
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
    ap.add_argument("--min-branch", type=float, default=10.0)
    ap.add_argument("--txt", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("skeleton_rate: no GPU: nothing here can be measured without one")
    dev = torch.device("cuda:0")
    h, w = (int(v) for v in args.image.lower().split("x"))
    shapes = []
    synthetic_photo(h, w, defects=args.defects, shapes=shapes)
    crops = [np.ascontiguousarray(inside) for _, _, _, inside in shapes]
    groups, arena_np, nbytes = MZ.pack_masks(crops)
    arena = torch.from_numpy(arena_np).to(dev)
    groups_dev = torch.from_numpy(groups).to(dev)
    G = len(crops)
    rows_out = []

    def put(**kw):
        rows_out.append(kw)
        print(json.dumps(kw), flush=True)

    m = MZ.measure_arena(groups, arena, nbytes, groups_dev)
    for mb in (0.0, args.min_branch):
        g = MZ.skeleton_graph(m, mb)
        ms, lo, hi = host_ms(lambda: MZ.skeleton_graph(m, mb))
        put(what="skeleton_graph per call", min_branch_px=mb, crops=G, arena_MB=round(nbytes / 1e6, 2),
            skeleton_px=int(m.skeleton_px.sum()), pruned_skeleton_px=int(g.pruned.skeleton_px.sum()),
            length_px=round(float(m.length_px.sum()), 1), pruned_length_px=round(float(g.pruned.length_px.sum()), 1),
            branches=int(g.n_branches.sum()), junction_px=int(g.junction_px.sum()), analyses=g.analyses,
            converged=bool(g.converged.all()), host_reads=g.analyses + 1, ms=round(ms, 2), min=round(lo, 2), max=round(hi, 2))

    links = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    skel = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    labels = torch.empty(nbytes, dtype=torch.int32, device=dev)
    rowid = torch.empty(nbytes, dtype=torch.int32, device=dev)
    cap = max(int(m.skeleton_px.sum()), 1)
    rows = torch.empty(cap, L.SKELETON_ROW, dtype=torch.int64, device=dev)
    ctrl = torch.zeros(G + 1, dtype=torch.int32, device=dev)
    junctions = torch.zeros(G, 4, dtype=torch.int64, device=dev)
    M2 = int(2 * args.min_branch)

    def rate(name, fn, moved, **kw):
        us, lo, hi = events_us(fn)
        put(kernel=name, us=round(us, 1), min=round(lo, 1), max=round(hi, 1), MB=round(moved / 1e6, 2),
            TBps=round(moved / us / 1e6, 3), of_copy_rate=round(moved / us / 1e6 / COPY_TBS, 4),
            us_at_copy_rate=round(moved / COPY_TBS / 1e6, 1), **kw)

    # bytes per pixel moved at least once (the 3x3 neighbourhoods come from the cache; what only skeleton pixels touch -- d2,
    # the labels of neighbours, the rows -- is small beside the arena): classify = the skeleton read, its copy and the links
    # written; label = init (skeleton 1 + links 1 read, labels 4 written), merge (links 1), flatten (labels 4);
    # rows = alloc (labels 4), accumulate (links 1 + labels 4), and the row buffer once; prune = labels 4
    rate("skeleton_classify (1 launch, with the copy)",
         lambda: L.skeleton_classify(groups, m.skeleton_arena, skel, links, groups_dev, nbytes), 3 * nbytes)
    rate("skeleton_label (init + merge + flatten)", lambda: L.skeleton_label(groups, skel, links, labels, groups_dev, nbytes),
         11 * nbytes)

    def rows_call():
        L.skeleton_rows(groups, links, labels, m.d2_arena, rowid, rows, M2, ctrl, junctions, groups_dev, nbytes)

    rows_call()
    rate("skeleton_rows (2 memsets + alloc + accumulate + finish)", rows_call, 9 * nbytes + 8 * L.SKELETON_ROW * cap,
         row_capacity=cap, branches=int(ctrl[0]))
    rate("skeleton_prune (1 launch)", lambda: L.skeleton_prune(groups, labels, rowid, rows, skel, groups_dev, nbytes), 4 * nbytes)
    if args.txt:
        with open(args.txt, "w") as f:
            f.write("tools/skeleton_rate.py --image %s --defects %d --min-branch %s\n" % (args.image, args.defects, args.min_branch))
            for r in rows_out:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()

"""What tracing the skeleton graph costs, on the drawn defects of one synthetic photograph, by HIP events and a host clock:

    python tools/trace_rate.py [--image 3000x4000] [--defects 36] [--min-branch 10] [--noise 80x140] [--txt F]

The crops are those of ``tools/skeleton_rate.py`` (long thin cracks at any angle, whose boxes are mostly background, and elliptic
blobs; they thin to one clean branch each, so --noise HxW adds one crop of random pixels at density 0.6, whose skeleton is
all junctions and short branches), measured once by ``measure.measure_arena`` and analysed once by ``measure.skeleton_graph``.
One process measures
* ``measure.skeleton_trace`` per call at min_branch_px 0 and at --min-branch (host clock around the call, which ends in its own
  copy to the host; median of 5), with the nodes, list entries and rounds it took, and the host's share: the trunk selection;
* the four entry points, each by HIP events (median of 7 calls from Python, so a short launch is the host's call time):
  disyolo_trace_nodes (a memset; init, merge, flatten, alloc, accumulate), disyolo_trace_rank (a memset; compact, link, K
  rounds, final), disyolo_trace_edges (one launch over the list) and disyolo_trace_gather (gather, trunk rows);
* the bytes each of them has to move at least once, against the 6.29 TB/s the project measured for a device copy.
No threshold is set: there is no parent to compare with.
"""
import argparse
import json
import os
import sys
import time

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
    ap.add_argument("--noise", default=None, metavar="HxW", help="add one crop of random pixels (density 0.6): many nodes and branches")
    ap.add_argument("--txt", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("trace_rate: no GPU: nothing here can be measured without one")
    dev = torch.device("cuda:0")
    h, w = (int(v) for v in args.image.lower().split("x"))
    shapes = []
    synthetic_photo(h, w, defects=args.defects, shapes=shapes)
    crops = [np.ascontiguousarray(inside) for _, _, _, inside in shapes]
    if args.noise:
        nh, nw = (int(v) for v in args.noise.lower().split("x"))
        crops.append(np.random.default_rng(0).random((nh, nw)) < 0.6)
    groups, arena_np, nbytes = MZ.pack_masks(crops)
    arena = torch.from_numpy(arena_np).to(dev)
    groups_dev = torch.from_numpy(groups).to(dev)
    G = len(crops)
    rows_out = []

    def put(**kw):
        rows_out.append(kw)
        print(json.dumps(kw), flush=True)

    m = MZ.measure_arena(groups, arena, nbytes, groups_dev)
    g = None
    for mb in (0.0, args.min_branch):
        g = MZ.skeleton_graph(m, mb)
        t = MZ.skeleton_trace(g)
        ms, lo, hi = host_ms(lambda: MZ.skeleton_trace(g))
        weights = MZ.W_ORTH * g.branches["n_orth"] + MZ.W_DIAG * g.branches["n_diag"] + MZ.W_END * g.branches["n_end"]
        t0 = time.perf_counter()
        for i in range(G):
            k0, k1 = int(g._first[i]), int(g._first[i + 1])
            MZ.select_trunk(weights[k0:k1], np.stack([t.edges[c][k0:k1] for c in MZ.EDGE_COLUMNS], 1))
        select_ms = (time.perf_counter() - t0) * 1e3
        px = g.branches["px"]
        put(what="skeleton_trace per call", min_branch_px=mb, crops=G, arena_MB=round(nbytes / 1e6, 2), branches=len(g.branches),
            list_entries=int(px.sum()), junction_px=int(g.junction_px.sum()), nodes=len(t.nodes),
            rounds=(int(px.max()) - 1).bit_length() if len(px) else 0, trunk_px=int(t.trunk["px"].sum()),
            trunk_branches=int(t.trunk["n_branches"].sum()), trunk_length_px=round(float(t.trunk["trunk_length_px"].sum()), 1),
            pruned_length_px=round(float(g.pruned.length_px.sum()), 1), host_reads=2, ms=round(ms, 2), min=round(lo, 2),
            max=round(hi, 2), of_which_trunk_selection_on_the_host_ms=round(select_ms, 2))

    # the entry points on the graph pruned at --min-branch, with the buffers skeleton_trace would allocate
    px = g.branches["px"].astype(np.int64)
    n_list, n_junction, nb = int(px.sum()), int(g.junction_px.sum()), len(g.branches)
    rounds = (int(px.max()) - 1).bit_length() if nb else 0
    i32 = dict(dtype=torch.int32, device=dev)
    node_labels, noderow, rank, rank_diag = (torch.empty(nbytes, **i32) for _ in range(4))
    nodes = torch.empty(n_junction, L.TRACE_NODE, dtype=torch.int64, device=dev)
    ents = torch.empty(n_list, L.TRACE_ENT, **i32)
    nxt, val = torch.empty(4 * n_list, **i32), torch.empty(4 * n_list, dtype=torch.int64, device=dev)
    ctrl, count = torch.zeros(1, **i32), torch.zeros(1, **i32)
    n_rows = int(g.row_order.max()) + 1 if nb else 0
    edges = torch.empty(n_rows, L.TRACE_EDGE, dtype=torch.int64, device=dev)
    profile = torch.empty(n_list, L.TRACE_PROFILE, **i32)
    d2, links = m.d2_arena, g.links_arena

    def rate(name, fn, moved, **kw):
        us, lo, hi = events_us(fn)
        put(kernel=name, us=round(us, 1), min=round(lo, 1), max=round(hi, 1), MB=round(moved / 1e6, 2),
            TBps=round(moved / us / 1e6, 3), of_copy_rate=round(moved / us / 1e6 / COPY_TBS, 4),
            us_at_copy_rate=round(moved / COPY_TBS / 1e6, 1), **kw)

    # bytes per pixel moved at least once (neighbourhoods come from the cache; what only skeleton pixels touch is small beside
    # the arena): nodes = init (links 1 read, labels 4 written), merge (links 1), flatten (labels 4), alloc (labels 4),
    # accumulate (labels 4); rank = compact (labels 4 read, rank 4 + rank_diag 4 written) and per list entry the entry written
    # (48) and read by link and final (96), the link's states written (24), each round 24 read + 24 written, the final's 24 read
    # and 8 written; edges = the entry (48) and a row (96) per branch; gather = the entry (48) and 16 written per list entry
    def nodes_call():
        L.trace_nodes(groups, links, d2, node_labels, noderow, nodes, ctrl, groups_dev, nbytes)

    nodes_call()
    rate("trace_nodes (memset + init + merge + flatten + alloc + accumulate)", nodes_call, 18 * nbytes, junction_px=n_junction,
         nodes=int(ctrl[0]))

    def rank_call():
        L.trace_rank(groups, links, g.labels_arena, d2, g.rowid_arena, g.rows_dev, ents, rounds, nxt, val, count, rank, rank_diag,
                     groups_dev, nbytes)

    rate("trace_rank (memset + compact + link + %d rounds + final)" % rounds, rank_call,
         12 * nbytes + n_list * (48 + 96 + 24 + 48 * rounds + 32), list_entries=n_list, rounds=rounds, launches=3 + rounds)
    rate("trace_edges (1 launch over the list)",
         lambda: L.trace_edges(groups, ents, count, rank, rank_diag, node_labels, edges, groups_dev, nbytes), 48 * n_list + 96 * nb)
    t = MZ.skeleton_trace(g)                                          # (for a plan of the right size: the one it built is not kept)
    n_trunk = int(t.trunk["px"].sum())
    offsets = torch.zeros(n_rows, **i32)
    offsets[torch.from_numpy(g.row_order).to(dev)] = torch.from_numpy(np.concatenate([[0], np.cumsum(px)[:-1]]).astype(np.int32)).to(dev)
    seg = torch.full((n_rows, L.TRACE_SEG), -1, **i32)                 # no branch on a trunk: the branch profiles alone
    attach = torch.empty(0, L.TRACE_ATTACH, **i32)
    tprofile = torch.empty(0, L.TRACE_TRUNK_PROFILE, **i32)
    tstart = torch.zeros(G + 1, **i32)
    trunkrows = torch.empty(G, L.TRACE_TRUNK, dtype=torch.int64, device=dev)
    rate("trace_gather (branch profiles + trunk rows, an empty trunk plan)",
         lambda: L.trace_gather(groups, ents, count, rank, rank_diag, d2, offsets, profile, seg, edges, attach, tprofile, tstart,
                                trunkrows, groups_dev, nbytes), 64 * n_list,
         note="the trunk entries add 20 bytes each: %d of them in skeleton_trace's own call, which is not timed apart" % n_trunk)
    if args.txt:
        with open(args.txt, "w") as f:
            f.write("tools/trace_rate.py --image %s --defects %d --min-branch %s%s\n" % (
                args.image, args.defects, args.min_branch, " --noise " + args.noise if args.noise else ""))
            for r in rows_out:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()

"""What tiled detection costs beside the network, on one synthetic photograph, by HIP events and a host clock:

    python tools/tiles_rate.py [--image 3000x4000] [--size 576] [--batch 8] [--overlap 64] [--evaluate] [--json F] [--txt F]

One process measures
* ``tiles.detect_tiled`` per image (host clock around the call and a device synchronise, median of 5 after a warm-up);
* the same ceil(T / B) inference replays alone, on inputs that are already in the net's buffers (HIP events);
* the stages of detect_tiled by the host clock (each ended by a synchronise): gather + network + copies, the merge;
* each of the four kernels of csrc/tiles.hip on the tensors of that very image (HIP events, median of 7 calls), and for gather
  and paste-bits -- which move known byte counts -- the rate against the 6.29 TB/s the project measured for a device copy.

``--evaluate`` measures tiled evaluation instead, with the photograph's drawn shapes as ground truth (cracks class 0, blobs
class 1): ``MAP.collect_tiled`` per image beside ``detect_tiled`` (host clock), disyolo_tile_group_counts alone (HIP events,
replayed from a command list) with the bytes it has to read against the copy rate, the pair table's and the ground-truth cache's sizes, and the kernel
against ``collect``'s [nd, HW] x [HW, ng] f32 product on as many groups as that product is given room for.

The net has random weights with the heads scaled up (as the inference tests do), so every tile returns its 30 rows: the
tile-side work of a photograph full of detections, not of a typical one.  The image is noise with a few dozen drawn defects."""
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
from disyolo_amd import tiles as TL  # noqa: E402
from disyolo_amd.net import YOLONet  # noqa: E402

COPY_TBS = 6.29


def synthetic_photo(h, w, seed=0, defects=36, shapes=None):
    """grey noise with dark cracks (polylines a few pixels wide) and blobs; ``shapes``: a list that receives (kind, y0, x0,
    bool [bh,bw]) per drawn shape with pixels, kind 0 a crack and 1 a blob"""
    rng = np.random.default_rng(seed)
    img = rng.normal(150, 12, size=(h, w)).clip(0, 255)
    for k in range(defects):
        cy, cx = rng.uniform(0, h), rng.uniform(0, w)
        ang, half, length = rng.uniform(0, np.pi), rng.uniform(1.5, 4.0), rng.uniform(300, 2000)
        ry, rx = (rng.uniform(20, 200, size=2) if k % 2 else (length / 2 + 4, length / 2 + 4))
        y0, y1, x0, x1 = max(int(cy - ry), 0), min(int(cy + ry) + 1, h), max(int(cx - rx), 0), min(int(cx + rx) + 1, w)
        yy, xx = np.mgrid[y0:y1, x0:x1]
        box = img[y0:y1, x0:x1]                        # (a view: the defect is drawn inside its bounding box only)
        if k % 2:
            inside = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
            box[inside] = 70
        else:
            d = (yy - cy) * np.cos(ang) - (xx - cx) * np.sin(ang)
            s = (yy - cy) * np.sin(ang) + (xx - cx) * np.cos(ang)
            inside = (np.abs(d) <= half) & (np.abs(s) <= length / 2)
            box[inside] = 40
        if shapes is not None and inside.any():
            shapes.append((k % 2, y0, x0, inside))
    return np.repeat(img.astype(np.uint8)[:, :, None], 3, axis=2)


def events_us(fn, repeats=7):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        ts.append(s.elapsed_time(e) * 1e3)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def replay_us(fn, launches=8, repeats=7):
    """fn recorded ``launches`` times into a command list and replayed back to back: the device time per call, without the
    host's part of a call (which is longer than a short kernel)"""
    keep = []
    prog = L.CmdList()
    with prog:
        for _ in range(launches):
            keep.append(fn())
    prog.run()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        prog.run()
        e.record()
        torch.cuda.synchronize()
        ts.append(s.elapsed_time(e) * 1e3 / launches)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def host_ms(fn, repeats=5):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e3)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--image", default="3000x4000")
    ap.add_argument("--size", type=int, default=576)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--overlap", type=int, default=64)
    ap.add_argument("--thresh", type=float, default=0.05)
    ap.add_argument("--evaluate", action="store_true", help="measure tiled evaluation (MAP.collect_tiled) instead of the tile kernels")
    ap.add_argument("--product-groups", type=int, default=16,
                    help="--evaluate: the groups the [nd, HW] x [HW, ng] f32 product of collect is run on (4 HW bytes each)")
    ap.add_argument("--json", default=None)
    ap.add_argument("--txt", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tiles_rate: no GPU: nothing here can be measured without one")
    dev = torch.device("cuda:0")
    h, w = (int(v) for v in args.image.lower().split("x"))
    S, B = args.size, args.batch
    net = YOLONet(training=False, device=dev, image_size=S, batch_size=B, stage=1, seed=0)
    with torch.no_grad():
        for i in (59, 67, 75, net.score_layer):
            net.params["yolo/convolutional%d/weights" % i].mul_(6.0)
    net.refresh_weights()
    net.build_infer_program(det_thresh=args.thresh, graph=True)
    shapes = []
    rgb = torch.from_numpy(synthetic_photo(h, w, shapes=shapes)).to(dev)
    tiles = TL.plan_tiles(h, w, S, args.overlap)
    T = len(tiles)
    chunks = -(-T // B)
    rows = []

    def put(**kw):
        rows.append(kw)
        print(json.dumps(kw), flush=True)

    ms, lo, hi = host_ms(lambda: TL.detect_tiled(net, rgb, overlap=args.overlap, det_thresh=args.thresh))
    put(what="detect_tiled per image", image=[h, w], net=S, B=B, overlap=args.overlap, tiles=T, chunks=chunks, ms=round(ms, 2),
        min=round(lo, 2), max=round(hi, 2))
    if args.evaluate:
        measure_evaluate(args, net, rgb, shapes, (h, w), put)
        return write_out(args, rows, S, B)

    def replays():
        for _ in range(chunks):
            net.infer()
    us, lo, hi = events_us(replays)
    net_ms = us / 1e3
    put(what="the %d inference replays alone (resident inputs)" % chunks, ms=round(net_ms, 2), min=round(lo / 1e3, 2), max=round(hi / 1e3, 2))

    # ---- the stages, by the host clock
    res = TL.detect_tiled(net, rgb, overlap=args.overlap, det_thresh=args.thresh, keep_tiles=True)
    det, keep, masks = res.tile_outputs
    probe = {}
    ms_merge, lo, hi = host_ms(lambda: TL.merge_tiles(tiles, (h, w), S, det, keep, masks, 0.5))
    TL.merge_tiles(tiles, (h, w), S, det, keep, masks, 0.5, probe=probe)
    torch.cuda.synchronize()
    N, P, G = probe["instances"], int(probe["pairs"].shape[0]), int(probe["groups"].shape[0])
    put(what="merge_tiles (host tables + 3 launches + copies)", instances=N, pairs=P, groups=G,
        merged_groups=int(sum(len(m) > 1 for m in res.members)), ms=round(ms_merge, 2), min=round(lo, 2), max=round(hi, 2))
    put(what="gather + network + copies of the outputs (detect_tiled - merge_tiles)", ms=round(ms - ms_merge, 2))

    # ---- the four kernels on this image's tensors
    origins_d = probe["origins_dev"]
    out = torch.empty(chunks * B, S, S, 3, device=dev)

    def gather():
        for c in range(chunks):
            L.tile_gather(rgb, origins_d, c * B, (c + 1) * B, out[c * B:(c + 1) * B], S)
    us, lo, hi = events_us(gather)
    nbytes = out.numel() * 4 + rgb.numel()
    put(kernel="tile_gather", launches=chunks, us=round(us, 1), min=round(lo, 1), max=round(hi, 1), MB=round(nbytes / 1e6, 1),
        TBps=round(nbytes / us / 1e6, 3), of_copy_rate=round(nbytes / us / 1e6 / COPY_TBS, 3))
    planes = probe["planes"]
    if N:
        us, lo, hi = events_us(lambda: L.tile_paste_bits(probe["masks"], probe["rects"], S, planes))
        r = probe["rects"].cpu().numpy().astype(np.int64)
        nbytes = int(((r[:, 2] - r[:, 0]) * (r[:, 3] - r[:, 1])).sum()) * 4 + planes.numel() * 4      # the crops read once + the planes
        put(kernel="tile_paste_bits", instances=N, us=round(us, 1), min=round(lo, 1), max=round(hi, 1), MB=round(nbytes / 1e6, 1),
            TBps=round(nbytes / us / 1e6, 3), of_copy_rate=round(nbytes / us / 1e6 / COPY_TBS, 3),
            Gpixel_per_s=round(N * S * S / us / 1e3, 1))
    if P:
        us, lo, hi = events_us(lambda: L.tile_seam_counts(probe["pairs"], probe["inst_tile"], tiles, (h, w), planes, S,
                                                          probe["inst_tile_dev"], origins_d))
        put(kernel="tile_seam_counts (with the upload of the pair table)", pairs=P, us=round(us, 1), min=round(lo, 1), max=round(hi, 1))
    us, lo, hi = events_us(lambda: L.tile_compose(probe["groups"], probe["members"], probe["inst_tile"], tiles, planes, S, (h, w),
                                                  probe["arena"], probe["owner"], probe["inst_tile_dev"], origins_d))
    covered = sum(int(res.mask(g).sum()) for g in range(len(res)))          # (pixel, group) incidences: one atomicMax each
    put(kernel="tile_compose (with the upload of the group table)", groups=G, arena_MB=round(probe["arena"].numel() / 1e6, 1),
        covered_pixels=covered, us=round(us, 1), min=round(lo, 1), max=round(hi, 1),
        M_atomics_per_s=round(covered / us, 1))
    write_out(args, rows, S, B)


def write_out(args, rows, S, B):
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)
    if args.txt:
        with open(args.txt, "w") as f:
            f.write("tools/tiles_rate.py --image %s --size %d --batch %d --overlap %d --thresh %g%s\n" % (
                args.image, S, B, args.overlap, args.thresh, " --evaluate" if args.evaluate else ""))
            for r in rows:
                f.write(json.dumps(r) + "\n")


def measure_evaluate(args, net, rgb, shapes, image_hw, put):
    from disyolo_amd.evaluate import MAP
    h, w = image_hw
    dev = rgb.device
    recs, true_map = [], np.zeros((h, w), np.uint8)
    for kind, y0, x0, inside in shapes:
        m = np.zeros((h, w), bool)
        m[y0:y0 + inside.shape[0], x0:x0 + inside.shape[1]] = inside
        recs.append({"imageid": "photo", "classid": int(kind), "difficult": 0, "mask": m})
        true_map[m] = kind + 1
    emap = MAP({"photo": recs}, {"photo": [h, w]}, ["photo"], merged={"photo": true_map})
    res = TL.detect_tiled(net, rgb, overlap=args.overlap, det_thresh=args.thresh)
    G = len(res)
    conf = torch.zeros(16, dtype=torch.int64, device=dev)

    def collect():
        emap.collect_tiled("photo", res, {str(c): [] for c in emap.classid}, true_map=true_map, conf=conf)
    ms, lo, hi = host_ms(collect)                      # (the warm-up call builds and uploads the ground-truth cache)
    put(what="collect_tiled per image (pair table, one launch, fetch, ov rows, confusion)", groups=G, gt=len(recs),
        ms=round(ms, 2), min=round(lo, 2), max=round(hi, 2))
    # ---- the launch alone, on this image's tables
    gt, gt_dev, gt_bits, _ = emap._gt_planes("photo", dev)
    boxes, cls = res.boxes.astype(np.int64), res.classid.astype(np.int64)
    meet = ((cls[:, None] == gt[None, :, 4]) & (np.minimum(boxes[:, None, 2], gt[None, :, 2]) > np.maximum(boxes[:, None, 0], gt[None, :, 0]))
            & (np.minimum(boxes[:, None, 3], gt[None, :, 3]) > np.maximum(boxes[:, None, 1], gt[None, :, 1])))
    pg, pj = np.nonzero(meet)
    pairs2 = np.concatenate([np.stack([np.arange(G), np.full(G, -1)], 1), np.stack([pg, pj], 1)])
    pairs, blocks = L.tile_group_counts_plan(res.groups, gt, pairs2)
    pairs_dev = torch.from_numpy(pairs).to(dev)

    def rect_bytes(p2):
        """what the launch has to read: a byte per rectangle pixel of the group, and of the plane the words under each row"""
        total = 0
        for g, j in p2.tolist():
            y1, x1, y2, x2 = boxes[g]
            if j >= 0:
                t = gt[j].astype(np.int64)
                y1, x1, y2, x2 = max(y1, t[0]), max(x1, t[1]), min(y2, t[2]), min(x2, t[3])
                if y2 > y1 and x2 > x1:
                    total += (y2 - y1) * (((x2 - 1 - t[1]) >> 5) - ((x1 - t[1]) >> 5) + 1) * 4
            total += max(y2 - y1, 0) * max(x2 - x1, 0)
        return int(total)

    def launch(p=pairs, p_dev=pairs_dev):
        return L.tile_group_counts(res.groups, res.arena, gt, gt_bits, p, (h, w), groups_dev=res.groups_dev, gt_dev=gt_dev,
                                   pairs_dev=p_dev, arena_bytes=res.arena_bytes)
    us, lo, hi = replay_us(launch)
    us_call = events_us(launch)[0]
    nbytes = rect_bytes(pairs2)
    cache = gt.nbytes + int(gt_bits.numel()) * 4
    put(kernel="tile_group_counts (with the zeroing of counts; 8 recorded launches replayed back to back)",
        pairs=int(pairs.shape[0]), blocks=blocks, us=round(us, 1), us_per_call_from_python=round(us_call, 1),
        min=round(lo, 1), max=round(hi, 1), MB=round(nbytes / 1e6, 2), TBps=round(nbytes / us / 1e6, 3),
        of_copy_rate=round(nbytes / us / 1e6 / COPY_TBS, 4), us_at_copy_rate=round(nbytes / COPY_TBS / 1e6, 1))
    put(what="ground-truth cache per image", gt=len(recs), bit_planes_MB=round(cache / 1e6, 3),
        uint8_stack_of_the_batched_path_MB=round(len(recs) * h * w / 1e6, 1), arena_MB=round(res.arena_bytes / 1e6, 1))
    # ---- against collect's f32 product, on the first nd groups (4 HW bytes per detection, 4 HW per ground-truth column)
    nd = min(G, args.product_groups)
    if nd:
        sel = pairs2[pairs2[:, 0] < nd]
        p_nd, _ = L.tile_group_counts_plan(res.groups, gt, sel)
        p_nd_dev = torch.from_numpy(p_nd).to(dev)
        us_k, lo_k, hi_k = replay_us(lambda: launch(p_nd, p_nd_dev))
        d = torch.stack([res.full_mask(g) for g in range(nd)]).reshape(nd, -1).to(torch.float32)
        g32 = torch.from_numpy(np.stack([r["mask"] for r in recs]).reshape(len(recs), -1)).to(dev).to(torch.float32).t().contiguous()
        us_p, lo_p, hi_p = events_us(lambda: (d @ g32, d.sum(1)))
        inter = (d @ g32).cpu().numpy()
        cnt = launch(p_nd, p_nd_dev).cpu().numpy()
        same = all(int(inter[g, j]) == int(c) for (g, j), c in zip(sel.tolist(), cnt) if j >= 0)
        put(what="the first %d groups: the kernel against collect's [nd, HW] x [HW, ng] f32 product and row sums" % nd,
            kernel_us=round(us_k, 1), kernel_pairs=int(p_nd.shape[0]), product_us=round(us_p, 1),
            product_operands_MB=round((d.numel() + g32.numel()) * 4 / 1e6, 1), ratio=round(us_p / us_k, 1), counts_equal=bool(same))


if __name__ == "__main__":
    main()

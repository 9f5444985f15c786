"""End-to-end example on synthetic data (needs an MI355X): polygon annotations -> GPU data pipeline ->
Solver (recorded pipelined step: the next batch's backbone and its data loading beside the current step) -> TF-format checkpoint -> reload into an
inference net -> detections + instance masks for one image.

    python examples/train_synthetic.py [--steps 40] [--size 192 | --size 128x192] [--batch 4] [--out /tmp/disyolo_example] [--lock 62-64]
                                       [--classes crack,spall,rebar,stain,joint,void]
                                       [--max-boxes 100] [--max-det 100] [--anchors auto | --anchors w,h,w,h,... (9 pairs)]
                                       [--tiled 500x700 [--measure [--mm-per-px 0.25] [--min-branch 10 [--trunk]]] [--shape [--axis-deg 0]]
                                                        [--outline [FILE.json]]]
                                       [--windows 600x800]

It mirrors what the reference's ``train_yolo3_mask.py:237-248`` (train) and ``calculate_test_map.py`` (test) do
with a real dataset; swap ``synthetic_labels`` for ``disyolo_amd.pre_process.load_verify_contour(path, 'train')``
records (plus the decoded images) to train on one.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import disyolo_amd  # noqa: E402,F401
from disyolo_amd import checkpoint, config as cfg, postprocess  # noqa: E402
from disyolo_amd.net import YOLONet  # noqa: E402
from disyolo_amd.solver import Solver  # noqa: E402
from disyolo_amd.train_data import cluster_anchors, defect_train  # noqa: E402


def synthetic_labels(rng, n, classes=None):
    """n records in the layout of the reference's ground-truth cache: an RGB image, one class name and one list of
    polygons ('out' = outline, 'in' = hole) per instance"""
    classes = cfg.CLASSES if classes is None else classes
    out = []
    for _ in range(n):
        h, w = rng.randint(200, 320), rng.randint(200, 320)
        image = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
        polys, names = [], []
        for _j in range(rng.randint(1, 4)):
            cy, cx = rng.uniform(0.3, 0.7) * h, rng.uniform(0.3, 0.7) * w
            ry, rx = rng.uniform(0.1, 0.25) * h, rng.uniform(0.1, 0.25) * w
            t = np.sort(rng.uniform(0, 2 * np.pi, rng.randint(6, 10)))
            polys.append([{"type": "out", "all_points_x": np.clip(cx + rx * np.cos(t), 0, w - 1).astype(int).tolist(),
                           "all_points_y": np.clip(cy + ry * np.sin(t), 0, h - 1).astype(int).tolist()}])
            names.append(classes[rng.randint(0, len(classes))])
        out.append({"image": image, "class_names": names, "polygons": polys})
    return out


def large_labels(rng, n, size, classes=None, instances=12):
    """n records of ``size`` = (h, w) -- inspection photographs far larger than the net -- each with ``instances`` small
    defects (radii of 6 .. 60 pixels, whatever the image's size); the image is one noise patch repeated"""
    classes = cfg.CLASSES if classes is None else classes
    h, w = (size, size) if isinstance(size, int) else size
    out = []
    for _ in range(n):
        patch = rng.randint(0, 256, (min(h, 256), min(w, 256), 3)).astype(np.uint8)
        image = np.ascontiguousarray(np.tile(patch, (-(-h // patch.shape[0]), -(-w // patch.shape[1]), 1))[:h, :w])
        polys, names = [], []
        for _j in range(instances):
            ry, rx = rng.uniform(6, min(60, h / 4)), rng.uniform(6, min(60, w / 4))
            cy, cx = rng.uniform(ry, h - 1 - ry), rng.uniform(rx, w - 1 - rx)
            t = np.sort(rng.uniform(0, 2 * np.pi, rng.randint(6, 10)))
            polys.append([{"type": "out", "all_points_x": np.clip(cx + rx * np.cos(t), 0, w - 1).astype(int).tolist(),
                           "all_points_y": np.clip(cy + ry * np.sin(t), 0, h - 1).astype(int).tolist()}])
            names.append(classes[rng.randint(0, len(classes))])
        out.append({"image": image, "class_names": names, "polygons": polys})
    return out


def parse_lock(text):
    """"5-9,62-64" -> {5: True, ..., 9: True, 62: True, 63: True, 64: True}; a leading "!" unlocks ("!40-52": train conv40-52
    in stage 1).  The reference's per-layer ``lock`` argument (yolo/yolo3_net_pos.py:71-146) over the stage's map."""
    lock = {}
    for part in filter(None, (p.strip() for p in (text or "").split(","))):
        value = not part.startswith("!")
        lo, _, hi = part.lstrip("!").partition("-")
        for i in range(int(lo), int(hi or lo) + 1):
            lock[i] = value
    return lock


def parse_size(text):
    """"192" -> 192 (a square net), "128x192" -> (128, 192) = (H, W): what YOLONet, defect_train, image_read and
    paste_detections take as the net's size"""
    if "x" in text.lower():
        h, _, w = text.lower().partition("x")
        return int(h), int(w)
    return int(text)


def parse_anchors(text):
    """"auto" -> "auto" (cluster the dataset's boxes); "w,h,w,h,..." -> float32 [9, 2]; "" -> None (cfg.ANCHORS)"""
    if not text:
        return None
    if text == "auto":
        return "auto"
    vals = [float(v) for v in text.split(",")]
    if len(vals) != 18:
        raise argparse.ArgumentTypeError("--anchors takes 'auto' or 18 numbers w,h,... (got %d)" % len(vals))
    return np.asarray(vals, np.float32).reshape(9, 2)


def parse_mask_rois(text):
    """"40,20" -> (40, 20) = (mask_roi_det, mask_roi_gt): the detections and the ground-truth boxes of an image the mask loss
    trains on per step, each 0..256, at least one in all (the reference's `[:7]` and `[:3]`, yolo/yolo3_net_pos.py:783)"""
    parts = text.split(",")
    if len(parts) != 2:
        raise argparse.ArgumentTypeError("--mask-rois takes N_DET,N_GT (got %r)" % text)
    return int(parts[0]), int(parts[1])


def print_measures(res, classes, mm_per_px, min_branch=None, trunk=False):
    """length, width and area of every merged instance, measured on the GPU from the result's cropped masks; with
    ``min_branch`` also the graph of every skeleton: its branches, its junction pixels and its length without the spurs; with
    ``trunk`` also the main path of every graph: its length, its widest point and where in the image that is"""
    from disyolo_amd.measure import measure_instances, skeleton_graph, skeleton_trace
    m = measure_instances(res, mm_per_px=mm_per_px)
    print("measured %d instances (%d thinning iterations):" % (len(m), m.iterations))
    graph = None if min_branch is None else skeleton_graph(m, min_branch_px=min_branch)
    if graph is not None:
        print("skeleton graphs: spurs below %.1f px pruned in %d analyses (%d of %d instances converged), %d branches" % (
            min_branch, graph.analyses, int(graph.converged.sum()), len(graph), len(graph.branches)))
    traced = skeleton_trace(graph) if trunk else None
    if traced is not None:
        print("skeleton traces: %d nodes, trunks of %d branches in all" % (len(traced.nodes), int(traced.trunk["n_branches"].sum())))
    for row in (m if graph is None else graph if traced is None else traced).table(classes):
        line = "  %3d %-8s %.2f  area %7d px  length %8.1f px  width max %6.1f mean %6.1f px" % (
            row["instance"], row["class"], row["score"], row["area_px"], row["length_px"], row["max_width_px"], row["mean_width_px"])
        if mm_per_px is not None:
            line += "  |  %8.1f mm2  length %7.1f mm  width max %5.1f mean %5.1f mm" % (
                row["area_mm2"], row["length_mm"], row["max_width_mm"], row["mean_width_mm"])
        if graph is not None:
            line += "  |  pruned length %8.1f px  %3d branches  %3d junction px" % (
                row["pruned_length_px"], row["n_branches"], row["junction_px"])
        if traced is not None:
            line += "  |  trunk %8.1f px over %2d branches, widest %5.1f px at (%d, %d)" % (
                row["trunk_length_px"], row["trunk_branches"], row["trunk_max_width_px"], row["trunk_widest_yx"][0], row["trunk_widest_yx"][1])
            if mm_per_px is not None:
                line += " = %7.1f mm, widest %5.1f mm" % (row["trunk_length_mm"], row["trunk_max_width_mm"])
        print(line)


def print_shapes(res, classes, mm_per_px, axis_deg=None):
    """orientation, enclosing rectangle, perimeter, parts and holes of every merged instance, from the result's cropped masks
    alone (no thinning); with ``axis_deg`` also whether it runs along, across or diagonal to the member's axis"""
    from disyolo_amd.measure import instance_shapes
    s = instance_shapes(res, mm_per_px=mm_per_px, axis_deg=axis_deg)
    print("shapes of %d instances (%d directions):" % (len(s), len(s.directions)))
    for row in s.table(classes):
        line = "  %3d %-8s %.2f  area %7d px  at %5.1f deg  rect %7.1f x %6.1f px at %5.1f deg  perimeter %8.1f px  %2d parts (largest %d px)  %2d holes" % (
            row["instance"], row["class"], row["score"], row["area_px"], row["orientation_deg"], row["rect_long_px"], row["rect_short_px"],
            row["rect_angle_deg"], row["perimeter_px"], row["n_parts"], row["largest_part_px"], row["n_holes"])
        if mm_per_px is not None:
            line += "  |  rect %6.1f x %5.1f mm  perimeter %7.1f mm" % (row["rect_long_mm"], row["rect_short_mm"], row["perimeter_mm"])
        if axis_deg is not None:
            line += "  |  %s" % row["direction"]
        print(line)


def print_outlines(res, classes, image_hw, path):
    """the loop table of ``instance_outlines`` and, with a path, the loader's record of the detections as JSON"""
    import json
    from disyolo_amd import measure
    o = measure.instance_outlines(res)
    print("outlines: %d loops of %d instances, %d border pixels, %d corners" % (len(o.loops), len(o), int(o.point_offsets[-1]),
                                                                            int(o.corner_offsets[-1])))
    print("  loop inst class    kind  depth parent   edges  points corners   area_px  first point")
    for i, row in enumerate(o.table(classes)):
        if i == 40:
            print("  ... and %d more" % (len(o.loops) - 40))
            break
        x, y = (int(v) for v in o.points(i)[0])
        print("  %4d %4d %-8s %-5s %5d %6d %7d %7d %7d %9.1f  (%d, %d)" % (
            i, row["instance"], row["class"], row["kind"], row["depth"], row["parent"], row["n_edges"], row["n_points"], row["n_corners"],
            row["area_px"], x, y))
    if path:
        with open(path, "w") as f:
            json.dump(o.record(image_size=image_hw, class_names=classes), f)
        print("outlines: the record of %d instances written to %s" % (len(set(o.loops[:, 0].tolist())), path))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--size", type=parse_size, default=192,
                    help="the net's input size: S (a square) or HxW, each side a multiple of 32 (e.g. 128x192)")
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--out", default="/tmp/disyolo_example")
    ap.add_argument("--k-map", type=int, default=cfg.K_MAP, choices=(3, 5, 7),
                    help="position-sensitive mask grid (k x k score maps, cfg.K_MAP)")
    ap.add_argument("--mask-stride", type=int, default=cfg.MASK_STRIDE, choices=(4, 2, 1),
                    help="mask subnet: score maps at size/4, size/2 (cfg.MASK_STRIDE) or size (m = 1/4, 1/2, 1)")
    ap.add_argument("--lock", default="", help="layer ranges to lock on top of stage 1, e.g. 5-9,62-64 (\"!40-52\" unlocks)")
    ap.add_argument("--classes", default=",".join(cfg.CLASSES),
                    help="comma-separated class list, 1 to 80 names (cfg.CLASSES): it sizes the heads, the targets and the metric")
    ap.add_argument("--nms", default=cfg.NMS_METHOD, choices=("per_class", "agnostic", "none"),
                    help="detection filter: greedy NMS inside each class (cfg.NMS_METHOD), one class-agnostic NMS per image, "
                         "or no suppression; it picks the mask-loss RoIs in training and what is pasted at test time")
    ap.add_argument("--max-boxes", type=int, default=cfg.MAX_BOX_PER_IMAGE,
                    help="ground-truth instances an image carries, 1..256 (cfg.MAX_BOX_PER_IMAGE): net and loader")
    ap.add_argument("--max-det", type=int, default=cfg.MAX_DETECTION,
                    help="detections an image yields, 1..256 (cfg.MAX_DETECTION)")
    ap.add_argument("--anchors", type=parse_anchors, default=None,
                    help="the nine anchors (w, h) in net pixels, smallest first: 'auto' clusters the dataset's boxes at --size "
                         "(train_data.cluster_anchors), or 18 numbers w,h,...; cfg.ANCHORS unless given")
    ap.add_argument("--mask-rois", type=parse_mask_rois, default=(cfg.MASK_ROI_DET, cfg.MASK_ROI_GT), metavar="N_DET,N_GT",
                    help="RoIs per image of the mask loss: the first N_DET detections and the first N_GT ground-truth boxes in "
                         "shuffled order, each 0..256 (cfg.MASK_ROI_DET, cfg.MASK_ROI_GT); 256,256 takes them all")
    ap.add_argument("--tiled", type=parse_size, default=None, metavar="HxW",
                    help="also run the trained net over one synthetic image of this size, larger than the net, cut into "
                         "overlapping tiles whose instances are merged over the seams (disyolo_amd.tiles.detect_tiled)")
    ap.add_argument("--measure", action="store_true",
                    help="with --tiled or --windows: print length, width and area of every merged instance "
                         "(disyolo_amd.measure.measure_instances)")
    ap.add_argument("--mm-per-px", type=float, default=None, help="--measure: the image's scale; adds the columns in mm and mm^2")
    ap.add_argument("--min-branch", type=float, default=None, metavar="PX",
                    help="--measure: also build the graph of every skeleton and prune its spurs shorter than this many pixels "
                         "(a multiple of 0.5; disyolo_amd.measure.skeleton_graph): adds the pruned length, the branches and "
                         "the junction pixels")
    ap.add_argument("--trunk", action="store_true",
                    help="--min-branch: also trace every pruned graph (disyolo_amd.measure.skeleton_trace) and print the trunk of "
                         "every instance -- the path between its two farthest ends -- with its length, its widest point and where "
                         "in the image that is")
    ap.add_argument("--shape", action="store_true",
                    help="with --tiled: print orientation, enclosing rectangle, perimeter, parts and holes of every merged instance "
                         "(disyolo_amd.measure.instance_shapes; --mm-per-px adds the columns in mm)")
    ap.add_argument("--axis-deg", type=float, default=None, metavar="DEG",
                    help="--shape: the member's longitudinal axis in the image, in degrees from +x towards +y; adds whether an "
                         "instance runs longitudinal, transverse or diagonal to it")
    ap.add_argument("--outline", nargs="?", const="", default=None, metavar="FILE.json",
                    help="with --tiled: print the ordered borders of every merged instance -- outer borders, holes, islands in "
                         "holes (disyolo_amd.measure.instance_outlines) -- and, with a file name, write them as one record of the "
                         "loader (image_size, class_names, polygons) to check in an annotation tool or to train on")
    ap.add_argument("--windows", type=parse_size, default=None, metavar="HxW",
                    help="window training: the records are synthetic images of this size, larger than the net, and every "
                         "batch image is a net-size window of one of them at scale 1 (defect_train(placement='window')); at "
                         "the end the trained net runs over one whole record with detect_tiled")
    args = ap.parse_args()
    if args.min_branch is not None and not args.measure:
        ap.error("--min-branch extends the table of --measure: give --measure too")
    if args.trunk and args.min_branch is None:
        ap.error("--trunk traces the graph of --min-branch: give --min-branch too (0 prunes nothing)")
    if args.shape and args.tiled is None:
        ap.error("--shape describes the instances of detect_tiled: give --tiled HxW")
    if args.outline is not None and args.tiled is None:
        ap.error("--outline outlines the instances of detect_tiled: give --tiled HxW")
    if args.axis_deg is not None and not args.shape:
        ap.error("--axis-deg classifies the orientations of --shape: give --shape too")
    if args.measure and args.tiled is None and args.windows is None:
        ap.error("--measure measures the instances of detect_tiled: give --tiled HxW or --windows HxW")
    classes = [c.strip() for c in args.classes.split(",")]
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(0)
    labels = synthetic_labels(rng, 16, classes) if args.windows is None else large_labels(rng, 8, args.windows, classes)
    placement = {} if args.windows is None else {"placement": "window"}
    anchors = args.anchors
    if isinstance(anchors, str):
        anchors = cluster_anchors(labels, args.size)
        print("anchors from the dataset's boxes at this size:", np.round(anchors, 1).tolist())
    limits = dict(anchors=anchors, max_box_per_image=args.max_boxes)

    # --- train: stage 1 (conv1-52 locked), batches built on the GPU from the polygon records
    data = defect_train(labels, batch_size=args.batch, image_size=args.size, device=dev, rng=np.random.RandomState(1),
                        classes=classes, **limits, **placement)
    net = YOLONet(training=True, device=dev, image_size=args.size, batch_size=args.batch, stage=1, seed=0, k_map=args.k_map,
                  mask_stride=args.mask_stride, lock=parse_lock(args.lock), classes=classes, nms=args.nms, max_detection=args.max_det,
                  mask_roi_det=args.mask_rois[0], mask_roi_gt=args.mask_rois[1], **limits)
    if net.pass_through_layers():
        print("locked layers the gradient crosses:", net.pass_through_layers())
    solver = Solver(net, data, output_dir=args.out, max_iter=args.steps, summary_iter=max(1, args.steps // 4),
                    save_iter=args.steps, log=print)
    hist = solver.train()
    finite = [h for h in hist if np.isfinite(h)]
    print("loss: first %.1f -> last %.1f over %d steps (%d finite)" % (finite[0], finite[-1], len(hist), len(finite)))

    # --- test: reload the checkpoint the Solver wrote into an inference net
    prefix = checkpoint.latest_checkpoint(os.path.join(args.out, "checkpoint"))
    print("restoring", prefix)
    inf = YOLONet(training=False, device=dev, image_size=args.size, batch_size=1, stage=1, seed=123, k_map=args.k_map,
                  mask_stride=args.mask_stride, classes=classes, nms=args.nms, max_detection=args.max_det, **limits)
    checkpoint.restore_net(inf, prefix)
    rec = labels[0]
    from disyolo_amd.evaluate import image_read
    image, window = image_read(rec["image"], args.size, device=dev)
    window = torch.as_tensor(window, dtype=torch.float32).reshape(1, 4)
    det_boxes, det_masks = inf.evaluation(image[None], window, det_thresh=0.05, masks_on_device=True)
    h, w = rec["image"].shape[:2]
    entries, merged = postprocess.paste_detections(det_boxes[0], det_masks[0], h, w, args.size)
    print("%d detections on a %dx%d image; class map has %d labelled pixels" % (len(entries), h, w, int((merged > 0).sum())))

    # --- window training: the net saw its records at scale 1, so it is run over a whole record the same way, as tiles
    if args.windows is not None:
        from disyolo_amd import tiles
        res = tiles.detect_tiled(inf, rec["image"], overlap=(inf.H // 8, inf.W // 8), det_thresh=0.05)
        print("windows: trained on %dx%d windows of %dx%d records; detect_tiled on the first record: %d tiles -> %d instances "
              "(%d annotated), class map has %d labelled pixels" % (inf.H, inf.W, h, w, len(res.tiles), len(res), len(rec["polygons"]),
                                                                   int((res.merged > 0).sum())))
        if args.measure:
            print_measures(res, classes, args.mm_per_px, args.min_branch, args.trunk)

    # --- an image larger than the net: tiles of the net's size, an instance that runs through several tiles becomes one
    if args.tiled is not None:
        from disyolo_amd import tiles
        th, tw = (args.tiled, args.tiled) if isinstance(args.tiled, int) else args.tiled
        big = np.tile(rec["image"], (-(-th // h), -(-tw // w), 1))[:th, :tw]        # the first record, repeated to HxW
        nh, nw = inf.H, inf.W
        res = tiles.detect_tiled(inf, big, overlap=(nh // 8, nw // 8), det_thresh=0.05)
        joined = sum(len(m) > 1 for m in res.members)
        print("tiled: %d tiles of %dx%d on a %dx%d image -> %d instances (%d of them joined over a seam); class map has %d "
              "labelled pixels" % (len(res.tiles), nh, nw, th, tw, len(res), joined, int((res.merged > 0).sum())))
        for g in range(min(len(res), 3)):
            y1, x1, y2, x2 = res.boxes[g]
            print("  %s %.2f box (%d, %d)-(%d, %d), %d pixels, from tiles %s" % (
                classes[res.classid[g]], res.score[g], y1, x1, y2, x2, int(res.mask(g).sum()), sorted({t for t, _ in res.members[g]})))
        if args.measure:
            print_measures(res, classes, args.mm_per_px, args.min_branch, args.trunk)
        if args.shape:
            print_shapes(res, classes, args.mm_per_px, args.axis_deg)
        if args.outline is not None:
            print_outlines(res, classes, (th, tw), args.outline)
        # the metric of the whole image against the records it was drawn from: every repeat of an instance is an instance
        from disyolo_amd.evaluate import MAP, evaluate
        from disyolo_amd.train_data import rasterize_instance
        recs, true_map = [], np.zeros((th, tw), np.uint8)
        for name, polys in zip(rec["class_names"], rec["polygons"]):
            one = rasterize_instance(polys, h, w, dev).cpu().numpy() > 0
            for y0 in range(0, th, h):
                for x0 in range(0, tw, w):
                    m = np.zeros((th, tw), bool)
                    m[y0:y0 + h, x0:x0 + w] = one[:th - y0, :tw - x0]
                    if m.any():
                        recs.append({"imageid": "big", "classid": classes.index(name), "difficult": 0, "mask": m})
                        true_map[m] = classes.index(name) + 1
        big_map = MAP({"big": recs}, {"big": [th, tw]}, ["big"], merged={"big": true_map}, classes=classes)
        thresh_out, mask_acc, timing = evaluate(inf, {"big": big}, big_map, det_thresh=0.05,
                                                tiled={"overlap": (nh // 8, nw // 8), "merge_overlap": 0.5})
        print("tiled evaluation against %d ground-truth instances: AP %s, (recall, precision, mAP) %s, mIoU %.3f; "
              "detect_tiled %.1f ms, collect_tiled %.1f ms" % (
                  len(recs), np.round(thresh_out[0]["AP"], 3).tolist(), np.round(thresh_out[0]["mAP"], 3).tolist(), mask_acc[-1],
                  timing["prediction_s"] * 1e3, timing["crop_assemble_s"] * 1e3))


if __name__ == "__main__":
    main()

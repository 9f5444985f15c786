"""Instance measurement: how long, how wide and how large every instance of a ``TiledDetections`` is -- the question an
inspection user asks of a crack or a spall -- in pixels and, given a scale, in millimetres.

The reference has nothing like it; the definition is tests/measure_ref.py and the pixel work csrc/measure.hip, a few launches
over the arena of cropped masks ``lib.tile_compose`` wrote:

    m = measure_instances(detect_tiled(net, image_rgb), mm_per_px=0.25)
    m.length_px, m.max_width_px, m.mean_width_px, m.area_px, m.table(class_names)
    m.d2(g), m.skeleton(g)

  d2        the exact squared Euclidean distance of every mask pixel to the background (everything outside the crop is
            background), in int32;
  skeleton  Zhang-Suen thinning of the mask, iterated until an iteration deletes nothing;
  length_px = n_orth + sqrt(2) n_diag + n_end / 2 over the skeleton's links and end points,
  max_width_px = 2 sqrt(max d2) - 1,  mean_width_px = 2 mean over the skeleton of sqrt(d2) - 1.

What Zhang-Suen thinning does to the numbers: a 2x2 square and a 2-pixel-wide diagonal stroke are deleted completely
(skeleton_px = 0: the length is 0 and the mean width is the maximum width); of an even-width bar one row is kept, so even
widths read one pixel low; a bar of width w comes out about w shorter.

Host synchronisations: the reads of the "still changing" flags, one per ``chunk`` thinning iterations, and the one copy of the
count tables at the end.  Nothing else waits for the device; G = 0 launches nothing.

The graph of the skeleton (csrc/skeleton.hip, defined by tests/skeleton_ref.py) goes on from there:

    g = skeleton_graph(m, min_branch_px=10)
    g.n_branches, g.junction_px, g.pruned.length_px, g.branches, g.branches_of(0), g.table(class_names)
    g.links(i), g.labels(i), g.pruned_skeleton(i)

  links     two skeleton pixels are linked when adjacent in a row or a column, or diagonal with neither pixel completing their
            2x2 square on the skeleton; a junction pixel has three links or more;
  branch    a connected run of the other pixels, named by its smallest pixel (root_y, root_x), with its pixel count, length,
            end points, attachments to junction pixels, mean / maximum / minimum width and kind (loop, free, terminal, inner);
  spur      a branch with one end, one attachment and a length below min_branch_px; every spur is deleted at once, the rest is
            analysed again, until no spur is left or max_rounds prunings were made.  All of it in integers.

What the pruning rule does to the numbers: the short end piece of a crack beyond its last spur is itself a spur and goes with
it, so up to min_branch_px is lost per end; a star whose arms are all short is pruned to its junction pixel; a plain T with
arms 10.5 / 10.5 / 9.5 loses the 9.5 arm at min_branch_px = 10.

The traced graph (csrc/trace.hip, defined by tests/trace_ref.py) orders what the graph left loose:

    t = skeleton_trace(g)
    t.nodes, t.nodes_of(i), t.edges, t.edges_of(i), t.rank(i), t.rank_diag(i), t.node_labels(i), t.branch_profile(i, root)
    t.trunk, t.trunk_branches(i), t.trunk_profile(i), t.table(class_names)

  node      a cluster of junction pixels joined by links, named by its smallest pixel, with its pixel count, centroid, largest
            d2 and attachments;
  rank      the steps of a branch pixel from its branch's start (a path's end pixel with the smaller index; a loop's root, walked
            first to the neighbour with the smaller index), rank_diag the diagonal ones among them; an edge row says what the two
            ends of a branch are: a node, a free end or a loop;
  trunk     the main path of an instance: between the two vertices (nodes and free ends) whose shortest-path distance over the
            branches is largest, with its ordered profile (y, x, d2, cum_orth, cum_diag), its length, mean and maximum width
            and where it is widest.  The pixel work is integers on the GPU; the path is chosen on the host from the tables.

What the trunk rule does to the numbers: a ring with a tail has the tail as its trunk (a branch from a node back to itself is
never on a shortest path); of two arms between the same two nodes the shorter is taken; a crossing through a thick junction is
measured straight from attach pixel to attach pixel; an instance of closed loops only has its heaviest loop as trunk.  Host
synchronisations of skeleton_trace: one read of the edge and node tables, one of the trunk rows.

The shape of an instance (csrc/shape.hip, defined by tests/shape_ref.py) needs no skeleton: it reads the
mask arena alone, so it takes a ``TiledDetections`` as well as anything above:

    s = instance_shapes(detect_tiled(net, image_rgb), mm_per_px=0.25, axis_deg=0.0)
    s.orientation_deg, s.rect_long_px, s.rect_short_px, s.rect_angle_deg, s.perimeter_px, s.n_parts, s.n_holes, s.direction
    s.extents(g), s.rect_corners(g), s.part_labels(g), s.table(class_names)

  sums      n, Sy, Sx, Syy, Sxx, Sxy over the mask, its tight box and Gray's bit quads Q1, Q2, Q3, Q4, QD: the raw int64 table.
            From it the centroid, the orientation of the major axis (image axes, from +x towards +y, y down: np.eye(9) lies at 45
            degrees), the axes of the ellipse with the same moments, the perimeter Q2 + (Q1 + Q3 + 2 QD) / sqrt(2), the exact count
            of pixel sides ``edges`` and the Euler number;
  parts     the 8-connected components (labels = their smallest pixel index), how many and the largest: whether the merge joined
            one piece or five fragments; n_holes = n_parts - euler8 counts the 4-connected holes;
  extents   the minimum and maximum of c x + s y over the mask for K directions (a fixed-point table made on the host): Feret
            diameters and the smallest of the K / 2 enclosing rectangles, with its long and short side, angle and corners;
  direction longitudinal / transverse / diagonal against the member's axis ``axis_deg``, "none" for a blob that is not elongated.

What the rules do to the numbers: the rectangle is the best of K / 2 orientations, not the true minimum (K = 180: the long side of
a bar is overestimated by at most short * sin 1 degree); feret_max of a 1 x 9 bar is 9.06 at 6 degrees, the diagonal of the pixel
squares; a diagonal gap closes a hole's wall but does not join two holes.  Host synchronisations of instance_shapes: one read of
the three tables at the end; G = 0, or groups without pixels, launch nothing and read nothing.

The outlines of an instance (csrc/outline.hip, defined by tests/outline_ref.py) turn it back into what
annotation tools and the loader exchange: closed borders.

    o = instance_outlines(s)            # s = instance_shapes(...), or anything instance_shapes takes
    o.loops, o.loops_of(g), o.points(i), o.corners(i), o.parts, o.polygons(g), o.record(image_size=(h, w)), o.table(class_names)

  loop      a cycle of the successor permutation of the boundary edges (pixel sides between foreground and background, walked
            clockwise, the diagonal tested first: 8-connected foreground); outer borders and holes, each with its depth and parent;
  points    the pixel border as cv2.findContours(RETR_TREE, CHAIN_APPROX_NONE) lists it, start point included;
  corners   the ring of turning corners on the corner grid, whose shoelace sum is exactly twice the enclosed area;
  record    the polygons sorted by (depth, key): 'out' and 'in' alternate with the depth, so an island in a hole is drawn after
            the hole -- with all 'out' before all 'in' the loader loses it.

Host synchronisations of instance_outlines with an InstanceShapes given: one read of the loop table, one of the points and
corners (none with points=False); G = 0, or masks without a pixel, launch nothing and read nothing.

Working memory of skeleton_graph beside what measure_arena holds: two int32 arenas (labels, row numbers), two byte arenas
(links, the pruned skeleton) and the row buffer.  Its host synchronisations: one read per analysis (the row counter and the
per-group spur flags in one copy; once more if the row buffer was too small) and the final copy.
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import lib as L

COUNT_COLUMNS = ("area", "skel_px", "n_orth", "n_diag", "n_end", "max_d2", "max_d2_skel", "zero")
MAX_SIDE = 32767      # the largest box side the kernels take (every intermediate of d2 then fits int32)


class InstanceMeasures:
    """What ``measure_instances`` / ``measure_masks`` return.  For the G instances, numpy [G]:
      area_px, skeleton_px, endpoints (int64); length_px, max_width_px, mean_width_px (float64)
      counts int64 [G,8] (COUNT_COLUMNS) and sum_sqrt float64 [G]: the raw tables the numbers are derived from
      group_iterations int32 [G]; iterations = their maximum: the thinning iterations that were run, counting each group's
                last one, which deleted nothing
      d2(g) int32 CUDA view [bh,bw]; skeleton(g) bool CUDA view [bh,bw]
      mm_per_px, and with it length_mm, max_width_mm, mean_width_mm, area_mm2
      table(class_names) one dict per instance
      groups, groups_dev, arena, arena_bytes: the groups table, its device copy, the mask arena and the bytes of it in use, for
                ``skeleton_graph`` to go on from"""

    def __init__(self, boxes, offsets, d2_arena, skel_arena, counts, sum_sqrt, group_iterations, mm_per_px=None, classid=None,
                 score=None):
        self.boxes, self._offsets = np.asarray(boxes, np.int32).reshape(-1, 4), list(offsets)
        self.d2_arena, self.skeleton_arena = d2_arena, skel_arena
        self.counts = np.asarray(counts, np.int64).reshape(-1, 8)
        self.sum_sqrt = np.asarray(sum_sqrt, np.float64).reshape(-1)
        self.group_iterations = np.asarray(group_iterations, np.int32).reshape(-1)
        self.iterations = int(self.group_iterations.max()) if self.group_iterations.size else 0
        self.classid, self.score = classid, score
        # what ``skeleton_graph`` needs to go on from here: the groups table, its device copy, the mask arena and the bytes of
        # it in use (set by measure_arena)
        self.groups, self.groups_dev, self.arena, self.arena_bytes = None, None, None, 0
        c = self.counts
        self.area_px, self.skeleton_px, self.endpoints = c[:, 0].copy(), c[:, 1].copy(), c[:, 4].copy()
        some, skel = c[:, 0] > 0, c[:, 1] > 0
        length = c[:, 2] + np.sqrt(2.0) * c[:, 3] + c[:, 4] / 2.0
        wmax = 2.0 * np.sqrt(c[:, 5].astype(np.float64)) - 1.0
        wmean = 2.0 * self.sum_sqrt / np.maximum(c[:, 1], 1) - 1.0
        self.length_px = np.where(some & skel, length, 0.0)
        self.max_width_px = np.where(some, wmax, 0.0)
        self.mean_width_px = np.where(some, np.where(skel, wmean, wmax), 0.0)
        self.mm_per_px = None if mm_per_px is None else float(mm_per_px)
        if self.mm_per_px is not None:
            s = self.mm_per_px
            self.length_mm, self.max_width_mm, self.mean_width_mm = self.length_px * s, self.max_width_px * s, self.mean_width_px * s
            self.area_mm2 = self.area_px * (s * s)

    def __len__(self) -> int:
        return int(self.boxes.shape[0])

    def _view(self, arena: torch.Tensor, g: int) -> torch.Tensor:
        y1, x1, y2, x2 = (int(v) for v in self.boxes[g])
        n = (y2 - y1) * (x2 - x1)
        return arena[self._offsets[g]:self._offsets[g] + n].view(y2 - y1, x2 - x1)

    def d2(self, g: int) -> torch.Tensor:
        return self._view(self.d2_arena, g)

    def skeleton(self, g: int) -> torch.Tensor:
        return self._view(self.skeleton_arena, g).view(torch.bool)

    def table(self, class_names: Optional[Sequence[str]] = None) -> List[dict]:
        rows = []
        for g in range(len(self)):
            row = {"instance": g, "box": tuple(int(v) for v in self.boxes[g])}
            if self.classid is not None:
                k = int(self.classid[g])
                row["class"] = class_names[k] if class_names is not None else k
            if self.score is not None:
                row["score"] = float(self.score[g])
            row.update(area_px=int(self.area_px[g]), length_px=float(self.length_px[g]),
                       max_width_px=float(self.max_width_px[g]), mean_width_px=float(self.mean_width_px[g]),
                       skeleton_px=int(self.skeleton_px[g]), endpoints=int(self.endpoints[g]))
            if self.mm_per_px is not None:
                row.update(length_mm=float(self.length_mm[g]), max_width_mm=float(self.max_width_mm[g]),
                           mean_width_mm=float(self.mean_width_mm[g]), area_mm2=float(self.area_mm2[g]))
            rows.append(row)
        return rows


def _check_scale(mm_per_px, chunk) -> None:
    if mm_per_px is not None and not (np.isfinite(float(mm_per_px)) and float(mm_per_px) > 0.0):
        raise ValueError("mm_per_px must be a positive number (got %r)" % (mm_per_px,))
    if isinstance(chunk, (bool, np.bool_)) or not isinstance(chunk, (int, np.integer)) or not 1 <= int(chunk) <= 1024:
        raise ValueError("chunk must be an int in 1 .. 1024 (got %r)" % (chunk,))


def measure_arena(groups, arena, arena_bytes=None, groups_dev=None, mm_per_px=None, chunk: int = 8, classid=None, score=None,
                  d2_out=None, skeleton_out=None) -> InstanceMeasures:
    """Measure the crops of an arena: groups int32 [G,8] and arena uint8 CUDA as ``lib.tile_compose`` takes and writes them (a
    non-zero byte is foreground).  ``d2_out`` (int32) and ``skeleton_out`` (uint8), CUDA of at least arena_bytes elements,
    are used for the two result arenas when given; their elements between two crops are left untouched."""
    _check_scale(mm_per_px, chunk)
    chunk = int(chunk)
    groups = np.ascontiguousarray(np.asarray(groups, np.int32).reshape(-1, 8))
    G = int(groups.shape[0])
    boxes = groups[:, 2:6]
    offsets = [int(v) * 16 for v in groups[:, 7]]
    if G == 0:
        dev = arena.device if torch.is_tensor(arena) else torch.device("cpu")
        m = InstanceMeasures(boxes, offsets, torch.empty(0, dtype=torch.int32, device=dev),
                             torch.empty(0, dtype=torch.uint8, device=dev), np.zeros((0, 8), np.int64), np.zeros(0),
                             np.zeros(0, np.int32), mm_per_px, classid, score)
        m.groups = groups
        return m
    dev = arena.device
    nbytes = int(arena.numel()) if arena_bytes is None else int(arena_bytes)
    if groups_dev is None:
        groups_dev = torch.from_numpy(groups).to(dev)
    n = max(nbytes, 1)
    d2 = torch.empty(n, dtype=torch.int32, device=dev) if d2_out is None else d2_out
    skel = torch.empty(n, dtype=torch.uint8, device=dev) if skeleton_out is None else skeleton_out
    colg = torch.empty(n, dtype=torch.int16, device=dev)
    tmp = torch.empty(n, dtype=torch.uint8, device=dev)
    flags = torch.empty(chunk + 1, G, dtype=torch.int32, device=dev)
    iters = torch.zeros(G, dtype=torch.int32, device=dev)
    L.measure_d2(groups, arena, colg, d2, groups_dev, nbytes)
    it0 = 0
    if L.measure_blocks(groups):
        while True:
            L.measure_thin(groups, arena, skel, tmp, flags, iters, it0, chunk, groups_dev, nbytes)
            it0 += chunk
            if not bool(flags[chunk].any()):          # the loop's host synchronisation: one per chunk of iterations
                break
    counts, sum_sqrt = L.measure_counts(groups, arena, skel, d2, groups_dev, nbytes)
    # the final copy: counts, sums and iteration numbers in one transfer (the float64 sums travel as their bit patterns)
    both = torch.cat([counts, sum_sqrt.view(torch.int64).view(G, 1), iters.to(torch.int64).view(G, 1)], dim=1).cpu().numpy()
    ssq = np.ascontiguousarray(both[:, 8]).view(np.float64)
    m = InstanceMeasures(boxes, offsets, d2, skel, both[:, :8], ssq, both[:, 9].astype(np.int32), mm_per_px, classid, score)
    m.groups, m.groups_dev, m.arena, m.arena_bytes = groups, groups_dev, arena, nbytes
    return m


def measure_instances(res, mm_per_px=None, chunk: int = 8) -> InstanceMeasures:
    """Measure every instance of a ``TiledDetections``.  ``mm_per_px``: the photograph's scale; the result then also holds
    the lengths and widths in mm and the area in mm^2.  ``chunk``: the thinning iterations enqueued between two reads of the
    flags; the result does not depend on it."""
    if len(res) == 0:
        _check_scale(mm_per_px, chunk)
        return measure_arena(np.zeros((0, 8), np.int32), res.arena, 0, None, mm_per_px, chunk, res.classid, res.score)
    if res.groups is None:
        raise ValueError("measure_instances needs the groups table of merge_tiles / detect_tiled")
    return measure_arena(res.groups, res.arena, res.arena_bytes, res.groups_dev, mm_per_px, chunk, res.classid, res.score)


# ---- the graph of the skeleton ---------------------------------------------------------------------------------------------
ROW_COLUMNS = ("instance", "root", "px", "n_orth", "n_diag", "n_end", "n_attach", "sum_q8", "max_d2", "min_d2", "spur")
JUNCTION_COLUMNS = ("junction_px", "jj_orth", "jj_diag", "n_branches")
MAX_BRANCH_PX = 32767


def _read(t: torch.Tensor) -> np.ndarray:
    """a copy to the host: every host synchronisation of skeleton_graph goes through here"""
    return t.cpu().numpy()


def _branch_table(rows, widths, mm_per_px):
    """rows int64 [n, 12] sorted by (instance, root), widths int [G] -> the structured array of SkeletonGraphs.branches"""
    rows = np.asarray(rows, np.int64).reshape(-1, L.SKELETON_ROW)
    fields = [(c, np.int64) for c in ROW_COLUMNS[:-1]] + [("spur", np.bool_), ("root_y", np.int64), ("root_x", np.int64)]
    floats = ["length_px", "mean_width_px", "max_width_px", "min_width_px"]
    if mm_per_px is not None:
        floats += ["length_mm", "mean_width_mm", "max_width_mm", "min_width_mm"]
    out = np.zeros(rows.shape[0], dtype=fields + [(f, np.float64) for f in floats] + [("kind", "U8")])
    for i, c in enumerate(ROW_COLUMNS):
        out[c] = rows[:, i]
    bw = np.asarray(widths, np.int64)[rows[:, 0]] if rows.shape[0] else np.zeros(0, np.int64)
    out["root_y"], out["root_x"] = rows[:, 1] // np.maximum(bw, 1), rows[:, 1] % np.maximum(bw, 1)
    out["length_px"] = out["n_orth"] + np.sqrt(2.0) * out["n_diag"] + out["n_end"] / 2.0
    out["mean_width_px"] = 2.0 * (out["sum_q8"] / 256.0) / np.maximum(out["px"], 1) - 1.0
    out["max_width_px"] = 2.0 * np.sqrt(out["max_d2"].astype(np.float64)) - 1.0
    out["min_width_px"] = 2.0 * np.sqrt(out["min_d2"].astype(np.float64)) - 1.0
    if mm_per_px is not None:
        for f in ("length", "mean_width", "max_width", "min_width"):
            out[f + "_mm"] = out[f + "_px"] * float(mm_per_px)
    free, ends = out["n_attach"] == 0, out["n_end"] >= 1
    out["kind"] = np.where(free, np.where(out["n_end"] == 0, "loop", "free"), np.where(ends, "terminal", "inner"))
    return out


class SkeletonGraphs:
    """What ``skeleton_graph`` returns.  For the G instances, numpy [G]:
      n_branches, junction_px, jj_orth, jj_diag (int64): of the returned (pruned) skeleton
      group_analyses int32: the analyses each instance took, the last one, which found no spur (or came after max_rounds
                prunings), included; analyses = their maximum; converged bool: the instance's final table holds no spur
      measures  the InstanceMeasures it was made from; pruned: an InstanceMeasures over the pruned skeleton that shares d2 (its
                length_px, mean_width_px, ... and the mm columns)
      branches  one structured array over all instances, sorted by (instance, root): the integer columns of ROW_COLUMNS, root_y,
                root_x, length_px, mean_width_px, max_width_px, min_width_px (and _mm with a scale), kind; branches_of(g)
      links(g) uint8, labels(g) int32, pruned_skeleton(g) bool: CUDA views [bh,bw]
      table(class_names) measures.table extended with pruned_length_px, n_branches, junction_px
      rows_dev int64 CUDA [capacity, 12], rowid_arena int32 CUDA, row_order int64 [len(branches)]: the per-branch integer tables
                on the device, for ``skeleton_trace`` to go on from"""

    def __init__(self, measures, pruned, links_arena, labels_arena, rows, junctions, group_analyses, converged, min_branch_px,
                 mm_per_px=None):
        self.measures, self.pruned = measures, pruned
        self.links_arena, self.labels_arena = links_arena, labels_arena
        self.min_branch_px, self.mm_per_px = float(min_branch_px), mm_per_px
        j = np.asarray(junctions, np.int64).reshape(-1, 4)
        self.junction_px, self.jj_orth, self.jj_diag, self.n_branches = (j[:, i].copy() for i in range(4))
        self.group_analyses = np.asarray(group_analyses, np.int32).reshape(-1)
        self.analyses = int(self.group_analyses.max()) if self.group_analyses.size else 0
        self.converged = np.asarray(converged, np.bool_).reshape(-1)
        b = measures.boxes
        self.branches = _branch_table(rows, b[:, 3] - b[:, 1], mm_per_px)
        self._first = np.searchsorted(self.branches["instance"], np.arange(len(measures) + 1))
        # what ``skeleton_trace`` goes on from (set by skeleton_graph): the row buffer on the device as disyolo_skeleton_rows
        # left it, the row numbers per root pixel, and row_order[k] = the device row of branches[k]
        self.rows_dev, self.rowid_arena, self.row_order = None, None, np.zeros(0, np.int64)

    def __len__(self) -> int:
        return len(self.measures)

    def branches_of(self, g: int) -> np.ndarray:
        return self.branches[self._first[g]:self._first[g + 1]]

    def links(self, g: int) -> torch.Tensor:
        return self.measures._view(self.links_arena, g)

    def labels(self, g: int) -> torch.Tensor:
        return self.measures._view(self.labels_arena, g)

    def pruned_skeleton(self, g: int) -> torch.Tensor:
        return self.pruned.skeleton(g)

    def table(self, class_names: Optional[Sequence[str]] = None) -> List[dict]:
        rows = self.measures.table(class_names)
        for g, row in enumerate(rows):
            row.update(pruned_length_px=float(self.pruned.length_px[g]), n_branches=int(self.n_branches[g]),
                       junction_px=int(self.junction_px[g]))
            if self.mm_per_px is not None:
                row.update(pruned_length_mm=float(self.pruned.length_px[g] * self.mm_per_px))
        return rows


def _check_graph(min_branch_px, max_rounds, mm_per_px, row_capacity) -> int:
    """-> M2 = 2 min_branch_px, the integer the kernels decide a spur with"""
    try:
        v = float(min_branch_px)
    except (TypeError, ValueError):
        v = float("nan")
    if not (v == v and 0.0 <= v <= MAX_BRANCH_PX and 2.0 * v == np.floor(2.0 * v)):
        raise ValueError("min_branch_px must be a multiple of 0.5 in 0 .. %d (got %r)" % (MAX_BRANCH_PX, min_branch_px))
    if isinstance(max_rounds, (bool, np.bool_)) or not isinstance(max_rounds, (int, np.integer)) or not 0 <= int(max_rounds) <= 1024:
        raise ValueError("max_rounds must be an int in 0 .. 1024 (got %r)" % (max_rounds,))
    if mm_per_px is not None and not (np.isfinite(float(mm_per_px)) and float(mm_per_px) > 0.0):
        raise ValueError("mm_per_px must be a positive number (got %r)" % (mm_per_px,))
    if row_capacity is not None and (isinstance(row_capacity, (bool, np.bool_)) or not isinstance(row_capacity, (int, np.integer))
                                     or not 0 <= int(row_capacity) < 1 << 31):
        raise ValueError("row_capacity must be an int in 0 .. 2^31 - 1 (got %r)" % (row_capacity,))
    return int(2.0 * v)


def skeleton_graph(m: InstanceMeasures, min_branch_px: float = 0.0, max_rounds: int = 8, mm_per_px=None, row_capacity=None,
                   links_out=None, labels_out=None, pruned_out=None) -> SkeletonGraphs:
    """The graph of every skeleton of ``m`` (what measure_instances / measure_masks / measure_arena returned): junction pixels,
    branches with their lengths and widths, and the skeleton pruned of its spurs -- branches with one free end, one attachment
    and a length below ``min_branch_px`` (a multiple of 0.5 in 0 .. 32767; 0 prunes nothing).  At most ``max_rounds`` prunings
    are made (0: analyse only); ``converged`` says per instance whether the final table is free of spurs.  ``mm_per_px``
    defaults to the scale of ``m``.  ``row_capacity``: the rows of the first row buffer (by default the skeleton pixels of
    ``m``, which always suffice); when a call finds more branches the rows are computed again into a buffer that holds them.
    ``links_out`` (uint8), ``labels_out`` (int32), ``pruned_out`` (uint8), CUDA of at least arena_bytes elements, are used
    for the result arenas when given; their elements between two crops are left untouched.  ``m`` is not changed."""
    if mm_per_px is None:
        mm_per_px = m.mm_per_px
    M2 = _check_graph(min_branch_px, max_rounds, mm_per_px, row_capacity)
    max_rounds = int(max_rounds)
    G = len(m)
    if G == 0:
        e8, e32 = m.skeleton_arena.new_empty(0), m.d2_arena.new_empty(0)
        pruned = InstanceMeasures(m.boxes, m._offsets, m.d2_arena, e8, np.zeros((0, 8), np.int64), np.zeros(0), np.zeros(0, np.int32),
                                  mm_per_px, m.classid, m.score)
        return SkeletonGraphs(m, pruned, e8, e32, np.zeros((0, L.SKELETON_ROW), np.int64), np.zeros((0, 4), np.int64),
                              np.zeros(0, np.int32), np.zeros(0, bool), min_branch_px, mm_per_px)
    if m.groups is None or m.arena is None:
        raise ValueError("skeleton_graph needs the InstanceMeasures of measure_arena / measure_instances / measure_masks")
    groups, groups_dev, nbytes, dev = m.groups, m.groups_dev, m.arena_bytes, m.arena.device
    n = max(nbytes, 1)
    links = torch.empty(n, dtype=torch.uint8, device=dev) if links_out is None else links_out
    labels = torch.empty(n, dtype=torch.int32, device=dev) if labels_out is None else labels_out
    pruned = torch.empty(n, dtype=torch.uint8, device=dev) if pruned_out is None else pruned_out
    rowid = torch.empty(n, dtype=torch.int32, device=dev)
    cap = max(int(m.skeleton_px.sum()), 1) if row_capacity is None else int(row_capacity)
    rows = torch.empty(cap, L.SKELETON_ROW, dtype=torch.int64, device=dev)
    ctrl = torch.zeros(G + 1, dtype=torch.int32, device=dev)
    junctions = torch.zeros(G, 4, dtype=torch.int64, device=dev)
    group_analyses, live = np.zeros(G, np.int32), np.ones(G, bool)
    src, analyses = m.skeleton_arena, 0
    while True:
        analyses += 1
        L.skeleton_classify(groups, src, pruned, links, groups_dev, nbytes)      # (the first one also copies the skeleton)
        src = pruned
        L.skeleton_label(groups, pruned, links, labels, groups_dev, nbytes)
        while True:
            L.skeleton_rows(groups, links, labels, m.d2_arena, rowid, rows, M2, ctrl, junctions, groups_dev, nbytes)
            c = _read(ctrl)                                                       # the analysis's host synchronisation
            if int(c[0]) <= cap:
                break
            cap = int(c[0])                                                       # the buffer was too small: once more
            rows = torch.empty(cap, L.SKELETON_ROW, dtype=torch.int64, device=dev)
        spur = c[1:] != 0
        group_analyses[live] = analyses
        live &= spur
        if not spur.any() or analyses > max_rounds:
            break
        L.skeleton_prune(groups, labels, rowid, rows, pruned, groups_dev, nbytes)
    count = int(c[0])
    counts, sum_sqrt = L.measure_counts(groups, m.arena, pruned, m.d2_arena, groups_dev, nbytes)
    # the final copy: rows, junction numbers, the pruned skeleton's counts and float64 sums (as bit patterns) in one transfer
    flat = _read(torch.cat([rows[:count].reshape(-1), junctions.reshape(-1), counts.reshape(-1), sum_sqrt.view(torch.int64)]))
    nr = count * L.SKELETON_ROW
    table = flat[:nr].reshape(count, L.SKELETON_ROW)
    row_order = np.lexsort((table[:, 1], table[:, 0]))
    table = table[row_order]
    ssq = np.ascontiguousarray(flat[nr + 12 * G:]).view(np.float64)
    pm = InstanceMeasures(m.boxes, m._offsets, m.d2_arena, pruned, flat[nr + 4 * G:nr + 12 * G].reshape(G, 8), ssq,
                          m.group_iterations, mm_per_px, m.classid, m.score)
    pm.groups, pm.groups_dev, pm.arena, pm.arena_bytes = groups, groups_dev, m.arena, nbytes
    g = SkeletonGraphs(m, pm, links, labels, table, flat[nr:nr + 4 * G].reshape(G, 4), group_analyses, ~spur, min_branch_px, mm_per_px)
    g.rows_dev, g.rowid_arena, g.row_order = rows, rowid, row_order.astype(np.int64)
    return g


# ---- the traced graph: nodes, ordered branches, the trunk ------------------------------------------------------------------
NODE_COLUMNS = ("instance", "root", "px", "sum_y", "sum_x", "max_d2", "n_attach")
EDGE_COLUMNS = ("instance", "root", "end0_kind", "end0_id", "end1_kind", "end1_id", "attach0_px", "attach1_px", "end0_px", "end1_px",
                "inner_diag", "last_rank")
TRUNK_COLUMNS = ("n_branches", "px", "n_orth", "n_diag", "n_end", "sum_q8", "max_d2", "max_pos", "max_y", "max_x", "weight")
END_FREE, END_NODE, END_LOOP = 0, 1, 2
W_ORTH, W_DIAG, W_END = 1024, 1448, 512       # the integer weights of the trunk selection: a fixed-point sqrt(2)


def _trace_read(t: torch.Tensor) -> np.ndarray:
    """a copy to the host: every host synchronisation of skeleton_trace goes through here"""
    return t.cpu().numpy()


def _octile(a: int, b: int, bw: int):
    """(orthogonal, diagonal) steps between two pixels of a crop of width bw"""
    dy, dx = abs(a // bw - b // bw), abs(a % bw - b % bw)
    return max(dy, dx) - min(dy, dx), min(dy, dx)


def select_trunk(weights, edges):
    """The trunk of one instance.  weights int [n]: 1024 n_orth + 1448 n_diag + 512 n_end of its branches; edges int [n, >= 8]
    (EDGE_COLUMNS), both sorted by root.  -> (path [(k, reversed)] of indices into them, distance).  Vertices are the nodes and
    the free ends, ordered by (pixel id, kind, end); a loop or a branch that attaches to one node at both ends is no edge.
    Dijkstra from every vertex in order, the heap popped by (distance, vertex order), edges relaxed in ascending root, a
    predecessor replaced only on a strictly smaller distance, the best pair only on a strictly larger one; without any edge the
    heaviest loop (the smallest root on a tie), without a loop nothing."""
    import heapq
    verts, ge = set(), []
    for k, e in enumerate(edges):
        k0, i0, k1, i1 = int(e[2]), int(e[3]), int(e[4]), int(e[5])
        if k0 == END_LOOP or (k0 == END_NODE and k1 == END_NODE and i0 == i1):
            continue
        a, b = (i0, k0, 0), (i1, k1, 1 if (k0 == END_FREE and k1 == END_FREE and i0 == i1) else 0)
        ge.append((k, int(weights[k]), a, b))
        verts.update((a, b))
    verts = sorted(verts)
    at = {v: i for i, v in enumerate(verts)}
    adj = [[] for _ in verts]
    for k, w, a, b in ge:
        adj[at[a]].append((k, w, at[b], False))
        adj[at[b]].append((k, w, at[a], True))
    best = (0, None, None, None)
    for u in range(len(verts)):
        dist, pred, done, heap = {u: 0}, {}, set(), [(0, u)]
        while heap:
            d, a = heapq.heappop(heap)
            if a in done:
                continue
            done.add(a)
            for k, w, b, rev in adj[a]:
                if b not in dist or d + w < dist[b]:
                    dist[b], pred[b] = d + w, (a, k, rev)
                    heapq.heappush(heap, (d + w, b))
        for v in sorted(dist):
            if dist[v] > best[0]:
                best = (dist[v], u, v, pred)
    if best[1] is not None:
        d, u, a, pred = best
        path = []
        while a != u:
            a, k, rev = pred[a]
            path.append((k, rev))
        return path[::-1], d
    loops = [(-int(weights[k]), k) for k, e in enumerate(edges) if int(e[2]) == END_LOOP]
    if loops:
        w, k = min(loops)
        return [(k, False)], -w
    return [], 0


class SkeletonTraces:
    """What ``skeleton_trace`` returns, for the G instances of its SkeletonGraphs ``graphs``:
      nodes     one structured array over all instances, sorted by (instance, root): NODE_COLUMNS (int64) and centroid_y,
                centroid_x (float64, crop coordinates); nodes_of(i)
      edges     one row per branch, in the order of graphs.branches: EDGE_COLUMNS (int64).  End 0 is at rank 0, end 1 at the last
                rank; kind 1 = a node (id its root, attach the junction pixel linked to), 0 = a free end (id the end pixel,
                attach -1), 2 = a loop (id the root); end0_px, end1_px the branch's first and last pixel; edges_of(i)
      rank(i), rank_diag(i), node_labels(i)  int32 CUDA views [bh,bw], -1 off the branch pixels / off the junction pixels
      branch_profile(i, root)  int32 CUDA view [px,4]: y, x, d2, rank_diag of the branch's pixels in rank order (all of them lie
                in profile_buffer in the order of graphs.branches).  A pixel's arc position is
                (rank - rank_diag) + sqrt(2) rank_diag
      trunk     structured array [G]: TRUNK_COLUMNS (int64), trunk_length_px, mean_width_px, max_width_px, widest_y, widest_x (the
                first widest point in image coordinates) and, with a scale, trunk_length_mm, mean_width_mm, max_width_mm
      trunk_branches(i)  [(root, reversed)] along the trunk; trunk_profile(i) int32 CUDA view [px,5]: y, x, d2, cum_orth, cum_diag
      table(class_names) graphs.table extended with the trunk columns"""

    def __init__(self, graphs, node_labels_arena, rank_arena, rank_diag_arena, nodes, edges, profile_buffer, trunk_ints, paths,
                 trunk_buffer, trunk_start, mm_per_px=None):
        self.graphs, self.mm_per_px = graphs, mm_per_px
        self.node_labels_arena, self.rank_arena, self.rank_diag_arena = node_labels_arena, rank_arena, rank_diag_arena
        self.profile_buffer, self.trunk_buffer = profile_buffer, trunk_buffer
        G = len(graphs)
        nodes = np.asarray(nodes, np.int64).reshape(-1, L.TRACE_NODE)
        self.nodes = np.zeros(nodes.shape[0], dtype=[(c, np.int64) for c in NODE_COLUMNS] + [("centroid_y", np.float64), ("centroid_x", np.float64)])
        for i, c in enumerate(NODE_COLUMNS):
            self.nodes[c] = nodes[:, i]
        self.nodes["centroid_y"] = nodes[:, 3] / np.maximum(nodes[:, 2], 1)
        self.nodes["centroid_x"] = nodes[:, 4] / np.maximum(nodes[:, 2], 1)
        self._node_first = np.searchsorted(self.nodes["instance"], np.arange(G + 1))
        edges = np.asarray(edges, np.int64).reshape(-1, L.TRACE_EDGE)
        self.edges = np.zeros(edges.shape[0], dtype=[(c, np.int64) for c in EDGE_COLUMNS])
        for i, c in enumerate(EDGE_COLUMNS):
            self.edges[c] = edges[:, i]
        self._profile_start = np.concatenate([[0], np.cumsum(graphs.branches["px"])]).astype(np.int64)
        self._paths, self._trunk_start = list(paths), np.asarray(trunk_start, np.int64)
        ti = np.asarray(trunk_ints, np.int64).reshape(-1, len(TRUNK_COLUMNS))
        floats = ["trunk_length_px", "mean_width_px", "max_width_px", "widest_y", "widest_x"]
        if mm_per_px is not None:
            floats += ["trunk_length_mm", "mean_width_mm", "max_width_mm"]
        self.trunk = np.zeros(G, dtype=[(c, np.int64) for c in TRUNK_COLUMNS] + [(f, np.float64) for f in floats])
        for i, c in enumerate(TRUNK_COLUMNS):
            self.trunk[c] = ti[:, i]
        t, some = self.trunk, ti[:, 1] > 0
        t["trunk_length_px"] = np.where(some, t["n_orth"] + np.sqrt(2.0) * t["n_diag"] + t["n_end"] / 2.0, 0.0)
        t["mean_width_px"] = np.where(some, 2.0 * (t["sum_q8"] / 256.0) / np.maximum(t["px"], 1) - 1.0, 0.0)
        t["max_width_px"] = np.where(some, 2.0 * np.sqrt(t["max_d2"].astype(np.float64)) - 1.0, 0.0)
        b = graphs.measures.boxes.astype(np.int64).reshape(-1, 4)
        t["widest_y"], t["widest_x"] = np.where(some, b[:, 0] + t["max_y"], 0), np.where(some, b[:, 1] + t["max_x"], 0)
        if mm_per_px is not None:
            for f in ("trunk_length", "mean_width", "max_width"):
                t[f + "_mm"] = t[f + "_px"] * float(mm_per_px)

    def __len__(self) -> int:
        return len(self.graphs)

    def nodes_of(self, g: int) -> np.ndarray:
        return self.nodes[self._node_first[g]:self._node_first[g + 1]]

    def edges_of(self, g: int) -> np.ndarray:
        return self.edges[self.graphs._first[g]:self.graphs._first[g + 1]]

    def rank(self, g: int) -> torch.Tensor:
        return self.graphs.measures._view(self.rank_arena, g)

    def rank_diag(self, g: int) -> torch.Tensor:
        return self.graphs.measures._view(self.rank_diag_arena, g)

    def node_labels(self, g: int) -> torch.Tensor:
        return self.graphs.measures._view(self.node_labels_arena, g)

    def branch_profile(self, g: int, root: int) -> torch.Tensor:
        b = self.graphs.branches_of(g)
        k = int(np.searchsorted(b["root"], int(root)))
        if k >= len(b) or int(b["root"][k]) != int(root):
            raise KeyError("instance %d has no branch with root %r" % (g, root))
        k += int(self.graphs._first[g])
        return self.profile_buffer[int(self._profile_start[k]):int(self._profile_start[k + 1])]

    def trunk_branches(self, g: int) -> List[tuple]:
        return list(self._paths[g])

    def trunk_profile(self, g: int) -> torch.Tensor:
        return self.trunk_buffer[int(self._trunk_start[g]):int(self._trunk_start[g + 1])]

    def table(self, class_names: Optional[Sequence[str]] = None) -> List[dict]:
        rows = self.graphs.table(class_names)
        t = self.trunk
        for g, row in enumerate(rows):
            row.update(trunk_length_px=float(t["trunk_length_px"][g]), trunk_branches=int(t["n_branches"][g]),
                       trunk_mean_width_px=float(t["mean_width_px"][g]), trunk_max_width_px=float(t["max_width_px"][g]),
                       trunk_widest_yx=(int(t["widest_y"][g]), int(t["widest_x"][g])))
            if self.mm_per_px is not None:
                row.update(trunk_length_mm=float(t["trunk_length_mm"][g]), trunk_mean_width_mm=float(t["mean_width_mm"][g]),
                           trunk_max_width_mm=float(t["max_width_mm"][g]))
        return rows


def skeleton_trace(g: SkeletonGraphs, mm_per_px=None, node_labels_out=None, rank_out=None, rank_diag_out=None) -> SkeletonTraces:
    """Trace the graphs of ``g`` (what skeleton_graph returned): the junction clusters as nodes, every branch ordered from one
    end to the other with what its ends are, and per instance the trunk -- the path between the two vertices that lie farthest
    apart -- with its profile.  ``mm_per_px`` defaults to the scale of ``g``.  ``node_labels_out``, ``rank_out``,
    ``rank_diag_out`` (int32 CUDA of at least arena_bytes elements) are used for the result arenas when given; their elements
    between two crops are left untouched.  ``g`` is not changed.  G = 0 launches nothing and reads nothing; without any skeleton
    pixel only the two maps are written."""
    if not isinstance(g, SkeletonGraphs):
        raise ValueError("skeleton_trace needs the SkeletonGraphs of skeleton_graph (got %s)" % type(g).__name__)
    if mm_per_px is None:
        mm_per_px = g.mm_per_px
    if mm_per_px is not None and not (np.isfinite(float(mm_per_px)) and float(mm_per_px) > 0.0):
        raise ValueError("mm_per_px must be a positive number (got %r)" % (mm_per_px,))
    m, G = g.measures, len(g)
    nb = len(g.branches)
    no_ints = np.zeros((G, len(TRUNK_COLUMNS)), np.int64)
    if G == 0:
        e32 = m.d2_arena.new_empty(0)
        return SkeletonTraces(g, e32, e32, e32, np.zeros((0, L.TRACE_NODE)), np.zeros((0, L.TRACE_EDGE)), e32.view(0, L.TRACE_PROFILE), no_ints,
                              [], e32.view(0, L.TRACE_TRUNK_PROFILE), np.zeros(1, np.int64), mm_per_px)
    if m.groups is None or g.rows_dev is None or g.rowid_arena is None or len(g.row_order) != nb:
        raise ValueError("skeleton_trace needs the SkeletonGraphs of skeleton_graph, with its row tables (rows_dev, rowid_arena, row_order)")
    groups, groups_dev, nbytes, dev = m.groups, m.groups_dev, m.arena_bytes, g.links_arena.device
    if nbytes >= 1 << 31:
        raise ValueError("skeleton_trace takes arenas below 2^31 elements (got %d)" % nbytes)
    n = max(nbytes, 1)
    i32 = dict(dtype=torch.int32, device=dev)
    node_labels = torch.empty(n, **i32) if node_labels_out is None else node_labels_out
    rank = torch.empty(n, **i32) if rank_out is None else rank_out
    rank_diag = torch.empty(n, **i32) if rank_diag_out is None else rank_diag_out
    noderow = torch.empty(n, **i32)
    px = g.branches["px"].astype(np.int64)
    n_list, n_junction = int(px.sum()), int(g.junction_px.sum())
    rounds = (int(px.max()) - 1).bit_length() if nb else 0           # 2^rounds >= the longest branch's pixels - 1
    nodes = torch.empty(n_junction, L.TRACE_NODE, dtype=torch.int64, device=dev)
    ents = torch.empty(n_list, L.TRACE_ENT, **i32)
    nxt = torch.empty(4 * n_list, **i32)
    val = torch.empty(4 * n_list, dtype=torch.int64, device=dev)
    ctrl, count = torch.zeros(1, **i32), torch.zeros(1, **i32)
    d2, links = m.d2_arena, g.links_arena
    L.trace_nodes(groups, links, d2, node_labels, noderow, nodes, ctrl, groups_dev, nbytes)
    L.trace_rank(groups, links, g.labels_arena, d2, g.rowid_arena, g.rows_dev, ents, rounds, nxt, val, count, rank, rank_diag, groups_dev,
                 nbytes)
    profile = torch.empty(n_list, L.TRACE_PROFILE, **i32)
    if n_list == 0 and n_junction == 0:
        return SkeletonTraces(g, node_labels, rank, rank_diag, np.zeros((0, L.TRACE_NODE)), np.zeros((0, L.TRACE_EDGE)), profile, no_ints,
                              [[] for _ in range(G)], profile.new_empty(0, L.TRACE_TRUNK_PROFILE), np.zeros(G + 1, np.int64), mm_per_px)
    n_rows = int(g.row_order.max()) + 1 if nb else 0
    edges_dev = torch.empty(n_rows, L.TRACE_EDGE, dtype=torch.int64, device=dev)
    L.trace_edges(groups, ents, count, rank, rank_diag, node_labels, edges_dev, groups_dev, nbytes)
    # the first read: the edge and node tables, which the trunk selection needs
    flat = _trace_read(torch.cat([edges_dev.reshape(-1), nodes.reshape(-1), ctrl.to(torch.int64)]))
    ne = n_rows * L.TRACE_EDGE
    edges = flat[:ne].reshape(n_rows, L.TRACE_EDGE)[g.row_order]
    n_nodes = int(flat[-1])
    if n_nodes > n_junction:
        raise L.DisyoloError("skeleton_trace: %d nodes from %d junction pixels" % (n_nodes, n_junction))
    ntab = flat[ne:ne + n_nodes * L.TRACE_NODE].reshape(n_nodes, L.TRACE_NODE)
    ntab = ntab[np.lexsort((ntab[:, 1], ntab[:, 0]))]
    b = g.branches
    if not (np.array_equal(edges[:, 0], b["instance"]) and np.array_equal(edges[:, 1], b["root"]) and np.array_equal(edges[:, 11], px - 1)):
        raise L.DisyoloError("skeleton_trace: the edge table does not describe the branches of the graph")
    weights = W_ORTH * b["n_orth"] + W_DIAG * b["n_diag"] + W_END * b["n_end"]
    widths = (m.boxes[:, 3] - m.boxes[:, 1]).astype(np.int64)
    offsets = np.zeros(n_rows, np.int32)
    offsets[g.row_order] = np.concatenate([[0], np.cumsum(px)[:-1]]) if nb else []
    seg = np.zeros((n_rows, L.TRACE_SEG), np.int32)
    seg[:, 0] = -1
    attach, paths, tstart, ints = [], [], np.zeros(G + 1, np.int64), no_ints.copy()
    cursor = 0
    for i in range(G):
        k0, k1 = int(g._first[i]), int(g._first[i + 1])
        bw, off = int(widths[i]), int(m._offsets[i])
        path, dist = select_trunk(weights[k0:k1], edges[k0:k1])
        co = cd = cross_o = cross_d = 0
        last_px = leave = None
        for k, rev in path:
            e = edges[k0 + k]
            enter, out = (int(e[7]), int(e[6])) if rev else (int(e[6]), int(e[7]))
            first, last = (int(e[9]), int(e[8])) if rev else (int(e[8]), int(e[9]))
            if leave is not None:
                for a in ([leave] if enter == leave else [leave, enter]):
                    so, sd = _octile(last_px, a, bw)                  # (onto the first one: a link; on to the second: the crossing)
                    if a != leave:
                        cross_o, cross_d = cross_o + so, cross_d + sd
                    co, cd, last_px = co + so, cd + sd, a
                    attach.append((off + a, cursor, a // bw, a % bw, co, cd))
                    cursor += 1
                so, sd = _octile(last_px, first, bw)
                co, cd = co + so, cd + sd
            seg[g.row_order[k0 + k]] = (cursor, int(rev), co, cd)
            co, cd = co + int(e[11]) - int(e[10]), cd + int(e[10])
            cursor += int(e[11]) + 1
            last_px, leave = last, out
        paths.append([(int(b["root"][k0 + k]), bool(rev)) for k, rev in path])
        tstart[i + 1] = cursor
        if path:
            ks = [k0 + k for k, _ in path]
            # n_orth, n_diag: those of the branches' rows plus the crossings between two attach pixels of one node
            ints[i, 0], ints[i, 4], ints[i, 10] = len(path), int(b["n_end"][ks].sum()), int(weights[ks].sum())
            ints[i, 2], ints[i, 3] = int(b["n_orth"][ks].sum()) + cross_o, int(b["n_diag"][ks].sum()) + cross_d
    if cursor >= 1 << 30:
        raise ValueError("skeleton_trace: trunk profiles of %d entries (need < 2^30)" % cursor)
    tprofile = torch.empty(cursor, L.TRACE_TRUNK_PROFILE, **i32)
    trunkrows = torch.empty(G, L.TRACE_TRUNK, dtype=torch.int64, device=dev)
    plan = np.concatenate([offsets, seg.reshape(-1), np.asarray(attach, np.int32).reshape(-1), tstart.astype(np.int32)]).astype(np.int32)
    plan_dev = torch.from_numpy(plan).to(dev)                            # one upload
    o0, o1 = n_rows, n_rows + seg.size
    o2 = o1 + len(attach) * L.TRACE_ATTACH
    L.trace_gather(groups, ents, count, rank, rank_diag, d2, plan_dev[:o0], profile, plan_dev[o0:o1].view(n_rows, L.TRACE_SEG), edges_dev,
                   plan_dev[o1:o2].view(len(attach), L.TRACE_ATTACH), tprofile, plan_dev[o2:], trunkrows, groups_dev, nbytes)
    # the final read: the trunk rows
    tr = _trace_read(trunkrows)
    ints[:, 1], ints[:, 5], ints[:, 6], ints[:, 7], ints[:, 8], ints[:, 9] = tr[:, 0], tr[:, 1], tr[:, 2], tr[:, 3], tr[:, 4], tr[:, 5]
    return SkeletonTraces(g, node_labels, rank, rank_diag, ntab, edges, profile, ints, paths, tprofile, tstart, mm_per_px)


# ---- the shape of an instance: orientation, oriented extent, perimeter, parts and holes ---------------------------------------
SHAPE_COLUMNS = ("n", "Sy", "Sx", "Syy", "Sxx", "Sxy", "ymin", "ymax", "xmin", "xmax", "Q1", "Q2", "Q3", "Q4", "QD", "zero")
SHAPE_UNIT = 16384                    # a direction's (c, s) and every extent are in 2^-14
SHAPE_INTS = ("area_px", "n_parts", "largest_part_px", "euler8", "n_holes", "edges", "rect_k")
SHAPE_FLOATS = ("centroid_y", "centroid_x", "orientation_deg", "axis_major_px", "axis_minor_px", "elongation", "feret_max_px",
                "feret_max_deg", "feret_min_px", "feret_min_deg", "rect_long_px", "rect_short_px", "rect_angle_deg", "rect_area_px2",
                "perimeter_px", "compactness", "solidity_rect")
SHAPE_LENGTHS = ("axis_major", "axis_minor", "feret_max", "feret_min", "rect_long", "rect_short", "perimeter")
_INT32_MAX, _INT32_MIN = 2 ** 31 - 1, -2 ** 31


def shape_directions(K) -> np.ndarray:
    """int32 [K, 2]: (round(16384 cos(k pi / K)), round(16384 sin(k pi / K))), the table the extents are taken along"""
    if isinstance(K, (bool, np.bool_)) or not isinstance(K, (int, np.integer)) or not 2 <= int(K) <= 360 or int(K) % 2:
        raise ValueError("directions must be an even int in 2 .. 360 (got %r)" % (K,))
    K = int(K)
    return np.array([[round(SHAPE_UNIT * math.cos(k * math.pi / K)), round(SHAPE_UNIT * math.sin(k * math.pi / K))] for k in range(K)], np.int32)


def _shape_read(t: torch.Tensor) -> np.ndarray:
    """a copy to the host: the one host synchronisation of instance_shapes goes through here"""
    return t.cpu().numpy()


def shape_ext(pminmax, dirs) -> np.ndarray:
    """int64 [K]: max - min + |c| + |s| per direction (2^-14 px; a pixel is a unit square), 0 for an empty crop"""
    pm, d = np.asarray(pminmax, np.int64), np.asarray(dirs, np.int64)
    return np.where(pm[:, 1] >= pm[:, 0], pm[:, 1] - pm[:, 0] + np.abs(d[:, 0]) + np.abs(d[:, 1]), 0)


def direction_kind(orientation_deg, elongation, axis_deg, axis_tol_deg=22.5, min_elongation=1.5) -> str:
    if elongation < min_elongation:
        return "none"
    delta = abs(((orientation_deg - axis_deg + 90.0) % 180.0) - 90.0)
    return "longitudinal" if delta <= axis_tol_deg else "transverse" if delta >= 90.0 - axis_tol_deg else "diagonal"


def derive_shape(s, p, pminmax, dirs, origin=(0, 0), mm_per_px=None, axis_deg=None, axis_tol_deg=22.5, min_elongation=1.5) -> dict:
    """The columns of one instance from its integers (s int [16], SHAPE_COLUMNS; p = n_parts, largest_part_px; pminmax, dirs int
    [K, 2]; origin = the box's y1, x1): exact Python ints until the last step of every column, then float64.  The expressions are
    those of tests/shape_ref.py, derive: the two agree bit for bit."""
    n, Sy, Sx, Syy, Sxx, Sxy = (int(v) for v in s[:6])
    q1, q2, q3, q4, qd = (int(v) for v in s[10:15])
    K = len(dirs)
    e8 = (q1 - q3 - 2 * qd) // 4
    out = {"area_px": n, "n_parts": int(p[0]), "largest_part_px": int(p[1]), "euler8": e8, "n_holes": int(p[0]) - e8,
           "edges": q1 + q2 + q3 + 2 * qd}
    if n == 0:
        out.update({c: 0.0 for c in SHAPE_FLOATS})
        out.update(rect_k=0, rect_center=np.zeros(2), rect_corners=np.zeros((4, 2)))
    else:
        out["centroid_y"], out["centroid_x"] = Sy / n, Sx / n
        Mxx, Myy, Mxy = n * Sxx - Sx * Sx, n * Syy - Sy * Sy, n * Sxy - Sx * Sy
        o = math.degrees(0.5 * math.atan2(2 * Mxy, Mxx - Myy)) % 180.0
        out["orientation_deg"] = 0.0 if o >= 180.0 else o
        a, b, c = Mxx / (n * n) + 1.0 / 12.0, Mxy / (n * n), Myy / (n * n) + 1.0 / 12.0
        l1 = 0.5 * (a + c) + math.hypot(0.5 * (a - c), b)
        l2 = (a * c - b * b) / l1
        out["axis_major_px"], out["axis_minor_px"], out["elongation"] = 4.0 * math.sqrt(l1), 4.0 * math.sqrt(l2), math.sqrt(l1 / l2)
        ext = [int(v) for v in shape_ext(pminmax, dirs)]
        kmax, kmin = ext.index(max(ext)), ext.index(min(ext))
        out["feret_max_px"], out["feret_max_deg"] = ext[kmax] / SHAPE_UNIT, 180.0 * kmax / K
        out["feret_min_px"], out["feret_min_deg"] = ext[kmin] / SHAPE_UNIT, 180.0 * kmin / K
        prod = [ext[k] * ext[k + K // 2] for k in range(K // 2)]
        k0 = prod.index(min(prod))
        k1 = k0 + K // 2
        kl = k0 if ext[k0] >= ext[k1] else k1
        out["rect_k"] = k0
        out["rect_long_px"], out["rect_short_px"] = max(ext[k0], ext[k1]) / SHAPE_UNIT, min(ext[k0], ext[k1]) / SHAPE_UNIT
        out["rect_angle_deg"], out["rect_area_px2"] = 180.0 * kl / K, prod[k0] / (SHAPE_UNIT * SHAPE_UNIT)
        # the rectangle in the image: the two projections P0 = c0 x + s0 y, P1 = c1 x + s1 y inverted
        (c0, s0), (c1, s1) = (int(v) for v in dirs[k0]), (int(v) for v in dirs[k1])
        h0, h1 = 0.5 * (abs(c0) + abs(s0)), 0.5 * (abs(c1) + abs(s1))
        lo0, hi0 = int(pminmax[k0][0]) - h0, int(pminmax[k0][1]) + h0
        lo1, hi1 = int(pminmax[k1][0]) - h1, int(pminmax[k1][1]) + h1
        det = float(c0 * s1 - s0 * c1)
        at = lambda P0, P1: (origin[0] + (c0 * P1 - c1 * P0) / det, origin[1] + (P0 * s1 - s0 * P1) / det)
        out["rect_corners"] = np.array([at(lo0, lo1), at(hi0, lo1), at(hi0, hi1), at(lo0, hi1)], np.float64)
        out["rect_center"] = np.array(at(0.5 * (lo0 + hi0), 0.5 * (lo1 + hi1)), np.float64)
        per = q2 + (q1 + q3 + 2 * qd) / math.sqrt(2.0)
        out["perimeter_px"], out["compactness"] = per, 4.0 * math.pi * n / (per * per)
        out["solidity_rect"] = n / out["rect_area_px2"]
    if mm_per_px is not None:
        f = float(mm_per_px)
        for c in SHAPE_LENGTHS:
            out[c + "_mm"] = out[c + "_px"] * f
        out["area_mm2"], out["rect_area_mm2"] = n * (f * f), out["rect_area_px2"] * (f * f)
    if axis_deg is not None:
        out["direction"] = direction_kind(out["orientation_deg"], out["elongation"], float(axis_deg), axis_tol_deg, min_elongation)
    return out


class InstanceShapes:
    """What ``instance_shapes`` / ``shape_masks`` return.  For the G instances:
      sums int64 [G,16] (SHAPE_COLUMNS), parts int64 [G,2] = n_parts, largest_part_px, pminmax int32 [G,K,2], directions int32
                [K,2]: the raw tables everything is derived from (numpy)
      area_px, n_parts, largest_part_px, euler8, n_holes, edges, rect_k (int64 [G])
      centroid_y, centroid_x (crop coordinates), orientation_deg, axis_major_px, axis_minor_px, elongation, feret_max_px,
                feret_max_deg, feret_min_px, feret_min_deg, rect_long_px, rect_short_px, rect_angle_deg, rect_area_px2,
                perimeter_px, compactness, solidity_rect (float64 [G]); rect_center float64 [G,2] (image y, x; a pixel's centre
                is at its integer coordinates)
      mm_per_px, and with it the _mm columns of every length, area_mm2 and rect_area_mm2
      axis_deg, and with it direction, a list of "longitudinal" / "transverse" / "diagonal" / "none"
      extents(g) float64 [K] in px; rect_corners(g) float64 [4,2] image y, x; part_labels(g) int32 CUDA view [bh,bw]
      table(class_names) one dict per instance"""

    def __init__(self, boxes, offsets, labels_arena, sums, parts, pminmax, dirs, mm_per_px=None, axis_deg=None, axis_tol_deg=22.5,
                 min_elongation=1.5, classid=None, score=None):
        self.boxes, self._offsets = np.asarray(boxes, np.int32).reshape(-1, 4), list(offsets)
        self.labels_arena = labels_arena
        self.directions = np.asarray(dirs, np.int32).reshape(-1, 2)
        K, G = int(self.directions.shape[0]), int(self.boxes.shape[0])
        self.sums = np.asarray(sums, np.int64).reshape(G, 16)
        self.parts = np.asarray(parts, np.int64).reshape(G, 2)
        self.pminmax = np.asarray(pminmax, np.int32).reshape(G, K, 2)
        self.mm_per_px = None if mm_per_px is None else float(mm_per_px)
        self.axis_deg = None if axis_deg is None else float(axis_deg)
        self.axis_tol_deg, self.min_elongation = float(axis_tol_deg), float(min_elongation)
        self.classid, self.score = classid, score
        rows = [derive_shape(self.sums[g], self.parts[g], self.pminmax[g], self.directions, (int(self.boxes[g][0]), int(self.boxes[g][1])),
                             self.mm_per_px, self.axis_deg, self.axis_tol_deg, self.min_elongation) for g in range(G)]
        for c in SHAPE_INTS:
            setattr(self, c, np.array([r[c] for r in rows], np.int64))
        floats = list(SHAPE_FLOATS)
        if self.mm_per_px is not None:
            floats += [c + "_mm" for c in SHAPE_LENGTHS] + ["area_mm2", "rect_area_mm2"]
        self._floats = tuple(floats)
        for c in floats:
            setattr(self, c, np.array([r[c] for r in rows], np.float64))
        self.rect_center = np.array([r["rect_center"] for r in rows], np.float64).reshape(G, 2)
        self._corners = np.array([r["rect_corners"] for r in rows], np.float64).reshape(G, 4, 2)
        if self.axis_deg is not None:
            self.direction = [r["direction"] for r in rows]

    def __len__(self) -> int:
        return int(self.boxes.shape[0])

    def extents(self, g: int) -> np.ndarray:
        return shape_ext(self.pminmax[g], self.directions) / float(SHAPE_UNIT)

    def rect_corners(self, g: int) -> np.ndarray:
        return self._corners[g].copy()

    def part_labels(self, g: int) -> torch.Tensor:
        y1, x1, y2, x2 = (int(v) for v in self.boxes[g])
        n = (y2 - y1) * (x2 - x1)
        return self.labels_arena[self._offsets[g]:self._offsets[g] + n].view(y2 - y1, x2 - x1)

    def table(self, class_names: Optional[Sequence[str]] = None) -> List[dict]:
        rows = []
        for g in range(len(self)):
            row = {"instance": g, "box": tuple(int(v) for v in self.boxes[g])}
            if self.classid is not None:
                k = int(self.classid[g])
                row["class"] = class_names[k] if class_names is not None else k
            if self.score is not None:
                row["score"] = float(self.score[g])
            row.update({c: int(getattr(self, c)[g]) for c in SHAPE_INTS if c != "rect_k"})
            row.update({c: float(getattr(self, c)[g]) for c in self._floats})
            row["rect_center_yx"] = (float(self.rect_center[g][0]), float(self.rect_center[g][1]))
            if self.axis_deg is not None:
                row["direction"] = self.direction[g]
            rows.append(row)
        return rows


def _check_shape(directions, mm_per_px, axis_deg, axis_tol_deg, min_elongation) -> np.ndarray:
    """-> the direction table"""
    dirs = shape_directions(directions)
    if mm_per_px is not None and not (np.isfinite(float(mm_per_px)) and float(mm_per_px) > 0.0):
        raise ValueError("mm_per_px must be a positive number (got %r)" % (mm_per_px,))
    if axis_deg is not None and not np.isfinite(float(axis_deg)):
        raise ValueError("axis_deg must be a finite number (got %r)" % (axis_deg,))
    if not 0.0 < float(axis_tol_deg) <= 45.0:
        raise ValueError("axis_tol_deg must be in (0, 45] (got %r)" % (axis_tol_deg,))
    if not float(min_elongation) >= 1.0:
        raise ValueError("min_elongation must be at least 1 (got %r)" % (min_elongation,))
    return dirs


def shape_arena(groups, arena, arena_bytes=None, groups_dev=None, directions=180, mm_per_px=None, axis_deg=None, axis_tol_deg=22.5,
                min_elongation=1.5, classid=None, score=None, labels_out=None) -> InstanceShapes:
    """The shapes of the crops of an arena: groups int32 [G,8] and arena uint8 CUDA as ``lib.tile_compose`` takes and writes them
    (a non-zero byte is foreground).  ``labels_out`` (int32 CUDA of at least arena_bytes elements) is used for the part labels
    when given; its elements between two crops are left untouched.  The arena is only read."""
    dirs = _check_shape(directions, mm_per_px, axis_deg, axis_tol_deg, min_elongation)
    groups = np.ascontiguousarray(np.asarray(groups, np.int32).reshape(-1, 8))
    G, K = int(groups.shape[0]), int(dirs.shape[0])
    boxes = groups[:, 2:6]
    offsets = [int(v) * 16 for v in groups[:, 7]]
    rest = (dirs, mm_per_px, axis_deg, axis_tol_deg, min_elongation, classid, score)
    if G == 0 or L.measure_blocks(groups) == 0:
        # nothing to launch and nothing to read: the tables of crops without a pixel are known
        dev = arena.device if torch.is_tensor(arena) else torch.device("cpu")
        labels = torch.empty(0, dtype=torch.int32, device=dev) if labels_out is None else labels_out
        sums = np.zeros((G, 16), np.int64)
        sums[:, 6], sums[:, 7], sums[:, 8], sums[:, 9] = boxes[:, 2] - boxes[:, 0], -1, boxes[:, 3] - boxes[:, 1], -1
        pm = np.empty((G, K, 2), np.int32)
        pm[:, :, 0], pm[:, :, 1] = _INT32_MAX, _INT32_MIN
        out = InstanceShapes(boxes, offsets, labels, sums, np.zeros((G, 2), np.int64), pm, *rest)
        out.groups, out.groups_dev, out.arena = groups, groups_dev, arena
        out.arena_bytes = (int(arena.numel()) if torch.is_tensor(arena) else 0) if arena_bytes is None else int(arena_bytes)
        return out
    dev = arena.device
    nbytes = int(arena.numel()) if arena_bytes is None else int(arena_bytes)
    if groups_dev is None:
        groups_dev = torch.from_numpy(groups).to(dev)
    n = max(nbytes, 1)
    labels = torch.empty(n, dtype=torch.int32, device=dev) if labels_out is None else labels_out
    px = torch.empty(n, dtype=torch.int32, device=dev)
    sums = torch.empty(G, 16, dtype=torch.int64, device=dev)
    parts = torch.empty(G, 2, dtype=torch.int64, device=dev)
    pminmax = torch.empty(G, K, 2, dtype=torch.int32, device=dev)
    L.shape_sums(groups, arena, sums, groups_dev, nbytes)
    L.shape_parts(groups, arena, labels, px, parts, groups_dev, nbytes)
    L.shape_extents(groups, arena, dirs, pminmax, groups_dev, None, nbytes)
    # the one read: the three tables in one transfer (the int32 extrema travel in pairs as int64 words)
    flat = _shape_read(torch.cat([sums.reshape(-1), parts.reshape(-1), pminmax.reshape(-1).view(torch.int64)]))
    pm = np.ascontiguousarray(flat[18 * G:]).view(np.int32).reshape(G, K, 2)
    out = InstanceShapes(boxes, offsets, labels, flat[:16 * G].reshape(G, 16), flat[16 * G:18 * G].reshape(G, 2), pm, *rest)
    out.groups, out.groups_dev, out.arena, out.arena_bytes = groups, groups_dev, arena, nbytes       # (what instance_outlines reads)
    return out


def instance_shapes(m, directions=180, mm_per_px=None, axis_deg=None, axis_tol_deg=22.5, min_elongation=1.5,
                    labels_out=None) -> InstanceShapes:
    """The shape of every instance of ``m``: an InstanceMeasures, a SkeletonGraphs or SkeletonTraces (their measures), or a
    ``TiledDetections``, which is read directly -- shapes need no thinning.  ``directions``: K, an even int in 2 .. 360, the
    directions the extents are taken along (180: one per degree).  ``mm_per_px`` defaults to the scale of ``m``; ``axis_deg``, the
    member's longitudinal axis in the image (degrees from +x towards +y), adds the direction kind: longitudinal within
    ``axis_tol_deg`` (in (0, 45]) of it, transverse within that of its normal, diagonal between, "none" for an instance whose
    elongation is below ``min_elongation`` (>= 1).  ``m`` is not changed."""
    if isinstance(m, SkeletonTraces):
        m = m.graphs
    if isinstance(m, SkeletonGraphs):
        if mm_per_px is None:
            mm_per_px = m.mm_per_px
        m = m.measures
    if isinstance(m, InstanceMeasures):
        if mm_per_px is None:
            mm_per_px = m.mm_per_px
        if len(m) and (m.groups is None or m.arena is None):
            _check_shape(directions, mm_per_px, axis_deg, axis_tol_deg, min_elongation)
            raise ValueError("instance_shapes needs the InstanceMeasures of measure_arena / measure_instances / measure_masks")
        groups = m.groups if m.groups is not None else np.zeros((0, 8), np.int32)
        arena = m.arena if m.arena is not None else m.d2_arena.new_empty(0, dtype=torch.uint8)
        return shape_arena(groups, arena, m.arena_bytes, m.groups_dev, directions, mm_per_px, axis_deg, axis_tol_deg, min_elongation,
                           m.classid, m.score, labels_out)
    if not all(hasattr(m, a) for a in ("groups", "groups_dev", "arena", "arena_bytes", "classid", "score")):
        raise ValueError("instance_shapes needs an InstanceMeasures, a SkeletonGraphs, a SkeletonTraces or a TiledDetections (got %s)"
                         % type(m).__name__)
    if mm_per_px is None:
        mm_per_px = getattr(m, "mm_per_px", None)
    if len(m) == 0:
        return shape_arena(np.zeros((0, 8), np.int32), m.arena, 0, None, directions, mm_per_px, axis_deg, axis_tol_deg, min_elongation,
                           m.classid, m.score, labels_out)
    if m.groups is None:
        _check_shape(directions, mm_per_px, axis_deg, axis_tol_deg, min_elongation)
        raise ValueError("instance_shapes needs the groups table of merge_tiles / detect_tiled")
    return shape_arena(m.groups, m.arena, m.arena_bytes, m.groups_dev, directions, mm_per_px, axis_deg, axis_tol_deg, min_elongation,
                       m.classid, m.score, labels_out)


def pack_masks(masks, fill: int = 0, foreground: int = 1):
    """a list of 2-D bool / uint8 arrays or tensors -> (groups int32 [G,8] with boxes at the origin, arena uint8 numpy,
    arena_bytes): the layout ``lib.tile_compose`` writes.  ``fill`` goes to the bytes between the crops, ``foreground`` to
    the non-zero pixels."""
    crops = []
    for i, m in enumerate(masks):
        a = m.detach().cpu().numpy() if torch.is_tensor(m) else np.asarray(m)
        if a.ndim != 2 or a.dtype not in (np.bool_, np.uint8):
            raise ValueError("mask %d must be a 2-D bool or uint8 array (got %s %s)" % (i, a.dtype, a.shape))
        if max(a.shape) > MAX_SIDE:
            raise ValueError("mask %d is %d x %d: the sides must be at most %d" % (i, a.shape[0], a.shape[1], MAX_SIDE))
        crops.append(a != 0)
    G = len(crops)
    boxes = np.array([[0, 0, c.shape[0], c.shape[1]] for c in crops], np.int32).reshape(-1, 4)
    groups, arena_bytes = L.tile_compose_plan(boxes, np.zeros(G + 1, np.int64))
    arena = np.full(max(arena_bytes, 16), fill, np.uint8)
    for c, off16 in zip(crops, groups[:, 7]):
        arena[int(off16) * 16:int(off16) * 16 + c.size] = np.where(c.reshape(-1), foreground, 0)
    return groups, arena, arena_bytes


def measure_masks(masks, mm_per_px=None, chunk: int = 8, device=None) -> InstanceMeasures:
    """Measure a list of masks of any sizes (2-D bool or uint8, arrays or tensors): the path for users of the plain, non-tiled
    detector.  The masks are packed into one arena on the host and uploaded in one copy."""
    _check_scale(mm_per_px, chunk)
    masks = list(masks)
    if device is None:
        device = next((m.device for m in masks if torch.is_tensor(m) and m.is_cuda), torch.device("cuda:0"))
    groups, arena, arena_bytes = pack_masks(masks)
    if len(masks) == 0:
        return measure_arena(groups, torch.empty(0, dtype=torch.uint8), 0, None, mm_per_px, chunk)
    return measure_arena(groups, torch.from_numpy(arena).to(device), arena_bytes, None, mm_per_px, chunk)


def shape_masks(masks, directions=180, mm_per_px=None, axis_deg=None, axis_tol_deg=22.5, min_elongation=1.5, device=None,
                labels_out=None) -> InstanceShapes:
    """The shapes of a list of masks of any sizes (2-D bool or uint8, arrays or tensors), packed into one arena on the host and
    uploaded in one copy: ``instance_shapes`` for users of the plain, non-tiled detector."""
    _check_shape(directions, mm_per_px, axis_deg, axis_tol_deg, min_elongation)
    masks = list(masks)
    if device is None:
        device = next((m.device for m in masks if torch.is_tensor(m) and m.is_cuda), torch.device("cuda:0"))
    groups, arena, arena_bytes = pack_masks(masks)
    if len(masks) == 0 or L.measure_blocks(groups) == 0:
        return shape_arena(groups, torch.empty(0, dtype=torch.uint8), 0, None, directions, mm_per_px, axis_deg, axis_tol_deg,
                           min_elongation, labels_out=labels_out)
    return shape_arena(groups, torch.from_numpy(arena).to(device), arena_bytes, None, directions, mm_per_px, axis_deg, axis_tol_deg,
                       min_elongation, labels_out=labels_out)


# ---- the outlines of an instance: ordered borders, holes, loader records -----------------------------------------------------------
OUTLINE_COLUMNS = ("instance", "kind", "depth", "parent", "part", "key_px", "key_side", "n_edges", "n_points", "n_corners", "area2")
OUTLINE_PART_COLUMNS = ("instance", "part", "area_px", "n_holes")


def _outline_read(t: torch.Tensor) -> np.ndarray:
    """a copy to the host: every host synchronisation of instance_outlines goes through here"""
    return t.cpu().numpy()


def _outline_bad(what: str):
    return L.DisyoloError("instance_outlines: the loop table does not describe the shapes (%s)" % what)


def order_loops(rows):
    """The rows of ``lib.outline_loops`` (int64 [L, 12], in any order) -> (table int64 [L, 11] (OUTLINE_COLUMNS) sorted by
    (instance, depth, key), order int64 [L] = the row of ``rows`` behind every row of the table).  The nesting follows the rule
    tests/outline_ref.py asserts against point-in-ring: a hole's parent is the outer loop of its part; an outer loop's parent is
    the loop through the E side of the first foreground pixel west of its key pixel if that is a hole, otherwise that loop's
    parent (a sibling further west: a smaller key, so the chain ends); none without such a pixel."""
    rows = np.asarray(rows, np.int64).reshape(-1, L.OUTLINE_ROW)
    n = int(rows.shape[0])
    by_key = np.lexsort((rows[:, 1], rows[:, 0]))
    r = rows[by_key]
    inst, key, area2, part, west = r[:, 0], r[:, 1], r[:, 5], r[:, 6], r[:, 7]
    ident = (inst << 32) | key
    kind = (area2 < 0).astype(np.int64)
    if n and ((area2 == 0).any() or (key < 0).any() or (np.diff(ident) <= 0).any() or (key % 4 != 2 * kind).any()):
        raise _outline_bad("keys")

    def find(i, k):
        at = np.minimum(np.searchsorted(ident, (i << 32) | k), max(n - 1, 0))
        if len(at) and (ident[at] != ((i << 32) | k)).any():
            raise _outline_bad("a loop names one that is not there")
        return at

    parent = np.full(n, -1, np.int64)
    holes = np.flatnonzero(kind == 1)
    parent[holes] = find(inst[holes], 4 * part[holes])
    outer = np.flatnonzero((kind == 0) & (west >= 0))
    met = find(inst[outer], west[outer])
    if (met >= outer).any() or (parent[holes] >= holes).any():
        raise _outline_bad("nesting")
    for i, w in zip(outer.tolist(), met.tolist()):                   # (ascending keys: the sibling to the west is resolved)
        parent[i] = w if kind[w] == 1 else parent[w]
    depth = np.zeros(n, np.int64)
    for _ in range(n):
        deeper = np.where(parent >= 0, depth[parent] + 1, 0)
        if np.array_equal(deeper, depth):
            break
        depth = deeper
    if (depth % 2 != kind).any():
        raise _outline_bad("depths")
    final = np.lexsort((key, depth, inst))
    pos = np.empty(n, np.int64)
    pos[final] = np.arange(n)
    table = np.stack([inst, kind, depth, np.where(parent >= 0, pos[np.maximum(parent, 0)], -1), part, key // 4, key % 4, r[:, 2], r[:, 3],
                      r[:, 4], area2], axis=1)[final].reshape(n, len(OUTLINE_COLUMNS))
    return table, by_key[final]


class InstanceOutlines:
    """What ``instance_outlines`` / ``outline_masks`` return.  For the L loops (closed borders) of the G instances:
      loops     int64 [L, 11] (OUTLINE_COLUMNS): instance, kind (0 an outer border, 1 a hole), depth (the loops around it), parent
                (a row of this table or -1), part (the smallest pixel index of its 8-connected part in the crop), key_px and
                key_side (its smallest edge: pixel index in the crop and 0 = N .. 3 = W), n_edges (pixel sides), n_points,
                n_corners, area2 (twice the enclosed area, negative for a hole); sorted by (instance, depth, key)
      loops_of(g)   the rows of instance g;  point_offsets, corner_offsets int64 [L + 1]
      points(i)     int32 [n_points, 2] (x, y), image coordinates: the pixel border of loop i as cv2.findContours(RETR_TREE,
                CHAIN_APPROX_NONE) lists it, start point included
      corners(i)    int32 [n_corners, 2] (x, y): the ring of turning corners on the corner grid, image coordinates -- pixel (x, y)
                covers [x, x + 1] x [y, y + 1], so a corner c lies at c - 0.5 in the convention where a pixel's centre has integer
                coordinates; its shoelace sum is area2
      points_dev, corners_dev   the same int32 CUDA arrays [N, 2] and [C, 2], every loop at its offset (None with points=False)
      parts     int64 [P, 4] (OUTLINE_PART_COLUMNS): per instance and 8-connected part its area and its holes
      polygons(g)   the loader's dicts {'type': 'out' | 'in', 'all_points_x', 'all_points_y'} of instance g in record order: the
                order matters, an island in a hole is drawn after the hole
      record(image=, image_size=, class_names=)   what ``train_data.defect_train`` takes;  table(class_names)  one dict per loop"""

    def __init__(self, shapes, loops, points=None, corners=None, points_dev=None, corners_dev=None):
        self.shapes, self.boxes, self.classid, self.score = shapes, shapes.boxes, shapes.classid, shapes.score
        self.loops = np.asarray(loops, np.int64).reshape(-1, len(OUTLINE_COLUMNS))
        self.point_offsets = np.concatenate([[0], np.cumsum(self.loops[:, 8])]).astype(np.int64)
        self.corner_offsets = np.concatenate([[0], np.cumsum(self.loops[:, 9])]).astype(np.int64)
        self._points, self._corners, self.points_dev, self.corners_dev = points, corners, points_dev, corners_dev
        self._first = np.searchsorted(self.loops[:, 0], np.arange(len(shapes) + 1))
        lp = self.loops
        ident = (lp[:, 0] << 32) | lp[:, 4]
        roots, inv = np.unique(ident, return_inverse=True)
        area2, holes = np.zeros(len(roots), np.int64), np.zeros(len(roots), np.int64)
        np.add.at(area2, inv, lp[:, 10])
        np.add.at(holes, inv, lp[:, 1])
        self.parts = np.stack([roots >> 32, roots & 0xffffffff, area2 // 2, holes], axis=1).reshape(-1, 4)

    def __len__(self) -> int:
        return int(self.boxes.shape[0])

    def loops_of(self, g: int) -> np.ndarray:
        return self.loops[self._first[g]:self._first[g + 1]]

    def _rows_of(self, g: int) -> range:
        return range(int(self._first[g]), int(self._first[g + 1]))

    def points(self, i: int) -> np.ndarray:
        if self._points is None:
            raise ValueError("instance_outlines was called with points=False")
        return self._points[self.point_offsets[i]:self.point_offsets[i + 1]]

    def corners(self, i: int) -> np.ndarray:
        if self._corners is None:
            raise ValueError("instance_outlines was called with points=False")
        return self._corners[self.corner_offsets[i]:self.corner_offsets[i + 1]]

    def polygons(self, g: int) -> List[dict]:
        out = []
        for i in self._rows_of(g):
            pts = self.points(i)
            out.append({"type": "out" if self.loops[i, 2] % 2 == 0 else "in", "all_points_x": pts[:, 0].tolist(),
                        "all_points_y": pts[:, 1].tolist()})
        return out

    def record(self, image=None, image_size=None, class_names: Optional[Sequence[str]] = None) -> dict:
        """One record of the loader: the instances that have a border (an empty mask has no polygon, and the loader refuses an
        instance that rasterises to nothing), their classes from ``classid`` (all class 0 without one), and ``image`` (RGB uint8
        [H, W, 3]) or ``image_size`` = (h, w).  ``class_names``: the class list (default: the configured one)."""
        if (image is None) == (image_size is None):
            raise ValueError("record needs image or image_size, one of them")
        if class_names is None:
            from . import config as cfg
            class_names = cfg.CLASSES
        keep = [g for g in range(len(self)) if self._first[g + 1] > self._first[g]]
        cls = [int(self.classid[g]) if self.classid is not None else 0 for g in keep]
        rec = {"image": image} if image is not None else {"image_size": (int(image_size[0]), int(image_size[1]))}
        rec["class_names"] = [class_names[k] for k in cls]
        rec["polygons"] = [self.polygons(g) for g in keep]
        return rec

    def table(self, class_names: Optional[Sequence[str]] = None) -> List[dict]:
        rows = []
        for i, r in enumerate(self.loops):
            row = {c: int(v) for c, v in zip(OUTLINE_COLUMNS, r)}
            row["kind"] = "hole" if r[1] else "outer"
            g = int(r[0])
            row["box"] = tuple(int(v) for v in self.boxes[g])
            if self.classid is not None:
                k = int(self.classid[g])
                row["class"] = class_names[k] if class_names is not None else k
            row["area_px"] = abs(int(r[10])) / 2.0
            rows.append(row)
        return rows


def _check_outline_sizes(arena_bytes: int, E: int) -> None:
    if 4 * int(arena_bytes) >= 2 ** 31:
        raise ValueError("instance_outlines: an arena of %d bytes (an edge's key is 4 (offset + pixel) + side: need 4 * arena_bytes < 2^31)"
                         % arena_bytes)
    if E > L.OUTLINE_MAX_LIST:
        raise ValueError("instance_outlines: %d boundary edges (need fewer than 2^30)" % E)


def instance_outlines(m, points: bool = True) -> InstanceOutlines:
    """The outlines of every instance of ``m``: an ``InstanceShapes`` of ``instance_shapes`` / ``shape_arena`` / ``shape_masks``, or
    anything ``instance_shapes`` takes (it is then called with directions=2).  The shapes say before any launch how many edges
    and loops there are; the borders are cycles of a permutation of the boundary edges (csrc/outline.hip, defined by
    tests/outline_ref.py).  ``points=False`` stops after the loop table.  Host synchronisations with an
    InstanceShapes given: one read of the loop table, one of the points and corners; none for G = 0 or masks without a pixel."""
    s = m if isinstance(m, InstanceShapes) else instance_shapes(m, directions=2)
    if any(getattr(s, a, None) is None for a in ("groups", "arena", "arena_bytes")):
        raise ValueError("instance_outlines needs the InstanceShapes of shape_arena / instance_shapes / shape_masks")
    G = len(s)
    E, n_loops = int(s.edges.sum()), int((s.n_parts + s.n_holes).sum())
    nbytes = int(s.arena_bytes)
    _check_outline_sizes(nbytes, E)
    empty = np.zeros((0, 2), np.int32)
    if G == 0 or E == 0:
        return InstanceOutlines(s, np.zeros((0, len(OUTLINE_COLUMNS)), np.int64), empty if points else None, empty if points else None)
    dev = s.arena.device
    groups = s.groups
    groups_dev = s.groups_dev if s.groups_dev is not None else torch.from_numpy(groups).to(dev)
    i32 = lambda *shape: torch.empty(*shape, dtype=torch.int32, device=dev)
    u8 = lambda *shape: torch.empty(*shape, dtype=torch.uint8, device=dev)
    first, sides = i32(max(nbytes, 1)), u8(max(nbytes, 1))
    ekey, nxt, aterm, flag, eidx = i32(E), i32(E), i32(E), u8(E), i32(E, 3)
    work = torch.empty(L.OUTLINE_WORK * E, dtype=torch.int64, device=dev)
    rows = torch.empty(n_loops, L.OUTLINE_ROW, dtype=torch.int64, device=dev)
    ctrl = i32(4)
    rounds = max(int(s.edges.max()) - 1, 0).bit_length()           # 2^rounds >= the edges of a group >= those of a loop of it
    L.outline_edges(groups, s.arena, first, sides, ekey, nxt, flag, aterm, work, ctrl, groups_dev, nbytes)
    L.outline_loops(groups, s.arena, s.labels_arena, first, sides, ekey, nxt, flag, aterm, rounds, work, eidx, rows, ctrl, groups_dev, nbytes)
    flat = _outline_read(torch.cat([rows.reshape(-1), ctrl.view(torch.int64)]))
    listed, taken, over, _ = (int(v) for v in np.ascontiguousarray(flat[-2:]).view(np.int32))
    if over or listed != E or taken != n_loops:
        raise _outline_bad("%d edges listed and %d loops found where the shapes give %d and %d%s"
                           % (listed, taken, E, n_loops, ", a list overflowed" if over else ""))
    raw = flat[:-2].reshape(n_loops, L.OUTLINE_ROW)
    loops, order = order_loops(raw)
    inst = loops[:, 0]
    if n_loops and (inst.min() < 0 or inst.max() >= G):
        raise _outline_bad("instances")
    if not (np.array_equal(_sum_by(inst, 1 - loops[:, 1], G), s.n_parts) and np.array_equal(_sum_by(inst, loops[:, 1], G), s.n_holes)
            and np.array_equal(_sum_by(inst, loops[:, 7], G), s.edges) and np.array_equal(_sum_by(inst, loops[:, 10], G), 2 * s.area_px)):
        raise _outline_bad("the parts, holes, edges or areas per instance differ")
    if not points:
        return InstanceOutlines(s, loops)
    out = InstanceOutlines(s, loops)
    N, C = int(out.point_offsets[-1]), int(out.corner_offsets[-1])
    if N > L.OUTLINE_MAX_LIST or C > L.OUTLINE_MAX_LIST:
        raise _outline_bad("points")
    plan = outline_plan(groups, out, raw, order)
    pts, cor = i32(N, 2), i32(C, 2)
    L.outline_gather(groups, s.arena, ekey, flag, eidx, ctrl, torch.from_numpy(plan).to(dev), pts, cor, groups_dev, nbytes)
    both = _outline_read(torch.cat([pts.reshape(-1), cor.reshape(-1)]))
    out._points, out._corners = both[:2 * N].reshape(N, 2), both[2 * N:].reshape(C, 2)
    out.points_dev, out.corners_dev = pts, cor
    return out


def outline_plan(groups, out: InstanceOutlines, raw, order) -> np.ndarray:
    """int32 [L, 8], what ``lib.outline_gather`` takes: per row of ``raw`` (the rows of ``lib.outline_loops`` as they arrived; ``order``
    from ``order_loops``) where its loop's points and corners begin in the sorted output, the run its chain starts with and its
    runs, and its crop's width, first arena element, x1 and y1"""
    plan = np.zeros((len(order), L.OUTLINE_PLAN), np.int32)
    gr = np.asarray(groups, np.int64).reshape(-1, 8)[out.loops[:, 0]]
    plan[order] = np.stack([out.point_offsets[:-1], out.corner_offsets[:-1], raw[order, 10], raw[order, 9], gr[:, 5] - gr[:, 3],
                            gr[:, 7] * 16, gr[:, 3], gr[:, 2]], axis=1).astype(np.int32)
    return plan


def _sum_by(inst, v, G) -> np.ndarray:
    out = np.zeros(G, np.int64)
    np.add.at(out, inst, v)
    return out


def outline_masks(masks, device=None) -> InstanceOutlines:
    """The outlines of a list of masks of any sizes (2-D bool or uint8, arrays or tensors): ``instance_outlines`` on top of
    ``pack_masks``, for users of the plain, non-tiled detector."""
    return instance_outlines(shape_masks(masks, directions=2, device=device))

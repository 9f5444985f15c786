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

Working memory of skeleton_graph beside what measure_arena holds: two int32 arenas (labels, row numbers), two byte arenas
(links, the pruned skeleton) and the row buffer.  Its host synchronisations: one read per analysis (the row counter and the
per-group spur flags in one copy; once more if the row buffer was too small) and the final copy.
"""
from __future__ import annotations

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
      table(class_names) measures.table extended with pruned_length_px, n_branches, junction_px"""

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
    table = table[np.lexsort((table[:, 1], table[:, 0]))]
    ssq = np.ascontiguousarray(flat[nr + 12 * G:]).view(np.float64)
    pm = InstanceMeasures(m.boxes, m._offsets, m.d2_arena, pruned, flat[nr + 4 * G:nr + 12 * G].reshape(G, 8), ssq,
                          m.group_iterations, mm_per_px, m.classid, m.score)
    pm.groups, pm.groups_dev, pm.arena, pm.arena_bytes = groups, groups_dev, m.arena, nbytes
    return SkeletonGraphs(m, pm, links, labels, table, flat[nr:nr + 4 * G].reshape(G, 4), group_analyses, ~spur, min_branch_px,
                          mm_per_px)


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

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
      table(class_names) one dict per instance"""

    def __init__(self, boxes, offsets, d2_arena, skel_arena, counts, sum_sqrt, group_iterations, mm_per_px=None, classid=None,
                 score=None):
        self.boxes, self._offsets = np.asarray(boxes, np.int32).reshape(-1, 4), list(offsets)
        self.d2_arena, self.skeleton_arena = d2_arena, skel_arena
        self.counts = np.asarray(counts, np.int64).reshape(-1, 8)
        self.sum_sqrt = np.asarray(sum_sqrt, np.float64).reshape(-1)
        self.group_iterations = np.asarray(group_iterations, np.int32).reshape(-1)
        self.iterations = int(self.group_iterations.max()) if self.group_iterations.size else 0
        self.classid, self.score = classid, score
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
        return InstanceMeasures(boxes, offsets, torch.empty(0, dtype=torch.int32, device=dev),
                                torch.empty(0, dtype=torch.uint8, device=dev), np.zeros((0, 8), np.int64), np.zeros(0),
                                np.zeros(0, np.int32), mm_per_px, classid, score)
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
    return InstanceMeasures(boxes, offsets, d2, skel, both[:, :8], ssq, both[:, 9].astype(np.int32), mm_per_px, classid, score)


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

"""Tiled detection: an image larger than the net is cut into overlapping tiles of the net's size, the tiles run through
``YOLONet.evaluation_device`` as batches, and what the tiles saw is joined -- an instance that runs through several tiles
becomes one, and the duplicates the overlaps produce are dropped.

The reference has nothing like it (``image_read``, calculate_test_map.py:149-176, letter-boxes the whole photograph to the
net's size: a 3-pixel crack on a 3000 x 4000 image is half a pixel at 576^2).  The definition is tests/tiles_ref.py; the pixel
work is csrc/tiles.hip (gather, paste into bit planes, seam counts, compose).  DESIGN.md section 4j.

    res = detect_tiled(net, image_rgb, overlap=64)
    res.boxes, res.classid, res.score, res.mask(g), res.merged

The merge rule: two instances of DIFFERENT tiles and the SAME class whose rects intersect are one object when, inside the seam
R both tiles saw, ``|A n B| > 0 and |A n B| >= merge_overlap * min(|A n R|, |B n R|)``.  In the seam both tiles saw the same
pixels, so two views of one defect coincide there; unrelated defects do not.  The same-class rule holds under every ``nms``
mode of the net: a rebar inside a spall stays two instances.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import numpy as np
import torch

from . import config as cfg
from . import lib as L
from .postprocess import paste_rects


def _pair(v, name: str) -> Tuple[int, int]:
    if isinstance(v, (bool, np.bool_)):
        raise ValueError("%s must be an int or a pair of ints (got %r)" % (name, v))
    if isinstance(v, (int, np.integer)):
        return int(v), int(v)
    try:
        a, b = v
    except (TypeError, ValueError):
        raise ValueError("%s must be an int or a pair of ints (got %r)" % (name, v))
    for x in (a, b):
        if isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, np.integer)):
            raise ValueError("%s must be an int or a pair of ints (got %r)" % (name, v))
    return int(a), int(b)


def _check_net(net_size) -> Tuple[int, int]:
    H, W = _pair(net_size, "net_size")
    if H <= 0 or W <= 0 or W % 32:
        raise ValueError("net_size must be positive with a width that is a multiple of 32 (got %r)" % (net_size,))
    return H, W


def plan_axis(n: int, N: int, o: int) -> List[int]:
    """the tile origins along one axis: image side n, net side N, overlap o"""
    if n <= N:
        return [0]
    cnt = -(-(n - o) // (N - o))
    return [(i * (n - N)) // (cnt - 1) for i in range(cnt)]


def plan_tiles(image_h: int, image_w: int, net_size, overlap) -> np.ndarray:
    """int32 [T,2]: the tile origins (y0, x0), row-major.  Neighbouring tiles share at least ``overlap`` pixels (an int, or
    (oy, ox), each 0 <= o <= side // 2), the last tile ends at the image's border, and nothing outside the image is covered
    unless the image is smaller than the net."""
    H, W = _check_net(net_size)
    oy, ox = _pair(overlap, "overlap")
    if image_h <= 0 or image_w <= 0:
        raise ValueError("the image must not be empty (got %d x %d)" % (image_h, image_w))
    if not (0 <= oy <= H // 2 and 0 <= ox <= W // 2):
        raise ValueError("overlap must be in 0 .. side // 2 = (%d, %d) (got %r)" % (H // 2, W // 2, overlap))
    ys, xs = plan_axis(int(image_h), H, oy), plan_axis(int(image_w), W, ox)
    return np.array([(y, x) for y in ys for x in xs], np.int32).reshape(-1, 2)


def tile_windows(tiles: np.ndarray, image_hw, net_size) -> np.ndarray:
    """f32 [T,4]: each tile's clip window [0, 0, min(H, h - y0) / H, min(W, w - x0) / W]"""
    H, W = _check_net(net_size)
    h, w = int(image_hw[0]), int(image_hw[1])
    t = np.asarray(tiles, np.int64).reshape(-1, 2)
    win = np.zeros((t.shape[0], 4), np.float64)
    win[:, 2] = np.minimum(H, h - t[:, 0]) / H
    win[:, 3] = np.minimum(W, w - t[:, 1]) / W
    return win.astype(np.float32)


class TiledDetections:
    """What ``merge_tiles`` / ``detect_tiled`` return.  G groups in rank order (score descending, ties to the lower first
    member):
      boxes int32 [G,4] (y1,x1,y2,x2 in the image), classid int32 [G], score f32 [G] (numpy)
      members   per group the (tile, row) of its detections
      mask(g)   bool CUDA view [y2-y1, x2-x1] of the group's mask cropped to its box; full_mask(g) bool CUDA [h,w]
      owner     int32 CUDA [h,w]: 0, or 1 + the rank of the LAST covering group; merged uint8 CUDA [h,w]: its class + 1
      tiles     int32 [T,2] the plan;  inputs, tile_outputs: the tiles' net inputs and outputs when detect_tiled was asked to keep them
      groups, groups_dev, arena, arena_bytes   the [G,8] table ``lib.tile_compose`` took (numpy and its CUDA copy), the arena
                it wrote the cropped masks into and the bytes of it in use: what ``lib.tile_group_counts`` reads"""

    def __init__(self, tiles, image_hw, boxes, classid, score, members, arena, offsets, owner, merged, groups=None,
                 groups_dev=None, arena_bytes=None):
        self.tiles, self.image_hw = tiles, (int(image_hw[0]), int(image_hw[1]))
        self.boxes, self.classid, self.score, self.members = boxes, classid, score, members
        self._arena, self._offsets = arena, offsets
        self.owner, self.merged = owner, merged
        self.inputs = self.tile_outputs = None
        self.groups, self.groups_dev, self.arena = groups, groups_dev, arena
        self.arena_bytes = int(arena.numel()) if arena_bytes is None else int(arena_bytes)

    def __len__(self) -> int:
        return int(self.boxes.shape[0])

    def mask(self, g: int) -> torch.Tensor:
        y1, x1, y2, x2 = (int(v) for v in self.boxes[g])
        n = (y2 - y1) * (x2 - x1)
        return self._arena[self._offsets[g]:self._offsets[g] + n].view(torch.bool).view(y2 - y1, x2 - x1)

    def full_mask(self, g: int) -> torch.Tensor:
        y1, x1, y2, x2 = (int(v) for v in self.boxes[g])
        out = torch.zeros(self.image_hw, dtype=torch.bool, device=self._arena.device)
        out[y1:y2, x1:x2] = self.mask(g)
        return out


def _host(a) -> np.ndarray:
    return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def _pair_table(rect: np.ndarray, tile: np.ndarray, row: np.ndarray, cls: np.ndarray, tiles: np.ndarray, net_hw, D: int) -> np.ndarray:
    """int32 [P,2]: the pairs a < b of instances of different tiles and the same class whose image rects intersect, in
    lexicographic order.  Only tiles whose windows overlap can hold such a pair, so the instances are laid out per tile
    ([T,D], the empty slots with an empty rect) and compared tile pair by tile pair, all pairs at once: Q D^2 tests for the Q
    overlapping tile pairs instead of N^2."""
    N, T = int(rect.shape[0]), int(tiles.shape[0])
    if N < 2:
        return np.zeros((0, 2), np.int32)
    H, W = net_hw
    ty, tx = tiles[:, 0].astype(np.int64), tiles[:, 1].astype(np.int64)
    near = (np.abs(ty[:, None] - ty[None, :]) < H) & (np.abs(tx[:, None] - tx[None, :]) < W)
    qa, qb = np.nonzero(np.triu(near, 1))
    slot_rect = np.zeros((T, D, 4), np.int64)
    slot_cls = np.full((T, D), -1, np.int64)
    slot_no = np.full((T, D), -1, np.int64)
    slot_rect[tile, row], slot_cls[tile, row], slot_no[tile, row] = rect, cls, np.arange(N)
    A, B = slot_rect[qa][:, :, None, :], slot_rect[qb][:, None, :, :]
    hit = ((np.minimum(A[..., 2], B[..., 2]) > np.maximum(A[..., 0], B[..., 0]))
           & (np.minimum(A[..., 3], B[..., 3]) > np.maximum(A[..., 1], B[..., 1]))
           & (slot_cls[qa][:, :, None] == slot_cls[qb][:, None, :]) & (slot_cls[qa][:, :, None] >= 0))
    q, i, j = np.nonzero(hit)
    a, b = slot_no[qa[q], i], slot_no[qb[q], j]            # (qa < qb and instances are numbered by tile: a < b)
    order = np.lexsort((b, a))
    return np.stack([a[order], b[order]], axis=1).astype(np.int32)


def merge_tiles(tiles, image_hw, net_size, detections, keep, masks, merge_overlap: float = 0.5,
                probe: Optional[dict] = None) -> TiledDetections:
    """The merge stage on its own.  tiles int32 [T,2]; detections [T,D,6] (normalised y1,x1,y2,x2 in the tile, class, score)
    and keep [T,D] (numpy or tensors); masks f32 CUDA [T,D,Hm,Wm] (rows beyond T are ignored)."""
    H, W = _check_net(net_size)
    h, w = int(image_hw[0]), int(image_hw[1])
    tiles = np.ascontiguousarray(np.asarray(tiles, np.int32).reshape(-1, 2))
    T = int(tiles.shape[0])
    if not torch.is_tensor(masks) or not masks.is_cuda or masks.dim() != 4 or masks.dtype != torch.float32:
        raise ValueError("masks must be a float32 CUDA tensor [T,D,Hm,Wm]")
    if not 0.0 <= float(merge_overlap) <= 1.0:
        raise ValueError("merge_overlap must be in 0 .. 1 (got %r)" % (merge_overlap,))
    dev = masks.device
    D, Hm, Wm = int(masks.shape[1]), int(masks.shape[2]), int(masks.shape[3])
    if (torch.is_tensor(detections) and torch.is_tensor(keep) and detections.is_cuda and keep.is_cuda
            and tuple(detections.shape[1:]) == (D, 6) and tuple(keep.shape[1:]) == (D,)):
        # the one host sync of the path: boxes and keep flags in one copy (0 / 1 are exact as float32)
        both = torch.cat([detections.reshape(-1, D * 6).float(), keep.reshape(-1, D).float()], dim=1).cpu().numpy()
        detections, keep = both[:, :D * 6].reshape(-1, D, 6), both[:, D * 6:]
    det = _host(detections).astype(np.float32)[:T]
    kp = _host(keep)[:T] != 0
    if T == 0 or det.shape != (T, D, 6) or kp.shape != (T, D) or masks.shape[0] < T:
        raise ValueError("detections [T,D,6], keep [T,D] and masks [T,D,Hm,Wm] must agree with the %d tiles" % T)
    # ---- the instances: kept rows with a non-empty paste, numbered in (tile, row) order
    kt, kr = np.nonzero(kp)
    rects, ok = paste_rects(det[kt, kr], H, W, (H, W), (Hm, Wm))
    kt, kr, rects = kt[ok].astype(np.int32), kr[ok].astype(np.int32), np.ascontiguousarray(rects[ok])
    N = int(kt.shape[0])
    cls = det[kt, kr, 4].astype(np.int32)
    score = det[kt, kr, 5]
    irect = rects[:, 4:8].astype(np.int64) + tiles[kt][:, [0, 1, 0, 1]]
    irect = np.clip(irect, 0, np.array([h, w, h, w]))
    origins_d = torch.from_numpy(tiles).to(dev)
    tile_d = torch.from_numpy(kt).to(dev)
    planes = torch.empty(N, H, W // 32, dtype=torch.int32, device=dev)
    if N:
        flat = torch.from_numpy(kt.astype(np.int64) * D + kr).to(dev)
        sel, rects_d = masks.reshape(-1, Hm, Wm).index_select(0, flat), torch.from_numpy(rects).to(dev)
        L.tile_paste_bits(sel, rects_d, (H, W), planes)
        if probe is not None:
            probe.update(masks=sel, rects=rects_d)
    # ---- seam counts of the candidate pairs, the join rule, union-find
    pairs = _pair_table(irect, kt, kr, cls, tiles, (H, W), D)
    parent = list(range(N))
    if pairs.shape[0]:
        cnt = L.tile_seam_counts(pairs, kt, tiles, (h, w), planes, (H, W), tile_d, origins_d).cpu().numpy().astype(np.float64)
        join = (cnt[:, 2] > 0) & (cnt[:, 2] >= float(merge_overlap) * np.minimum(cnt[:, 0], cnt[:, 1]))

        def find(i):
            while parent[i] != i:
                parent[i] = parent[parent[i]]
                i = parent[i]
            return i
        for a, b in pairs[join].tolist():
            ra, rb = find(a), find(b)
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)
        parent = [find(i) for i in range(N)]
    # ---- the groups, in rank order: score descending, ties to the lower first member (a root is its group's lowest instance)
    roots, inv = np.unique(np.asarray(parent, np.int64), return_inverse=True)
    G = int(roots.shape[0])
    gscore = np.full(G, -np.inf, np.float32)
    np.maximum.at(gscore, inv, score)
    order = np.lexsort((roots, -gscore))
    rank = np.empty(G, np.int64)
    rank[order] = np.arange(G)
    mem_flat = np.lexsort((np.arange(N), rank[inv.reshape(N)])).astype(np.int32)      # by group rank, then instance number
    start = np.concatenate([[0], np.cumsum(np.bincount(rank[inv.reshape(N)], minlength=G))]).astype(np.int64)
    boxes = np.zeros((G, 4), np.int32)
    gcls = np.zeros(G, np.int32)
    if G:
        r = irect[mem_flat]
        boxes[:, :2] = np.minimum.reduceat(r[:, :2], start[:-1], axis=0)
        boxes[:, 2:] = np.maximum.reduceat(r[:, 2:], start[:-1], axis=0)
        gcls = cls[mem_flat[start[:-1]]].astype(np.int32)
    rows = list(zip(kt[mem_flat].tolist(), kr[mem_flat].tolist()))
    members = [rows[start[g]:start[g + 1]] for g in range(G)]
    groups, arena_bytes = L.tile_compose_plan(boxes, start)
    arena = torch.empty(max(arena_bytes, 16), dtype=torch.uint8, device=dev)
    owner = torch.empty(h, w, dtype=torch.int32, device=dev)
    groups_d = torch.from_numpy(groups).to(dev)
    L.tile_compose(groups, mem_flat, kt, tiles, planes, (H, W), (h, w), arena, owner, tile_d, origins_d, groups_d)
    lut = torch.from_numpy(np.concatenate([[0], gcls + 1]).astype(np.uint8)).to(dev)
    merged = lut[owner.long()]
    if probe is not None:           # what each launch took, for tools/tiles_rate.py
        probe.update(instances=N, pairs=pairs, inst_tile=kt, planes=planes, groups=groups, members=mem_flat,
                     arena=arena, owner=owner, inst_tile_dev=tile_d, origins_dev=origins_d)
    offsets = [int(v) * 16 for v in groups[:, 7]]
    return TiledDetections(tiles, (h, w), boxes, gcls, gscore[order], members, arena, offsets, owner, merged, groups, groups_d,
                           arena_bytes)


def detect_tiled(net, image_rgb, overlap=64, det_thresh=cfg.OBJ_THRESHOLD, merge_overlap: float = 0.5,
                 keep_tiles: bool = False) -> TiledDetections:
    """Detect on an image of any size with an inference net of any batch size and option set.  image_rgb: uint8 [h,w,3]
    (numpy or CUDA).  The T tiles of ``plan_tiles`` run as ceil(T / B) calls of ``net.evaluation_device`` (the recorded
    program where one was built for ``det_thresh``); the last batch is filled with pad tiles whose results are dropped.
    ``keep_tiles``: the result's ``inputs`` holds the tiles' net inputs f32 [T,H,W,3] and ``tile_outputs`` the net's per-tile
    (detections [T,D,6], keep [T,D], masks [T,D,Hm,Wm]), all on the device."""
    if net.training:
        raise ValueError("detect_tiled takes an inference net (training=False)")
    H, W, B = int(net.H), int(net.W), int(net.B)
    dev = net.device
    if not torch.is_tensor(image_rgb):
        image_rgb = torch.from_numpy(np.ascontiguousarray(image_rgb))
    if image_rgb.dim() != 3 or image_rgb.shape[2] != 3 or image_rgb.dtype != torch.uint8:
        raise ValueError("image_rgb must be uint8 [h,w,3] (got %s %s)" % (image_rgb.dtype, list(image_rgb.shape)))
    rgb = image_rgb.to(dev).contiguous()
    h, w = int(rgb.shape[0]), int(rgb.shape[1])
    tiles = plan_tiles(h, w, (H, W), overlap)
    T = int(tiles.shape[0])
    chunks = -(-T // B)
    origins_d = torch.from_numpy(tiles).to(dev)
    windows = np.concatenate([tile_windows(tiles, (h, w), (H, W)),
                              np.tile(np.array([[0, 0, 1, 1]], np.float32), (chunks * B - T, 1))])
    Hm, Wm = net.mask_map_size()
    D = int(net.max_detection)
    det_all = torch.empty(chunks * B, D, 6, dtype=torch.float32, device=dev)
    keep_all = torch.empty(chunks * B, D, dtype=torch.int32, device=dev)
    masks_all = torch.empty(chunks * B, D, Hm, Wm, dtype=torch.float32, device=dev)
    inputs = torch.empty(chunks * B, H, W, 3, dtype=torch.float32, device=dev) if keep_tiles else None
    batch = torch.empty(B, H, W, 3, dtype=torch.float32, device=dev)
    for c in range(chunks):
        t0 = c * B
        buf = inputs[t0:t0 + B] if keep_tiles else batch
        L.tile_gather(rgb, origins_d, t0, t0 + B, buf, (H, W))
        det, keep, masks = net.evaluation_device(buf, windows[t0:t0 + B], det_thresh)
        # copied out before the next chunk overwrites the net's buffers (same stream: no sync)
        det_all[t0:t0 + B].copy_(det)
        keep_all[t0:t0 + B].copy_(keep)
        masks_all[t0:t0 + B].copy_(masks)
    res = merge_tiles(tiles, (h, w), (H, W), det_all[:T], keep_all[:T], masks_all, merge_overlap)
    if keep_tiles:
        res.inputs, res.tile_outputs = inputs[:T], (det_all[:T], keep_all[:T], masks_all[:T])
    return res

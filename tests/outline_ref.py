"""The definition of instance outlines (dis-yolo_amd/measure.py ``instance_outlines``, csrc/outline.hip), in numpy and Python ints:
there is no float in this file.

A crop M is a 2-D array of bh x bw; F = M != 0 is foreground, everything outside the crop is background; foreground is
8-connected and background 4-connected, as in tests/shape_ref.py.  Pixel (x, y) has the index p = y bw + x and covers the square
[x, x + 1] x [y, y + 1] of the corner grid.

  edge       (p, s): p a foreground pixel, s a side whose 4-neighbour across it is background (0 = N, 1 = E, 2 = S, 3 = W); its
             key is 4 p + s.  It is walked clockwise with y down: N from corner (x, y) to (x + 1, y), E on to (x + 1, y + 1), S on
             to (x, y + 1), W back to (x, y).  FWD[s] is the direction of travel, OUT[s] the step to the neighbour across the side.
  successor  the first that applies: the pixel at p + FWD[s] + OUT[s] is foreground -> that pixel, side (s + 3) % 4 (a left turn:
             testing the diagonal first is the 8-connectivity rule); the pixel at p + FWD[s] is foreground -> that pixel, side s;
             otherwise (p, (s + 1) % 4).  A permutation of the boundary edges: its cycles are the loops.
  loop       key = its smallest edge key; n_edges; area2 = the sum over its edges of N: -y, E: x + 1, S: y + 1, W: -x (the shoelace
             sum, twice the enclosed area: > 0 an outer border, kind 0; < 0 a hole, kind 1); part = the smallest pixel index of the
             8-connected part that owns its pixels; ring = the start corners of the edges whose predecessor has another side, from
             the first such edge at or after the key edge; chain = the pixel border as cv2.findContours(CHAIN_APPROX_NONE) lists
             it: cut the cycle of owner pixels into maximal cyclic runs of one owner, start with the run that holds the key edge
             (outer) or the loop's smallest-key E-side edge (hole), then the other runs in REVERSE cyclic order.
  nesting    depth = the number of other loops that enclose the loop, parent = the innermost of them or -1: by brute force here
             (point in ring with the integer crossing rule), and the rule a device may use instead is asserted (``west``).
  order      the loops of a crop sorted by (depth, key); polygons in that order, 'out' for even and 'in' for odd depth, are the
             instance's record as the loader (train_data.rasterize_instance, the oracle's instance_mask) takes it.

``outline`` asserts on every crop: sum of area2 = 2 n, sum of n_edges = shape_ref's edges, outer loops = n_parts, holes = n_holes,
every chain equals disyolo_oracle.find_contours_tree's contour (crops of at most ORACLE_PIXELS pixels: the oracle is a Python
loop), and the record drawn by disyolo_oracle.instance_mask gives back F (while the polygon test stays below MASK_WORK point
tests)."""
import numpy as np

import shape_ref as S

FWD = ((1, 0), (0, 1), (-1, 0), (0, -1))          # (dx, dy) of travel along side s
OUT = ((0, -1), (1, 0), (0, 1), (-1, 0))          # (dx, dy) to the neighbour across side s
CORNER = ((0, 0), (1, 0), (1, 1), (0, 1))         # the start corner of side s, relative to the pixel
LOOP_COLUMNS = ("instance", "kind", "depth", "parent", "part", "key_px", "key_side", "n_edges", "n_points", "n_corners", "area2")
ORACLE_PIXELS = 40000
MASK_WORK = 200000


def successor(P, bw, x, y, s):
    """P = F padded by one ring; -> (x, y, s) of the next edge"""
    fx, fy = FWD[s]
    ox, oy = OUT[s]
    if P[y + fy + oy + 1, x + fx + ox + 1]:
        return x + fx + ox, y + fy + oy, (s + 3) % 4
    if P[y + fy + 1, x + fx + 1]:
        return x + fx, y + fy, s
    return x, y, (s + 1) % 4


def area_term(x, y, s):
    return (-y, x + 1, y + 1, -x)[s]


def boundary_keys(F):
    """the keys of all boundary edges, ascending"""
    P = np.pad(F, 1)
    c = P[1:-1, 1:-1]
    sides = [c & ~P[:-2, 1:-1], c & ~P[1:-1, 2:], c & ~P[2:, 1:-1], c & ~P[1:-1, :-2]]
    keys = [4 * np.flatnonzero(m.reshape(-1)).astype(np.int64) + s for s, m in enumerate(sides)]
    return np.sort(np.concatenate(keys)) if F.size else np.zeros(0, np.int64)


def inside(ring, cx, cy):
    """is the centre of pixel (cx, cy) inside the ring (corner-grid points, axis-parallel sides)?  The crossing rule on a ray to
    the west: the vertical sides at X <= cx that span cy .. cy + 1"""
    n, r = 0, ring
    x0, y0 = r[:, 0], r[:, 1]
    x1, y1 = np.roll(x0, -1), np.roll(y0, -1)
    hit = (x0 == x1) & (x0 <= cx) & (np.minimum(y0, y1) <= cy) & (cy < np.maximum(y0, y1))
    return int(hit.sum()) & 1 == 1


def trace(M):
    """the loops of a crop in key order, without nesting: a list of dicts"""
    F = np.asarray(M) != 0
    bh, bw = F.shape
    P = np.pad(F, 1)
    labels = S.components(F, True)
    seen = set()
    loops = []
    for key in boundary_keys(F).tolist():
        if key in seen:
            continue
        p, s = divmod(key, 4)
        y, x = divmod(p, bw)
        seq = []
        cx, cy, cs = x, y, s
        while True:
            seq.append((cx, cy, cs))
            seen.add(4 * (cy * bw + cx) + cs)
            cx, cy, cs = successor(P, bw, cx, cy, cs)
            if (cx, cy, cs) == (x, y, s):
                break
        n = len(seq)
        area2 = sum(area_term(*e) for e in seq)
        kind = 0 if area2 > 0 else 1
        assert area2 != 0 and s == (0, 2)[kind]                   # an outer loop's key edge is a N side, a hole's a S side
        heads = [i for i in range(n) if seq[i][:2] != seq[i - 1][:2]]
        runs = heads or [0]
        start = 0
        if kind == 1:
            east = [(4 * (e[1] * bw + e[0]) + 1, i) for i, e in enumerate(seq) if e[2] == 1]
            start = min(east)[1]
        at = [j for j, h in enumerate(runs) if h <= start]
        j0 = at[-1] if at else len(runs) - 1
        chain = np.array([seq[runs[(j0 - k) % len(runs)]][:2] for k in range(len(runs))], np.int32).reshape(-1, 2)
        turns = [i for i in range(n) if seq[i][2] != seq[i - 1][2]]
        ring = np.array([(seq[i][0] + CORNER[seq[i][2]][0], seq[i][1] + CORNER[seq[i][2]][1]) for i in turns], np.int32).reshape(-1, 2)
        rx, ry = ring[:, 0].astype(np.int64), ring[:, 1].astype(np.int64)
        assert int((rx * np.roll(ry, -1) - np.roll(rx, -1) * ry).sum()) == area2       # the ring alone gives the area
        loops.append({"key": key, "key_px": p, "key_side": s, "n_edges": n, "area2": area2, "kind": kind, "part": int(labels[y, x]),
                      "n_points": len(runs), "n_corners": len(turns), "chain": chain, "ring": ring,
                      "edge_keys": [4 * (e[1] * bw + e[0]) + e[2] for e in seq]})
    return loops


def nest(loops, F):
    """adds depth, parent (an index into ``loops``) and west (the key of the loop through (Q, E), or -1) to every loop: by brute
    force, and asserts the rule a device may use"""
    bh, bw = F.shape
    of_edge = {k: i for i, l in enumerate(loops) for k in l["edge_keys"]}
    box = np.array([[l["ring"][:, 0].min(), l["ring"][:, 0].max(), l["ring"][:, 1].min(), l["ring"][:, 1].max()] for l in loops]).reshape(-1, 4)
    for i, l in enumerate(loops):
        y, x = divmod(l["key_px"], bw)
        if l["kind"] == 1:
            y += 1                                                  # the background pixel across the key edge (a S side)
        near = np.flatnonzero((box[:, 0] <= x) & (x < box[:, 1]) & (box[:, 2] <= y) & (y < box[:, 3]))      # (a ring lies in its box)
        around = [j for j in near.tolist() if j != i and inside(loops[j]["ring"], x, y)]
        l["depth"] = len(around)
        assert (l["depth"] % 2 == 0) == (l["kind"] == 0)
        # the innermost: the one every other encloser encloses, i.e. the one with the most enclosers itself -- found after the loop
        l["_around"] = around
    for i, l in enumerate(loops):
        l["parent"] = max(l["_around"], key=lambda j: loops[j]["depth"]) if l["_around"] else -1
        assert l["parent"] < 0 or loops[l["parent"]]["depth"] == l["depth"] - 1
    for i, l in enumerate(loops):
        l["west"] = -1
        if l["kind"] == 1:
            want = next(j for j, o in enumerate(loops) if o["kind"] == 0 and o["key_px"] == l["part"])
        else:
            assert l["part"] == l["key_px"]
            y, x = divmod(l["key_px"], bw)
            q = next((qx for qx in range(x - 1, -1, -1) if F[y, qx]), -1)
            if q < 0:
                want = -1
            else:
                j = of_edge[4 * (y * bw + q) + 1]
                l["west"] = loops[j]["key"]
                want = j if loops[j]["kind"] == 1 else loops[j]["parent"]
        assert want == l["parent"], "the parent rule"
    for l in loops:
        del l["_around"]


def instance_mask_work(polys):
    return sum((max(p["all_points_y"]) - min(p["all_points_y"]) + 1) * (max(p["all_points_x"]) - min(p["all_points_x"]) + 1) *
               len(p["all_points_x"]) for p in polys)


def polygons_of(loops, origin=(0, 0)):
    """the loader's record of one instance: origin = the crop's (y1, x1) in the image"""
    return [{"type": "out" if l["depth"] % 2 == 0 else "in", "all_points_x": [int(v) + int(origin[1]) for v in l["chain"][:, 0]],
             "all_points_y": [int(v) + int(origin[0]) for v in l["chain"][:, 1]]} for l in loops]


def outline(M, origin=(0, 0), oracle=None):
    """everything about one crop: {"loops": the loops sorted by (depth, key), parent an index into that order; "table": int64
    [L, 11] (LOOP_COLUMNS, instance = 0); "points": int32 [N, 2] and "corners": int32 [C, 2], the chains and rings one behind the
    other in image (x, y); "parts": int64 [n_parts, 3] = part, area_px, n_holes by part; "polygons"}.  ``oracle``: compare with
    the oracle's tracer and rasteriser (None: where the crop is small enough for them)."""
    M = np.asarray(M)
    F = M != 0
    loops = trace(F)
    nest(loops, F)
    order = sorted(range(len(loops)), key=lambda i: (loops[i]["depth"], loops[i]["key"]))
    new = {old: k for k, old in enumerate(order)}
    loops = [loops[i] for i in order]
    for l in loops:
        l["parent"] = new[l["parent"]] if l["parent"] >= 0 else -1
    s = S.sums(F)
    labels, n_parts, _ = S.parts(F)
    assert sum(l["area2"] for l in loops) == 2 * int(s[0])
    assert sum(l["n_edges"] for l in loops) == S.edges(s)
    assert sum(l["kind"] == 0 for l in loops) == n_parts and sum(l["kind"] == 1 for l in loops) == n_parts - S.euler8(s)
    table = np.array([[0, l["kind"], l["depth"], l["parent"], l["part"], l["key_px"], l["key_side"], l["n_edges"], l["n_points"],
                       l["n_corners"], l["area2"]] for l in loops], np.int64).reshape(-1, len(LOOP_COLUMNS))
    off = np.array([origin[1], origin[0]], np.int32)
    points = np.concatenate([l["chain"] + off for l in loops] + [np.zeros((0, 2), np.int32)]).astype(np.int32)
    corners = np.concatenate([l["ring"] + off for l in loops] + [np.zeros((0, 2), np.int32)]).astype(np.int32)
    parts = []
    for l in loops:
        if l["kind"] == 0:
            mine = [h for h in loops if h["kind"] == 1 and h["part"] == l["part"]]
            a2 = l["area2"] + sum(h["area2"] for h in mine)
            assert a2 % 2 == 0 and a2 // 2 == int((labels == l["part"]).sum())
            parts.append((l["part"], a2 // 2, len(mine)))
    parts = np.array(sorted(parts), np.int64).reshape(-1, 3)
    polys = polygons_of(loops)
    if oracle or (oracle is None and F.size <= ORACLE_PIXELS):
        import disyolo_oracle as O
        contours, _ = O.find_contours_tree(F.astype(np.uint8))
        assert sorted(c.tobytes() for c in contours) == sorted(np.ascontiguousarray(l["chain"]).tobytes() for l in loops)
        if oracle or instance_mask_work(polys) <= MASK_WORK:
            assert np.array_equal(O.instance_mask(polys, F.shape[0], F.shape[1]), F)
    return {"loops": loops, "table": table, "points": points, "corners": corners, "parts": parts,
            "polygons": polygons_of(loops, origin)}


# ---- crops with known answers: name -> rows (key_px, key_side, n_edges, area2, n_points) in (depth, key) order -------------------
def frame():
    M = np.ones((70, 300), np.uint8)
    M[1:-1, 1:-1] = 0
    return M


def nest11():
    M = np.ones((11, 11), np.uint8)
    M[2:9, 2:9] = 0
    M[4:7, 4:7] = 1
    M[5, 5] = 0
    return M


def nest11_open():
    M = nest11()
    M[1, 1] = 0
    return M


def checker33():
    yy, xx = np.mgrid[:33, :33]
    return ((yy + xx) % 2 == 0).astype(np.uint8)


def known_crops():
    ring = np.ones((3, 3), np.uint8)
    ring[1, 1] = 0
    return {"1x1": np.ones((1, 1), np.uint8), "1x3": np.ones((1, 3), np.uint8), "eye3": np.eye(3, dtype=np.uint8),
            "2x2": np.ones((2, 2), np.uint8), "ring3": ring, "frame": frame(), "checker33": checker33(), "nest11": nest11(),
            "nest11_open": nest11_open()}


def known_rows():
    return {
        "1x1": [(0, 0, 4, 2, 1)],
        "1x3": [(0, 0, 8, 6, 4)],
        "eye3": [(0, 0, 12, 6, 4)],
        "2x2": [(0, 0, 8, 8, 4)],
        "ring3": [(0, 0, 12, 18, 8), (1, 2, 4, -2, 4)],
        "frame": [(0, 0, 740, 42000, 736), (1, 2, 732, -40528, 732)],
        "nest11": [(0, 0, 44, 242, 40), (13, 2, 28, -98, 28), (48, 0, 12, 18, 8), (49, 2, 4, -2, 4)],
        "nest11_open": [(0, 0, 44, 242, 40), (1, 2, 4, -2, 4), (13, 2, 28, -98, 28), (48, 0, 12, 18, 8), (49, 2, 4, -2, 4)],
    }

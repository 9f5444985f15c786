"""The definition of instance shape (dis-yolo_amd/measure.py ``instance_shapes``, csrc/shape.hip), in plain numpy.

The reference project has nothing of this kind, so these functions ARE the semantics.  Everything the device computes is an
integer, and the HIP path agrees with it exactly; the float64 columns come from those integers by ``derive``, which
``measure.py`` repeats expression for expression, so they agree bit for bit as well.

A crop M is a 2-D array of bh x bw; F = M != 0 is foreground, everything outside the crop is background.  Pixel (y, x) has the
linear index y bw + x and stands for the unit square around (y, x).

  sums(M)      int64 [16] = n, Sy, Sx, Syy, Sxx, Sxy over F; the tight box ymin, ymax, xmin, xmax (inclusive; an empty crop
               gives bh, -1, bw, -1); the bit quads Q1, Q2, Q3, Q4, QD; 0.
               With sides <= 32767 every sum fits int64: the largest, Sxx of a full crop of the largest box, is
               n (bw - 1)(2 bw - 1) / 6 = 32767 * (32766 * 32767 * 65533 / 6) < 3.9e17 < 2^63.
  quads(M)     Gray (1971): over all (bh + 1)(bw + 1) 2x2 windows of the crop padded by one ring of background, Q1 / Q3 / Q4 =
               the windows with one / three / four pixels set, Q2 = two in a row or a column, QD = two on a diagonal.
               Q1 + 2 (Q2 + QD) + 3 Q3 + 4 Q4 = 4 n;  euler8 = (Q1 - Q3 - 2 QD) / 4 (the division is exact);
               edges = Q1 + Q2 + Q3 + 2 QD = the pixel sides between a foreground and a background pixel.
  parts(M)     (labels int32: on F the smallest linear index of the pixel's 8-connected component, -1 off F; n_parts;
               largest_part_px).  n_holes = n_parts - euler8 = the 4-connected background components of the ring-padded crop
               that do not contain the ring (asserted on every crop ``shape`` is given).
  directions(K)  int32 [K, 2], K even in 2 .. 360: (c_k, s_k) = (round(16384 cos(k pi / K)), round(16384 sin(k pi / K))).
  extents(M, dirs)  pminmax int32 [K, 2]: the minimum and maximum over F of p = c_k x + s_k y ((INT32_MAX, INT32_MIN) for an
               empty crop); the same over the boundary pixels of F alone (asserted).  ext[k] = max - min + |c_k| + |s_k|, in
               2^-14 px; 0 for an empty crop.
  derive(...)  the float64 columns of one instance from its integers: see there.

What the rules do to the numbers:
  * the rectangle is the best of K / 2 orientations, not the true minimum: with K = 180 the long side of a bar is overestimated
    by at most short * sin 1 degree;
  * feret_max of a 1 x 9 bar is 9.06 at 6 degrees: the diagonal of the pixel squares, not 9;
  * n_holes counts 4-connected background: a diagonal gap closes a hole's wall but does not join two holes;
  * orientation is measured in image axes from +x towards +y (y runs down): np.eye(9) lies at 45 degrees.
"""
import math

import numpy as np

COLS = ("n", "Sy", "Sx", "Syy", "Sxx", "Sxy", "ymin", "ymax", "xmin", "xmax", "Q1", "Q2", "Q3", "Q4", "QD", "zero")
Q14 = 16384
INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31


def directions(K) -> np.ndarray:
    if isinstance(K, (bool, np.bool_)) or not isinstance(K, (int, np.integer)) or not 2 <= int(K) <= 360 or int(K) % 2:
        raise ValueError("directions must be an even int in 2 .. 360 (got %r)" % (K,))
    K = int(K)
    return np.array([[round(Q14 * math.cos(k * math.pi / K)), round(Q14 * math.sin(k * math.pi / K))] for k in range(K)], np.int32)


def quads(M):
    """-> (Q1, Q2, Q3, Q4, QD)"""
    P = np.pad(np.asarray(M) != 0, 1).astype(np.int64)
    a, b, c, d = P[:-1, :-1], P[:-1, 1:], P[1:, :-1], P[1:, 1:]
    s = a + b + c + d
    two = s == 2
    return (int((s == 1).sum()), int((two & (a != d)).sum()), int((s == 3).sum()), int((s == 4).sum()), int((two & (a == d)).sum()))


def edges_direct(M) -> int:
    P = np.pad(np.asarray(M) != 0, 1)
    return int((P[:, :-1] != P[:, 1:]).sum() + (P[:-1, :] != P[1:, :]).sum())


def sums(M) -> np.ndarray:
    F = np.asarray(M) != 0
    bh, bw = F.shape
    y, x = (v.astype(np.int64) for v in np.nonzero(F))
    out = np.zeros(16, np.int64)
    out[:6] = len(y), y.sum(), x.sum(), (y * y).sum(), (x * x).sum(), (x * y).sum()
    out[6:10] = (y.min(), y.max(), x.min(), x.max()) if len(y) else (bh, -1, bw, -1)
    out[10:15] = quads(F) if F.size else 0
    n, (q1, q2, q3, q4, qd) = int(out[0]), (int(v) for v in out[10:15])
    assert q1 + 2 * (q2 + qd) + 3 * q3 + 4 * q4 == 4 * n and (q1 - q3 - 2 * qd) % 4 == 0
    assert q1 + q2 + q3 + 2 * qd == edges_direct(F)
    return out


def euler8(s) -> int:
    return (int(s[10]) - int(s[12]) - 2 * int(s[14])) // 4


def edges(s) -> int:
    return int(s[10]) + int(s[11]) + int(s[12]) + 2 * int(s[14])


def components(F, eight: bool) -> np.ndarray:
    """int64 map: on F the smallest linear index of the pixel's component (8- or 4-connected), -1 off F.  Union-find over the
    runs of the rows: two runs of neighbouring rows are joined when their columns overlap (reaching one further for 8)."""
    F = np.asarray(F, bool)
    bh, bw = F.shape
    out = np.full((bh, bw), -1, np.int64)
    if F.size == 0:
        return out
    d = np.diff(np.pad(F, ((0, 0), (1, 1))).astype(np.int8), axis=1)
    ry, rs = np.nonzero(d == 1)
    re = np.nonzero(d == -1)[1]                                   # one past the run's last column
    parent = list(range(len(ry)))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    first = np.searchsorted(ry, np.arange(bh + 1))
    reach = 1 if eight else 0
    for y in range(1, bh):
        i, j, ie, je = int(first[y - 1]), int(first[y]), int(first[y]), int(first[y + 1])
        while i < ie and j < je:
            if rs[i] < re[j] + reach and rs[j] < re[i] + reach:
                a, b = find(i), find(j)
                if a != b:
                    parent[max(a, b)] = min(a, b)                   # (runs are in index order: the smaller run is the smaller pixel)
            if re[i] <= re[j]:
                i += 1
            else:
                j += 1
    for r in range(len(ry)):
        root = find(r)
        out[ry[r], rs[r]:re[r]] = int(ry[root]) * bw + int(rs[root])
    return out


def parts(M):
    """-> (labels int32, n_parts, largest_part_px)"""
    labels = components(np.asarray(M) != 0, True)
    roots, px = np.unique(labels[labels >= 0], return_counts=True)
    return labels.astype(np.int32), int(len(roots)), int(px.max()) if len(px) else 0


def holes_direct(M) -> int:
    """the 4-connected background components of the ring-padded crop that do not contain the ring"""
    B = ~np.pad(np.asarray(M) != 0, 1)
    lab = components(B, False)
    return int(len(np.unique(lab[B]))) - 1


def boundary(M) -> np.ndarray:
    """the foreground pixels with a background 4-neighbour, the ring included"""
    P = np.pad(np.asarray(M) != 0, 1)
    return P[1:-1, 1:-1] & ~(P[:-2, 1:-1] & P[2:, 1:-1] & P[1:-1, :-2] & P[1:-1, 2:])


def _pminmax(F, dirs) -> np.ndarray:
    y, x = (v.astype(np.int64) for v in np.nonzero(F))
    out = np.empty((len(dirs), 2), np.int64)
    out[:, 0], out[:, 1] = INT32_MAX, INT32_MIN
    if len(y):
        p = dirs[:, :1].astype(np.int64) * x[None, :] + dirs[:, 1:].astype(np.int64) * y[None, :]
        assert np.abs(p).max() <= Q14 * 65532
        out[:, 0], out[:, 1] = p.min(axis=1), p.max(axis=1)
    return out.astype(np.int32)


def extents(M, dirs) -> np.ndarray:
    F = np.asarray(M) != 0
    out = _pminmax(F, dirs)
    assert np.array_equal(out, _pminmax(boundary(F), dirs))
    return out


def ext_of(pminmax, dirs) -> np.ndarray:
    """int64 [K]: max - min + |c| + |s| (2^-14 px), 0 for an empty crop"""
    pm, d = np.asarray(pminmax, np.int64), np.asarray(dirs, np.int64)
    return np.where(pm[:, 1] >= pm[:, 0], pm[:, 1] - pm[:, 0] + np.abs(d[:, 0]) + np.abs(d[:, 1]), 0)


LENGTHS = ("axis_major", "axis_minor", "feret_max", "feret_min", "rect_long", "rect_short", "perimeter")


def direction_kind(orientation_deg, elongation, axis_deg, axis_tol_deg=22.5, min_elongation=1.5) -> str:
    if elongation < min_elongation:
        return "none"
    delta = abs(((orientation_deg - axis_deg + 90.0) % 180.0) - 90.0)
    return "longitudinal" if delta <= axis_tol_deg else "transverse" if delta >= 90.0 - axis_tol_deg else "diagonal"


def derive(s, p, pminmax, dirs, origin=(0, 0), mm_per_px=None, axis_deg=None, axis_tol_deg=22.5, min_elongation=1.5) -> dict:
    """One instance: s int [16] (COLS), p int [2] = (n_parts, largest_part_px), pminmax int [K, 2], dirs int [K, 2], origin =
    the crop's (y1, x1) in the image.  Exact Python ints until the last step of every column, then float64.
      area_px, n_parts, largest_part_px, n_holes, euler8, edges (int)
      centroid_y, centroid_x = Sy / n, Sx / n (crop coordinates)
      orientation_deg = degrees(atan2(2 Mxy, Mxx - Myy) / 2) mod 180 of the central moments Mxx = n Sxx - Sx^2, ...
      axis_major_px, axis_minor_px = 4 sqrt(l1), 4 sqrt(l2), elongation = sqrt(l1 / l2): l1 >= l2 the eigenvalues of the covariance
            with 1/12 added to its diagonal (a pixel is a unit square)
      feret_max_px, feret_max_deg, feret_min_px, feret_min_deg: the largest and smallest ext[k] / 16384 at 180 k / K, first k on a tie
      rect_k, rect_long_px, rect_short_px, rect_angle_deg (of the long side), rect_area_px2, rect_center (y, x), rect_corners [4, 2]
            (y, x): the smallest ext[k] ext[k + K/2] over k < K/2, compared as integers, first k on a tie; image coordinates
      perimeter_px = Q2 + (Q1 + Q3 + 2 QD) / sqrt(2), compactness = 4 pi n / perimeter^2, solidity_rect = n / rect_area_px2
      with mm_per_px the _mm / _mm2 columns; with axis_deg the direction kind.  An empty crop: every number 0."""
    n, Sy, Sx, Syy, Sxx, Sxy = (int(v) for v in s[:6])
    q1, q2, q3, q4, qd = (int(v) for v in s[10:15])
    K = len(dirs)
    e8 = (q1 - q3 - 2 * qd) // 4
    out = {"area_px": n, "n_parts": int(p[0]), "largest_part_px": int(p[1]), "euler8": e8, "n_holes": int(p[0]) - e8,
           "edges": q1 + q2 + q3 + 2 * qd}
    zero = ("centroid_y", "centroid_x", "orientation_deg", "axis_major_px", "axis_minor_px", "elongation", "feret_max_px",
            "feret_max_deg", "feret_min_px", "feret_min_deg", "rect_long_px", "rect_short_px", "rect_angle_deg", "rect_area_px2",
            "perimeter_px", "compactness", "solidity_rect")
    if n == 0:
        out.update({c: 0.0 for c in zero})
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
        ext = [int(v) for v in ext_of(pminmax, dirs)]
        kmax, kmin = ext.index(max(ext)), ext.index(min(ext))
        out["feret_max_px"], out["feret_max_deg"] = ext[kmax] / Q14, 180.0 * kmax / K
        out["feret_min_px"], out["feret_min_deg"] = ext[kmin] / Q14, 180.0 * kmin / K
        prod = [ext[k] * ext[k + K // 2] for k in range(K // 2)]
        k0 = prod.index(min(prod))
        k1 = k0 + K // 2
        kl = k0 if ext[k0] >= ext[k1] else k1
        out["rect_k"] = k0
        out["rect_long_px"], out["rect_short_px"] = max(ext[k0], ext[k1]) / Q14, min(ext[k0], ext[k1]) / Q14
        out["rect_angle_deg"], out["rect_area_px2"] = 180.0 * kl / K, prod[k0] / (Q14 * Q14)
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
        for c in LENGTHS:
            out[c + "_mm"] = out[c + "_px"] * f
        out["area_mm2"], out["rect_area_mm2"] = n * (f * f), out["rect_area_px2"] * (f * f)
    if axis_deg is not None:
        out["direction"] = direction_kind(out["orientation_deg"], out["elongation"], float(axis_deg), axis_tol_deg, min_elongation)
    return out


def shape(M, K=180, **kw) -> dict:
    """everything about one crop: sums, parts [2], labels, pminmax, ext, and the columns of ``derive``"""
    M = np.asarray(M)
    dirs = directions(K)
    s = sums(M)
    labels, n_parts, largest = parts(M)
    assert n_parts - euler8(s) == holes_direct(M)
    pm = extents(M, dirs)
    out = {"sums": s, "parts": np.array([n_parts, largest], np.int64), "labels": labels, "pminmax": pm, "ext": ext_of(pm, dirs)}
    out.update(derive(s, out["parts"], pm, dirs, **kw))
    return out


# ---- the crops with known answers (K = 180): name -> (n, (Q1, Q2, Q3, Q4, QD), euler8, edges, (parts, largest, holes),
# (ext[0], ext[90]), (k*, ext[k*], ext[k* + 90]) or None where the table does not print them, orientation)
def bar30():
    yy, xx = np.mgrid[:120, :160]
    c, s = math.cos(math.radians(30.0)), math.sin(math.radians(30.0))
    u, v = (xx - 80) * c + (yy - 60) * s, -(xx - 80) * s + (yy - 60) * c
    return ((np.abs(u) <= 60) & (np.abs(v) <= 10)).astype(np.uint8)


def two_parts():
    M = np.zeros((5, 9), np.uint8)
    M[1:4, 1:4] = 1
    M[2, 2] = 0
    M[0, 6:9] = 1
    return M


def ring3():
    M = np.ones((3, 3), np.uint8)
    M[1, 1] = 0
    return M


def extra_crops():
    yy, xx = np.mgrid[:4, :4]
    return {"ring3": ring3(), "checker4": ((yy + xx) % 2 == 0).astype(np.uint8), "bar30": bar30(), "two_parts": two_parts(),
            "zeros3x5": np.zeros((3, 5), np.uint8)}


def known_shapes():
    return {
        "1x1": (1, (4, 0, 0, 0, 0), 1, 4, (1, 1, 0), (16384, 16384), (0, 16384, 16384), 0.0),
        "2x2": (4, (4, 4, 0, 1, 0), 1, 8, (1, 4, 0), (32768, 32768), (0, 32768, 32768), 0.0),
        "1x9": (9, (4, 16, 0, 0, 0), 1, 20, (1, 9, 0), (147456, 16384), (0, 147456, 16384), 0.0),
        "eye9": (9, (20, 0, 0, 0, 8), 1, 36, (1, 9, 0), (147456, 147456), (45, 208530, 23170), 45.0),
        "70x300": (21000, (4, 736, 0, 20631, 0), 1, 740, (1, 21000, 0), (4915200, 1146880), None, 0.0),
        "sinusoid": (1199, (181, 230, 177, 906, 0), 1, 588, (1, 1199, 0), (3276800, 589824), (5, 3310096, 443150), 3.6565),
        "ellipse": (7513, (96, 248, 92, 7296, 0), 1, 436, (1, 7513, 0), (2605056, 966656), None, 0.0),
        "noise": (1705, (496, 682, 968, 359, 310), -273, 2766, (2, 1692, 275), (1146880, 655360), None, 179.319),
        "ring3": (8, (4, 8, 4, 0, 0), 0, 16, (1, 8, 1), (49152, 49152), None, 0.0),
        "checker4": (8, (14, 0, 0, 0, 9), -1, 32, (1, 8, 2), (65536, 65536), None, 45.0),
        "bar30": (2401, (140, 104, 136, 2212, 0), 1, 380, (1, 2401, 0), (1851392, 1261568), (30, 1988381, 350061), 30.0043),
        "two_parts": (11, (8, 12, 4, 0, 0), 1, 24, (2, 8, 1), (131072, 65536), (79, 58080, 141168), 158.809),
        "zeros3x5": (0, (0, 0, 0, 0, 0), 0, 0, (0, 0, 0), (0, 0), None, 0.0),
    }


BAR30_RECTS = {4: (1, 1992620, 834120), 36: (6, 1988381, 350061), 360: (60, 1988381, 350061)}

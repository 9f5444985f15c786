"""The definition of the skeleton graph (dis-yolo_amd/measure.py ``skeleton_graph``, csrc/skeleton.hip), in plain numpy.

The reference project has nothing of this kind, so these functions ARE the semantics.  Everything here is an integer and the HIP
path equals it exactly; floats appear only in ``derive_rows``, which the host computes from the integers in float64.

A crop is a pair (S, D): S a 0/1 map (the skeleton bytes of ``measure_ref.thin``, or any map; non-zero = set), D the ``d2`` map
of the same crop.  Everything outside the crop is 0.  Neighbours are numbered as in measure_ref: P2..P9 = N, NE, E, SE, S, SW,
W, NW, and bit k of a links byte stands for P(2+k).

  links(S)     uint8: two S pixels are linked when they are adjacent in a row or a column, or diagonal neighbours of which
               neither of the two pixels completing their 2x2 square is in S (the pairs measure_ref.counts calls n_orth and
               n_diag).  Bit k is set when the pixel is linked to P(2+k); 0 off the skeleton.  deg = popcount(links).
  J, P         the S pixels with deg >= 3 (junction pixels) and with deg <= 2.
  labels(S)    int32: a branch is a connected component of P under the links between two P pixels; its label is the smallest
               linear index y bw + x of its pixels.  -1 everywhere else in the crop.
  rows(S, D, M2)  (table int64 [n_branches, len(ROW_COLS)] sorted by root, crop int64 [4] = CROP_COLS):
               px; n_orth, n_diag = the links between two of the branch's pixels counted once plus its links to J pixels;
               n_end = its pixels with deg 1 plus twice those with deg 0; n_attach = its links to J pixels;
               sum_q8 = the sum over its pixels of isqrt(65536 d2), the half-width in 1/256 px; max_d2, min_d2; spur.
               crop: junction_px, jj_orth, jj_diag (the links between two J pixels, which belong to no branch), n_branches.
  is_spur      n_end = 1, n_attach = 1 and length_px < min_branch_px, decided in integers: with M2 = 2 min_branch_px and
               t2 = M2 - 2 n_orth - n_end, a spur iff t2 > 0 and 8 n_diag^2 < t2^2.
  graph(S, D, min_branch_px, max_rounds)  for n = 1, 2, ...: analyse S; stop when no row is a spur or n > max_rounds; otherwise
               delete the pixels of every spur at once (junction pixels stay) and go round again.  The returned table always
               describes the returned skeleton.

What the pruning rule does:
  * the short end piece of a crack beyond its last spur is itself a spur and goes with it: below min_branch_px lost per end;
  * a star whose arms are all short is pruned to its junction pixel;
  * a plain T with arms 10.5 / 10.5 / 9.5 loses the 9.5 arm at min_branch_px = 10.
"""
import math

import numpy as np

import measure_ref as MR

ROW_COLS = ("root", "px", "n_orth", "n_diag", "n_end", "n_attach", "sum_q8", "max_d2", "min_d2", "spur")
CROP_COLS = ("junction_px", "jj_orth", "jj_diag", "n_branches")
OFFSETS = ((-1, 0), (-1, 1), (0, 1), (1, 1), (1, 0), (1, -1), (0, -1), (-1, -1))       # P2 .. P9 as (dy, dx)
MAX_BRANCH_PX = 32767


def check_min_branch(min_branch_px) -> int:
    """-> M2 = 2 min_branch_px; ValueError unless min_branch_px is a multiple of 0.5 in 0 .. 32767"""
    v = float(min_branch_px)
    if not (v == v and 0.0 <= v <= MAX_BRANCH_PX and 2.0 * v == math.floor(2.0 * v)):
        raise ValueError("min_branch_px must be a multiple of 0.5 in 0 .. %d (got %r)" % (MAX_BRANCH_PX, min_branch_px))
    return int(2.0 * v)


def links(S) -> np.ndarray:
    s = np.asarray(S) != 0
    if s.size == 0:
        return np.zeros(s.shape, np.uint8)
    N, NE, E, SE, So, SW, W, NW = MR._neighbours(s)
    linked = (N, NE & ~N & ~E, E, SE & ~E & ~So, So, SW & ~So & ~W, W, NW & ~N & ~W)
    out = np.zeros(s.shape, np.uint8)
    for k, q in enumerate(linked):
        out |= (s & q).astype(np.uint8) << k
    return out


def degree(Lk) -> np.ndarray:
    return np.unpackbits(np.asarray(Lk, np.uint8)[..., None], axis=-1).sum(-1).astype(np.int32)


def labels(S, Lk=None) -> np.ndarray:
    """union-find over the P-P links; the label of a set is its smallest linear index"""
    s = np.asarray(S) != 0
    Lk = links(s) if Lk is None else np.asarray(Lk)
    bh, bw = s.shape
    isP = s & (degree(Lk) <= 2)
    parent = {int(i): int(i) for i in np.flatnonzero(isP.reshape(-1))}

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    for p in list(parent):
        y, x = divmod(p, bw)
        for k in (2, 3, 4, 5):                                                # each pair once, from its upper / left pixel
            if Lk[y, x] >> k & 1:
                q = (y + OFFSETS[k][0]) * bw + x + OFFSETS[k][1]
                if q in parent:
                    a, b = find(p), find(q)
                    if a != b:
                        parent[max(a, b)] = min(a, b)
    out = np.full((bh, bw), -1, np.int32)
    for p in parent:
        out[p // bw, p % bw] = find(p)
    return out


def is_spur(n_orth, n_diag, n_end, n_attach, M2) -> bool:
    t2 = int(M2) - 2 * int(n_orth) - int(n_end)
    return int(n_end) == 1 and int(n_attach) == 1 and t2 > 0 and 8 * int(n_diag) ** 2 < t2 * t2


def rows(S, D, M2=0, Lk=None, Lb=None):
    s = np.asarray(S) != 0
    D = np.asarray(D)
    Lk = links(s) if Lk is None else np.asarray(Lk)
    Lb = labels(s, Lk) if Lb is None else np.asarray(Lb)
    bh, bw = s.shape
    deg = degree(Lk)
    isJ = s & (deg >= 3)
    crop = np.zeros(4, np.int64)
    table = {}
    for y, x in zip(*np.nonzero(s)):
        lk = int(Lk[y, x])
        if isJ[y, x]:
            crop[0] += 1
            for k in (2, 3, 4, 5):
                if lk >> k & 1 and isJ[y + OFFSETS[k][0], x + OFFSETS[k][1]]:
                    crop[1 + (k & 1)] += 1
            continue
        r = table.setdefault(int(Lb[y, x]), dict(px=0, n_orth=0, n_diag=0, n_end=0, n_attach=0, sum_q8=0, max_d2=0,
                                                  min_d2=2 ** 31 - 1))
        d = int(D[y, x])
        r["px"] += 1
        r["n_end"] += 1 if deg[y, x] == 1 else 2 if deg[y, x] == 0 else 0
        r["sum_q8"] += math.isqrt(65536 * d)
        r["max_d2"], r["min_d2"] = max(r["max_d2"], d), min(r["min_d2"], d)
        for k in range(8):
            if lk >> k & 1:
                toJ = bool(isJ[y + OFFSETS[k][0], x + OFFSETS[k][1]])
                if toJ or k in (2, 3, 4, 5):
                    r["n_diag" if k & 1 else "n_orth"] += 1
                r["n_attach"] += toJ
    out = np.zeros((len(table), len(ROW_COLS)), np.int64)
    for i, root in enumerate(sorted(table)):
        r = table[root]
        out[i] = [root] + [r[c] for c in ROW_COLS[1:-1]] + [is_spur(r["n_orth"], r["n_diag"], r["n_end"], r["n_attach"], M2)]
    crop[3] = len(table)
    return out, crop


def graph(S, D, min_branch_px=0.0, max_rounds=8):
    """-> dict: skeleton uint8, links, labels, rows, crop, analyses, converged"""
    M2 = check_min_branch(min_branch_px)
    S = (np.asarray(S) != 0).astype(np.uint8)
    n = 0
    while True:
        n += 1
        Lk = links(S)
        Lb = labels(S, Lk)
        table, crop = rows(S, D, M2, Lk, Lb)
        spurs = table[table[:, -1] != 0, 0]
        if spurs.size == 0 or n > max_rounds:
            return {"skeleton": S, "links": Lk, "labels": Lb, "rows": table, "crop": crop, "analyses": n,
                    "converged": spurs.size == 0}
        S = np.where(np.isin(Lb, spurs), 0, S).astype(np.uint8)


def kind(n_end, n_attach) -> str:
    if n_attach == 0:
        return "loop" if n_end == 0 else "free"
    return "terminal" if n_end >= 1 else "inner"


def derive_rows(table):
    """rows int64 [n, len(ROW_COLS)] -> (length_px, mean_width_px, max_width_px, min_width_px float64 [n], kinds list)"""
    t = np.asarray(table, np.int64).reshape(-1, len(ROW_COLS))
    c = {name: t[:, i] for i, name in enumerate(ROW_COLS)}
    length = c["n_orth"] + np.sqrt(2.0) * c["n_diag"] + c["n_end"] / 2.0
    wmean = 2.0 * (c["sum_q8"] / 256.0) / c["px"] - 1.0
    wmax = 2.0 * np.sqrt(c["max_d2"].astype(np.float64)) - 1.0
    wmin = 2.0 * np.sqrt(c["min_d2"].astype(np.float64)) - 1.0
    return length, wmean, wmax, wmin, [kind(int(e), int(a)) for e, a in zip(c["n_end"], c["n_attach"])]


def extra_crops():
    """the crops of the issue's table that measure_ref.known_crops does not hold: name -> mask"""
    t3 = np.zeros((30, 61), np.uint8)
    t3[8:11, :] = 1
    t3[8:30, 29:32] = 1
    t3[4:8, 14:17] = 1
    yy, xx = np.mgrid[:80, :240]
    r2 = (yy - 40) ** 2 + (xx - 60) ** 2
    ring_tail = (((24 ** 2 < r2) & (r2 < 30 ** 2)) | ((np.abs(yy - 40) < 2) & (88 < xx) & (xx < 140))).astype(np.uint8)
    serp = np.zeros((41, 300), np.uint8)
    serp[0::2, :] = 1
    serp[1::4, 299] = 1
    serp[3::4, 0] = 1
    plus9 = np.zeros((9, 9), np.uint8)
    plus9[4, :] = 1
    plus9[:, 4] = 1
    return {"T3spur": t3, "ring_tail": ring_tail, "serp": serp, "plus9": plus9}

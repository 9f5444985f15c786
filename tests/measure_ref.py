"""The definition of instance measurement (dis-yolo_amd/measure.py, csrc/measure.hip), in plain numpy.

The reference project has nothing of this kind, so these functions ARE the semantics; the HIP path agrees with them exactly,
apart from the one float64 sum ``sum_sqrt`` (a sum of n positive doubles in another order: relative (n + 2) 2^-52).

A crop M is a 2-D array; a non-zero element is foreground, everything outside the crop is background.

  d2(M)        int32: for a foreground pixel the minimum over background pixels q of |p - q|^2, the pixels of a one-pixel ring
               around the crop counting as background; 0 on background.  The exact Euclidean transform, in integers.
  thin(M)      (S, iterations): Zhang-Suen thinning.  Neighbours P2..P9 clockwise from north (P2 = N, P3 = NE, P4 = E, P5 = SE,
               P6 = S, P7 = SW, P8 = W, P9 = NW), zero outside the crop; B = the non-zero neighbours, A = the 0 -> 1 steps in the
               cycle P2, P3, ..., P9, P2.  An iteration is sub-step 1 then sub-step 2; each decides for all pixels from the state
               at its start and deletes the foreground pixels with 2 <= B <= 6, A = 1 and
                 sub-step 1: P2 P4 P6 = 0 and P4 P6 P8 = 0        sub-step 2: P2 P4 P8 = 0 and P2 P6 P8 = 0.
               S is the state after the first iteration that deletes nothing; ``iterations`` counts that one too (an empty
               crop takes none).  The count is NOT bounded by ceil(sqrt(max d2)) + 1: convergence has to be observed.
  counts(M)    int64 [8] = area |M|, skel_px |S|, n_orth (pairs of S pixels adjacent along a row or a column), n_diag (diagonal
               pairs of S pixels of which neither of the two pixels completing the 2x2 square is in S), n_end (S pixels with
               exactly one 8-neighbour in S, plus twice those with none), max_d2 (over M), max_d2_skel (over S), 0.
  sum_sqrt(M)  float64: the sum over S of sqrt(d2).
  derive(counts, sum_sqrt)  float64: length_px = n_orth + sqrt(2) n_diag + n_end / 2, max_width_px = 2 sqrt(max_d2) - 1,
               mean_width_px = 2 sum_sqrt / skel_px - 1; with skel_px = 0 the length is 0 and the mean width the maximum width;
               with area = 0 everything is 0.

Known properties of Zhang-Suen thinning, which the derived numbers inherit:
  * it deletes a 2x2 square completely (skel_px = 0: such an instance has a width and no length);
  * it deletes 2-pixel-wide diagonal strokes;
  * it keeps ONE row of an even-width bar, so the mean width of an even-width stroke reads one pixel low;
  * it shortens a bar of width w by about w (the skeleton of a 3 x 9 bar is 6 pixels long: n_end / 2 gives one of them back).
"""
import numpy as np

COLS = ("area", "skel_px", "n_orth", "n_diag", "n_end", "max_d2", "max_d2_skel", "zero")


def d2(M) -> np.ndarray:
    """the separable exact form: g = the distance within the column to the nearest zero (rows -1 and bh are zeros), then
    D2(y, x) = min over x' in -1 .. bw of (x - x')^2 + g(y, x')^2 with g = 0 at the two virtual columns"""
    M = np.asarray(M) != 0
    bh, bw = M.shape
    if bh == 0 or bw == 0:
        return np.zeros((bh, bw), np.int32)
    g = np.zeros((bh, bw + 2), np.int64)
    run = np.zeros(bw, np.int64)
    for y in range(bh):
        run = np.where(M[y], run + 1, 0)
        g[y, 1:-1] = run
    run = np.zeros(bw, np.int64)
    for y in range(bh - 1, -1, -1):
        run = np.where(M[y], run + 1, 0)
        g[y, 1:-1] = np.minimum(g[y, 1:-1], run)
    x = np.arange(bw + 2, dtype=np.int64)
    dx2 = (x[1:-1, None] - x[None, :]) ** 2                                   # [bw, bw + 2]
    out = np.empty((bh, bw), np.int64)
    for y in range(bh):
        out[y] = (dx2 + g[y][None, :] ** 2).min(axis=1)
    return np.where(M, out, 0).astype(np.int32)


def d2_brute(M) -> np.ndarray:
    """the definition itself, pixel against pixel (small crops only)"""
    M = np.asarray(M) != 0
    P = np.pad(M, 1)
    by, bx = np.nonzero(~P)
    out = np.zeros(M.shape, np.int32)
    for y, x in zip(*np.nonzero(M)):
        out[y, x] = ((by - (y + 1)) ** 2 + (bx - (x + 1)) ** 2).min()
    return out


def _neighbours(S):
    P = np.pad(S, 1)
    h, w = S.shape
    sl = lambda dy, dx: P[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
    # P2 .. P9: N, NE, E, SE, S, SW, W, NW
    return [sl(-1, 0), sl(-1, 1), sl(0, 1), sl(1, 1), sl(1, 0), sl(1, -1), sl(0, -1), sl(-1, -1)]


def thin(M):
    S = (np.asarray(M) != 0).astype(np.uint8)
    if S.size == 0:
        return S, 0
    it = 0
    while True:
        it += 1
        deleted = False
        for step in (1, 2):
            p = [q.astype(np.int32) for q in _neighbours(S)]
            B = sum(p)
            A = sum(((p[k] == 0) & (p[(k + 1) % 8] == 1)).astype(np.int32) for k in range(8))
            P2, P4, P6, P8 = p[0], p[2], p[4], p[6]
            if step == 1:
                c = (P2 * P4 * P6 == 0) & (P4 * P6 * P8 == 0)
            else:
                c = (P2 * P4 * P8 == 0) & (P2 * P6 * P8 == 0)
            kill = (S == 1) & (B >= 2) & (B <= 6) & (A == 1) & c
            if kill.any():
                deleted = True
                S = np.where(kill, 0, S).astype(np.uint8)
        if not deleted:
            return S, it


def counts(M, S=None, D=None) -> np.ndarray:
    M = np.asarray(M) != 0
    S = thin(M)[0] if S is None else np.asarray(S)
    D = d2(M) if D is None else np.asarray(D)
    s = S != 0
    out = np.zeros(8, np.int64)
    out[0], out[1] = M.sum(), s.sum()
    if M.size == 0:
        return out
    N, NE, E, SE, So, SW, W, NW = _neighbours(s)
    out[2] = (s & E).sum() + (s & So).sum()
    out[3] = (s & SE & ~E & ~So).sum() + (s & SW & ~W & ~So).sum()
    nb = sum(q.astype(np.int32) for q in (N, NE, E, SE, So, SW, W, NW))
    out[4] = (s & (nb == 1)).sum() + 2 * (s & (nb == 0)).sum()
    out[5] = D[M].max() if M.any() else 0
    out[6] = D[s].max() if s.any() else 0
    return out


def sum_sqrt(S, D) -> float:
    s = np.asarray(S) != 0
    return float(np.sqrt(np.asarray(D)[s].astype(np.float64)).sum())


def measure(M):
    """everything about one crop: dict with d2, skeleton, iterations, counts int64 [8], sum_sqrt"""
    D = d2(M)
    S, it = thin(M)
    return {"d2": D, "skeleton": S, "iterations": it, "counts": counts(M, S, D), "sum_sqrt": sum_sqrt(S, D)}


def derive(cnt, ssq):
    """counts int64 [G,8], sum_sqrt float64 [G] -> (length_px, max_width_px, mean_width_px), float64 [G]"""
    cnt = np.asarray(cnt, np.int64).reshape(-1, 8)
    ssq = np.asarray(ssq, np.float64).reshape(-1)
    area, skel = cnt[:, 0], cnt[:, 1]
    length = cnt[:, 2] + np.sqrt(2.0) * cnt[:, 3] + cnt[:, 4] / 2.0
    wmax = 2.0 * np.sqrt(cnt[:, 5].astype(np.float64)) - 1.0
    wmean = 2.0 * ssq / np.maximum(skel, 1) - 1.0
    length = np.where(skel > 0, length, 0.0)
    wmean = np.where(skel > 0, wmean, wmax)
    zero = area == 0
    return np.where(zero, 0.0, length), np.where(zero, 0.0, wmax), np.where(zero, 0.0, wmean)


# ---- the crops with known answers (the issue's table): name -> (crop, area, skel_px, n_orth, n_diag, n_end, max_d2, sum_sqrt,
# iterations)
def known_crops():
    yy, xx = np.mgrid[:64, :200]
    return {
        "1x1": (np.ones((1, 1), np.uint8), 1, 1, 0, 0, 2, 1, 1.0, 1),
        "2x2": (np.ones((2, 2), np.uint8), 4, 0, 0, 0, 0, 1, 0.0, 2),
        "1x9": (np.ones((1, 9), np.uint8), 9, 9, 8, 0, 2, 1, 9.0, 1),
        "eye9": (np.eye(9, dtype=np.uint8), 9, 9, 0, 8, 2, 1, 9.0, 1),
        "3x9": (np.ones((3, 9), np.uint8), 27, 6, 5, 0, 2, 4, 12.0, 2),
        "5x17": (np.ones((5, 17), np.uint8), 85, 12, 11, 0, 2, 9, 36.0, 3),
        "17x33": (np.ones((17, 33), np.uint8), 561, 16, 15, 0, 2, 81, 144.0, 9),
        "70x300": (np.ones((70, 300), np.uint8), 21000, 230, 229, 0, 2, 1225, 8050.0, 36),
        "sinusoid": ((np.abs(yy - (20 + 10 * np.sin(xx / 15) + 0.1 * xx)) < 3).astype(np.uint8), 1199, 223, 161, 61, None, 9,
                     None, 4),
        "ellipse": (((yy - 32) ** 2 / 900 + (xx - 100) ** 2 / 6400 < 1).astype(np.uint8), 7513, 119, 118, 0, None, 900, None, 29),
        "noise": ((np.random.default_rng(0).random((40, 70)) < 0.6).astype(np.uint8), 1705, 1415, 1434, 327, None, 5, None, 3),
    }


# the skeleton rows the table prints: name -> (row, first column, last column)
KNOWN_SKELETON_ROWS = {"3x9": (1, 1, 6), "5x17": (2, 2, 13), "17x33": (8, 8, 23)}

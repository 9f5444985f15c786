"""The definition of the traced skeleton graph (dis-yolo_amd/measure.py ``skeleton_trace``, csrc/trace.hip), in plain numpy.

The reference project has nothing of this kind, so these functions ARE the semantics.  Everything here is an integer and the HIP
path equals it exactly; floats appear only in ``derive_trunk``, which the host computes from the integers in float64.  It goes on
from skeleton_ref: S is a 0/1 map (the pruned skeleton ``skeleton_graph`` returned), D the ``d2`` map of the same crop, and
``links`` / ``labels`` / ``rows`` are skeleton_ref's.  A pixel's linear index is y bw + x; J pixels have deg >= 3, P pixels less.

  nodes        a node is a connected component of J under the links between two J pixels, named by its smallest linear index.
               node_labels int32, -1 off J; one row per node (NODE_COLS): root, px, sum_y, sum_x, max_d2, n_attach (the links
               from its pixels to P pixels).
  shape        P pixels have deg <= 2, so a branch is a simple path (two end pixels with fewer than two in-branch links, or one
               pixel) or a closed loop (every pixel two in-branch links, no attachment).  An end pixel of a path of two or more
               pixels has at most one link to a J pixel, a single pixel at most two.  ``order`` asserts all of it.
  order        start of a path = its end pixel with the smaller linear index; start of a loop = its root, walked first to the
               linked neighbour with the smaller linear index.  rank int32 = steps from start (-1 off P), rank_diag int32 = how
               many of them were diagonal links (-1 off P).
  edges        one row per branch (EDGE_COLS): root, end0_kind, end0_id, end1_kind, end1_id, attach0_px, attach1_px.  End 0 is at
               rank 0, end 1 at rank px - 1.  kind 1: a node, id = its root, attach = the J pixel linked to; kind 0: a free
               end, id = the end pixel, attach = -1; kind 2: a loop, both ends, id = the root, attach = -1.  A single pixel hands
               its attachments out in ascending link bit, end 0 first; an end that gets none is free.
  trunk        vertices = nodes and free ends (an isolated pixel gives two), ordered by (pixel id, kind, end); edges = branches
               that are neither loops nor attached to one node at both ends, weight 1024 n_orth + 1448 n_diag + 512 n_end.  The
               trunk joins the pair of vertices whose shortest-path distance is largest.  Ties by procedure: Dijkstra from every
               vertex u in order, the heap popped by (distance, vertex order), a vertex's edges relaxed in ascending branch
               root, a predecessor replaced only on a strictly smaller distance, the best pair (u, v; v in vertex order)
               replaced only on a strictly larger distance.  No such edge at all: the heaviest loop (the smallest root on a tie),
               walked in rank order; no loop either: empty, every number 0.
  profile      the trunk's branches in order, each in rank order or reversed when entered at end 1, and between two
               consecutive branches the J pixels they attach to (once if it is one pixel).  Per entry (y, x, d2, cum_orth,
               cum_diag) int32.  Steps inside a branch and onto an attach pixel are the links; the step between two attach
               pixels of one node is octile: min(|dy|, |dx|) diagonal and max - min orthogonal steps.
  trunk row    TRUNK_COLS: n_branches; px = profile entries; n_orth, n_diag = those of its branches' rows plus the crossings;
               n_end = those of its branches' rows; sum_q8 = sum of isqrt(65536 d2) over the profile; max_d2 with the profile
               position, y and x of its first occurrence; weight = the sum of its branches' weights (crossings cost nothing).

What the rule does: a ring with a tail has the tail as its trunk (a branch from a node back to itself is
never on a shortest path); of two arms between the same two nodes the shorter is taken; a crossing through a thick junction is
measured straight.
"""
import heapq
import math

import numpy as np

import skeleton_ref as SR

NODE_COLS = ("root", "px", "sum_y", "sum_x", "max_d2", "n_attach")
EDGE_COLS = ("root", "end0_kind", "end0_id", "end1_kind", "end1_id", "attach0_px", "attach1_px")
TRUNK_COLS = ("n_branches", "px", "n_orth", "n_diag", "n_end", "sum_q8", "max_d2", "max_pos", "max_y", "max_x", "weight")
PROFILE_COLS = ("y", "x", "d2", "cum_orth", "cum_diag")
W_ORTH, W_DIAG, W_END = 1024, 1448, 512
C = {name: i for i, name in enumerate(SR.ROW_COLS)}


def weight(row) -> int:
    return W_ORTH * int(row[C["n_orth"]]) + W_DIAG * int(row[C["n_diag"]]) + W_END * int(row[C["n_end"]])


def _neighbours(Lk, p, bw):
    """the linked neighbours of pixel p in ascending link bit: [(k, q)]"""
    lk = int(Lk[p // bw, p % bw])
    return [(k, p + SR.OFFSETS[k][0] * bw + SR.OFFSETS[k][1]) for k in range(8) if lk >> k & 1]


def nodes(S, D, Lk=None):
    """-> (node_labels int32, table int64 [n, len(NODE_COLS)] sorted by root)"""
    s = np.asarray(S) != 0
    D = np.asarray(D)
    Lk = SR.links(s) if Lk is None else np.asarray(Lk)
    bh, bw = s.shape
    isJ = (s & (SR.degree(Lk) >= 3)).reshape(-1)
    parent = {int(i): int(i) for i in np.flatnonzero(isJ)}

    def find(a):
        while parent[a] != a:
            a = parent[a]
        return a

    for p in parent:
        for k, q in _neighbours(Lk, p, bw):
            if q in parent:
                a, b = find(p), find(q)
                if a != b:
                    parent[max(a, b)] = min(a, b)
    out = np.full(bh * bw, -1, np.int32)
    table = {}
    for p in parent:
        r = find(p)
        out[p] = r
        row = table.setdefault(r, [r, 0, 0, 0, 0, 0])
        row[1] += 1
        row[2] += p // bw
        row[3] += p % bw
        row[4] = max(row[4], int(D[p // bw, p % bw]))
        row[5] += sum(1 for _, q in _neighbours(Lk, p, bw) if not isJ[q])
    return out.reshape(bh, bw), np.array([table[r] for r in sorted(table)], np.int64).reshape(-1, len(NODE_COLS))


def order(S, Lk=None, Lb=None, node_labels=None):
    """-> (rank int32, rank_diag int32, edges int64 [n_branches, len(EDGE_COLS)] sorted by root, walks {root: [pixels in rank
    order]}); asserts the shape of every branch"""
    s = np.asarray(S) != 0
    Lk = SR.links(s) if Lk is None else np.asarray(Lk)
    Lb = SR.labels(s, Lk) if Lb is None else np.asarray(Lb)
    if node_labels is None:
        node_labels = nodes(s, np.zeros(s.shape, np.int32), Lk)[0]
    bh, bw = s.shape
    flat, nl = Lb.reshape(-1), node_labels.reshape(-1)
    members = {}
    for p in np.flatnonzero(flat >= 0):
        members.setdefault(int(flat[p]), []).append(int(p))
    rank = np.full(bh * bw, -1, np.int32)
    rank_diag = np.full(bh * bw, -1, np.int32)
    edges, walks = [], {}
    for root in sorted(members):
        px = members[root]
        inner = {p: [(k, q) for k, q in _neighbours(Lk, p, bw) if flat[q] >= 0] for p in px}
        attach = {p: [(k, q) for k, q in _neighbours(Lk, p, bw) if flat[q] < 0] for p in px}
        assert all(flat[q] == root for p in px for _, q in inner[p])
        ends = [p for p in px if len(inner[p]) < 2]
        loop = not ends
        if loop:
            assert len(px) >= 4 and all(not attach[p] for p in px), "a loop with an attachment"
            start, second = root, min(q for _, q in inner[root])
        else:
            assert len(ends) == (2 if len(px) > 1 else 1), "a branch that is neither a path nor a loop"
            assert all(len(attach[p]) == 0 for p in px if p not in ends)
            assert all(len(attach[p]) <= (1 if len(px) > 1 else 2) for p in ends), "an end with two attachments"
            start = min(ends)
            second = inner[start][0][1] if inner[start] else None
        walk, diag, before, here, nd = [start], [0], None, start, 0
        nxt = second
        while nxt is not None and nxt != start:
            k = next(k for k, q in inner[here] if q == nxt)
            nd += k & 1
            before, here = here, nxt
            walk.append(here)
            diag.append(nd)
            nxt = next((q for _, q in inner[here] if q != before), None)
        assert sorted(walk) == sorted(px), "the walk misses pixels of its branch"
        rank[walk] = np.arange(len(walk))
        rank_diag[walk] = diag
        walks[root] = walk
        if loop:
            edges.append([root, 2, root, 2, root, -1, -1])
            continue
        if len(px) == 1:
            slots = [q for _, q in attach[start]] + [None, None]
            e = [(1, int(nl[q]), q) if q is not None else (0, start, -1) for q in slots[:2]]
        else:
            e = []
            for p in (walk[0], walk[-1]):
                e.append((1, int(nl[attach[p][0][1]]), attach[p][0][1]) if attach[p] else (0, p, -1))
        edges.append([root, e[0][0], e[0][1], e[1][0], e[1][1], e[0][2], e[1][2]])
    shape = (bh, bw)
    return rank.reshape(shape), rank_diag.reshape(shape), np.array(edges, np.int64).reshape(-1, len(EDGE_COLS)), walks


def vertices_and_edges(rows, edges):
    """-> (vertices: sorted list of (id, kind, end), graph edges: [(root, weight, vertex index at end 0, at end 1)] by root)"""
    verts, ge = set(), []
    for row, e in zip(rows, edges):
        assert row[0] == e[0]
        if e[1] == 2 or (e[1] == 1 and e[3] == 1 and e[2] == e[4]):
            continue
        both_free_on_one_pixel = e[1] == 0 and e[3] == 0 and e[2] == e[4]
        ge.append((int(e[0]), weight(row), (int(e[2]), int(e[1]), 0), (int(e[4]), int(e[3]), 1 if both_free_on_one_pixel else 0)))
        verts.update(ge[-1][2:])
    verts = sorted(verts)
    at = {v: i for i, v in enumerate(verts)}
    return verts, [(r, w, at[a], at[b]) for r, w, a, b in ge]


def select_trunk(rows, edges):
    """rows (skeleton_ref.rows' table) and edges of one crop, both sorted by root -> (path [(root, reversed)], distance, u, v):
    u, v = (id, kind, end) of the two ends, None for a loop or an empty trunk"""
    verts, ge = vertices_and_edges(rows, edges)
    adj = [[] for _ in verts]
    for r, w, a, b in ge:                      # (ge is in ascending root: so is every adjacency list)
        adj[a].append((r, w, b, False))
        adj[b].append((r, w, a, True))
    best = (0, None, None, None)
    for u in range(len(verts)):
        dist, pred, done = {u: 0}, {}, set()
        heap = [(0, u)]
        while heap:
            d, a = heapq.heappop(heap)
            if a in done:
                continue
            done.add(a)
            for r, w, b, rev in adj[a]:
                if b not in dist or d + w < dist[b]:
                    dist[b], pred[b] = d + w, (a, r, rev)
                    heapq.heappush(heap, (d + w, b))
        for v in sorted(dist):
            if dist[v] > best[0]:
                best = (dist[v], u, v, pred)
    if best[1] is not None:
        d, u, v, pred = best
        path, a = [], v
        while a != u:
            a, r, rev = pred[a]
            path.append((r, rev))
        return path[::-1], d, verts[u], verts[v]
    loops = [(-weight(row), int(row[0])) for row, e in zip(rows, edges) if e[1] == 2]
    if loops:
        w, r = min(loops)
        return [(r, False)], -w, None, None
    return [], 0, None, None


def trunk_profile(path, D, rows, edges, walks, rank_diag):
    """-> (profile int32 [n, 5], trunk row int64 [len(TRUNK_COLS)])"""
    D = np.asarray(D)
    bw = D.shape[1]
    by_root = {int(r[0]): (r, e) for r, e in zip(rows, edges)}
    rd = rank_diag.reshape(-1)
    prof, pos, co, cd = [], None, 0, 0

    def step_to(q):
        nonlocal pos, co, cd
        if pos is not None:
            dy, dx = abs(q // bw - pos // bw), abs(q % bw - pos % bw)
            co, cd = co + max(dy, dx) - min(dy, dx), cd + min(dy, dx)
        pos = q
        prof.append([q // bw, q % bw, int(D[q // bw, q % bw]), co, cd])

    n_orth = n_diag = n_end = w = 0
    cross_o = cross_d = 0
    leave = None                                       # the attach pixel the branch before left through
    for root, rev in path:
        row, e = by_root[root]
        enter, out = (e[6], e[5]) if rev else (e[5], e[6])
        if leave is not None:
            assert leave >= 0 and enter >= 0
            step_to(int(leave))
            if enter != leave:
                dy, dx = abs(enter // bw - leave // bw), abs(enter % bw - leave % bw)
                cross_o, cross_d = cross_o + max(dy, dx) - min(dy, dx), cross_d + min(dy, dx)
                step_to(int(enter))
        walk = walks[root][::-1] if rev else walks[root]
        for q in walk:                         # (a link is one step: the octile distance of two neighbours)
            step_to(q)
        assert rd[walks[root][-1]] == sum(1 for a, b in zip(walks[root], walks[root][1:]) if (a // bw != b // bw) and (a % bw != b % bw))
        n_orth, n_diag, n_end, w = n_orth + int(row[C["n_orth"]]), n_diag + int(row[C["n_diag"]]), n_end + int(row[C["n_end"]]), w + weight(row)
        leave = out
    prof = np.array(prof, np.int32).reshape(-1, len(PROFILE_COLS))
    out = np.zeros(len(TRUNK_COLS), np.int64)
    if len(prof):
        at = int(np.argmax(prof[:, 2]))
        out[:] = [len(path), len(prof), n_orth + cross_o, n_diag + cross_d, n_end, sum(math.isqrt(65536 * int(d)) for d in prof[:, 2]),
                  prof[at, 2], at, prof[at, 0], prof[at, 1], w]
    return prof, out


def trace(S, D):
    """-> dict: node_labels, nodes, rank, rank_diag, edges, rows, profiles {root: int32 [px, 4] = y, x, d2, rank_diag}, path, distance,
    u, v, trunk_profile, trunk"""
    S = (np.asarray(S) != 0).astype(np.uint8)
    D = np.asarray(D)
    bw = S.shape[1]
    Lk = SR.links(S)
    Lb = SR.labels(S, Lk)
    rows, _ = SR.rows(S, D, 0, Lk, Lb)
    nl, ntab = nodes(S, D, Lk)
    rank, rank_diag, edges, walks = order(S, Lk, Lb, nl)
    profiles = {}
    for root, walk in walks.items():
        w = np.asarray(walk)
        profiles[root] = np.stack([w // bw, w % bw, D.reshape(-1)[w], rank_diag.reshape(-1)[w]], 1).astype(np.int32)
    path, dist, u, v = select_trunk(rows, edges)
    prof, trow = trunk_profile(path, D, rows, edges, walks, rank_diag)
    return {"node_labels": nl, "nodes": ntab, "rank": rank, "rank_diag": rank_diag, "edges": edges, "rows": rows, "walks": walks,
            "profiles": profiles, "path": path, "distance": dist, "u": u, "v": v, "trunk_profile": prof, "trunk": trow}


def derive_trunk(trow):
    """trunk row -> (trunk_length_px, mean_width_px, max_width_px) float64, as section 4m derives a branch's"""
    t = {name: int(trow[i]) for i, name in enumerate(TRUNK_COLS)}
    if t["px"] == 0:
        return 0.0, 0.0, 0.0
    length = t["n_orth"] + np.sqrt(2.0) * t["n_diag"] + t["n_end"] / 2.0
    return float(length), 2.0 * (t["sum_q8"] / 256.0) / t["px"] - 1.0, 2.0 * float(np.sqrt(np.float64(t["max_d2"]))) - 1.0


def extra_crops():
    """the crops the trace adds to skeleton_ref.extra_crops: name -> map (used as it is: S = the map, no thinning)"""
    diamond = np.array([[0, 1, 0], [1, 0, 1], [0, 1, 0]], np.uint8)
    two_arms = np.zeros((13, 40), np.uint8)            # a ring with a tail at each side: arms of different length between two nodes
    two_arms[6, 0:10] = 1
    two_arms[6, 24:40] = 1
    two_arms[2, 10:24] = 1                             # the upper arm: 4 up, across, 4 down
    two_arms[2:6, 10] = 1
    two_arms[2:6, 23] = 1
    two_arms[6, 10:24] = 1                             # ... and the straight one
    thick = np.zeros((10, 12), np.uint8)               # two strokes one row apart, joined by a node of two J pixels
    thick[4, 0:6] = 1
    thick[5, 5:12] = 1
    thick[1:4, 5] = 1
    thick[6:9, 5] = 1
    return {"diamond": diamond, "two_arms": two_arms, "thick": thick}

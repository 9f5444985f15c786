"""The traced skeleton graph without a GPU: the numpy definition (tests/trace_ref.py) against the known answers, the documented
consequences of the trunk rule, its identities and a brute-force second opinion on the trunk's distance, the host's trunk
selection (``measure.select_trunk``) against the definition's, and the argument checks of csrc/trace.hip and
``measure.skeleton_trace``, which happen before any launch."""
import ctypes

import numpy as np
import pytest

import measure_ref as MR
import skeleton_ref as SR
import trace_ref as TR
from disyolo_amd import lib as L
from disyolo_amd import measure as MZ

CROPS = {n: v[0] for n, v in MR.known_crops().items()}
CROPS.update(SR.extra_crops())
RAW = TR.extra_crops()                       # used as they are: the map is the skeleton
_TRACED = {}
C = TR.C
T = {name: i for i, name in enumerate(TR.TRUNK_COLS)}


def traced(name, mb=0.0):
    """the definition's trace of a known crop's skeleton, pruned at mb (computed once)"""
    if (name, mb) not in _TRACED:
        if name in RAW:
            S, D = RAW[name], MR.d2(RAW[name])
        else:
            m = MR.measure(CROPS[name])
            S, D = SR.graph(m["skeleton"], m["d2"], mb)["skeleton"], m["d2"]
        t = TR.trace(S, D)
        t["S"], t["D"] = S, D
        _TRACED[(name, mb)] = t
    return _TRACED[(name, mb)]


def length(t):
    return TR.derive_trunk(t["trunk"])[0]


def random_maps(n, seed, side=24):
    rng = np.random.default_rng(seed)
    for i in range(n):
        M = (rng.random((side, side)) < rng.uniform(0.3, 0.9)).astype(np.uint8)
        yield (MR.thin(M)[0] if i % 2 == 0 else M), MR.d2(M)          # thinned and raw, as the issue's prototype


# ------------------------------------------------------------------------------------------------ the known answers
def test_single_strokes():
    t = traced("1x1")
    assert t["path"] == [(0, False)] and length(t) == 1.0 and t["trunk"][T["weight"]] == 1024 and t["trunk"][T["px"]] == 1
    assert (t["u"], t["v"]) == ((0, 0, 0), (0, 0, 1))                  # an isolated pixel: two distinct free ends
    t = traced("2x2")
    assert t["path"] == [] and not t["trunk"].any() and t["trunk_profile"].shape == (0, 5) and length(t) == 0.0
    t = traced("1x9")
    assert length(t) == 9.0 and (t["u"][0], t["v"][0]) == (0, 8) and t["trunk_profile"][:, 1].tolist() == list(range(9))
    assert traced("eye9")["trunk"][T["weight"]] == 12608
    t = traced("sinusoid")
    assert t["trunk"][T["weight"]] == 254216 and t["trunk"][T["px"]] == 223
    assert length(traced("70x300")) == 230.0
    t = traced("serp")
    assert len(t["path"]) == 1 and t["trunk"][T["px"]] == 6320 and t["trunk"][T["weight"]] == 6471680
    assert t["rank"].reshape(-1)[0] == 0 and t["rank"].reshape(-1)[12299] == 6319


def test_t3spur_plus9_ring_tail():
    t = traced("T3spur", 0.0)
    assert len(t["path"]) == 3 and len(t["nodes"]) == 2 and (t["u"], t["v"]) == ((550, 0, 0), (607, 0, 0))
    assert t["trunk"][T["weight"]] == 59392 and length(t) == 58.0 and t["distance"] == 59392
    t = traced("T3spur", 10.0)
    assert len(t["path"]) == 2 and (t["u"], t["v"]) == ((550, 0, 0), (607, 0, 0)) and length(t) == 58.0
    t = traced("ring_tail")
    assert t["path"] == [(9688, False)] and (t["u"], t["v"]) == ((9687, 1, 0), (9737, 0, 0)) and length(t) == 50.5
    t = traced("plus9", 0.0)
    lens = SR.derive_rows(t["rows"])[0].tolist()
    assert lens == [4.5] * 4 and (t["u"], t["v"]) == ((4, 0, 0), (36, 0, 0)) and length(t) == 9.0      # the tie of four equal arms
    t = traced("plus9", 10.0)
    assert t["trunk"][T["px"]] == 1 and length(t) == 1.0


def test_noise():
    assert traced("noise", 0.0)["distance"] == 59112 and traced("noise", 10.0)["distance"] == 41704
    t = traced("noise", 0.0)
    assert (t["nodes"][:, 1] > 1).any()                                               # multi-pixel nodes
    single = t["rows"][:, C["px"]] == 1
    assert ((t["edges"][:, 1] == 1) & (t["edges"][:, 3] == 1) & single).any()         # single pixels with two attachments


# ------------------------------------------------------------------------------------------------ the documented consequences
def test_a_ring_with_a_tail_has_the_tail_as_its_trunk():
    t = traced("ring_tail")
    ring = t["edges"][t["edges"][:, 0] != 9688][0]
    assert ring[1] == 1 and ring[3] == 1 and ring[2] == ring[4] == 9687              # from the node back to itself: no edge
    assert [r for r, _ in t["path"]] == [9688]


def test_of_two_arms_between_two_nodes_the_shorter_is_taken():
    t = traced("two_arms")
    e = {int(r[0]): r for r in t["edges"]}
    assert e[90][[1, 2, 3, 4]].tolist() == e[251][[1, 2, 3, 4]].tolist() == [1, 250, 1, 263]
    w = {int(r[0]): TR.weight(r) for r in t["rows"]}
    assert w[251] < w[90] and [r for r, _ in t["path"]] == [240, 251, 264] and length(t) == 40.0


def test_a_crossing_through_a_thick_junction_is_measured_straight():
    t = traced("thick")
    assert t["nodes"].tolist() == [[53, 2, 9, 10, 1, 4]]
    assert t["path"] == [(48, False), (66, False)]
    e = {int(r[0]): r for r in t["edges"]}
    assert e[48][6] == 53 and e[66][5] == 65                                            # two different attach pixels of one node
    prof = t["trunk_profile"]
    assert prof[5, :2].tolist() == [4, 5] and prof[6, :2].tolist() == [5, 5] and len(prof) == 13
    rows = {int(r[0]): r for r in t["rows"]}
    assert t["trunk"][T["n_orth"]] == rows[48][C["n_orth"]] + rows[66][C["n_orth"]] + 1 and length(t) == 13.0
    assert t["trunk"][T["weight"]] == 12288                                              # the selection ignores the crossing


def test_the_diamond_is_the_smallest_loop():
    t = traced("diamond")
    assert t["edges"].tolist() == [[1, 2, 1, 2, 1, -1, -1]] and t["path"] == [(1, False)] and t["u"] is None
    assert t["walks"][1] == [1, 3, 7, 5] and t["rank_diag"].reshape(-1)[[1, 3, 7, 5]].tolist() == [0, 1, 2, 3]
    assert t["trunk"][T["weight"]] == 4 * 1448 and t["trunk"][T["n_diag"]] == 4


# ------------------------------------------------------------------------------------------------ identities
def check_identities(S, D):
    t = TR.trace(S, D)
    bw = S.shape[1]
    Lk = SR.links(S)
    rows, crop = t["rows"], SR.rows(S, D)[1]
    rank, rd = t["rank"].reshape(-1), t["rank_diag"].reshape(-1)
    assert ((rank >= 0) == (SR.labels(S).reshape(-1) >= 0)).all() and ((rd >= 0) == (rank >= 0)).all()
    for row, e in zip(rows, t["edges"]):
        walk = t["walks"][int(row[0])]
        assert sorted(rank[walk].tolist()) == list(range(int(row[C["px"]])))        # a bijection onto 0 .. px - 1
        diag = 0
        for a, b in zip(walk, walk[1:]):                                             # consecutive ranks are linked
            k = SR.OFFSETS.index((b // bw - a // bw, b % bw - a % bw))
            assert Lk[a // bw, a % bw] >> k & 1
            diag += k & 1
        assert rd[walk[-1]] == diag
        inner_diag = sum(1 for p in walk for k in (3, 5) if Lk[p // bw, p % bw] >> k & 1 and rank[p + SR.OFFSETS[k][0] * bw + SR.OFFSETS[k][1]] >= 0)
        if e[1] != 2:
            assert diag == inner_diag                                                  # (a loop's closing link is not walked)
            assert int(e[1] == 1) + int(e[3] == 1) == row[C["n_attach"]]
    assert (t["edges"][:, [1, 3]] == 1).sum() == t["nodes"][:, 5].sum() if len(rows) else True
    assert t["nodes"][:, 1].sum() == crop[0] and (t["node_labels"] >= 0).sum() == crop[0]
    path = t["path"]
    if path:
        by = {int(r[0]): r for r in rows}
        prof = t["trunk_profile"]
        cross_o = cross_d = 0
        steps = np.abs(np.diff(prof[:, :2].astype(np.int64), axis=0))
        assert (steps.max(1) >= 1).all() if len(steps) else True
        for (r0, v0), (r1, v1) in zip(path, path[1:]):
            e0, e1 = (next(e for e in t["edges"] if e[0] == r) for r in (r0, r1))
            a, b = int(e0[5] if v0 else e0[6]), int(e1[6] if v1 else e1[5])
            dy, dx = abs(a // bw - b // bw), abs(a % bw - b % bw)
            cross_o, cross_d = cross_o + max(dy, dx) - min(dy, dx), cross_d + min(dy, dx)
        assert t["trunk"][T["n_orth"]] == sum(by[r][C["n_orth"]] for r, _ in path) + cross_o
        assert t["trunk"][T["n_diag"]] == sum(by[r][C["n_diag"]] for r, _ in path) + cross_d
        assert t["trunk"][T["px"]] == len(prof) and (np.diff(prof[:, 3]) >= 0).all() and (np.diff(prof[:, 4]) >= 0).all()
        assert t["trunk"][T["max_d2"]] == prof[:, 2].max() and prof[t["trunk"][T["max_pos"]], 2] == prof[:, 2].max()
    return t


@pytest.mark.parametrize("name", list(CROPS) + list(RAW))
def test_identities_on_the_known_crops(name):
    for mb in ((0.0,) if name in RAW else (0.0, 10.0)):
        t = traced(name, mb)
        check_identities(t["S"], t["D"])


def test_identities_on_random_masks():
    for S, D in random_maps(200, 31, side=20):
        check_identities(S, D)


# ------------------------------------------------------------------------------------------------ second opinions
def brute_force_distance(rows, edges):
    """the largest finite shortest-path distance over all pairs, by scipy (parallel branches keep the lighter one)"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import shortest_path
    verts, ge = TR.vertices_and_edges(rows, edges)
    if not ge:
        return 0
    w = {}
    for r, wt, a, b in ge:
        w[(a, b)] = min(w.get((a, b), wt), wt)
        w[(b, a)] = w[(a, b)]
    m = coo_matrix((np.array(list(w.values()), np.float64), ([k[0] for k in w], [k[1] for k in w])), shape=(len(verts), len(verts))).tocsr()
    d = shortest_path(m, directed=False)
    return int(d[np.isfinite(d)].max())


def host_edges(t, instance=0):
    """the definition's edge table as measure.select_trunk takes it (EDGE_COLUMNS; the end pixels are not needed)"""
    e = t["edges"]
    return np.concatenate([np.full((len(e), 1), instance), e, np.zeros((len(e), 4), np.int64)], 1)


def check_selection(t):
    rows, edges = t["rows"], t["edges"]
    if any(e[1] != 2 for e in edges) and TR.vertices_and_edges(rows, edges)[1]:
        assert t["distance"] == brute_force_distance(rows, edges)
    weights = [TR.weight(r) for r in rows]
    path, dist = MZ.select_trunk(weights, host_edges(t))
    assert dist == t["distance"] and [(int(rows[k][0]), rev) for k, rev in path] == t["path"]


def test_the_trunk_is_the_longest_shortest_path_and_the_host_selects_the_same():
    for name in list(CROPS) + list(RAW):
        for mb in ((0.0,) if name in RAW else (0.0, 10.0)):
            check_selection(traced(name, mb))
    for S, D in random_maps(60, 7, side=20):
        check_selection(TR.trace(S, D))


def test_weights_and_columns_agree_between_the_definition_and_the_host():
    assert (MZ.W_ORTH, MZ.W_DIAG, MZ.W_END) == (TR.W_ORTH, TR.W_DIAG, TR.W_END) and MZ.TRUNK_COLUMNS == TR.TRUNK_COLS
    assert MZ.EDGE_COLUMNS[1:8] == TR.EDGE_COLS and MZ.NODE_COLUMNS[1:] == TR.NODE_COLS
    assert (L.TRACE_NODE, L.TRACE_EDGE, L.TRACE_ENT) == (8, 12, 12)


# ------------------------------------------------------------------------------------------------ the ABI's argument checks
def groups_table(boxes):
    return L.tile_compose_plan(np.asarray(boxes, np.int32).reshape(-1, 4), np.zeros(len(boxes) + 1, np.int64))


def calls(lib, p):
    """the four entry points with every buffer pointer p (host memory that a launch would fault on):
    name -> fn(groups_host, groups_dev, G, arena_bytes, capacity, rounds)"""
    return {
        "trace_nodes": lambda gh, gd, G, nb, cap, K: lib.disyolo_trace_nodes(gh, gd, G, nb, p, p, p, p, p, cap, p, None),
        "trace_rank": lambda gh, gd, G, nb, cap, K: lib.disyolo_trace_rank(gh, gd, G, nb, p, p, p, p, p, 16, p, cap, K, p, p, p, p, p, None),
        "trace_edges": lambda gh, gd, G, nb, cap, K: lib.disyolo_trace_edges(gh, gd, G, nb, p, p, cap, p, p, p, p, 16, None),
        "trace_gather": lambda gh, gd, G, nb, cap, K: lib.disyolo_trace_gather(gh, gd, G, nb, p, p, cap, p, p, p, p, 16, p, p, p, p, 1, p, 16,
                                                                              p, p, None),
    }


@pytest.mark.parametrize("name", ["trace_nodes", "trace_rank", "trace_edges", "trace_gather"])
def test_trace_entry_points_refuse_bad_arguments_before_any_launch(name):
    lib = L.load()
    buf = ctypes.create_string_buffer(1 << 16)
    p = ctypes.cast(buf, ctypes.c_void_p)
    fn = calls(lib, p)[name]
    tag = name.encode()

    def run(groups, G=None, nbytes=None, null=False, cap=16, K=4):
        g = np.ascontiguousarray(groups, dtype=np.int32)
        return fn(None if null else g.ctypes.data, g.ctypes.data, len(g) if G is None else G, 1 << 16 if nbytes is None else nbytes, cap, K)

    good, nbytes = groups_table([[0, 0, 3, 9], [5, 5, 9, 10]])
    wide, wide_bytes = groups_table([[0, 0, 1, 40000]])
    assert run(wide, nbytes=wide_bytes) == -1 and tag in lib.disyolo_last_error() and b"32767" in lib.disyolo_last_error()
    tall, tall_bytes = groups_table([[0, 0, 32768, 1]])
    assert run(tall, nbytes=tall_bytes) == -1 and b"32767" in lib.disyolo_last_error()
    assert run(good, nbytes=nbytes - 16) == -1 and b"arena" in lib.disyolo_last_error()
    far = good.copy()
    far[1, 7] = 1 << 20
    assert run(far) == -1 and b"arena" in lib.disyolo_last_error()
    assert run(good, G=-1) == -1 and tag in lib.disyolo_last_error()
    assert run(good, null=True) == -1 and b"null pointer" in lib.disyolo_last_error()
    bad = good.copy()
    bad[1, 6] = 5
    assert run(bad) == -1 and b"block0" in lib.disyolo_last_error()
    bad = good.copy()
    bad[0, 4] = -1
    assert run(bad) == -1
    bad = good.copy()
    bad[1, 7] = 0
    assert run(bad) == -1
    assert run(good, cap=-1) == -1 and b"capacity" in lib.disyolo_last_error()
    assert run(good, cap=1 << 31) == -1 and b"capacity" in lib.disyolo_last_error()
    if name != "trace_nodes":
        assert run(good, nbytes=1 << 31) == -1 and b"2^31" in lib.disyolo_last_error()
    if name == "trace_rank":
        for K in (-1, 32):
            assert run(good, K=K) == -1 and b"rounds" in lib.disyolo_last_error()
    # nothing to do is no error: G = 0 (with no pointers at all), and for the launches over the list, groups without a pixel
    assert fn(None, None, 0, 0, 0, 0) == 0
    if name == "trace_edges":
        empty, _ = groups_table([[4, 4, 4, 9], [0, 0, 0, 0]])
        assert run(empty, nbytes=0) == 0


# ------------------------------------------------------------------------------------------------ skeleton_trace's ValueErrors
def host_graph():
    """a SkeletonGraphs over host tensors: every check below has to come before anything touches a device"""
    import torch
    groups, arena, nbytes = MZ.pack_masks([np.ones((1, 9), np.uint8)])
    z32, z8 = torch.zeros(16, dtype=torch.int32), torch.zeros(16, dtype=torch.uint8)
    m = MZ.InstanceMeasures(groups[:, 2:6], [0], z32, z8, [[9, 9, 8, 0, 2, 1, 1, 0]], [9.0], [1])
    m.groups, m.arena, m.arena_bytes = groups, torch.from_numpy(arena), nbytes
    row = [[0, 0, 9, 8, 0, 2, 0, 2304, 1, 1, 0, 0]]
    return MZ.SkeletonGraphs(m, m, z8, z32, row, [[0, 0, 0, 1]], [1], [True], 0.0)


def test_skeleton_trace_refuses_bad_arguments():
    with pytest.raises(ValueError, match="SkeletonGraphs"):
        MZ.skeleton_trace(host_graph().measures)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="mm_per_px"):
            MZ.skeleton_trace(host_graph(), mm_per_px=bad)
    with pytest.raises(ValueError, match="row tables"):
        MZ.skeleton_trace(host_graph())                      # a graph that did not come from skeleton_graph: no rows_dev
    g = host_graph()
    g.measures.groups = None
    with pytest.raises(ValueError, match="skeleton_graph"):
        MZ.skeleton_trace(g)


def test_skeleton_graphs_keeps_what_it_had_and_the_row_tables():
    g = host_graph()
    assert g.rows_dev is None and g.rowid_arena is None and g.row_order.shape == (0,)
    assert g.branches["length_px"].tolist() == [9.0] and g.n_branches.tolist() == [1] and g.table()[0]["n_branches"] == 1

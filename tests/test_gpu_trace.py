"""The traced skeleton graph on the GPU: csrc/trace.hip through ``measure.skeleton_trace`` against the numpy definition
(tests/trace_ref.py).  Node labels, ranks, the node and edge tables, branch profiles, trunk rows and trunk profiles are integers:
equality, row order included.  The derived float64 columns come from those integers by the same formulas on the host: equality
too."""
import numpy as np
import pytest
import torch

import measure_ref as MR
import skeleton_ref as SR
import tiles_ref as TLR
import trace_ref as TR
from disyolo_amd import lib as L
from disyolo_amd import measure as MZ
from disyolo_amd import tiles as TL

pytestmark = pytest.mark.gpu

_MEASURED, _TRACE = {}, {}
SENT = (-5, -6, -7)                     # what the three result arenas hold before a call: node labels, rank, rank_diag


def key_of(M):
    return (M.shape, np.asarray(M != 0).tobytes())


def ref(M, mb):
    """the definition's answer for a crop, computed once per (crop, min_branch_px)"""
    k = key_of(M)
    if k not in _MEASURED:
        _MEASURED[k] = MR.measure(M)
    if k + (float(mb),) not in _TRACE:
        m = _MEASURED[k]
        _TRACE[k + (float(mb),)] = TR.trace(SR.graph(m["skeleton"], m["d2"], mb)["skeleton"], m["d2"])
    return _TRACE[k + (float(mb),)]


def ring():
    yy, xx = np.mgrid[:40, :40]
    r2 = (yy - 20) ** 2 + (xx - 20) ** 2
    return ((10 ** 2 < r2) & (r2 < 15 ** 2)).astype(np.uint8)


def thick_strokes():
    """two 3-pixel-wide strokes one apart in height with stubs at the joint: thinning leaves a node of several pixels"""
    M = np.zeros((24, 48), np.uint8)
    M[8:11, 0:26] = 1
    M[11:14, 22:48] = 1
    M[0:8, 22:25] = 1
    M[14:24, 23:26] = 1
    return M


def crops_by_name():
    c = {n: v[0] for n, v in MR.known_crops().items()}
    c.update(SR.extra_crops())
    c.update({"raw_" + n: M for n, M in TR.extra_crops().items()})
    c.update(ring=ring(), thick_strokes=thick_strokes())
    return c


def known_set():
    """every crop with a known answer but serp, the extra ones, an all-zero 4x5 and one more 1x1; crops whose area is no
    multiple of 16 first: their neighbours in the arena start behind padding bytes"""
    crops = [M for n, M in crops_by_name().items() if n != "serp"] + [np.zeros((4, 5), np.uint8), np.ones((1, 1), np.uint8)]
    return sorted(crops, key=lambda c: (c.size % 16 == 0, c.size))


def graph(dev, crops, mb, fill=0, foreground=1):
    groups, arena, nbytes = MZ.pack_masks(crops, fill=fill, foreground=foreground)
    m = MZ.measure_arena(groups, torch.from_numpy(arena).to(dev), nbytes)
    return MZ.skeleton_graph(m, mb), groups, nbytes


def trace(dev, g, nbytes, **kw):
    out = [torch.full((max(nbytes, 1),), v, dtype=torch.int32, device=dev) for v in SENT]
    return MZ.skeleton_trace(g, node_labels_out=out[0], rank_out=out[1], rank_diag_out=out[2], **kw)


def assert_matches_ref(t, crops, mb):
    g = t.graphs
    assert len(t) == len(crops)
    for i, M in enumerate(crops):
        want = ref(M, mb)
        rk, rd, nl = t.rank(i), t.rank_diag(i), t.node_labels(i)
        assert rk.dtype == rd.dtype == nl.dtype == torch.int32 and rk.is_cuda and tuple(rk.shape) == tuple(nl.shape) == M.shape
        np.testing.assert_array_equal(nl.cpu().numpy(), want["node_labels"], err_msg="node labels of crop %d" % i)
        np.testing.assert_array_equal(rk.cpu().numpy(), want["rank"], err_msg="rank of crop %d" % i)
        np.testing.assert_array_equal(rd.cpu().numpy(), want["rank_diag"], err_msg="rank_diag of crop %d" % i)
        nodes = t.nodes_of(i)
        assert (nodes["instance"] == i).all() and len(nodes) == len(want["nodes"]), "nodes of crop %d" % i
        for c, name in enumerate(TR.NODE_COLS):
            np.testing.assert_array_equal(nodes[name], want["nodes"][:, c], err_msg="node %s of crop %d" % (name, i))
        np.testing.assert_array_equal(nodes["centroid_y"], want["nodes"][:, 2] / np.maximum(want["nodes"][:, 1], 1))
        edges = t.edges_of(i)
        assert (edges["instance"] == i).all() and len(edges) == len(want["edges"]) == len(g.branches_of(i)), "edges of crop %d" % i
        for c, name in enumerate(TR.EDGE_COLS):
            np.testing.assert_array_equal(edges[name], want["edges"][:, c], err_msg="edge %s of crop %d" % (name, i))
        for root, prof in want["profiles"].items():
            got = t.branch_profile(i, root)
            assert got.dtype == torch.int32 and got.is_cuda
            np.testing.assert_array_equal(got.cpu().numpy(), prof, err_msg="profile of branch %d of crop %d" % (root, i))
            assert edges["end0_px"][edges["root"] == root][0] == want["walks"][root][0]
            assert edges["end1_px"][edges["root"] == root][0] == want["walks"][root][-1]
        assert t.trunk_branches(i) == want["path"], "trunk of crop %d" % i
        for c, name in enumerate(TR.TRUNK_COLS):
            assert int(t.trunk[name][i]) == int(want["trunk"][c]), "trunk %s of crop %d" % (name, i)
        np.testing.assert_array_equal(t.trunk_profile(i).cpu().numpy(), want["trunk_profile"], err_msg="trunk profile of crop %d" % i)
        length, wmean, wmax = TR.derive_trunk(want["trunk"])
        assert (t.trunk["trunk_length_px"][i], t.trunk["mean_width_px"][i], t.trunk["max_width_px"][i]) == (length, wmean, wmax)
        y1, x1 = int(g.measures.boxes[i][0]), int(g.measures.boxes[i][1])
        if want["trunk"][1]:
            assert (t.trunk["widest_y"][i], t.trunk["widest_x"][i]) == (y1 + want["trunk"][8], x1 + want["trunk"][9])
    assert len(t.edges) == len(g.branches) and int(t.profile_buffer.shape[0]) == int(g.branches["px"].sum())


def same_bits(a, b, nbytes):
    for f in ("node_labels_arena", "rank_arena", "rank_diag_arena"):
        assert torch.equal(getattr(a, f)[:nbytes], getattr(b, f)[:nbytes]), f
    assert torch.equal(a.profile_buffer, b.profile_buffer) and torch.equal(a.trunk_buffer, b.trunk_buffer)
    assert a.nodes.tobytes() == b.nodes.tobytes() and a.edges.tobytes() == b.edges.tobytes() and a.trunk.tobytes() == b.trunk.tobytes()
    assert [a.trunk_branches(i) for i in range(len(a))] == [b.trunk_branches(i) for i in range(len(b))]


def padding_of(groups, crops, nbytes):
    pad = np.ones(nbytes, bool)
    for gr, c in zip(groups, crops):
        pad[int(gr[7]) * 16:int(gr[7]) * 16 + c.size] = False
    return pad


# ------------------------------------------------------------------------------------------------ the known answers
@pytest.mark.parametrize("mb", [0.0, 10.0])
def test_known_answers_in_one_arena(dev, mb):
    crops = known_set()
    assert any(c.size % 16 for c in crops[:-1])
    g, groups, nbytes = graph(dev, crops, mb)
    before = (g.links_arena.clone(), g.labels_arena.clone(), g.rows_dev.clone(), g.branches.copy())
    a = trace(dev, g, nbytes)
    assert a.graphs is g and torch.equal(g.links_arena, before[0]) and torch.equal(g.labels_arena, before[1])
    assert torch.equal(g.rows_dev, before[2]) and g.branches.tobytes() == before[3].tobytes()
    assert_matches_ref(a, crops, mb)
    names = crops_by_name()
    at = {n: next(i for i, c in enumerate(crops) if c.shape == M.shape and (c == M).all()) for n, M in names.items() if n != "serp"}
    tr = a.trunk
    assert tr["trunk_length_px"][at["1x1"]] == 1.0 and tr["weight"][at["1x1"]] == 1024 and tr["px"][at["2x2"]] == 0
    assert tr["trunk_length_px"][at["1x9"]] == 9.0 and tr["weight"][at["eye9"]] == 12608 and tr["trunk_length_px"][at["70x300"]] == 230.0
    assert (tr["weight"][at["sinusoid"]], tr["px"][at["sinusoid"]]) == (254216, 223)
    assert tr["trunk_length_px"][at["ring_tail"]] == 50.5 and a.trunk_branches(at["ring_tail"]) == [(9688, False)]
    assert tr["weight"][at["T3spur"]] == 59392 and tr["trunk_length_px"][at["T3spur"]] == 58.0
    assert tr["n_branches"][at["T3spur"]] == (3 if mb == 0 else 2)
    assert tr["trunk_length_px"][at["plus9"]] == (9.0 if mb == 0 else 1.0) and tr["weight"][at["noise"]] == (59112 if mb == 0 else 41704)
    loop = a.edges_of(at["ring"])
    assert len(loop) == 1 and loop["end0_kind"][0] == 2 and tr["n_branches"][at["ring"]] == 1 and tr["n_end"][at["ring"]] == 0
    assert (a.nodes_of(at["thick_strokes"])["px"] > 1).any() or (a.nodes_of(at["noise"])["px"] > 1).any()
    noise_e, noise_b = a.edges_of(at["noise"]), g.branches_of(at["noise"])
    assert (a.nodes_of(at["noise"])["px"] > 1).sum() > 10                                  # multi-pixel nodes
    assert ((noise_b["px"] == 1) & (noise_e["end0_kind"] == 1) & (noise_e["end1_kind"] == 1)).any()     # single pixels, two attachments
    pad = padding_of(groups, crops, nbytes)
    for arena, s in zip((a.node_labels_arena, a.rank_arena, a.rank_diag_arena), SENT):
        assert pad.sum() > 0 and (arena.cpu().numpy()[:nbytes][pad] == s).all()
    same_bits(a, trace(dev, g, nbytes), nbytes)                # the same call again: the same bits


# ------------------------------------------------------------------------------------------------ long branches, block borders
def test_one_list_through_many_chunks_and_thirteen_rounds(dev, monkeypatch):
    bar = np.zeros((7, 1030), np.uint8)            # a 3 x 1030 bar with three one-pixel-wide spurs of length 4 on it
    bar[4:7, :] = 1
    for x in (100, 1023, 1026):
        bar[0:4, x] = 1
    crops = [SR.extra_crops()["serp"], bar]
    assert crops[0].size > 12 * L.COMPOSE_CHUNK and bar.shape[1] > L.COMPOSE_CHUNK
    seen = []
    rank_call = L.trace_rank
    monkeypatch.setattr(L, "trace_rank", lambda *a, **k: (seen.append(a[7]), rank_call(*a, **k))[1])
    for mb in (0.0, 10.0):
        g, groups, nbytes = graph(dev, crops, mb)
        t = trace(dev, g, nbytes)
        assert_matches_ref(t, crops, mb)
        assert seen[-1] == 13 and g.branches_of(0)["px"].tolist() == [6320]             # ceil(log2 6320) rounds
        rk = t.rank(0).cpu().numpy().reshape(-1)
        assert rk[0] == 0 and rk[12299] == 6319 and t.trunk["weight"][0] == 6471680 and t.trunk["px"][0] == 6320
        prof = t.branch_profile(0, 0).cpu().numpy()
        assert prof.shape == (6320, 4) and prof[0].tolist() == [0, 0, 1, 0] and prof[-1, :2].tolist() == [40, 299]
    assert len(ref(bar, 0.0)["edges"]) > 1 and len(ref(bar, 0.0)["nodes"]) >= 1


# ------------------------------------------------------------------------------------------------ padding
def test_padding_is_neither_read_nor_written(dev):
    crops = known_set()
    g, groups, nbytes = graph(dev, crops, 10.0, fill=0xFF, foreground=0x80)
    a = trace(dev, g, nbytes)
    assert_matches_ref(a, crops, 10.0)
    g0, _, _ = graph(dev, crops, 10.0)
    same_bits(a, trace(dev, g0, nbytes), nbytes)
    pad = padding_of(groups, crops, nbytes)
    assert pad.sum() > 0
    for arena, s in zip((a.node_labels_arena, a.rank_arena, a.rank_diag_arena), SENT):
        assert (arena.cpu().numpy()[:nbytes][pad] == s).all()


# ------------------------------------------------------------------------------------------------ nothing to do, host reads
def counted(monkeypatch):
    calls = {"read": 0}
    read = MZ._trace_read
    monkeypatch.setattr(MZ, "_trace_read", lambda t: (calls.__setitem__("read", calls["read"] + 1), read(t))[1])
    return calls


def test_no_groups_empty_boxes_and_the_host_reads(dev, monkeypatch):
    calls = counted(monkeypatch)
    launched = []
    for name in ("trace_nodes", "trace_rank", "trace_edges", "trace_gather"):
        fn = getattr(L, name)
        monkeypatch.setattr(L, name, lambda *a, _fn=fn, _n=name, **k: (launched.append(_n), _fn(*a, **k))[1])
    t = MZ.skeleton_trace(MZ.skeleton_graph(MZ.measure_masks([], device=dev), 10.0))
    assert len(t) == 0 and t.nodes.shape == (0,) and t.edges.shape == (0,) and t.trunk.shape == (0,) and t.table() == []
    sc = TLR.scene()
    res = TL.merge_tiles(sc.tiles, sc.image_hw, sc.net_size, sc.detections, np.zeros_like(sc.keep), torch.from_numpy(sc.masks).to(dev))
    t = MZ.skeleton_trace(MZ.skeleton_graph(MZ.measure_instances(res, mm_per_px=0.5), 10.0))
    assert len(t) == 0 and "trunk_length_mm" in t.trunk.dtype.names
    assert calls["read"] == 0 and launched == []                       # G = 0: nothing launched, nothing read
    only_empty = MZ.skeleton_trace(MZ.skeleton_graph(MZ.measure_masks([np.zeros((0, 3), np.uint8), np.zeros((4, 5), np.uint8)], device=dev), 3.0))
    assert calls["read"] == 0 and only_empty.trunk["px"].tolist() == [0, 0] and only_empty.trunk_profile(1).shape == (0, 5)
    assert (only_empty.rank(1).cpu().numpy() == -1).all() and (only_empty.node_labels(1).cpu().numpy() == -1).all()
    crops = [np.ones((3, 9), np.uint8), np.zeros((0, 7), np.uint8), np.zeros((4, 5), np.uint8), np.ones((2, 2), np.uint8), np.ones((1, 9), np.uint8)]
    g, groups, nbytes = graph(dev, crops, 10.0)
    launched.clear()
    t = trace(dev, g, nbytes)
    assert calls["read"] == 2 and launched == ["trace_nodes", "trace_rank", "trace_edges", "trace_gather"]
    assert_matches_ref(t, crops, 10.0)
    np.testing.assert_array_equal(t.trunk["trunk_length_px"], [6.0, 0.0, 0.0, 0.0, 9.0])
    assert t.trunk_branches(1) == [] and t.trunk_branches(3) == [] and t.trunk_profile(3).shape == (0, 5) and len(t.edges_of(2)) == 0
    with pytest.raises(KeyError):
        t.branch_profile(0, 3)
    calls["read"] = 0
    g, groups, nbytes = graph(dev, [MR.known_crops()["noise"][0]], 10.0)
    trace(dev, g, nbytes)
    assert calls["read"] == 2                                           # whatever the number of branches, nodes and rounds


# ------------------------------------------------------------------------------------------------ end to end
def test_skeleton_trace_on_the_scene(dev):
    sc = TLR.scene()
    res = TL.merge_tiles(sc.tiles, sc.image_hw, sc.net_size, sc.detections, sc.keep, torch.from_numpy(sc.masks).to(dev))
    assert len(res) == 5
    g = MZ.skeleton_graph(MZ.measure_instances(res), 10.0, mm_per_px=0.5)
    t = MZ.skeleton_trace(g)
    crops = [res.mask(i).cpu().numpy().astype(np.uint8) for i in range(len(res))]
    assert_matches_ref(t, crops, 10.0)
    tr = t.trunk
    np.testing.assert_array_equal(tr["trunk_length_mm"], 0.5 * tr["trunk_length_px"])
    np.testing.assert_array_equal(tr["mean_width_mm"], 0.5 * tr["mean_width_px"])
    np.testing.assert_array_equal(tr["max_width_mm"], 0.5 * tr["max_width_px"])
    rows, base = t.table(["crack", "spall", "rebar"]), g.table(["crack", "spall", "rebar"])
    for i, row in enumerate(rows):
        assert {k: row[k] for k in base[i]} == base[i]
        assert row["trunk_length_px"] == tr["trunk_length_px"][i] and row["trunk_length_mm"] == tr["trunk_length_mm"][i]
        y1, x1, y2, x2 = row["box"]
        assert tr["px"][i] == 0 or (y1 <= row["trunk_widest_yx"][0] < y2 and x1 <= row["trunk_widest_yx"][1] < x2)
        assert row["trunk_max_width_px"] <= row["max_width_px"] and row["trunk_branches"] == tr["n_branches"][i]
    g0 = MZ.skeleton_graph(MZ.measure_instances(res), 10.0)
    assert "trunk_length_mm" not in MZ.skeleton_trace(g0).trunk.dtype.names and "trunk_length_mm" in MZ.skeleton_trace(g0, mm_per_px=2.0).trunk.dtype.names


def test_skeleton_trace_of_masks_of_different_sizes(dev):
    rng = np.random.default_rng(3)
    yy, xx = np.mgrid[:37, :53]
    crops = [rng.random((23, 41)) < 0.7,
             ((yy - 18) ** 2 + (xx - 26) ** 2 < 200).astype(np.uint8) * 255,
             (np.abs(yy[:9, :31] - 4) < 2).astype(np.uint8)]
    m = MZ.measure_masks([crops[0], torch.from_numpy(crops[1]).to(dev), crops[2]], device=dev)
    for mb in (0.0, 4.5):
        assert_matches_ref(MZ.skeleton_trace(MZ.skeleton_graph(m, mb)), [np.asarray(c != 0, np.uint8) for c in crops], mb)

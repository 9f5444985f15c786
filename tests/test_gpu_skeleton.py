"""The skeleton graph on the GPU: csrc/skeleton.hip through ``measure.skeleton_graph`` against the numpy definition
(tests/skeleton_ref.py).  Links, labels, pruned skeletons, branch rows, junction numbers, analyses and the pruned skeleton's
counts are integers: equality, row order included.  The derived float64 columns come from those integers by the same formulas
on the host: equality too.  The one float64 sum of the pruned skeleton, ``pruned.sum_sqrt``, agrees within relative
(n + 2) 2^-52 for n skeleton pixels as in test_gpu_measure.py; 1e-12 covers n <= 2000, and the one crop with more (serp, 6320
pixels) is held to (n + 2) 2^-52 itself."""
import numpy as np
import pytest
import torch

import measure_ref as MR
import skeleton_ref as SR
import tiles_ref as TR
from disyolo_amd import lib as L
from disyolo_amd import measure as MZ
from disyolo_amd import tiles as TL

pytestmark = pytest.mark.gpu

_MEASURED, _GRAPH = {}, {}
INT_COLUMNS = ("px", "n_orth", "n_diag", "n_end", "n_attach", "sum_q8", "max_d2", "min_d2", "spur")


def key_of(M):
    return (M.shape, np.asarray(M != 0).tobytes())


def measured(M):
    k = key_of(M)
    if k not in _MEASURED:
        _MEASURED[k] = MR.measure(M)
    return _MEASURED[k]


def ref(M, mb, max_rounds=8):
    """the definition's answer for a crop, computed once per (crop, min_branch_px, max_rounds)"""
    k = key_of(M) + (float(mb), max_rounds)
    if k not in _GRAPH:
        m = measured(M)
        g = SR.graph(m["skeleton"], m["d2"], mb, max_rounds)
        g["counts"] = MR.counts(M, g["skeleton"], m["d2"])
        g["sum_sqrt"] = MR.sum_sqrt(g["skeleton"], m["d2"])
        _GRAPH[k] = g
    return _GRAPH[k]


def crops_by_name():
    c = {n: v[0] for n, v in MR.known_crops().items()}
    c.update(SR.extra_crops())
    return c


def known_set():
    """every crop with a known answer but serp, an all-zero 4x5 and one more 1x1, crops whose area is no multiple of 16
    first: their neighbours in the arena start behind padding bytes"""
    crops = [M for n, M in crops_by_name().items() if n != "serp"] + [np.zeros((4, 5), np.uint8), np.ones((1, 1), np.uint8)]
    return sorted(crops, key=lambda c: (c.size % 16 == 0, c.size))


def measure(dev, crops, fill=0, foreground=1, sentinel=0):
    groups, arena, nbytes = MZ.pack_masks(crops, fill=fill, foreground=foreground)
    m = MZ.measure_arena(groups, torch.from_numpy(arena).to(dev), nbytes,
                         d2_out=torch.full((nbytes,), -7, dtype=torch.int32, device=dev),
                         skeleton_out=torch.full((nbytes,), sentinel, dtype=torch.uint8, device=dev))
    return m, groups, nbytes


def assert_matches_ref(g, crops, mb, max_rounds=8, big=()):
    assert len(g) == len(crops)
    firsts = 0
    for i, M in enumerate(crops):
        want = ref(M, mb, max_rounds)
        lk, lb, sk = g.links(i), g.labels(i), g.pruned_skeleton(i)
        assert lk.dtype == torch.uint8 and lb.dtype == torch.int32 and sk.dtype == torch.bool and lk.is_cuda and lb.is_cuda
        assert tuple(lk.shape) == tuple(lb.shape) == tuple(sk.shape) == M.shape
        np.testing.assert_array_equal(lk.cpu().numpy(), want["links"], err_msg="links of crop %d" % i)
        np.testing.assert_array_equal(lb.cpu().numpy(), want["labels"], err_msg="labels of crop %d" % i)
        np.testing.assert_array_equal(sk.cpu().numpy().view(np.uint8), want["skeleton"], err_msg="pruned skeleton of crop %d" % i)
        b = g.branches_of(i)
        rows = want["rows"]
        assert (b["instance"] == i).all() and len(b) == len(rows), "branches of crop %d" % i
        np.testing.assert_array_equal(b["root"], rows[:, 0], err_msg="roots of crop %d" % i)
        for c in INT_COLUMNS:
            np.testing.assert_array_equal(b[c].astype(np.int64), rows[:, SR.ROW_COLS.index(c)], err_msg="%s of crop %d" % (c, i))
        np.testing.assert_array_equal(b["root_y"] * M.shape[1] + b["root_x"], rows[:, 0])
        length, wmean, wmax, wmin, kinds = SR.derive_rows(rows)
        np.testing.assert_array_equal(b["length_px"], length)
        np.testing.assert_array_equal(b["mean_width_px"], wmean)
        np.testing.assert_array_equal(b["max_width_px"], wmax)
        np.testing.assert_array_equal(b["min_width_px"], wmin)
        assert b["kind"].tolist() == kinds
        got = [int(g.junction_px[i]), int(g.jj_orth[i]), int(g.jj_diag[i]), int(g.n_branches[i])]
        assert got == want["crop"].tolist(), "junction numbers of crop %d" % i
        assert g.group_analyses[i] == want["analyses"] and bool(g.converged[i]) == bool(want["converged"]), "analyses of crop %d" % i
        np.testing.assert_array_equal(g.pruned.counts[i], want["counts"], err_msg="pruned counts of crop %d" % i)
        n = int(want["counts"][1])
        bound = 1e-12 if i not in big else (n + 2) * 2.0 ** -52
        assert n <= 2000 or i in big
        assert abs(g.pruned.sum_sqrt[i] - want["sum_sqrt"]) <= bound * want["sum_sqrt"], "sum_sqrt of crop %d" % i
        # the identity: the links of the branches and those between junction pixels are the links of the skeleton
        assert b["n_orth"].sum() + g.jj_orth[i] == want["counts"][2] and b["n_diag"].sum() + g.jj_diag[i] == want["counts"][3]
        firsts += len(b)
    assert firsts == len(g.branches)
    assert g.analyses == max([ref(M, mb, max_rounds)["analyses"] for M in crops])
    cnt = np.stack([ref(M, mb, max_rounds)["counts"] for M in crops])
    length, wmax, wmean = MR.derive(cnt, g.pruned.sum_sqrt)
    np.testing.assert_array_equal(g.pruned.length_px, length)
    np.testing.assert_array_equal(g.pruned.mean_width_px, wmean)
    np.testing.assert_array_equal(g.pruned.max_width_px, wmax)


def same_bits(a, b, nbytes):
    assert torch.equal(a.links_arena[:nbytes], b.links_arena[:nbytes]) and torch.equal(a.labels_arena[:nbytes], b.labels_arena[:nbytes])
    assert torch.equal(a.pruned.skeleton_arena[:nbytes], b.pruned.skeleton_arena[:nbytes])
    assert a.branches.tobytes() == b.branches.tobytes()                                       # row order included
    for f in ("junction_px", "jj_orth", "jj_diag", "n_branches", "group_analyses", "converged"):
        np.testing.assert_array_equal(getattr(a, f), getattr(b, f))
    np.testing.assert_array_equal(a.pruned.counts, b.pruned.counts)
    np.testing.assert_array_equal(a.pruned.sum_sqrt.view(np.int64), b.pruned.sum_sqrt.view(np.int64))


def graph_with_sentinels(dev, m, nbytes, mb, sentinels=(0, 0, 0), **kw):
    return MZ.skeleton_graph(m, mb, links_out=torch.full((nbytes,), sentinels[0], dtype=torch.uint8, device=dev),
                             labels_out=torch.full((nbytes,), sentinels[1], dtype=torch.int32, device=dev),
                             pruned_out=torch.full((nbytes,), sentinels[2], dtype=torch.uint8, device=dev), **kw)


# ------------------------------------------------------------------------------------------------ the known answers
@pytest.mark.parametrize("mb", [0.0, 3.0, 10.0])
def test_known_answers_in_one_arena(dev, mb):
    crops = known_set()
    assert any(c.size % 16 for c in crops[:-1])
    m, groups, nbytes = measure(dev, crops)
    skel_before = m.skeleton_arena.clone()
    a = graph_with_sentinels(dev, m, nbytes, mb)
    assert torch.equal(m.skeleton_arena, skel_before) and a.measures is m and a.pruned.d2_arena is m.d2_arena
    assert_matches_ref(a, crops, mb)
    assert a.analyses == (1 if mb == 0 else 2 if mb == 3 else 3)
    names = crops_by_name()
    at = {n: next(i for i, c in enumerate(crops) if c.shape == M.shape and (c == M).all()) for n, M in names.items() if n != "serp"}
    for n in ("1x1", "1x9", "eye9", "3x9", "5x17", "17x33", "70x300", "sinusoid", "ellipse"):    # the table itself
        b = a.branches_of(at[n])
        v = MR.known_crops()[n]
        assert len(b) == 1 and b["kind"][0] == "free" and b["n_end"][0] == 2 and a.junction_px[at[n]] == 0
        assert (int(b["px"][0]), int(b["n_orth"][0]), int(b["n_diag"][0])) == (v[2], v[3], v[4])
    assert a.branches_of(at["ellipse"])["sum_q8"][0] == 806896 and a.branches_of(at["ellipse"])["min_d2"][0] == 337
    assert a.n_branches[at["2x2"]] == 0 and a.junction_px[at["2x2"]] == 0
    t3, plus, ring, noise = (a.branches_of(at[n]) for n in ("T3spur", "plus9", "ring_tail", "noise"))
    assert ring["px"].tolist() == [159, 50] and ring["kind"].tolist() == ["inner", "terminal"] and ring["length_px"][1] == 50.5
    if mb == 0:
        assert t3["length_px"].tolist() == [4.5, 14.5, 15.0, 28.5, 18.5] and t3["sum_q8"].tolist() == [2108, 7168, 7168, 14336, 9276]
        assert list(zip(t3["root_y"], t3["root_x"])) == [(5, 15), (9, 1), (9, 16), (9, 31), (10, 30)]
        assert len(noise) == 456 and (a.junction_px[at["noise"]], a.jj_orth[at["noise"]], a.jj_diag[at["noise"]]) == (672, 475, 123)
        assert noise["px"].sum() == 743 and noise["sum_q8"].sum() == 195242
    if mb == 3:
        assert plus["length_px"].tolist() == [4.5] * 4 and plus["kind"].tolist() == ["terminal"] * 4
    if mb == 10:
        assert t3["px"].tolist() == [29, 28, 18] and t3["length_px"].tolist() == [29.5, 28.5, 18.5] and a.pruned.length_px[at["T3spur"]] == 76.5
        assert a.group_analyses[at["T3spur"]] == 2 and a.pruned.skeleton_px[at["T3spur"]] == 76 and a.junction_px[at["T3spur"]] == 1
        assert plus["px"].tolist() == [1] and plus["sum_q8"].tolist() == [362] and plus["kind"].tolist() == ["free"]
        assert len(noise) == 411 and a.pruned.skeleton_px[at["noise"]] == 1330 and a.group_analyses[at["noise"]] == 3
        assert abs(a.pruned.length_px[at["noise"]] - 1800.0214) < 1e-4
    b = graph_with_sentinels(dev, m, nbytes, mb)           # the same call again: the same bits, row order included
    same_bits(a, b, nbytes)


# ------------------------------------------------------------------------------------------------ long branches, block borders
def test_one_branch_through_many_chunks_and_spurs_on_a_long_bar(dev):
    bar = np.zeros((7, 1030), np.uint8)            # a 3 x 1030 bar with three one-pixel-wide spurs of length 4 on it
    bar[4:7, :] = 1
    for x in (100, 1023, 1026):
        bar[0:4, x] = 1
    crops = [SR.extra_crops()["serp"], bar]
    assert crops[0].size > 12 * L.COMPOSE_CHUNK and bar.shape[1] > L.COMPOSE_CHUNK
    m, groups, nbytes = measure(dev, crops)
    for mb in (0.0, 10.0):
        g = MZ.skeleton_graph(m, mb)
        assert_matches_ref(g, crops, mb, big=(0,))
        s = g.branches_of(0)
        assert len(s) == 1 and (s["root"][0], s["px"][0], s["n_orth"][0], s["sum_q8"][0], s["kind"][0]) == (0, 6320, 6319, 1617920, "free")
    assert ref(bar, 0.0)["crop"][3] > 1 and ref(bar, 10.0)["analyses"] >= 2 and ref(bar, 10.0)["crop"][3] < ref(bar, 0.0)["crop"][3]


# ------------------------------------------------------------------------------------------------ noise: rounds, overflow
def test_noise_rounds_and_a_row_buffer_too_small(dev, monkeypatch):
    noise = MR.known_crops()["noise"][0]
    m, groups, nbytes = measure(dev, [noise])
    full = MZ.skeleton_graph(m, 10.0)
    assert_matches_ref(full, [noise], 10.0)
    assert full.analyses == 3 and full.converged.tolist() == [True]
    one = MZ.skeleton_graph(m, 10.0, max_rounds=1)
    assert_matches_ref(one, [noise], 10.0, max_rounds=1)
    assert one.analyses == 2 and one.converged.tolist() == [False] and one.pruned.skeleton_px[0] == 1338
    assert one.n_branches[0] == 417 and one.junction_px[0] == 641 and (one.branches["kind"] == "terminal").sum() == 3
    none = MZ.skeleton_graph(m, 10.0, max_rounds=0)
    assert_matches_ref(none, [noise], 10.0, max_rounds=0)
    assert none.analyses == 1 and none.converged.tolist() == [False] and none.pruned.skeleton_px[0] == 1415
    assert torch.equal(none.pruned.skeleton_arena[:nbytes], m.skeleton_arena[:nbytes]) and none.branches["spur"].sum() > 0
    # host synchronisations: one read per analysis and the final copy; a row buffer of 4 rows costs the first analysis one more
    calls = {"read": 0, "rows": 0}
    read, rows = MZ._read, L.skeleton_rows
    monkeypatch.setattr(MZ, "_read", lambda t: (calls.__setitem__("read", calls["read"] + 1), read(t))[1])
    monkeypatch.setattr(L, "skeleton_rows", lambda *a, **k: (calls.__setitem__("rows", calls["rows"] + 1), rows(*a, **k))[1])
    again = MZ.skeleton_graph(m, 10.0)
    assert calls == {"read": 4, "rows": 3}
    calls.update(read=0, rows=0)
    small = MZ.skeleton_graph(m, 10.0, row_capacity=4)
    assert calls == {"read": 5, "rows": 4}
    same_bits(full, again, nbytes)
    same_bits(full, small, nbytes)


# ------------------------------------------------------------------------------------------------ padding
def test_padding_is_neither_read_nor_written(dev):
    crops = known_set()
    m, groups, nbytes = measure(dev, crops, fill=0xFF, foreground=0x80, sentinel=0xEE)
    sent = (0xEE, -7, 0xDD)
    a = graph_with_sentinels(dev, m, nbytes, 10.0, sentinels=sent)
    assert_matches_ref(a, crops, 10.0)
    m0, _, _ = measure(dev, crops)
    same_bits(a, graph_with_sentinels(dev, m0, nbytes, 10.0, sentinels=sent), nbytes)
    pad = np.ones(nbytes, bool)
    for g, c in zip(groups, crops):
        pad[int(g[7]) * 16:int(g[7]) * 16 + c.size] = False
    assert pad.sum() > 0
    assert (a.links_arena.cpu().numpy()[:nbytes][pad] == sent[0]).all() and (a.labels_arena.cpu().numpy()[:nbytes][pad] == sent[1]).all()
    assert (a.pruned.skeleton_arena.cpu().numpy()[:nbytes][pad] == sent[2]).all()


# ------------------------------------------------------------------------------------------------ nothing to do
def test_no_groups_and_empty_boxes(dev):
    g = MZ.skeleton_graph(MZ.measure_masks([], device=dev), 10.0)
    assert len(g) == 0 and g.branches.shape == (0,) and g.n_branches.shape == (0,) and g.analyses == 0 and g.table() == []
    assert len(g.pruned) == 0 and g.converged.shape == (0,)
    sc = TR.scene()
    res = TL.merge_tiles(sc.tiles, sc.image_hw, sc.net_size, sc.detections, np.zeros_like(sc.keep), torch.from_numpy(sc.masks).to(dev))
    g = MZ.skeleton_graph(MZ.measure_instances(res, mm_per_px=0.5), 10.0)
    assert len(g) == 0 and g.branches.shape == (0,) and "length_mm" in g.branches.dtype.names
    crops = [np.ones((3, 9), np.uint8), np.zeros((0, 7), np.uint8), np.zeros((4, 5), np.uint8), np.ones((1, 9), np.uint8)]
    g = MZ.skeleton_graph(MZ.measure_masks(crops, device=dev), 10.0)
    assert g.n_branches.tolist() == [1, 0, 0, 1] and g.group_analyses.tolist() == [1, 1, 1, 1] and g.converged.all()
    assert len(g.branches_of(1)) == 0 and len(g.branches_of(2)) == 0 and g.branches["instance"].tolist() == [0, 3]
    np.testing.assert_array_equal(g.pruned.length_px, [6.0, 0.0, 0.0, 9.0])
    only_empty = MZ.skeleton_graph(MZ.measure_masks([np.zeros((0, 3), np.uint8)], device=dev), 3.0)
    assert only_empty.n_branches.tolist() == [0] and only_empty.analyses == 1


def test_argument_errors_come_before_any_launch(dev, monkeypatch):
    m = MZ.measure_masks([np.ones((3, 9), np.uint8)], device=dev)
    monkeypatch.setattr(L, "skeleton_classify", lambda *a, **k: pytest.fail("launched"))
    for bad in (0.25, -1.0, 32767.5, float("nan"), float("inf"), "x"):
        with pytest.raises(ValueError, match="min_branch_px"):
            MZ.skeleton_graph(m, bad)
    for bad in (-1, 1025, 2.0, True, None):
        with pytest.raises(ValueError, match="max_rounds"):
            MZ.skeleton_graph(m, 10.0, max_rounds=bad)


# ------------------------------------------------------------------------------------------------ groups are independent
def test_a_group_that_converges_early_is_not_touched_by_the_others(dev):
    c = crops_by_name()
    pair = [c["ring_tail"], c["noise"]]
    m2, _, _ = measure(dev, pair)
    both = MZ.skeleton_graph(m2, 10.0)
    assert_matches_ref(both, pair, 10.0)
    assert both.group_analyses.tolist() == [1, 3] and both.analyses == 3
    m1, _, _ = measure(dev, pair[:1])
    alone = MZ.skeleton_graph(m1, 10.0)
    assert alone.analyses == 1
    assert torch.equal(both.links(0), alone.links(0)) and torch.equal(both.labels(0), alone.labels(0))
    assert torch.equal(both.pruned_skeleton(0), alone.pruned_skeleton(0))
    assert both.branches_of(0).tobytes() == alone.branches_of(0).tobytes()
    np.testing.assert_array_equal(both.pruned.counts[0], alone.pruned.counts[0])
    assert both.pruned.sum_sqrt[0] == alone.pruned.sum_sqrt[0]


# ------------------------------------------------------------------------------------------------ end to end
def test_skeleton_graph_on_the_scene(dev):
    sc = TR.scene()
    res = TL.merge_tiles(sc.tiles, sc.image_hw, sc.net_size, sc.detections, sc.keep, torch.from_numpy(sc.masks).to(dev))
    assert len(res) == 5
    m = MZ.measure_instances(res)
    g = MZ.skeleton_graph(m, 10.0, mm_per_px=0.5)
    crops = [res.mask(i).cpu().numpy().astype(np.uint8) for i in range(len(res))]
    assert_matches_ref(g, crops, 10.0)
    b = g.branches
    np.testing.assert_array_equal(b["length_mm"], 0.5 * b["length_px"])
    np.testing.assert_array_equal(b["mean_width_mm"], 0.5 * b["mean_width_px"])
    np.testing.assert_array_equal(b["max_width_mm"], 0.5 * b["max_width_px"])
    np.testing.assert_array_equal(b["min_width_mm"], 0.5 * b["min_width_px"])
    np.testing.assert_array_equal(g.pruned.length_mm, 0.5 * g.pruned.length_px)
    rows, base = g.table(["crack", "spall", "rebar"]), m.table(["crack", "spall", "rebar"])
    for i, row in enumerate(rows):
        assert {k: row[k] for k in base[i]} == base[i]
        assert row["pruned_length_px"] == g.pruned.length_px[i] <= row["length_px"]
        assert row["n_branches"] == g.n_branches[i] and row["junction_px"] == g.junction_px[i]
    m5 = MZ.measure_instances(res, mm_per_px=0.5)                     # the scale of the measures is the default
    assert "length_mm" in MZ.skeleton_graph(m5, 10.0).branches.dtype.names and "length_mm" not in MZ.skeleton_graph(m, 10.0).branches.dtype.names


def test_skeleton_graph_of_masks_of_different_sizes(dev):
    rng = np.random.default_rng(3)
    yy, xx = np.mgrid[:37, :53]
    crops = [rng.random((23, 41)) < 0.7,
             ((yy - 18) ** 2 + (xx - 26) ** 2 < 200).astype(np.uint8) * 255,
             (np.abs(yy[:9, :31] - 4) < 2).astype(np.uint8)]
    m = MZ.measure_masks([crops[0], torch.from_numpy(crops[1]).to(dev), crops[2]], device=dev)
    for mb in (0.0, 4.5):
        assert_matches_ref(MZ.skeleton_graph(m, mb), [np.asarray(c != 0, np.uint8) for c in crops], mb)

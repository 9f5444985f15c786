"""Instance shape on the GPU: csrc/shape.hip through ``measure.instance_shapes`` / ``shape_arena`` / ``shape_masks`` against the
numpy definition (tests/shape_ref.py).  The three tables and the part labels are integers: equality.  The derived float64 columns
come from those integers by the same expressions on the host: equality too, bit for bit."""
import numpy as np
import pytest
import torch

import measure_ref as MR
import shape_ref as S
import tiles_ref as TLR
from disyolo_amd import lib as L
from disyolo_amd import measure as MZ
from disyolo_amd import tiles as TL

pytestmark = pytest.mark.gpu

_REF = {}
SENT = -7                               # what the label arena holds before a call


def ref(M, K=180, **kw):
    """the definition's answer for a crop, computed once per (crop, K, options)"""
    M = np.asarray(M)
    key = (M.shape, np.asarray(M != 0).tobytes(), K, tuple(sorted(kw.items())))
    if key not in _REF:
        _REF[key] = S.shape(M, K, **kw)
    return _REF[key]


def crops_by_name():
    c = {n: v[0] for n, v in MR.known_crops().items()}
    c.update(S.extra_crops())
    return c


def known_set():
    """every crop with a known answer and one more 1x1; crops whose area is no multiple of 16 first: their neighbours in the
    arena start behind padding bytes"""
    crops = list(crops_by_name().values()) + [np.ones((1, 1), np.uint8)]
    return sorted(crops, key=lambda c: (c.size % 16 == 0, c.size))


def run(dev, crops, K=180, fill=0, foreground=1, **kw):
    groups, arena, nbytes = MZ.pack_masks(crops, fill=fill, foreground=foreground)
    arena = torch.from_numpy(arena).to(dev)
    before = arena.clone()
    labels = torch.full((max(nbytes, 1),), SENT, dtype=torch.int32, device=dev)
    s = MZ.shape_arena(groups, arena, nbytes, None, K, labels_out=labels, **kw)
    assert torch.equal(arena, before), "the arena is only read"
    return s, groups, nbytes


def same_float(a, b, what):
    assert np.float64(a).tobytes() == np.float64(b).tobytes(), "%s: %r != %r" % (what, a, b)


def assert_matches_ref(s, crops, K=180, origins=None, **kw):
    assert len(s) == len(crops) and s.sums.dtype == np.int64 and s.parts.dtype == np.int64 and s.pminmax.dtype == np.int32
    assert s.sums.shape == (len(crops), 16) and s.parts.shape == (len(crops), 2) and s.pminmax.shape == (len(crops), K, 2)
    for i, M in enumerate(crops):
        o = (0, 0) if origins is None else origins[i]
        want = ref(M, K, origin=o, **kw)
        np.testing.assert_array_equal(s.sums[i], want["sums"], err_msg="sums of crop %d" % i)
        np.testing.assert_array_equal(s.parts[i], want["parts"], err_msg="parts of crop %d" % i)
        np.testing.assert_array_equal(s.pminmax[i], want["pminmax"], err_msg="pminmax of crop %d" % i)
        lab = s.part_labels(i)
        assert lab.dtype == torch.int32 and lab.is_cuda and tuple(lab.shape) == np.asarray(M).shape
        np.testing.assert_array_equal(lab.cpu().numpy(), want["labels"], err_msg="labels of crop %d" % i)
        for c in MZ.SHAPE_INTS:
            assert int(getattr(s, c)[i]) == want[c], "%s of crop %d" % (c, i)
        for c in s._floats:
            same_float(getattr(s, c)[i], want[c], "%s of crop %d" % (c, i))
        assert s.rect_corners(i).tobytes() == want["rect_corners"].tobytes() and s.rect_center[i].tobytes() == want["rect_center"].tobytes()
        assert s.extents(i).tobytes() == (want["ext"] / 16384.0).tobytes()
        if "axis_deg" in kw:
            assert s.direction[i] == want["direction"]


def same_bits(a, b):
    assert len(a) == len(b) and all(torch.equal(a.part_labels(i), b.part_labels(i)) for i in range(len(a)))
    assert a.sums.tobytes() == b.sums.tobytes() and a.parts.tobytes() == b.parts.tobytes() and a.pminmax.tobytes() == b.pminmax.tobytes()
    for c in a._floats:
        assert getattr(a, c).tobytes() == getattr(b, c).tobytes(), c


def padding_of(groups, crops, nbytes):
    pad = np.ones(nbytes, bool)
    for gr, c in zip(groups, crops):
        pad[int(gr[7]) * 16:int(gr[7]) * 16 + c.size] = False
    return pad


# ------------------------------------------------------------------------------------------------ the known answers
def test_known_answers_in_one_arena(dev):
    crops = known_set()
    assert any(c.size % 16 for c in crops[:-1])
    a, groups, nbytes = run(dev, crops, fill=0xFF, foreground=0x80, mm_per_px=0.25, axis_deg=30.0)
    assert_matches_ref(a, crops, mm_per_px=0.25, axis_deg=30.0)
    names = crops_by_name()
    at = {n: next(i for i, c in enumerate(crops) if c.shape == M.shape and (c == M).all()) for n, M in names.items()}
    for name, (n, q, e8, edges, (n_parts, largest, holes), (e0, e90), rect, orient) in S.known_shapes().items():
        i = at[name]
        assert int(a.sums[i, 0]) == n and tuple(a.sums[i, 10:15].tolist()) == q and (a.euler8[i], a.edges[i]) == (e8, edges)
        assert (a.n_parts[i], a.largest_part_px[i], a.n_holes[i]) == (n_parts, largest, holes)
        ext = MZ.shape_ext(a.pminmax[i], a.directions)
        assert (int(ext[0]), int(ext[90])) == (e0, e90)
        if rect is not None and n:
            assert (int(a.rect_k[i]), int(ext[a.rect_k[i]]), int(ext[a.rect_k[i] + 90])) == rect
        assert abs(a.orientation_deg[i] - orient) < 1e-3
    assert a.direction[at["bar30"]] == "longitudinal" and a.direction[at["2x2"]] == "none" and a.direction[at["zeros3x5"]] == "none"
    pad = padding_of(groups, crops, nbytes)
    assert pad.sum() > 0 and (a.labels_arena.cpu().numpy()[:nbytes][pad] == SENT).all()       # between two crops: untouched
    b, _, _ = run(dev, crops, fill=0xFF, foreground=0x80, mm_per_px=0.25, axis_deg=30.0)
    same_bits(a, b)                                                                    # the same call again: the same bits
    c, _, _ = run(dev, crops, mm_per_px=0.25, axis_deg=30.0)                                   # the padding and the byte value: not read
    same_bits(a, c)


@pytest.mark.parametrize("K", [2, 4, 36, 360])
def test_other_direction_counts_on_bar30(dev, K):
    crops = [S.bar30(), np.ones((1, 9), np.uint8)]
    s, _, _ = run(dev, crops, K)
    assert_matches_ref(s, crops, K)
    if K in S.BAR30_RECTS:
        ext = MZ.shape_ext(s.pminmax[0], s.directions)
        assert (int(s.rect_k[0]), int(ext[s.rect_k[0]]), int(ext[s.rect_k[0] + K // 2])) == S.BAR30_RECTS[K]


# ------------------------------------------------------------------------------------------------ chunk boundaries
def serpentine():
    M = np.zeros((5, 1030), np.uint8)
    M[0::2, :] = 1
    M[1, 1029] = M[3, 0] = 1
    return M


def frame():
    M = np.ones((70, 300), np.uint8)
    M[1:-1, 1:-1] = 0
    return M


def test_chunk_boundaries(dev):
    yy, xx = np.mgrid[:33, :33]
    crops = [np.ones((3, 1030), np.uint8), serpentine(), ((yy + xx) % 2 == 0).astype(np.uint8), frame(), np.ones((1030, 1), np.uint8)]
    assert all(c.size > L.COMPOSE_CHUNK for c in crops) and crops[0].shape[1] > L.COMPOSE_CHUNK
    s, groups, nbytes = run(dev, crops, mm_per_px=0.5)
    assert_matches_ref(s, crops, mm_per_px=0.5)
    serp = s.part_labels(1).cpu().numpy()
    assert s.n_parts[1] == 1 and s.largest_part_px[1] == 3 * 1030 + 2 and (serp[serpentine() != 0] == 0).all()
    # under 8-connectivity the checkerboard is one part of 545 pixels, every one of its unions diagonal; the 480 gaps off its border are holes
    assert (s.n_parts[2], s.largest_part_px[2], s.n_holes[2], s.sums[2, 14]) == (1, 545, 480, 32 * 32)
    assert (s.n_parts[3], s.n_holes[3], s.area_px[3]) == (1, 1, 2 * 300 + 2 * 68)
    assert (s.rect_long_px[3], s.rect_short_px[3], s.rect_angle_deg[3]) == (300.0, 70.0, 0.0)
    assert (s.rect_long_px[4], s.rect_short_px[4], s.rect_angle_deg[4], s.orientation_deg[4]) == (1030.0, 1.0, 90.0, 90.0)
    pad = padding_of(groups, crops, nbytes)
    assert (s.labels_arena.cpu().numpy()[:nbytes][pad] == SENT).all()


def test_many_parts_and_long_chains(dev):
    rng = np.random.default_rng(4)
    yy, xx = np.mgrid[:90, :90]
    crops = [rng.random((45, 77)) < 0.35, (rng.random((31, 130)) < 0.5).astype(np.uint8) * 255, ((yy - 44) ** 2 + (xx - 44) ** 2 < 43 ** 2)]
    s, _, _ = run(dev, crops, 36)
    assert_matches_ref(s, crops, 36)
    assert s.n_parts[0] > 50 and s.n_holes[1] > 10 and s.n_parts[2] == 1 and s.largest_part_px[2] == s.area_px[2] > 5 * L.COMPOSE_CHUNK


# ------------------------------------------------------------------------------------------------ int64 and int32 range
def test_the_longest_bar_and_its_transpose(dev):
    w = MZ.MAX_SIDE
    crops = [np.ones((1, w), np.uint8), np.ones((w, 1), np.uint8)]
    s, _, _ = run(dev, crops)
    assert_matches_ref(s, crops)
    sxx = (w - 1) * w * (2 * w - 1) // 6
    assert sxx == 11726513487871 > 1 << 32 and s.sums[0, 4] == sxx == s.sums[1, 3] and s.sums[0, 3] == 0 == s.sums[1, 4]
    d = s.directions.astype(np.int64)
    assert s.pminmax[0, 0].tolist() == [0, 16384 * 32766] and s.pminmax[1, 90].tolist() == [0, 16384 * 32766]
    np.testing.assert_array_equal(MZ.shape_ext(s.pminmax[0], d), np.abs(d[:, 0]) * w + np.abs(d[:, 1]))
    np.testing.assert_array_equal(MZ.shape_ext(s.pminmax[1], d), np.abs(d[:, 1]) * w + np.abs(d[:, 0]))
    assert (s.part_labels(0) == 0).all() and (s.part_labels(1) == 0).all() and s.orientation_deg.tolist() == [0.0, 90.0]


# ------------------------------------------------------------------------------------------------ nothing to do, host reads
def counted(monkeypatch):
    calls = {"read": 0}
    read = MZ._shape_read
    monkeypatch.setattr(MZ, "_shape_read", lambda t: (calls.__setitem__("read", calls["read"] + 1), read(t))[1])
    launched = []
    for name in ("shape_sums", "shape_parts", "shape_extents"):
        fn = getattr(L, name)
        monkeypatch.setattr(L, name, lambda *a, _fn=fn, _n=name, **k: (launched.append(_n), _fn(*a, **k))[1])
    return calls, launched


def test_no_groups_empty_boxes_and_the_host_reads(dev, monkeypatch):
    calls, launched = counted(monkeypatch)
    s = MZ.shape_masks([], device=dev)
    assert len(s) == 0 and s.sums.shape == (0, 16) and s.pminmax.shape == (0, 180, 2) and s.table() == [] and s.area_px.shape == (0,)
    sc = TLR.scene()
    res = TL.merge_tiles(sc.tiles, sc.image_hw, sc.net_size, sc.detections, np.zeros_like(sc.keep), torch.from_numpy(sc.masks).to(dev))
    s = MZ.instance_shapes(res, mm_per_px=0.5, axis_deg=10.0)                # a TiledDetections without groups
    assert len(res) == 0 and len(s) == 0 and s.rect_long_mm.shape == (0,) and s.direction == []
    s = MZ.instance_shapes(MZ.measure_masks([], device=dev))
    assert len(s) == 0
    empty = [np.zeros((0, 3), np.uint8), np.zeros((4, 0), np.uint8)]          # empty boxes alone: no block at all
    s = MZ.shape_masks(empty, 36, device=dev)
    assert calls["read"] == 0 and launched == []                              # nothing launched, nothing read
    assert s.sums[:, 6:10].tolist() == [[0, -1, 3, -1], [4, -1, 0, -1]] and (s.pminmax == [2 ** 31 - 1, -2 ** 31]).all()
    assert not s.parts.any() and not s.rect_long_px.any() and s.part_labels(0).shape == (0, 3)
    crops = [np.ones((3, 9), np.uint8), np.zeros((0, 7), np.uint8), np.zeros((4, 5), np.uint8), np.zeros((6, 0), np.uint8), S.two_parts()]
    s, groups, nbytes = run(dev, crops)
    assert calls["read"] == 1 and launched == ["shape_sums", "shape_parts", "shape_extents"]
    assert_matches_ref(s, crops)
    assert (s.pminmax[2] == [2 ** 31 - 1, -2 ** 31]).all() and not s.sums[2, :6].any() and s.sums[2, 6:10].tolist() == [4, -1, 5, -1]
    assert (s.part_labels(2).cpu().numpy() == -1).all() and s.n_parts.tolist() == [1, 0, 0, 0, 2] and s.rect_long_px[2] == 0.0
    calls["read"] = 0
    run(dev, [MR.known_crops()["noise"][0]], 360)
    assert calls["read"] == 1                                                 # whatever the number of parts and directions


# ------------------------------------------------------------------------------------------------ end to end
def test_instance_shapes_on_the_scene(dev, monkeypatch):
    sc = TLR.scene()
    res = TL.merge_tiles(sc.tiles, sc.image_hw, sc.net_size, sc.detections, sc.keep, torch.from_numpy(sc.masks).to(dev))
    assert len(res) == 5
    measure_arena = MZ.measure_arena
    monkeypatch.setattr(MZ, "measure_arena", lambda *a, **k: pytest.fail("instance_shapes of a TiledDetections must not thin"))
    s = MZ.instance_shapes(res, mm_per_px=0.25, axis_deg=0)
    monkeypatch.setattr(MZ, "measure_arena", measure_arena)
    crops = [res.mask(i).cpu().numpy().astype(np.uint8) for i in range(len(res))]
    origins = [(int(b[0]), int(b[1])) for b in res.boxes]
    assert_matches_ref(s, crops, origins=origins, mm_per_px=0.25, axis_deg=0.0)
    np.testing.assert_array_equal(s.boxes, res.boxes)
    np.testing.assert_array_equal(s.rect_long_mm, 0.25 * s.rect_long_px)
    np.testing.assert_array_equal(s.area_mm2, s.area_px * (0.25 * 0.25))
    names = ["crack", "spall", "rebar"]
    rows = s.table(names)
    for i, row in enumerate(rows):
        y1, x1, y2, x2 = row["box"]
        assert row["instance"] == i and row["class"] == names[int(res.classid[i])] and row["score"] == float(res.score[i])
        assert row["direction"] in ("longitudinal", "transverse", "diagonal", "none") and row["area_px"] == int(crops[i].sum())
        assert row["rect_short_px"] <= row["rect_long_px"] <= row["feret_max_px"] and row["feret_min_px"] <= row["rect_short_px"]
        assert row["rect_area_px2"] <= (y2 - y1) * (x2 - x1) and 0 < row["solidity_rect"] <= 1.0     # (k = 0 is the tight box)
        np.testing.assert_allclose(s.rect_corners(i).mean(axis=0), row["rect_center_yx"], rtol=0, atol=1e-9)
    # the same numbers whatever the shapes are asked of
    m = MZ.measure_instances(res, mm_per_px=0.25)
    via = MZ.instance_shapes(m, axis_deg=0)
    assert via.mm_per_px == 0.25 and via.table(names) == rows
    same_bits(s, via)
    g = MZ.skeleton_graph(m, 10.0)
    assert MZ.instance_shapes(g, axis_deg=0).table(names) == rows and MZ.instance_shapes(MZ.skeleton_trace(g), axis_deg=0).table(names) == rows
    assert "rect_long_mm" not in MZ.instance_shapes(res).table()[0] and MZ.instance_shapes(res, mm_per_px=2.0).rect_long_mm[0] == 2.0 * s.rect_long_px[0]


def test_shape_masks_of_masks_of_different_sizes(dev):
    rng = np.random.default_rng(3)
    yy, xx = np.mgrid[:37, :53]
    crops = [rng.random((23, 41)) < 0.7,
             ((yy - 18) ** 2 + (xx - 26) ** 2 < 200).astype(np.uint8) * 255,
             (np.abs(yy[:9, :31] - 4) < 2).astype(np.uint8)]
    s = MZ.shape_masks([crops[0], torch.from_numpy(crops[1]).to(dev), crops[2]], 36, mm_per_px=0.5, axis_deg=90.0, device=dev)
    assert_matches_ref(s, [np.asarray(c != 0, np.uint8) for c in crops], 36, mm_per_px=0.5, axis_deg=90.0)
    assert s.direction[2] == "transverse" and s.classid is None and "class" not in s.table()[0]

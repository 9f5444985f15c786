"""Instance outlines on the GPU: csrc/outline.hip through ``measure.instance_outlines`` / ``outline_masks`` against the definition
(tests/outline_ref.py).  Everything is an integer: equality, of the loop table, the points, the corners and the parts."""
import numpy as np
import pytest
import torch

import measure_ref as MR
import outline_ref as R
import shape_ref as S
import tiles_ref as TLR
from disyolo_amd import lib as L
from disyolo_amd import measure as MZ
from disyolo_amd import tiles as TL
from disyolo_amd import train_data as TD

pytestmark = pytest.mark.gpu

_REF = {}
SENT = -7


def ref(M, origin=(0, 0)):
    """the definition's answer for a crop, computed once (its comparison with the oracle is tests/test_outline.py's)"""
    M = np.asarray(M)
    key = (M.shape, np.asarray(M != 0).tobytes(), tuple(origin))
    if key not in _REF:
        _REF[key] = R.outline(M, origin=origin, oracle=False)
    return _REF[key]


def known_set():
    """the crops with known outlines and those with known shapes; crops whose area is no multiple of 16 first: their neighbours
    in the arena start behind padding bytes"""
    crops = list(R.known_crops().values()) + [v[0] for v in MR.known_crops().values()] + list(S.extra_crops().values())
    return sorted(crops, key=lambda c: (c.size % 16 == 0, c.size))


def shapes(dev, crops, fill=0, foreground=1, origins=None):
    groups, arena, nbytes = MZ.pack_masks(crops, fill=fill, foreground=foreground)
    if origins is not None:
        groups = groups.copy()
        for gr, (oy, ox) in zip(groups, origins):
            gr[2], gr[4], gr[3], gr[5] = gr[2] + oy, gr[4] + oy, gr[3] + ox, gr[5] + ox
    arena = torch.from_numpy(arena).to(dev)
    return MZ.shape_arena(groups, arena, nbytes, None, 2), arena


def assert_matches_ref(o, crops, origins=None):
    assert len(o) == len(crops) and o.loops.dtype == np.int64 and o.loops.shape[1] == 11
    at = 0
    for g, M in enumerate(crops):
        org = (0, 0) if origins is None else origins[g]
        want = ref(M, org)
        t = want["table"].copy()
        t[:, 0], t[:, 3] = g, np.where(t[:, 3] >= 0, t[:, 3] + at, -1)
        np.testing.assert_array_equal(o.loops_of(g), t, err_msg="loops of crop %d" % g)
        a, b = int(o.point_offsets[at]), int(o.point_offsets[at + len(t)])
        np.testing.assert_array_equal(o._points[a:b], want["points"], err_msg="points of crop %d" % g)
        a, b = int(o.corner_offsets[at]), int(o.corner_offsets[at + len(t)])
        np.testing.assert_array_equal(o._corners[a:b], want["corners"], err_msg="corners of crop %d" % g)
        np.testing.assert_array_equal(o.parts[o.parts[:, 0] == g][:, 1:], want["parts"], err_msg="parts of crop %d" % g)
        if len(t):
            assert o.points(at).dtype == np.int32 and np.array_equal(o.points(at), want["loops"][0]["chain"] + [org[1], org[0]])
            assert o.corners(at).dtype == np.int32 and np.array_equal(o.corners(at + len(t) - 1), want["loops"][-1]["ring"] + [org[1], org[0]])
        at += len(t)
    assert at == len(o.loops) and o.points_dev.is_cuda and o.points_dev.dtype == torch.int32
    np.testing.assert_array_equal(o.points_dev.cpu().numpy(), o._points)
    np.testing.assert_array_equal(o.corners_dev.cpu().numpy(), o._corners)


def same_bits(a, b):
    assert a.loops.tobytes() == b.loops.tobytes() and a._points.tobytes() == b._points.tobytes() and a._corners.tobytes() == b._corners.tobytes()
    assert a.parts.tobytes() == b.parts.tobytes()


def round_trip(o, crops, dev, origins=None):
    for g, M in enumerate(crops):
        bh, bw = np.asarray(M).shape
        if max(bh, bw) > 2048 or bh * bw == 0:
            continue
        oy, ox = (0, 0) if origins is None else origins[g]
        back = TD.rasterize_instance(o.polygons(g), bh, bw, dev, origin=(ox, oy))
        assert torch.equal(back != 0, torch.from_numpy(np.asarray(M) != 0).to(dev)), "crop %d drawn from its outline" % g


# ------------------------------------------------------------------------------------------------ the main arena
def test_known_outlines_in_one_arena(dev):
    crops = known_set()
    origins = [(3 * i, 1000 - 7 * i) for i in range(len(crops))]
    assert any(c.size % 16 for c in crops[:-1])
    s, arena = shapes(dev, crops, fill=0xFF, foreground=0x80, origins=origins)
    before = arena.clone()
    a = MZ.instance_outlines(s)
    assert torch.equal(arena, before), "the arena is only read"
    assert_matches_ref(a, crops, origins)
    round_trip(a, crops, dev, origins)
    # the rows the issue names, by their crop
    for name, rows in R.known_rows().items():
        M = R.known_crops()[name]
        g = next(i for i, c in enumerate(crops) if c.shape == M.shape and (c == M).all())
        assert [tuple(int(v) for v in r[[5, 6, 7, 10, 8]]) for r in a.loops_of(g)] == rows, name
    b = MZ.instance_outlines(s)                                       # the same call again: the same bits
    same_bits(a, b)
    plain, _ = shapes(dev, crops, origins=origins)                    # the padding and the byte value: not read
    same_bits(a, MZ.instance_outlines(plain))


def test_the_per_pixel_buffers_between_two_crops_stay_untouched(dev):
    crops = known_set()
    s, arena = shapes(dev, crops, fill=0xFF, foreground=0x80)
    nbytes, E = s.arena_bytes, int(s.edges.sum())
    first = torch.full((nbytes,), SENT, dtype=torch.int32, device=dev)
    sides = torch.full((nbytes,), 0xEE, dtype=torch.uint8, device=dev)
    i32 = lambda *sh: torch.empty(*sh, dtype=torch.int32, device=dev)
    ekey, nxt, aterm, flag, ctrl = i32(E), i32(E), i32(E), torch.empty(E, dtype=torch.uint8, device=dev), i32(4)
    work = torch.empty(L.OUTLINE_WORK * E, dtype=torch.int64, device=dev)
    L.outline_edges(s.groups, arena, first, sides, ekey, nxt, flag, aterm, work, ctrl, s.groups_dev, nbytes)
    pad = np.ones(nbytes, bool)
    inside = []
    for gr, c in zip(s.groups, crops):
        pad[int(gr[7]) * 16:int(gr[7]) * 16 + c.size] = False
        inside.append(np.asarray(c).reshape(-1) != 0)
    assert pad.sum() > 0 and (first.cpu().numpy()[pad] == SENT).all() and (sides.cpu().numpy()[pad] == 0xEE).all()
    assert ctrl.cpu().tolist() == [E, 0, 0, 0]
    # inside the crops: the side mask is that of the definition's edges, and a pixel's entries stand in a row
    keys = np.sort(ekey.cpu().numpy().astype(np.int64))
    want = np.concatenate([R.boundary_keys(np.asarray(c) != 0) + 4 * int(gr[7]) * 16 for gr, c in zip(s.groups, crops)])
    np.testing.assert_array_equal(keys, np.sort(want))
    nx = nxt.cpu().numpy()
    assert np.array_equal(np.sort(nx), np.arange(E))                  # the successor is a permutation of the list
    small = torch.empty(E - 1, dtype=torch.int32, device=dev)         # a list that is too short: reported, nothing faults
    L.outline_edges(s.groups, arena, first, sides, small, nxt, flag, aterm, work, ctrl, s.groups_dev, nbytes)
    c = ctrl.cpu().tolist()
    assert c[0] == E and c[2] & 1
    with pytest.raises(L.DisyoloError, match="work"):
        L.outline_edges(s.groups, arena, first, sides, ekey, nxt, flag, aterm, work[:-1], ctrl, s.groups_dev, nbytes)


# ------------------------------------------------------------------------------------------------ chunks and lengths
def serpentine(rows=5):
    M = np.zeros((rows, 1030), np.uint8)
    M[0::2, :] = 1
    M[1::4, 1029] = M[3::4, 0] = 1
    return M


def test_chunk_boundaries_and_long_loops(dev):
    yy, xx = np.mgrid[:90, :90]
    dots = np.zeros((20, 40), np.uint8)
    dots[::2, ::2] = 1
    crops = [np.ones((3, 1030), np.uint8), serpentine(), np.ones((1030, 1), np.uint8), ((yy - 44) ** 2 + (xx - 44) ** 2 < 43 ** 2), dots,
             serpentine(9)]
    assert all(c.size > L.COMPOSE_CHUNK for c in crops[:4])
    s, _ = shapes(dev, crops)
    o = MZ.instance_outlines(s)
    assert_matches_ref(o, crops)
    round_trip(o, crops, dev)
    # one loop across the chunks: the ranking rounds matter.  The 5-row serpentine has 6186 edges; the 9-row one passes 10 000
    serp, long = o.loops_of(1), o.loops_of(5)
    assert len(serp) == 1 and serp[0, 7] == 6186 == s.edges[1] and serp[0, 10] == 2 * (3 * 1030 + 2)
    assert len(long) == 1 and long[0, 7] > 10000 and long[0, 10] == 2 * (5 * 1030 + 4)
    assert len(o.loops_of(4)) == 200 and (o.loops_of(4)[:, 7:10] == [4, 1, 4]).all() and len(o.parts[o.parts[:, 0] == 4]) == 200
    assert len(o.loops_of(3)) == 1 and o.loops_of(3)[0, 10] == 2 * int(crops[3].sum()) > 10 * L.COMPOSE_CHUNK


def test_the_longest_bar_and_its_transpose(dev):
    w = MZ.MAX_SIDE
    crops = [np.ones((1, w), np.uint8), np.ones((w, 1), np.uint8)]
    s, _ = shapes(dev, crops)
    o = MZ.instance_outlines(s)
    assert_matches_ref(o, crops)
    assert o.loops[:, 7].tolist() == [2 * w + 2] * 2 and o.loops[:, 8].tolist() == [2 * w - 2] * 2 and o.loops[:, 10].tolist() == [2 * w] * 2
    assert o.corners(0).tolist() == [[0, 0], [w, 0], [w, 1], [0, 1]] and o.corners(1).tolist() == [[0, 0], [1, 0], [1, w], [0, w]]
    assert o.points(0)[:3].tolist() == [[0, 0], [1, 0], [2, 0]] and o.points(1)[:3].tolist() == [[0, 0], [0, 1], [0, 2]]


# ------------------------------------------------------------------------------------------------ nothing to do, host reads
def counted(monkeypatch):
    calls = {"read": 0}
    read = MZ._outline_read
    monkeypatch.setattr(MZ, "_outline_read", lambda t: (calls.__setitem__("read", calls["read"] + 1), read(t))[1])
    launched = []
    for name in ("outline_edges", "outline_loops", "outline_gather"):
        fn = getattr(L, name)
        monkeypatch.setattr(L, name, lambda *a, _fn=fn, _n=name, **k: (launched.append(_n), _fn(*a, **k))[1])
    return calls, launched


def test_no_groups_empty_boxes_and_the_host_reads(dev, monkeypatch):
    calls, launched = counted(monkeypatch)
    o = MZ.outline_masks([], device=dev)
    assert len(o) == 0 and o.loops.shape == (0, 11) and o.table() == [] and o.record(image_size=(4, 4))["polygons"] == []
    sc = TLR.scene()
    res = TL.merge_tiles(sc.tiles, sc.image_hw, sc.net_size, sc.detections, np.zeros_like(sc.keep), torch.from_numpy(sc.masks).to(dev))
    o = MZ.instance_outlines(res)                                             # a TiledDetections without groups
    assert len(res) == 0 and len(o) == 0 and o.parts.shape == (0, 4)
    empty = [np.zeros((0, 3), np.uint8), np.zeros((4, 0), np.uint8)]          # empty boxes alone: no block at all
    o = MZ.outline_masks(empty, device=dev)
    assert len(o) == 2 and len(o.loops) == 0 and o.polygons(1) == []
    o = MZ.outline_masks([np.zeros((4, 5), np.uint8)], device=dev)            # background alone: no edge
    assert len(o.loops) == 0 and o._points.shape == (0, 2) and o.polygons(0) == []
    assert calls["read"] == 0 and launched == []                              # nothing launched, nothing read
    crops = [np.ones((3, 9), np.uint8), np.zeros((0, 7), np.uint8), np.zeros((4, 5), np.uint8), np.zeros((6, 0), np.uint8), S.two_parts()]
    s, _ = shapes(dev, crops)
    o = MZ.instance_outlines(s)
    assert calls["read"] == 2 and launched == ["outline_edges", "outline_loops", "outline_gather"]
    assert_matches_ref(o, crops)
    assert [len(o.loops_of(g)) for g in range(5)] == [1, 0, 0, 0, 3] and o.polygons(2) == []
    assert len(o.record(image_size=(9, 9))["polygons"]) == 2                   # the instances with a border
    calls["read"] = 0
    del launched[:]
    t = MZ.instance_outlines(s, points=False)
    assert calls["read"] == 1 and launched == ["outline_edges", "outline_loops"] and t.points_dev is None
    np.testing.assert_array_equal(t.loops, o.loops)
    np.testing.assert_array_equal(t.parts, o.parts)
    with pytest.raises(ValueError, match="points=False"):
        t.points(0)


def test_a_loop_table_that_does_not_fit_the_shapes_is_refused(dev):
    crops = [R.nest11(), S.two_parts()]
    s, _ = shapes(dev, crops)
    s.n_holes = s.n_holes.copy()
    s.n_holes[0] += 1                                                         # one row too many: the count differs
    with pytest.raises(L.DisyoloError, match="loop table"):
        MZ.instance_outlines(s)
    s, _ = shapes(dev, crops)
    s.n_parts, s.n_holes = s.n_parts.copy(), s.n_holes.copy()
    s.n_parts[0], s.n_holes[0] = 3, 1                                         # the count holds, the kinds per instance do not
    with pytest.raises(L.DisyoloError, match="loop table"):
        MZ.instance_outlines(s)
    s, _ = shapes(dev, crops)
    s.area_px = s.area_px + 1
    with pytest.raises(L.DisyoloError, match="loop table"):
        MZ.instance_outlines(s)


# ------------------------------------------------------------------------------------------------ end to end
def test_instance_outlines_on_the_scene(dev):
    sc = TLR.scene()
    res = TL.merge_tiles(sc.tiles, sc.image_hw, sc.net_size, sc.detections, sc.keep, torch.from_numpy(sc.masks).to(dev))
    assert len(res) == 5
    o = MZ.instance_outlines(res)
    crops = [res.mask(i).cpu().numpy().astype(np.uint8) for i in range(len(res))]
    origins = [(int(b[0]), int(b[1])) for b in res.boxes]
    assert_matches_ref(o, crops, origins)
    round_trip(o, crops, dev, origins)
    via = MZ.instance_outlines(MZ.instance_shapes(res))
    same_bits(o, via)
    names = ["crack", "spall", "rebar"]
    rows = o.table(names)
    assert len(rows) == len(o.loops) and rows[0]["class"] == names[int(res.classid[0])] and rows[0]["kind"] == "outer"
    h, w = sc.image_hw
    rec = o.record(image_size=(h, w), class_names=names)
    assert rec["image_size"] == (h, w) and rec["class_names"] == [names[int(k)] for k in res.classid] and len(rec["polygons"]) == 5
    boxes = TD.letterbox_boxes([rec], 64)                                     # the loader's helpers take the record as it is
    assert boxes.shape[0] == 5
    # one batch of the loader from the record: it draws every instance back to its mask
    image = np.zeros((h, w, 3), np.uint8)
    rec = o.record(image=image, class_names=names)
    data = TD.defect_train([rec], batch_size=1, image_size=(160, 224), device=dev, rng=np.random.RandomState(0), flipped=False,
                           blur_noise_light=False, classes=names)
    images, masks, tboxes = data.get()[:3]
    torch.cuda.synchronize()
    assert images.shape == (1, 160, 224, 3) and tboxes.shape[:5] == (1, 1, 1, 1, masks.shape[1])
    assert 1 <= int(masks[0].flatten(1).any(dim=1).sum()) <= 5                # (the placement may move an instance out of the frame)
    for g in range(5):
        full = TD.rasterize_instance(rec["polygons"][g], h, w, dev)
        y1, x1, y2, x2 = (int(v) for v in res.boxes[g])
        assert torch.equal(full[y1:y2, x1:x2] != 0, res.mask(g) != 0) and int(full.sum()) == int(res.mask(g).sum())


def test_outline_masks_of_masks_of_different_sizes(dev):
    rng = np.random.default_rng(3)
    yy, xx = np.mgrid[:37, :53]
    crops = [rng.random((23, 41)) < 0.7,
             ((yy - 18) ** 2 + (xx - 26) ** 2 < 200).astype(np.uint8) * 255,
             (np.abs(yy[:9, :31] - 4) < 2).astype(np.uint8)]
    o = MZ.outline_masks([crops[0], torch.from_numpy(crops[1]).to(dev), crops[2]], device=dev)
    assert_matches_ref(o, [np.asarray(c != 0, np.uint8) for c in crops])
    round_trip(o, crops, dev)
    assert o.classid is None and "class" not in o.table()[0] and o.record(image_size=(40, 60))["class_names"] == ["crack"] * 3

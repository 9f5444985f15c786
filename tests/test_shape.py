"""Instance shape without a GPU: the numpy definition (tests/shape_ref.py) against its known answers, its invariants and its
symmetries; ``measure.derive_shape`` against the definition's ``derive`` bit for bit; the direction kinds; the ValueErrors of
``measure.instance_shapes``; and the argument checks of the three entry points of csrc/shape.hip, which come before any launch."""
import ctypes
import math

import numpy as np
import pytest
import scipy.ndimage

import measure_ref as MR
import shape_ref as S
from disyolo_amd import lib as L
from disyolo_amd import measure as MZ


def crops_by_name():
    c = {n: v[0] for n, v in MR.known_crops().items()}
    c.update(S.extra_crops())
    return c


CROPS = crops_by_name()
_SHAPES = {}


def shape_of(name, K=180):
    if (name, K) not in _SHAPES:
        _SHAPES[(name, K)] = S.shape(CROPS[name], K)
    return _SHAPES[(name, K)]


# ------------------------------------------------------------------------------------------------ the known answers
@pytest.mark.parametrize("name", sorted(S.known_shapes()))
def test_known_answers(name):
    n, q, e8, edges, (n_parts, largest, holes), (e0, e90), rect, orient = S.known_shapes()[name]
    r = shape_of(name)
    s = r["sums"]
    assert int(s[0]) == n == r["area_px"] and tuple(int(v) for v in s[10:15]) == q and int(s[15]) == 0
    assert (r["euler8"], r["edges"]) == (e8, edges)
    assert (r["n_parts"], r["largest_part_px"], r["n_holes"]) == (n_parts, largest, holes)
    assert (int(r["ext"][0]), int(r["ext"][90])) == (e0, e90)
    if rect is not None and n:
        k = r["rect_k"]
        assert (k, int(r["ext"][k]), int(r["ext"][k + 90])) == rect
    assert abs(r["orientation_deg"] - orient) < 1e-3
    if n == 0:
        assert s[6:10].tolist() == [3, -1, 5, -1] and (r["pminmax"] == [S.INT32_MAX, S.INT32_MIN]).all()
        assert all(r[c] == 0 for c in MZ.SHAPE_FLOATS) and not r["rect_corners"].any()


def test_known_answers_in_words():
    assert S.directions(4).tolist() == [[16384, 0], [11585, 11585], [0, 16384], [-11585, 11585]]
    for K, want in S.BAR30_RECTS.items():
        r = shape_of("bar30", K)
        k = r["rect_k"]
        assert (k, int(r["ext"][k]), int(r["ext"][k + K // 2])) == want
    bar = shape_of("1x9")
    assert round(bar["feret_max_px"], 2) == 9.06 and bar["feret_max_deg"] == 6.0 and bar["feret_min_px"] == 1.0
    assert (bar["rect_long_px"], bar["rect_short_px"], bar["rect_angle_deg"], bar["rect_area_px2"], bar["solidity_rect"]) == (9, 1, 0, 9, 1)
    np.testing.assert_array_equal(bar["rect_corners"], [[-0.5, -0.5], [-0.5, 8.5], [0.5, 8.5], [0.5, -0.5]])
    np.testing.assert_array_equal(bar["rect_center"], [0.0, 4.0])
    assert bar["perimeter_px"] == 16 + 4 / math.sqrt(2.0) and bar["centroid_x"] == 4.0 and bar["centroid_y"] == 0.0
    eye = shape_of("eye9")
    assert eye["rect_angle_deg"] == 45.0 and abs(eye["rect_long_px"] - 9 * math.sqrt(2.0)) < 1e-3
    b30 = shape_of("bar30")
    assert b30["rect_angle_deg"] == 30.0 and abs(b30["rect_long_px"] - 121.4) < 0.1 and abs(b30["rect_short_px"] - 21.4) < 0.1
    assert abs(b30["axis_major_px"] / b30["axis_minor_px"] - b30["elongation"]) < 1e-9 and 5.0 < b30["elongation"] < 6.5
    sq = shape_of("2x2")
    assert sq["elongation"] == 1.0 and sq["orientation_deg"] == 0.0 and abs(sq["axis_major_px"] - 4 / math.sqrt(3.0)) < 1e-12
    moved = S.shape(CROPS["1x9"], origin=(100, 200))
    np.testing.assert_array_equal(moved["rect_center"], [100.0, 204.0])
    # a diagonal gap closes a hole's wall but does not join two holes
    assert shape_of("checker4")["n_holes"] == 2 and shape_of("ring3")["n_holes"] == 1 and shape_of("two_parts")["n_holes"] == 1


# ------------------------------------------------------------------------------------------------ invariants
def check_invariants(M, K=36):
    r = S.shape(M, K)        # (asserts the area from the quads, the edges against a direct count, the holes against the
    s = r["sums"]            # background labelling, and the boundary-only extents against the all-pixel ones)
    F = np.asarray(M) != 0
    assert int(s[0]) == int(F.sum())
    assert r["edges"] == S.edges_direct(F) and r["n_holes"] == S.holes_direct(F)
    np.testing.assert_array_equal(r["pminmax"], S._pminmax(S.boundary(F), S.directions(K)))
    lab, n = scipy.ndimage.label(F, structure=np.ones((3, 3), int))
    labels = r["labels"]
    assert labels.dtype == np.int32 and n == r["n_parts"] and ((labels >= 0) == F).all()
    idx = np.arange(F.size).reshape(F.shape)
    for i in range(1, n + 1):
        sel = lab == i
        assert (labels[sel] == idx[sel].min()).all()
    assert r["largest_part_px"] == (np.bincount(lab[F]).max() if n else 0)
    if F.any():
        y, x = np.nonzero(F)
        assert s[6:10].tolist() == [y.min(), y.max(), x.min(), x.max()]
        assert (int(s[1]), int(s[2]), int(s[3]), int(s[4]), int(s[5])) == (y.sum(), x.sum(), (y * y).sum(), (x * x).sum(), (x * y).sum())
    return r


@pytest.mark.parametrize("name", sorted(CROPS))
def test_invariants_on_the_known_crops_raw_and_thinned(name):
    check_invariants(CROPS[name])
    check_invariants(MR.thin(CROPS[name])[0])


def test_invariants_on_random_maps():
    rng = np.random.default_rng(11)
    for i in range(200):
        bh, bw = (int(v) for v in rng.integers(1, 41, 2))
        check_invariants(rng.random((bh, bw)) < 0.1 + 0.8 * (i % 9) / 8.0, K=(2, 4, 36)[i % 3])


@pytest.mark.parametrize("w", [1, 2, 9, 1030])
def test_the_extents_of_a_bar_in_closed_form(w):
    for K in (2, 180, 360):
        d = S.directions(K).astype(np.int64)
        r = S.shape(np.ones((1, w), np.uint8), K)
        np.testing.assert_array_equal(r["ext"], np.abs(d[:, 0]) * w + np.abs(d[:, 1]))
        np.testing.assert_array_equal(S.shape(np.ones((w, 1), np.uint8), K)["ext"], np.abs(d[:, 1]) * w + np.abs(d[:, 0]))


# ------------------------------------------------------------------------------------------------ symmetries
def some_maps():
    rng = np.random.default_rng(5)
    return [CROPS[n] for n in ("sinusoid", "bar30", "two_parts", "noise", "eye9", "1x9")] + \
           [rng.random((int(h), int(w))) < 0.5 for h, w in rng.integers(2, 30, (20, 2))]


def test_transposing_swaps_the_axes():
    for M in some_maps():
        a, b = S.shape(M), S.shape(np.ascontiguousarray(np.asarray(M).T))
        sa, sb = a["sums"], b["sums"]
        assert sb[[0, 1, 2, 3, 4, 5]].tolist() == sa[[0, 2, 1, 4, 3, 5]].tolist() and sb[6:10].tolist() == sa[[8, 9, 6, 7]].tolist()
        assert sb[10:15].tolist() == sa[10:15].tolist()
        assert (b["n_parts"], b["largest_part_px"], b["n_holes"]) == (a["n_parts"], a["largest_part_px"], a["n_holes"])
        d = (b["orientation_deg"] - (90.0 - a["orientation_deg"])) % 180.0
        assert min(d, 180.0 - d) < 1e-9 or a["elongation"] < 1.0 + 1e-9


def test_flipping_keeps_quads_parts_and_the_extents_as_a_multiset():
    for M in some_maps():
        a, b = S.shape(M), S.shape(np.ascontiguousarray(np.asarray(M)[:, ::-1]))
        assert b["sums"][10:15].tolist() == a["sums"][10:15].tolist() and b["sums"][[0, 1, 3]].tolist() == a["sums"][[0, 1, 3]].tolist()
        assert (b["n_parts"], b["largest_part_px"], b["n_holes"]) == (a["n_parts"], a["largest_part_px"], a["n_holes"])
        assert sorted(b["ext"].tolist()) == sorted(a["ext"].tolist())
        k = np.arange(1, 180)
        np.testing.assert_array_equal(b["ext"][k], a["ext"][180 - k])        # direction k mirrors to K - k


# ------------------------------------------------------------------------------------------------ the host's derive
def same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k
        elif isinstance(a[k], float):
            assert isinstance(b[k], float) and np.float64(a[k]).tobytes() == np.float64(b[k]).tobytes(), k
        else:
            assert type(a[k]) is type(b[k]) and a[k] == b[k], k


def test_derive_of_measure_py_is_the_definitions_bit_for_bit():
    rng = np.random.default_rng(2)
    maps = [(n, CROPS[n]) for n in sorted(CROPS)] + [("random", rng.random((int(h), int(w))) < 0.6) for h, w in rng.integers(1, 40, (40, 2))]
    for K in (2, 36, 180):
        np.testing.assert_array_equal(MZ.shape_directions(K), S.directions(K))
    assert MZ.SHAPE_COLUMNS == S.COLS and MZ.SHAPE_UNIT == S.Q14 and MZ.SHAPE_LENGTHS == S.LENGTHS
    for i, (name, M) in enumerate(maps):
        K = (180, 36, 2, 360)[i % 4]
        r = S.shape(M, K)
        dirs = S.directions(K)
        np.testing.assert_array_equal(MZ.shape_ext(r["pminmax"], dirs), r["ext"])
        for kw in ({}, dict(origin=(7, 1000), mm_per_px=0.25), dict(mm_per_px=3.0, axis_deg=31.5, axis_tol_deg=10.0, min_elongation=1.0)):
            same(MZ.derive_shape(r["sums"], r["parts"], r["pminmax"], dirs, **kw), S.derive(r["sums"], r["parts"], r["pminmax"], dirs, **kw))
    huge = np.zeros(16, np.int64)          # central moments beyond int64: Python ints until the last step
    n, sq = 32767 * 32767, 32766 * 32767 * 65533 // 6        # a full 32767 x 32767 crop; sq = the sum of x^2 over one row
    huge[:6] = n, n * 16383, n * 16383, 32767 * sq, 32767 * sq, n * 16383 * 16383
    huge[10:15] = 4, 4 * 32766, 0, 32766 * 32766, 0
    dirs = S.directions(4)
    pm = S.extents(np.ones((3, 3), np.uint8), dirs)
    d = MZ.derive_shape(huge, [1, n], pm, dirs)
    same(d, S.derive(huge, [1, n], pm, dirs))
    assert abs(d["axis_major_px"] - 4 * math.sqrt((32767 ** 2 - 1) / 12 + 1 / 12)) < 1e-6 and abs(d["elongation"] - 1.0) < 1e-9


# ------------------------------------------------------------------------------------------------ direction kinds
@pytest.mark.parametrize("name,kinds", [("1x9", ("longitudinal", "diagonal", "transverse")), ("eye9", ("diagonal", "longitudinal", "diagonal")),
                                        ("bar30", ("diagonal", "longitudinal", "diagonal")),
                                        ("ellipse", ("longitudinal", "diagonal", "transverse")), ("2x2", ("none", "none", "none"))])
def test_direction_kinds(name, kinds):
    r = shape_of(name)
    for axis, kind in zip((0.0, 30.0, 90.0), kinds):
        for turn in (0.0, 180.0, -360.0):
            got = MZ.derive_shape(r["sums"], r["parts"], r["pminmax"], S.directions(180), axis_deg=axis + turn)["direction"]
            assert got == kind == S.shape(CROPS[name], axis_deg=axis + turn)["direction"]
    assert "direction" not in r


def test_the_direction_thresholds_are_keyword_arguments():
    assert MZ.direction_kind(22.5, 2.0, 0.0) == "longitudinal" and MZ.direction_kind(22.6, 2.0, 0.0) == "diagonal"
    assert MZ.direction_kind(67.5, 2.0, 0.0) == "transverse" and MZ.direction_kind(67.4, 2.0, 0.0) == "diagonal"
    assert MZ.direction_kind(179.0, 2.0, 0.0) == "longitudinal" and MZ.direction_kind(1.0, 2.0, 179.0) == "longitudinal"
    assert MZ.direction_kind(40.0, 2.0, 0.0, axis_tol_deg=45.0) == "longitudinal" and MZ.direction_kind(50.0, 2.0, 0.0, axis_tol_deg=45.0) == "transverse"
    assert MZ.direction_kind(0.0, 1.49, 0.0) == "none" and MZ.direction_kind(0.0, 1.49, 0.0, min_elongation=1.0) == "longitudinal"


# ------------------------------------------------------------------------------------------------ instance_shapes' ValueErrors
def host_measures():
    """an InstanceMeasures over host tensors: every check below has to come before anything touches a device"""
    import torch
    groups, arena, nbytes = MZ.pack_masks([np.ones((1, 9), np.uint8)])
    m = MZ.InstanceMeasures(groups[:, 2:6], [0], torch.zeros(16, dtype=torch.int32), torch.zeros(16, dtype=torch.uint8),
                            [[9, 9, 8, 0, 2, 1, 1, 0]], [9.0], [1])
    m.groups, m.arena, m.arena_bytes = groups, torch.from_numpy(arena), nbytes
    return m


def test_instance_shapes_refuses_bad_arguments():
    for bad in (0, 1, 3, 179, 362, 180.0, True, "180", None):
        with pytest.raises(ValueError, match="directions"):
            MZ.instance_shapes(host_measures(), directions=bad)
        with pytest.raises(ValueError, match="directions"):
            MZ.shape_masks([np.ones((2, 2), np.uint8)], directions=bad)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="mm_per_px"):
            MZ.instance_shapes(host_measures(), mm_per_px=bad)
    for bad in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="axis_deg"):
            MZ.instance_shapes(host_measures(), axis_deg=bad)
    for bad in (0.0, -1.0, 45.1, float("nan")):
        with pytest.raises(ValueError, match="axis_tol_deg"):
            MZ.instance_shapes(host_measures(), axis_deg=0.0, axis_tol_deg=bad)
    for bad in (0.99, 0.0, float("nan")):
        with pytest.raises(ValueError, match="min_elongation"):
            MZ.instance_shapes(host_measures(), min_elongation=bad)
    with pytest.raises(ValueError, match="TiledDetections"):
        MZ.instance_shapes(np.ones((3, 3)))
    m = host_measures()
    m.groups = None
    with pytest.raises(ValueError, match="measure_arena"):
        MZ.instance_shapes(m)


def test_instance_shapes_from_tables_alone():
    """the class derives its columns from the raw tables: no device is touched"""
    import torch
    names = ["1x9", "bar30", "zeros3x5", "two_parts"]
    ref = [S.shape(CROPS[n], 36, origin=(0, 0), mm_per_px=0.5, axis_deg=0.0) for n in names]
    groups, _, _ = MZ.pack_masks([CROPS[n] for n in names])
    s = MZ.InstanceShapes(groups[:, 2:6], [int(v) * 16 for v in groups[:, 7]], torch.zeros(0, dtype=torch.int32),
                          [r["sums"] for r in ref], [r["parts"] for r in ref], [r["pminmax"] for r in ref], S.directions(36), 0.5, 0.0,
                          classid=np.array([0, 0, 1, 1]), score=np.array([0.9, 0.8, 0.7, 0.6], np.float32))
    assert len(s) == 4 and s.direction == ["longitudinal", "diagonal", "none", "longitudinal"]   # (two_parts lies at 158.8 degrees: 21.2 from the axis) and s.n_holes.tolist() == [0, 0, 0, 1]
    for g, r in enumerate(ref):
        for c in MZ.SHAPE_FLOATS + tuple(x + "_mm" for x in MZ.SHAPE_LENGTHS) + ("area_mm2", "rect_area_mm2"):
            assert np.float64(getattr(s, c)[g]).tobytes() == np.float64(r[c]).tobytes(), c
        np.testing.assert_array_equal(s.rect_corners(g), r["rect_corners"])
        np.testing.assert_array_equal(s.extents(g), r["ext"] / 16384.0)
    rows = s.table(["crack", "spall", "rebar"])
    assert rows[1]["class"] == "crack" and rows[3]["class"] == "spall" and rows[0]["rect_long_mm"] == 4.5 and rows[0]["area_mm2"] == 2.25
    assert rows[3]["n_parts"] == 2 and rows[3]["largest_part_px"] == 8 and rows[2]["perimeter_px"] == 0.0 and rows[0]["instance"] == 0
    assert rows[0]["box"] == (0, 0, 1, 9) and abs(rows[0]["score"] - 0.9) < 1e-6 and rows[1]["direction"] == "diagonal"


# ------------------------------------------------------------------------------------------------ the ABI's argument checks
def groups_table(boxes):
    return L.tile_compose_plan(np.asarray(boxes, np.int32).reshape(-1, 4), np.zeros(len(boxes) + 1, np.int64))


def calls(lib, p, dirs):
    """the three entry points with every buffer pointer p (host memory that a launch would fault on):
    name -> fn(groups_host, groups_dev, G, arena_bytes)"""
    d = np.ascontiguousarray(dirs, dtype=np.int32)
    return {
        "shape_sums": lambda gh, gd, G, nb: lib.disyolo_shape_sums(gh, gd, G, p, nb, p, None),
        "shape_parts": lambda gh, gd, G, nb: lib.disyolo_shape_parts(gh, gd, G, p, nb, p, p, p, None),
        "shape_extents": lambda gh, gd, G, nb: (d, lib.disyolo_shape_extents(gh, gd, G, p, nb, d.ctypes.data, p, len(d), p, None))[1],
    }


@pytest.mark.parametrize("name", ["shape_sums", "shape_parts", "shape_extents"])
def test_shape_entry_points_refuse_bad_arguments_before_any_launch(name):
    lib = L.load()
    buf = ctypes.create_string_buffer(1 << 16)
    p = ctypes.cast(buf, ctypes.c_void_p)
    fn = calls(lib, p, S.directions(180))[name]
    tag = name.encode()

    def run(groups, G=None, nbytes=None, null=False, f=None):
        g = np.ascontiguousarray(groups, dtype=np.int32)
        return (f or fn)(None if null else g.ctypes.data, g.ctypes.data, len(g) if G is None else G, 1 << 16 if nbytes is None else nbytes)

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
    if name == "shape_extents":
        odd = np.concatenate([S.directions(180), [[0, 0]]])
        assert run(good, f=calls(lib, p, odd)[name]) == -1 and b"directions" in lib.disyolo_last_error()
        many = np.concatenate([S.directions(360), [[0, 0], [0, 0]]])
        assert len(many) == 362 and run(good, f=calls(lib, p, many)[name]) == -1 and b"directions" in lib.disyolo_last_error()
        assert run(good, f=calls(lib, p, np.zeros((0, 2)))[name]) == -1 and b"directions" in lib.disyolo_last_error()
        for bad_dir in ([16385, 0], [0, -16385], [1 << 30, 1 << 30]):
            d = S.directions(180).copy()
            d[77] = bad_dir
            assert run(good, f=calls(lib, p, d)[name]) == -1 and b"direction 77" in lib.disyolo_last_error()
        assert lib.disyolo_shape_extents(good.ctypes.data, good.ctypes.data, 2, p, 1 << 16, None, p, 180, p, None) == -1
    # nothing to do is no error: G = 0, with no pointers at all
    assert fn(None, None, 0, 0) == 0

"""Instance outlines without a GPU: the definition (tests/outline_ref.py) against its known answers, against the oracle's contour
tracer and rasteriser (asserted inside ``outline``), its symmetries; the host side of ``measure.instance_outlines`` -- the nesting
rule of ``order_loops`` and the class's tables -- from rows made by the definition; the ValueErrors; and the argument checks of the
three entry points of csrc/outline.hip, which come before any launch."""
import ctypes

import numpy as np
import pytest
import torch

import disyolo_oracle as O
import measure_ref as MR
import outline_ref as R
import shape_ref as S
from disyolo_amd import lib as L
from disyolo_amd import measure as MZ


def rows_of(o):
    return [(l["key_px"], l["key_side"], l["n_edges"], l["area2"], l["n_points"]) for l in o["loops"]]


# ------------------------------------------------------------------------------------------------ the known answers
@pytest.mark.parametrize("name", sorted(R.known_rows()))
def test_known_answers(name):
    o = R.outline(R.known_crops()[name])
    assert rows_of(o) == R.known_rows()[name]
    assert o["table"].dtype == np.int64 and o["points"].dtype == np.int32 and o["corners"].dtype == np.int32
    assert len(o["points"]) == o["table"][:, 8].sum() and len(o["corners"]) == o["table"][:, 9].sum()


def test_known_answers_in_words():
    bar = R.outline(np.ones((1, 3), np.uint8))
    assert bar["points"].tolist() == [[0, 0], [1, 0], [2, 0], [1, 0]]              # pixels 0, 1, 2, 1: reversed from the start
    assert bar["corners"].tolist() == [[0, 0], [3, 0], [3, 1], [0, 1]]
    eye = R.outline(np.eye(3, dtype=np.uint8))
    assert len(eye["loops"]) == 1 and eye["points"].tolist() == [[0, 0], [1, 1], [2, 2], [1, 1]]      # two diagonal links, one loop
    ring = R.outline(R.known_crops()["ring3"])
    assert [l["depth"] for l in ring["loops"]] == [0, 1] and ring["loops"][1]["parent"] == 0
    # (a hole starts at the pixel west of it, the owner of its smallest E side, as cv2's raster scan meets it)
    assert ring["polygons"][1] == {"type": "in", "all_points_x": [0, 1, 2, 1], "all_points_y": [1, 0, 1, 2]}
    assert ring["parts"].tolist() == [[0, 8, 1]]
    nest = R.outline(R.nest11())
    assert [(l["depth"], l["parent"]) for l in nest["loops"]] == [(0, -1), (1, 0), (2, 1), (3, 2)]
    assert [p["type"] for p in nest["polygons"]] == ["out", "in", "out", "in"]
    assert nest["parts"].tolist() == [[0, 72, 1], [48, 8, 1]]
    opened = R.outline(R.nest11_open())
    assert [(l["depth"], l["parent"], l["key_px"]) for l in opened["loops"]] == [(0, -1, 0), (1, 0, 1), (1, 0, 13), (2, 2, 48), (3, 3, 49)]
    moved = R.outline(np.ones((1, 3), np.uint8), origin=(100, 200))
    assert moved["points"][0].tolist() == [200, 100] and moved["polygons"][0]["all_points_y"] == [100] * 4


def test_the_checkerboard():
    o = R.outline(R.checker33())
    t = o["table"]
    assert len(t) == 481 and rows_of(o)[0] == (0, 0, 260, 2050, 128) and (t[1:, 1] == 1).all() and (t[1:, 2] == 1).all()
    assert t[:, 7].sum() == 2180 and t[:, 10].sum() == 1090 and (t[1:, 3] == 0).all()
    assert o["parts"].tolist() == [[0, 545, 480]]


# ------------------------------------------------------------------------------------------------ the definition's asserts
def crops_by_name():
    c = {n: v[0] for n, v in MR.known_crops().items()}
    c.update(S.extra_crops())
    return c


@pytest.mark.parametrize("name", sorted(S.known_shapes()))
def test_the_asserts_on_the_crops_of_the_shapes(name):
    M = crops_by_name()[name]
    o = R.outline(M)                 # (sum of area2, of n_edges, the loops against parts and holes, chains against the oracle)
    n, _, _, edges, (n_parts, _, holes), _, _, _ = S.known_shapes()[name]
    t = o["table"]
    assert (t[:, 1] == 0).sum() == n_parts and (t[:, 1] == 1).sum() == holes and t[:, 7].sum() == edges and t[:, 10].sum() == 2 * n


def random_masks(count=300):
    rng = np.random.default_rng(0)
    for i in range(count):
        bh, bw = (int(v) for v in rng.integers(1, 15, 2))
        yield rng.random((bh, bw)) < 0.4 + 0.5 * (i % 6) / 5.0


def test_the_asserts_on_random_masks():
    outer = holes = 0
    for M in random_masks():
        o = R.outline(M, oracle=True)
        outer, holes = outer + int((o["table"][:, 1] == 0).sum()), holes + int((o["table"][:, 1] == 1).sum())
    assert outer > 300 and holes > 300


def test_records_round_trip_and_the_order_matters():
    rng = np.random.default_rng(7)
    wrong = 0
    for _ in range(40):
        M = rng.random((22, 22)) < 0.62
        polys = R.outline(M, oracle=True)["polygons"]             # (asserts instance_mask(polys) == M)
        flat = [p for p in polys if p["type"] == "out"] + [p for p in polys if p["type"] == "in"]
        wrong += not np.array_equal(O.instance_mask(flat, 22, 22), M)
    assert wrong >= 1                                               # all 'out' before all 'in' loses the islands in holes
    nest = R.outline(R.nest11())["polygons"]
    assert not np.array_equal(O.instance_mask([nest[0], nest[2], nest[1], nest[3]], 11, 11), R.nest11() != 0)


def test_flipping_and_transposing_keep_the_loops_as_a_multiset():
    maps = [crops_by_name()[n] for n in ("sinusoid", "two_parts", "eye9", "ring3")] + [R.nest11_open()] + list(random_masks(30))
    for M in maps:
        M = np.asarray(M)
        want = sorted((int(r[7]), abs(int(r[10])), int(r[8])) for r in R.outline(M, oracle=False)["table"])
        for T in (M[:, ::-1], M[::-1], M.T, M[::-1, ::-1].T):
            assert sorted((int(r[7]), abs(int(r[10])), int(r[8])) for r in R.outline(np.ascontiguousarray(T), oracle=False)["table"]) == want


# ------------------------------------------------------------------------------------------------ the host side
def device_rows(crops, rng):
    """the rows csrc/outline.hip writes, made by the definition, in a random order"""
    rows = []
    for g, M in enumerate(crops):
        for l in R.outline(M, oracle=False)["loops"]:
            rows.append([g, l["key"], l["n_edges"], l["n_points"], l["n_corners"], l["area2"], l["part"], l["west"], 0, 0, 0, 0])
    rows = np.array(rows, np.int64).reshape(-1, L.OUTLINE_ROW)
    return rows[rng.permutation(len(rows))]


def test_order_loops_nests_by_the_rule():
    rng = np.random.default_rng(3)
    crops = [R.nest11(), R.nest11_open(), R.checker33(), np.zeros((3, 5), np.uint8), S.two_parts()] + list(random_masks(40))
    raw = device_rows(crops, rng)
    table, order = MZ.order_loops(raw)
    want, at = [], 0
    for g, M in enumerate(crops):
        t = R.outline(M, oracle=False)["table"].copy()
        t[:, 0], t[:, 3] = g, np.where(t[:, 3] >= 0, t[:, 3] + at, -1)
        want.append(t)
        at += len(t)
    np.testing.assert_array_equal(table, np.concatenate(want))
    np.testing.assert_array_equal(raw[order][:, 1], table[:, 5] * 4 + table[:, 6])
    assert MZ.OUTLINE_COLUMNS == R.LOOP_COLUMNS and MZ.order_loops(np.zeros((0, 12)))[0].shape == (0, 11)
    for px, col, value in ((49, 5, 0), (48, 7, 2), (49, 6, 5)):   # no area; a loop to the west that is not there; no such part
        bad = device_rows([R.nest11()], rng)
        bad[np.flatnonzero(bad[:, 1] // 4 == px)[0], col] = value
        with pytest.raises(L.DisyoloError, match="loop table"):
            MZ.order_loops(bad)


def host_shapes(crops):
    """an InstanceShapes over host tensors, from the definition's tables"""
    ref = [S.shape(c, 2) for c in crops]
    groups, arena, nbytes = MZ.pack_masks(crops)
    s = MZ.InstanceShapes(groups[:, 2:6], [int(v) * 16 for v in groups[:, 7]], torch.zeros(max(nbytes, 1), dtype=torch.int32),
                          [r["sums"] for r in ref], [r["parts"] for r in ref], [r["pminmax"] for r in ref], S.directions(2))
    s.groups, s.groups_dev, s.arena, s.arena_bytes = groups, None, torch.from_numpy(arena), nbytes
    return s


def test_the_class_from_tables_alone():
    crops = [R.nest11(), np.ones((1, 3), np.uint8)]
    refs = [R.outline(c, origin=o) for c, o in zip(crops, ((0, 0), (0, 0)))]
    table = np.concatenate([refs[0]["table"], refs[1]["table"]])
    table[4:, 0] = 1
    s = host_shapes(crops)
    s.classid = np.array([2, 0])
    o = MZ.InstanceOutlines(s, table, np.concatenate([r["points"] for r in refs]), np.concatenate([r["corners"] for r in refs]))
    assert len(o) == 2 and o.loops_of(0).shape == (4, 11) and o.loops_of(1)[0, 7] == 8
    assert o.polygons(0) == refs[0]["polygons"] and o.polygons(1) == refs[1]["polygons"]
    np.testing.assert_array_equal(o.corners(4), refs[1]["corners"])
    assert o.parts.tolist() == [[0, 0, 72, 1], [0, 48, 8, 1], [1, 0, 3, 0]]
    rec = o.record(image_size=(40, 50), class_names=["crack", "spall", "rebar"])
    assert rec["image_size"] == (40, 50) and rec["class_names"] == ["rebar", "crack"] and rec["polygons"][1] == refs[1]["polygons"]
    assert "image" in o.record(image=np.zeros((4, 4, 3), np.uint8)) and o.table(["a", "b", "c"])[1]["kind"] == "hole"
    assert o.table(["a", "b", "c"])[4]["class"] == "a" and o.table()[0]["area_px"] == 121.0
    with pytest.raises(ValueError, match="image"):
        o.record()
    with pytest.raises(ValueError, match="points=False"):
        MZ.InstanceOutlines(s, table).points(0)


def test_instance_outlines_refuses_bad_arguments_and_reads_nothing_for_nothing(monkeypatch):
    monkeypatch.setattr(MZ, "_outline_read", lambda t: pytest.fail("nothing to read"))
    with pytest.raises(ValueError, match="TiledDetections"):
        MZ.instance_outlines(np.ones((3, 3)))
    s = host_shapes([np.ones((2, 2), np.uint8)])
    s.arena = None
    with pytest.raises(ValueError, match="shape_arena"):
        MZ.instance_outlines(s)
    s = host_shapes([np.ones((2, 2), np.uint8)])
    s.arena_bytes = 2 ** 29
    with pytest.raises(ValueError, match="arena_bytes"):
        MZ.instance_outlines(s)
    s = host_shapes([np.ones((2, 2), np.uint8)])
    s.edges = np.array([2 ** 30], np.int64)
    with pytest.raises(ValueError, match="2\\^30"):
        MZ.instance_outlines(s)
    with pytest.raises(ValueError, match="mask 0"):
        MZ.outline_masks([np.ones(3)])
    # G = 0, and masks without a pixel: no device is touched
    o = MZ.outline_masks([], device="cpu")
    assert len(o) == 0 and o.loops.shape == (0, 11) and o.parts.shape == (0, 4) and o.table() == []
    o = MZ.instance_outlines(host_shapes([np.zeros((3, 5), np.uint8), np.zeros((0, 4), np.uint8)]))
    assert len(o) == 2 and o.loops_of(1).shape == (0, 11) and o.polygons(0) == [] and o.points_dev is None
    assert o.record(image_size=(3, 5))["polygons"] == []


# ------------------------------------------------------------------------------------------------ the ABI's argument checks
def groups_table(boxes):
    return L.tile_compose_plan(np.asarray(boxes, np.int32).reshape(-1, 4), np.zeros(len(boxes) + 1, np.int64))


def calls(lib, p, cap=64, work=640, rounds=5, rows=8, n=64):
    """the three entry points with every buffer pointer p (host memory that a launch would fault on):
    name -> fn(groups_host, groups_dev, G, arena_bytes)"""
    return {
        "outline_edges": lambda gh, gd, G, nb: lib.disyolo_outline_edges(gh, gd, G, p, nb, p, p, p, p, p, p, cap, p, work, p, None),
        "outline_loops": lambda gh, gd, G, nb: lib.disyolo_outline_loops(gh, gd, G, p, nb, p, p, p, p, p, p, p, cap, rounds, p, work, p, p,
                                                                         rows, p, None),
        "outline_gather": lambda gh, gd, G, nb: lib.disyolo_outline_gather(gh, gd, G, nb, p, p, p, cap, p, p, rows, p, n, p, n, None),
    }


@pytest.mark.parametrize("name", ["outline_edges", "outline_loops", "outline_gather"])
def test_outline_entry_points_refuse_bad_arguments_before_any_launch(name):
    lib = L.load()
    buf = ctypes.create_string_buffer(1 << 16)
    p = ctypes.cast(buf, ctypes.c_void_p)
    fn = calls(lib, p)[name]
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
    # the limits: an edge's key must fit int32, the list 2^30 - 1 entries
    assert run(good, nbytes=1 << 29) == -1 and b"2^31" in lib.disyolo_last_error()
    assert run(good, f=calls(lib, p, cap=1 << 30, work=10 << 30)[name]) == -1 and b"2^30" in lib.disyolo_last_error()
    assert run(good, f=calls(lib, p, cap=-1)[name]) == -1
    if name != "outline_gather":
        assert run(good, f=calls(lib, p, cap=64, work=639)[name]) == -1 and b"work" in lib.disyolo_last_error()
    if name == "outline_loops":
        assert run(good, f=calls(lib, p, rounds=32)[name]) == -1 and b"rounds" in lib.disyolo_last_error()
        assert run(good, f=calls(lib, p, rows=-1)[name]) == -1 and b"rows" in lib.disyolo_last_error()
    if name == "outline_gather":
        assert run(good, f=calls(lib, p, n=1 << 30)[name]) == -1 and b"points" in lib.disyolo_last_error()
        assert run(good, f=calls(lib, p, rows=1 << 31)[name]) == -1 and b"rows" in lib.disyolo_last_error()
    # nothing to do is no error: G = 0, with no pointers at all
    assert fn(None, None, 0, 0) == 0
    assert lib.disyolo_outline_gather(None, None, 0, 0, None, None, None, 0, None, None, 0, None, 0, None, 0, None) == 0

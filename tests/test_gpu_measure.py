"""Instance measurement on the GPU: csrc/measure.hip through ``disyolo_amd.measure`` against the numpy definition
(tests/measure_ref.py).  Distances, skeletons, counts and iteration numbers are integers: equality.  The one float64 sum agrees
within relative (n + 2) 2^-52 for n skeleton pixels (a correctly rounded sqrt and the reordering of a sum of n positive
doubles); 1e-12 covers that for n <= 2000, and no crop here has more."""
import numpy as np
import pytest
import torch

import measure_ref as MR
import tiles_ref as TR
from disyolo_amd import lib as L
from disyolo_amd import measure as MZ
from disyolo_amd import tiles as TL

pytestmark = pytest.mark.gpu

_REF = {}


def ref(M):
    """the definition's answer for a crop, computed once per crop"""
    key = (M.shape, np.asarray(M != 0).tobytes())
    if key not in _REF:
        _REF[key] = MR.measure(M)
    return _REF[key]


def known_set():
    """every crop with a known answer and the three generated ones, crops whose area is no multiple of 16 first: their
    neighbours in the arena start behind padding bytes"""
    crops = [v[0] for v in MR.known_crops().values()] + [np.ones((4, 8), np.uint8)]
    return sorted(crops, key=lambda c: (c.size % 16 == 0, c.size))


def on_arena(dev, crops, chunk=8, fill=0, foreground=1, sentinels=None):
    groups, arena, nbytes = MZ.pack_masks(crops, fill=fill, foreground=foreground)
    kw = {}
    if sentinels is not None:
        kw = dict(d2_out=torch.full((nbytes,), sentinels[0], dtype=torch.int32, device=dev),
                  skeleton_out=torch.full((nbytes,), sentinels[1], dtype=torch.uint8, device=dev))
    return MZ.measure_arena(groups, torch.from_numpy(arena).to(dev), nbytes, chunk=chunk, **kw), groups, nbytes


def assert_matches_ref(m, crops):
    assert len(m) == len(crops) and m.counts.dtype == np.int64 and m.sum_sqrt.dtype == np.float64
    for g, M in enumerate(crops):
        want = ref(M)
        d2, sk = m.d2(g), m.skeleton(g)
        assert d2.dtype == torch.int32 and sk.dtype == torch.bool and d2.is_cuda and sk.is_cuda
        assert tuple(d2.shape) == tuple(sk.shape) == M.shape
        np.testing.assert_array_equal(d2.cpu().numpy(), want["d2"], err_msg="d2 of crop %d" % g)
        np.testing.assert_array_equal(sk.cpu().numpy().view(np.uint8), want["skeleton"], err_msg="skeleton of crop %d" % g)
        np.testing.assert_array_equal(m.counts[g], want["counts"], err_msg="counts of crop %d" % g)
        assert m.group_iterations[g] == want["iterations"], "iterations of crop %d" % g
        n = int(want["counts"][1])
        assert n <= 2000
        assert abs(m.sum_sqrt[g] - want["sum_sqrt"]) <= 1e-12 * want["sum_sqrt"], "sum_sqrt of crop %d" % g
    cnt = np.stack([ref(M)["counts"] for M in crops])
    length, wmax, wmean = MR.derive(cnt, m.sum_sqrt)            # (the derived numbers from the path's own float64 sums: exact)
    np.testing.assert_array_equal(m.length_px, length)
    np.testing.assert_array_equal(m.max_width_px, wmax)
    np.testing.assert_array_equal(m.mean_width_px, wmean)
    np.testing.assert_array_equal(m.area_px, cnt[:, 0])
    np.testing.assert_array_equal(m.skeleton_px, cnt[:, 1])
    np.testing.assert_array_equal(m.endpoints, cnt[:, 4])
    assert m.iterations == max(ref(M)["iterations"] for M in crops)


def same_bytes(a, b, nbytes):
    assert torch.equal(a.d2_arena[:nbytes], b.d2_arena[:nbytes]) and torch.equal(a.skeleton_arena[:nbytes], b.skeleton_arena[:nbytes])
    np.testing.assert_array_equal(a.counts, b.counts)
    np.testing.assert_array_equal(a.sum_sqrt.view(np.int64), b.sum_sqrt.view(np.int64))           # bit for bit
    np.testing.assert_array_equal(a.group_iterations, b.group_iterations)


# ------------------------------------------------------------------------------------------------ 1, 2: the known answers
def test_known_answers_in_one_arena(dev):
    crops = known_set()
    assert any(c.size % 16 for c in crops[:-1])
    z = (0, 0)
    a, groups, nbytes = on_arena(dev, crops, sentinels=z)
    assert_matches_ref(a, crops)
    assert a.iterations == 36
    assert sorted(set(a.group_iterations.tolist())) == [1, 2, 3, 4, 9, 29, 36]
    by_name = {n: np.flatnonzero([c.shape == v[0].shape and (c == v[0]).all() for c in crops])[0] for n, v in MR.known_crops().items()}
    for n, v in MR.known_crops().items():                  # the table itself, not only the ref
        g = by_name[n]
        assert a.counts[g, [0, 1, 2, 3, 5]].tolist() == [v[1], v[2], v[3], v[4], v[6]] and a.group_iterations[g] == v[8]
    g = by_name["3x9"], by_name["17x33"], by_name["1x9"]
    np.testing.assert_array_equal(a.length_px[list(g)], [6.0, 16.0, 9.0])
    np.testing.assert_array_equal(a.max_width_px[list(g)], [3.0, 17.0, 1.0])
    np.testing.assert_array_equal(a.mean_width_px[list(g)], [3.0, 17.0, 1.0])
    b, _, _ = on_arena(dev, crops, sentinels=z)             # the same call again: the same bits, the float64 sums included
    same_bytes(a, b, nbytes)


def test_chunk_does_not_change_the_result(dev):
    crops = known_set()
    z = (0, 0)
    a, _, nbytes = on_arena(dev, crops, chunk=8, sentinels=z)
    for chunk in (1, 2):
        b, _, _ = on_arena(dev, crops, chunk=chunk, sentinels=z)
        same_bytes(a, b, nbytes)
        assert b.iterations == 36


# ------------------------------------------------------------------------------------------------ 3: padding bytes
def test_padding_bytes_are_neither_read_nor_written(dev):
    """any non-zero byte is foreground, the bytes between two crops are nobody's pixels, and the elements of the two result
    arenas between two crops are left untouched"""
    crops = known_set()
    SD, SS = -7, 0xEE
    a, groups, nbytes = on_arena(dev, crops, fill=0xFF, foreground=0x80, sentinels=(SD, SS))
    assert_matches_ref(a, crops)
    b, _, _ = on_arena(dev, crops, sentinels=(SD, SS))
    same_bytes(a, b, nbytes)
    pad = np.ones(nbytes, bool)
    for g, c in zip(groups, crops):
        pad[int(g[7]) * 16:int(g[7]) * 16 + c.size] = False
    assert pad.sum() > 0
    assert (a.d2_arena.cpu().numpy()[pad] == SD).all() and (a.skeleton_arena.cpu().numpy()[pad] == SS).all()


# ------------------------------------------------------------------------------------------------ 4: block and row boundaries
def test_crops_over_block_and_row_boundaries(dev):
    ellipse = MR.known_crops()["ellipse"][0]
    crops = [np.ones((3, 1030), np.uint8),       # rows longer than a block's chunk of 1024 pixels (and than the staged width)
             np.ones((70, 300), np.uint8),       # 21 chunks, the last one partial
             np.zeros((4, 5), np.uint8),         # nothing in it, between two others
             ellipse]                            # 12 full chunks and a partial one
    assert L.COMPOSE_CHUNK == 1024 and ellipse.size % 1024 and (70 * 300) % 1024
    m, groups, _ = on_arena(dev, crops)
    assert groups[:, 6].tolist() == [0, 4, 25, 26]
    assert_matches_ref(m, crops)
    assert m.counts[2].tolist() == [0] * 8 and m.length_px[2] == 0 and m.max_width_px[2] == 0 and m.mean_width_px[2] == 0


# ------------------------------------------------------------------------------------------------ 5: empty and invalid input
def test_nothing_to_measure_and_a_box_too_long(dev):
    m = MZ.measure_masks([], device=dev)
    assert len(m) == 0 and m.counts.shape == (0, 8) and m.length_px.shape == (0,) and m.iterations == 0 and m.table() == []
    sc = TR.scene()
    res = TL.merge_tiles(sc.tiles, sc.image_hw, sc.net_size, sc.detections, np.zeros_like(sc.keep), torch.from_numpy(sc.masks).to(dev))
    m = MZ.measure_instances(res, mm_per_px=0.5)
    assert len(m) == 0 and m.area_px.shape == (0,) and m.area_mm2.shape == (0,) and m.iterations == 0
    # a box with an empty side among others
    crops = [np.ones((3, 9), np.uint8), np.zeros((0, 7), np.uint8), np.ones((1, 9), np.uint8)]
    m = MZ.measure_masks(crops, device=dev)
    assert m.counts[1].tolist() == [0] * 8 and m.group_iterations.tolist() == [2, 0, 1]
    np.testing.assert_array_equal(m.length_px, [6.0, 0.0, 9.0])
    # 40000 x 1: refused by the packer, and by the library when the table comes from elsewhere
    with pytest.raises(ValueError):
        MZ.measure_masks([np.ones((40000, 1), np.uint8)], device=dev)
    groups, nbytes = L.tile_compose_plan(np.array([[0, 0, 40000, 1]], np.int32), np.zeros(2, np.int64))
    with pytest.raises(L.DisyoloError, match="32767"):
        MZ.measure_arena(groups, torch.ones(nbytes, dtype=torch.uint8, device=dev), nbytes)
    with pytest.raises(ValueError):
        MZ.measure_masks([np.ones((3, 3), np.uint8)], chunk=0, device=dev)
    with pytest.raises(ValueError):
        MZ.measure_masks([np.ones((3, 3), np.float32)], device=dev)


# ------------------------------------------------------------------------------------------------ 6: end to end without a net
def test_measure_instances_on_the_scene(dev):
    sc = TR.scene()
    res = TL.merge_tiles(sc.tiles, sc.image_hw, sc.net_size, sc.detections, sc.keep, torch.from_numpy(sc.masks).to(dev))
    assert len(res) == 5
    arena_before = res.arena.clone()
    m = MZ.measure_instances(res, mm_per_px=0.5)
    assert torch.equal(res.arena, arena_before)
    crops = [res.mask(g).cpu().numpy().astype(np.uint8) for g in range(len(res))]
    assert_matches_ref(m, crops)
    np.testing.assert_array_equal(m.boxes, res.boxes)
    # the crack through the image is the long thin one
    crack = int(np.argmax(m.length_px))
    assert res.classid[crack] == 0 and m.length_px[crack] > 200 and m.mean_width_px[crack] < 12
    rows = m.table(["crack", "spall", "rebar"])
    assert len(rows) == 5 and rows[crack]["class"] == "crack"
    for g, row in enumerate(rows):
        assert row["length_px"] == m.length_px[g] and row["area_px"] == m.area_px[g] and row["score"] == float(res.score[g])
        assert row["length_mm"] == 0.5 * row["length_px"] and row["area_mm2"] == 0.25 * row["area_px"]
        assert row["max_width_mm"] == 0.5 * row["max_width_px"] and row["mean_width_mm"] == 0.5 * row["mean_width_px"]
    assert "length_mm" not in MZ.measure_instances(res).table()[0]


# ------------------------------------------------------------------------------------------------ 7: the generic path
def test_measure_masks_of_different_sizes(dev):
    rng = np.random.default_rng(3)
    yy, xx = np.mgrid[:37, :53]
    crops = [rng.random((23, 41)) < 0.7,                                        # bool
             ((yy - 18) ** 2 + (xx - 26) ** 2 < 200).astype(np.uint8) * 255,    # uint8, foreground 255
             (np.abs(yy[:9, :31] - 4) < 2).astype(np.uint8)]
    m = MZ.measure_masks([crops[0], torch.from_numpy(crops[1]).to(dev), crops[2]], device=dev)
    assert_matches_ref(m, [np.asarray(c != 0, np.uint8) for c in crops])

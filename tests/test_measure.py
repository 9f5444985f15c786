"""Instance measurement without a GPU: the numpy definition (tests/measure_ref.py) against the known answers and scipy's
Euclidean transform, and the argument checks of csrc/measure.hip, which happen before any launch."""
import ctypes

import numpy as np
import pytest

import measure_ref as MR
from disyolo_amd import lib as L


KNOWN = MR.known_crops()


@pytest.mark.parametrize("name", list(KNOWN))
def test_ref_reproduces_the_known_answers(name):
    M, area, skel_px, n_orth, n_diag, n_end, max_d2, ssq, iterations = KNOWN[name]
    m = MR.measure(M)
    c = m["counts"]
    assert c.dtype == np.int64 and m["d2"].dtype == np.int32 and m["skeleton"].dtype == np.uint8
    assert (int(c[0]), int(c[1]), int(c[2]), int(c[3]), int(c[5])) == (area, skel_px, n_orth, n_diag, max_d2)
    assert m["iterations"] == iterations and c[7] == 0
    if n_end is not None:
        assert c[4] == n_end
    if ssq is not None:
        assert m["sum_sqrt"] == ssq
    assert c[6] <= c[5] and not (m["skeleton"].astype(bool) & ~M.astype(bool)).any()      # S is a subset of M
    if name in MR.KNOWN_SKELETON_ROWS:
        row, a, b = MR.KNOWN_SKELETON_ROWS[name]
        want = np.zeros_like(M)
        want[row, a:b + 1] = 1
        np.testing.assert_array_equal(m["skeleton"], want)


def test_ref_derived_numbers():
    rows = [MR.measure(KNOWN[n][0]) for n in ("3x9", "17x33", "1x9", "2x2")]
    cnt = np.stack([r["counts"] for r in rows] + [np.zeros(8, np.int64)])
    length, wmax, wmean = MR.derive(cnt, [r["sum_sqrt"] for r in rows] + [0.0])
    np.testing.assert_array_equal(length, [6.0, 16.0, 9.0, 0.0, 0.0])
    np.testing.assert_array_equal(wmax, [3.0, 17.0, 1.0, 1.0, 0.0])
    np.testing.assert_array_equal(wmean, [3.0, 17.0, 1.0, 1.0, 0.0])     # 2x2: no skeleton, the mean is the maximum; area 0: all 0


def test_ref_d2_is_the_euclidean_transform():
    from scipy import ndimage as ndi
    rng = np.random.default_rng(7)
    for _ in range(50):
        M = rng.random((int(rng.integers(1, 41)), int(rng.integers(1, 41)))) < rng.uniform(0.3, 0.98)
        want = np.rint(ndi.distance_transform_edt(np.pad(M, 1)) ** 2)[1:-1, 1:-1].astype(np.int32)
        got = MR.d2(M)
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(got, MR.d2_brute(M))


def test_thinning_iterations_exceed_the_distance_bound_on_some_masks():
    """why convergence is observed, not computed: iterations > ceil(sqrt(max d2)) + 1 happens"""
    rng = np.random.default_rng(0)
    broke = 0
    for _ in range(40):
        M = rng.random((int(rng.integers(8, 33)), int(rng.integers(8, 33)))) < 0.8
        broke += MR.thin(M)[1] > int(np.ceil(np.sqrt(MR.d2(M).max()))) + 1
    assert broke > 0


# ------------------------------------------------------------------------------------------------ the ABI's argument checks
def groups_table(boxes):
    return L.tile_compose_plan(np.asarray(boxes, np.int32).reshape(-1, 4), np.zeros(len(boxes) + 1, np.int64))


def calls(lib, p):
    """the three entry points on a groups table g (a ctypes pointer or None) with every buffer pointer p (host memory that a
    launch would fault on): name -> fn(groups_host, groups_dev, G, arena_bytes)"""
    return {
        "measure_d2": lambda gh, gd, G, nb: lib.disyolo_measure_d2(gh, gd, G, p, nb, p, p, None),
        "measure_thin": lambda gh, gd, G, nb: lib.disyolo_measure_thin(gh, gd, G, p, nb, p, p, p, p, 0, 8, None),
        "measure_counts": lambda gh, gd, G, nb: lib.disyolo_measure_counts(gh, gd, G, p, nb, p, p, p, p, 1 << 20, p, None),
    }


@pytest.mark.parametrize("name", ["measure_d2", "measure_thin", "measure_counts"])
def test_measure_entry_points_refuse_bad_tables_before_any_launch(name):
    lib = L.load()
    buf = ctypes.create_string_buffer(1 << 16)
    p = ctypes.cast(buf, ctypes.c_void_p)
    fn = calls(lib, p)[name]
    tag = name.encode()

    def run(groups, G=None, nbytes=None, null=False):
        g = np.ascontiguousarray(groups, dtype=np.int32)
        return fn(None if null else g.ctypes.data, g.ctypes.data, len(g) if G is None else G, 1 << 16 if nbytes is None else nbytes)

    good, nbytes = groups_table([[0, 0, 3, 9], [5, 5, 9, 10]])
    # a box side above 32767 (its plan is consistent, and the arena is said to be large enough: only the side is wrong)
    wide, wide_bytes = groups_table([[0, 0, 1, 40000]])
    assert run(wide, nbytes=wide_bytes) == -1 and tag in lib.disyolo_last_error() and b"32767" in lib.disyolo_last_error()
    tall, tall_bytes = groups_table([[0, 0, 32768, 1]])
    assert run(tall, nbytes=tall_bytes) == -1 and b"32767" in lib.disyolo_last_error()
    # an off16 beyond arena_bytes
    assert run(good, nbytes=nbytes - 16) == -1 and b"arena" in lib.disyolo_last_error()
    far = good.copy()
    far[1, 7] = 1 << 20
    assert run(far) == -1 and b"arena" in lib.disyolo_last_error()
    # a negative G, a null pointer
    assert run(good, G=-1) == -1 and tag in lib.disyolo_last_error()
    assert run(good, null=True) == -1 and b"null pointer" in lib.disyolo_last_error()
    # a block0 that is not the plan's, a negative side, crops that overlap
    bad = good.copy()
    bad[1, 6] = 5
    assert run(bad) == -1 and b"block0" in lib.disyolo_last_error()
    bad = good.copy()
    bad[0, 4] = -1
    assert run(bad) == -1
    bad = good.copy()
    bad[1, 7] = 0
    assert run(bad) == -1
    # nothing to do is no error: G = 0 (with no pointers at all), and groups without a pixel
    assert fn(None, None, 0, 0) == 0
    if name != "measure_counts":        # (measure_counts would launch: it writes the zero rows of empty groups)
        empty, _ = groups_table([[4, 4, 4, 9], [0, 0, 0, 0]])
        assert run(empty, nbytes=0) == 0


def test_measure_thin_refuses_a_bad_iteration_range():
    lib = L.load()
    buf = ctypes.create_string_buffer(1 << 12)
    p = ctypes.cast(buf, ctypes.c_void_p)
    g, nbytes = groups_table([[0, 0, 3, 9]])
    for it0, chunk in ((-1, 8), (0, 0), (0, 1025)):
        assert lib.disyolo_measure_thin(g.ctypes.data, g.ctypes.data, 1, p, nbytes, p, p, p, p, it0, chunk, None) == -1
        assert b"chunk" in lib.disyolo_last_error()
    assert lib.disyolo_measure_counts(g.ctypes.data, g.ctypes.data, 1, p, nbytes, p, p, p, p, 0, p, None) == -1
    assert b"partials" in lib.disyolo_last_error()

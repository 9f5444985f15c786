"""The skeleton graph without a GPU: the numpy definition (tests/skeleton_ref.py) against the known answers, its identities and
independent checks of its parts, and the argument checks of csrc/skeleton.hip and ``measure.skeleton_graph``, which happen
before any launch."""
import ctypes
import decimal
import math
from fractions import Fraction

import numpy as np
import pytest

import measure_ref as MR
import skeleton_ref as SR
from disyolo_amd import lib as L
from disyolo_amd import measure as MZ

CROPS = {n: v[0] for n, v in MR.known_crops().items()}
CROPS.update(SR.extra_crops())
_MEASURED = {}
C = {name: i for i, name in enumerate(SR.ROW_COLS)}


def measured(name):
    if name not in _MEASURED:
        _MEASURED[name] = MR.measure(CROPS[name])
    return _MEASURED[name]


def graph(name, mb, max_rounds=8):
    m = measured(name)
    g = SR.graph(m["skeleton"], m["d2"], mb, max_rounds)
    g["length"], g["wmean"], g["wmax"], g["wmin"], g["kinds"] = SR.derive_rows(g["rows"])
    cnt = MR.counts(CROPS[name], g["skeleton"], m["d2"])
    g["counts"], g["pruned_length"] = cnt, float(MR.derive(cnt, MR.sum_sqrt(g["skeleton"], m["d2"]))[0][0])
    return g


def roots(g, name):
    bw = CROPS[name].shape[1]
    return [divmod(int(r), bw) for r in g["rows"][:, 0]]


def random_skeletons(n, seed, side=24):
    rng = np.random.default_rng(seed)
    for _ in range(n):
        M = (rng.random((side, side)) < rng.uniform(0.3, 0.9)).astype(np.uint8)
        yield M, MR.thin(M)[0], MR.d2(M)


# ------------------------------------------------------------------------------------------------ the known answers
SUM_Q8 = {"1x1": 256, "1x9": 2304, "eye9": 2304, "3x9": 3072, "5x17": 9216, "17x33": 36864, "70x300": 2060800, "sinusoid": 155500,
          "ellipse": 806896}


@pytest.mark.parametrize("name", list(SUM_Q8))
@pytest.mark.parametrize("mb", [0.0, 10.0, 300.5])
def test_single_strokes_are_one_free_branch(name, mb):
    v = MR.known_crops()[name]
    g = graph(name, mb)
    r = g["rows"]
    assert r.dtype == np.int64 and g["links"].dtype == np.uint8 and g["labels"].dtype == np.int32 and g["skeleton"].dtype == np.uint8
    assert len(r) == 1 and g["kinds"] == ["free"] and g["analyses"] == 1 and g["converged"]
    assert (r[0, C["px"]], r[0, C["n_orth"]], r[0, C["n_diag"]], r[0, C["n_end"]]) == (v[2], v[3], v[4], 2)
    assert r[0, C["sum_q8"]] == SUM_Q8[name] and g["crop"].tolist() == [0, 0, 0, 1]
    np.testing.assert_array_equal(g["skeleton"], measured(name)["skeleton"])
    if name == "ellipse":
        assert r[0, C["min_d2"]] == 337


def test_2x2_has_no_branch_and_no_junction():
    g = graph("2x2", 10.0)
    assert g["rows"].shape == (0, len(SR.ROW_COLS)) and g["crop"].tolist() == [0, 0, 0, 0] and g["analyses"] == 1
    assert (g["labels"] == -1).all() and (g["links"] == 0).all()


def test_t3spur():
    g = graph("T3spur", 0.0)
    assert g["skeleton"].sum() == 80 and g["crop"].tolist() == [2, 0, 0, 5] and g["analyses"] == 1
    assert roots(g, "T3spur") == [(5, 15), (9, 1), (9, 16), (9, 31), (10, 30)]
    assert g["length"].tolist() == [4.5, 14.5, 15.0, 28.5, 18.5] and g["kinds"][2] == "inner"
    assert g["rows"][:, C["sum_q8"]].tolist() == [2108, 7168, 7168, 14336, 9276]
    g = graph("T3spur", 10.0)
    assert g["analyses"] == 2 and g["converged"] and g["skeleton"].sum() == 76 and g["pruned_length"] == 76.5
    assert g["crop"].tolist() == [1, 0, 0, 3] and g["kinds"] == ["terminal"] * 3 and roots(g, "T3spur") == [(9, 1), (9, 31), (10, 30)]
    assert g["rows"][:, C["px"]].tolist() == [29, 28, 18] and g["length"].tolist() == [29.5, 28.5, 18.5]


def test_noise():
    g = graph("noise", 0.0)
    assert len(g["rows"]) == 456 and g["kinds"].count("inner") == 420 and g["kinds"].count("terminal") == 36
    assert g["crop"].tolist() == [672, 475, 123, 456] and g["rows"][:, C["px"]].sum() == 743 and g["rows"][:, C["sum_q8"]].sum() == 195242
    assert abs(g["pruned_length"] - 1914.45) < 0.005
    g = graph("noise", 10.0)
    assert g["analyses"] == 3 and g["converged"] and g["skeleton"].sum() == 1330 and abs(g["pruned_length"] - 1800.0214) < 5e-5
    assert len(g["rows"]) == 411 and g["kinds"].count("inner") == 410 and g["kinds"].count("free") == 1
    assert g["crop"].tolist() == [638, 458, 117, 411] and g["rows"][:, C["px"]].sum() == 692 and g["rows"][:, C["sum_q8"]].sum() == 182380
    g = graph("noise", 10.0, max_rounds=1)
    assert g["analyses"] == 2 and not g["converged"] and g["skeleton"].sum() == 1338
    assert len(g["rows"]) == 417 and g["kinds"].count("terminal") == 3 and g["crop"][0] == 641
    g = graph("noise", 10.0, max_rounds=0)
    assert g["analyses"] == 1 and not g["converged"] and g["skeleton"].sum() == 1415


def test_ring_tail_serp_plus9():
    g = graph("ring_tail", 10.0)
    assert g["analyses"] == 1 and g["skeleton"].sum() == 210 and g["crop"].tolist() == [1, 0, 0, 2]
    assert roots(g, "ring_tail") == [(13, 56), (40, 88)] and g["kinds"] == ["inner", "terminal"]
    assert g["rows"][:, C["px"]].tolist() == [159, 50] and abs(g["length"][0] - 183.196) < 5e-4 and g["length"][1] == 50.5
    g = graph("serp", 10.0)
    assert roots(g, "serp") == [(0, 0)] and g["kinds"] == ["free"]
    assert g["rows"][0, [C["px"], C["n_orth"], C["sum_q8"]]].tolist() == [6320, 6319, 1617920]
    g = graph("plus9", 10.0)
    assert g["analyses"] == 2 and g["skeleton"].sum() == 1 and roots(g, "plus9") == [(4, 4)] and g["kinds"] == ["free"]
    assert g["rows"][0, C["sum_q8"]] == 362
    g = graph("plus9", 3.0)
    assert g["analyses"] == 1 and g["skeleton"].sum() == 17 and g["kinds"] == ["terminal"] * 4 and g["length"].tolist() == [4.5] * 4


def test_the_documented_consequences_of_the_rule():
    # a plain T with arms 10.5 / 10.5 / 9.5 loses the 9.5 arm at 10, and the two others become one branch
    T = np.zeros((11, 21), np.uint8)
    T[0, :] = 1
    T[0:10, 10] = 1
    g = SR.graph(T, T, 0.0)
    assert sorted(SR.derive_rows(g["rows"])[0].tolist()) == [9.5, 10.5, 10.5] and g["crop"][0] == 1
    g = SR.graph(T, T, 10.0)
    assert g["analyses"] == 2 and g["skeleton"].sum() == 21 and SR.derive_rows(g["rows"])[0].tolist() == [21.0]
    # the end piece of a crack beyond its last spur goes with the spur
    K = np.zeros((9, 40), np.uint8)
    K[8, :] = 1
    K[0:8, 33] = 1
    g = SR.graph(K, K, 10.0)
    assert g["skeleton"][8].sum() == 34 and g["skeleton"][:8].sum() == 0 and g["converged"]
    # a star of short arms is pruned to its junction pixel (plus9 above is the other example)
    g = SR.graph(CROPS["plus9"], CROPS["plus9"], 5.0)
    assert g["skeleton"].sum() == 1 and g["skeleton"][4, 4] == 1


# ------------------------------------------------------------------------------------------------ identities, second opinions
def check_identities(M, S, D):
    cnt = MR.counts(M, S, D)
    table, crop = SR.rows(S, D)
    assert table[:, C["n_orth"]].sum() + crop[1] == cnt[2]
    assert table[:, C["n_diag"]].sum() + crop[2] == cnt[3]
    assert table[:, C["px"]].sum() + crop[0] == cnt[1]
    deg = SR.degree(SR.links(S))
    assert deg[S == 0].sum() == 0 and deg.sum() == 2 * (cnt[2] + cnt[3])


@pytest.mark.parametrize("name", list(CROPS))
def test_link_identities_on_the_known_crops(name):
    m = measured(name)
    check_identities(CROPS[name], m["skeleton"], m["d2"])
    g = SR.graph(m["skeleton"], m["d2"], 10.0)
    check_identities(CROPS[name], g["skeleton"], m["d2"])


def test_link_identities_on_random_masks():
    for M, S, D in random_skeletons(50, 11):
        check_identities(M, S, D)
        check_identities(M, M, D)             # and on maps that are no skeletons at all


def second_labelling(S):
    """scipy's connected components on an explicit adjacency of the P pixels"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    s = S != 0
    bh, bw = s.shape
    P = np.pad(s, 1)
    nb = [P[1 + dy:1 + dy + bh, 1 + dx:1 + dx + bw] for dy, dx in SR.OFFSETS]
    linked = [None] * 8
    for k, (dy, dx) in enumerate(SR.OFFSETS):
        linked[k] = s & nb[k] if dy == 0 or dx == 0 else s & nb[k] & ~nb[(k - 1) % 8] & ~nb[(k + 1) % 8]
    deg = sum(q.astype(np.int32) for q in linked)
    isP = s & (deg <= 2)
    Pp = np.pad(isP, 1)
    a, b = [], []
    idx = np.arange(bh * bw).reshape(bh, bw)
    for k, (dy, dx) in enumerate(SR.OFFSETS):
        both = isP & linked[k] & Pp[1 + dy:1 + dy + bh, 1 + dx:1 + dx + bw]
        a.append(idx[both])
        b.append(idx[both] + dy * bw + dx)
    a, b = np.concatenate(a), np.concatenate(b)
    n, comp = connected_components(coo_matrix((np.ones(a.size), (a, b)), shape=(bh * bw, bh * bw)), directed=False)
    smallest = np.full(n, bh * bw)
    np.minimum.at(smallest, comp[isP.reshape(-1)], idx.reshape(-1)[isP.reshape(-1)])
    return np.where(isP, smallest[comp].reshape(bh, bw), -1).astype(np.int32)


def test_labels_equal_a_second_labelling():
    for name in CROPS:
        S = measured(name)["skeleton"]
        np.testing.assert_array_equal(SR.labels(S), second_labelling(S), err_msg=name)
    for M, S, _ in random_skeletons(30, 5):
        np.testing.assert_array_equal(SR.labels(S), second_labelling(S))
        np.testing.assert_array_equal(SR.labels(M), second_labelling(M))


def test_the_integer_spur_test_is_the_exact_comparison():
    """length < min_branch_px in exact arithmetic: 2 sqrt(2) n_diag < t2 <=> t2 > 0 and 8 n_diag^2 < t2^2 (sqrt(2) is irrational,
    so apart from n_diag = 0 there is no tie in the square; the ties of the rational part are on the grid)"""
    decimal.getcontext().prec = 60
    r2 = decimal.Decimal(2).sqrt()
    for n_orth in range(0, 14):
        for n_diag in range(0, 14):
            for M2 in range(0, 70):
                twice = 2 * n_orth + 1 + 2 * r2 * n_diag             # twice the length of a branch with one end
                assert SR.is_spur(n_orth, n_diag, 1, 1, M2) == (twice < M2), (n_orth, n_diag, M2)
                if n_diag == 0:
                    assert SR.is_spur(n_orth, 0, 1, 1, M2) == (Fraction(2 * n_orth + 1, 2) < Fraction(M2, 2))
    assert not SR.is_spur(9, 0, 1, 1, 19) and SR.is_spur(9, 0, 1, 1, 20)          # a length of 9.5 at 9.5 and at 10
    assert not SR.is_spur(3, 0, 2, 1, 100) and not SR.is_spur(3, 0, 1, 0, 100) and not SR.is_spur(3, 0, 1, 2, 100)
    edge = int((decimal.Decimal(65533) / (2 * r2)).to_integral_value(rounding=decimal.ROUND_FLOOR))    # the largest M2
    assert SR.is_spur(0, edge, 1, 1, 65534) and not SR.is_spur(0, edge + 1, 1, 1, 65534) and not SR.is_spur(0, 2 ** 30, 1, 1, 65534)


def test_isqrt_is_the_floor_of_the_square_root():
    decimal.getcontext().prec = 60
    rng = np.random.default_rng(1)
    values = list(range(0, 300)) + [2 * 32767 ** 2, 2 ** 31 - 1] + [int(v) for v in rng.integers(0, 2 ** 31, 300)]
    for d in values:
        want = int((decimal.Decimal(65536 * d).sqrt()).to_integral_value(rounding=decimal.ROUND_FLOOR))
        assert math.isqrt(65536 * d) == want
    D = np.array([[0, 1, 2, 900]], np.int32)
    table, _ = SR.rows(np.ones((1, 4), np.uint8), D)
    assert table[0, C["sum_q8"]] == 0 + 256 + 362 + 7680


def test_end_points_by_link_degree_and_by_neighbour_count_agree():
    """the two definitions are allowed to differ; on every skeleton tried they do not.  A failure here is a finding to write
    down, not a bug."""
    for M, S, D in random_skeletons(200, 23):
        table, _ = SR.rows(S, D)
        assert table[:, C["n_end"]].sum() == MR.counts(M, S, D)[4]
    for name in CROPS:
        m = measured(name)
        assert SR.rows(m["skeleton"], m["d2"])[0][:, C["n_end"]].sum() == m["counts"][4], name


def test_min_branch_px_of_the_definition():
    assert SR.check_min_branch(0) == 0 and SR.check_min_branch(10.5) == 21 and SR.check_min_branch(32767) == 65534
    for bad in (-0.5, 0.25, 32767.5, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            SR.check_min_branch(bad)


# ------------------------------------------------------------------------------------------------ the ABI's argument checks
def groups_table(boxes):
    return L.tile_compose_plan(np.asarray(boxes, np.int32).reshape(-1, 4), np.zeros(len(boxes) + 1, np.int64))


def calls(lib, p):
    """the four entry points with every buffer pointer p (host memory that a launch would fault on):
    name -> fn(groups_host, groups_dev, G, arena_bytes, capacity, M2)"""
    return {
        "skeleton_classify": lambda gh, gd, G, nb, cap, M2: lib.disyolo_skeleton_classify(gh, gd, G, nb, p, p, p, None),
        "skeleton_label": lambda gh, gd, G, nb, cap, M2: lib.disyolo_skeleton_label(gh, gd, G, nb, p, p, p, None),
        "skeleton_rows": lambda gh, gd, G, nb, cap, M2: lib.disyolo_skeleton_rows(gh, gd, G, nb, p, p, p, p, p, cap, M2, p, p, None),
        "skeleton_prune": lambda gh, gd, G, nb, cap, M2: lib.disyolo_skeleton_prune(gh, gd, G, nb, p, p, p, cap, p, None),
    }


@pytest.mark.parametrize("name", ["skeleton_classify", "skeleton_label", "skeleton_rows", "skeleton_prune"])
def test_skeleton_entry_points_refuse_bad_arguments_before_any_launch(name):
    lib = L.load()
    buf = ctypes.create_string_buffer(1 << 16)
    p = ctypes.cast(buf, ctypes.c_void_p)
    fn = calls(lib, p)[name]
    tag = name.encode()

    def run(groups, G=None, nbytes=None, null=False, cap=16, M2=20):
        g = np.ascontiguousarray(groups, dtype=np.int32)
        return fn(None if null else g.ctypes.data, g.ctypes.data, len(g) if G is None else G, 1 << 16 if nbytes is None else nbytes,
                  cap, M2)

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
    if name in ("skeleton_rows", "skeleton_prune"):
        assert run(good, cap=-1) == -1 and b"capacity" in lib.disyolo_last_error()
        assert run(good, cap=1 << 31) == -1 and b"capacity" in lib.disyolo_last_error()
    if name == "skeleton_rows":
        for M2 in (-1, 65535):
            assert run(good, M2=M2) == -1 and b"M2" in lib.disyolo_last_error()
    # nothing to do is no error: G = 0 (with no pointers at all), and groups without a pixel
    assert fn(None, None, 0, 0, 0, 0) == 0
    if name != "skeleton_rows":          # (skeleton_rows would zero its tables: the zero rows of empty groups)
        empty, _ = groups_table([[4, 4, 4, 9], [0, 0, 0, 0]])
        assert run(empty, nbytes=0) == 0


# ------------------------------------------------------------------------------------------------ skeleton_graph's ValueErrors
def host_measures():
    """an InstanceMeasures over host tensors: every check below has to come before anything touches a device"""
    import torch
    groups, arena, nbytes = MZ.pack_masks([np.ones((1, 9), np.uint8)])
    m = MZ.InstanceMeasures(groups[:, 2:6], [0], torch.zeros(16, dtype=torch.int32), torch.zeros(16, dtype=torch.uint8),
                            [[9, 9, 8, 0, 2, 1, 1, 0]], [9.0], [1])
    m.groups, m.arena, m.arena_bytes = groups, torch.from_numpy(arena), nbytes
    return m


@pytest.mark.parametrize("bad", [0.25, -0.5, 32767.5, float("nan"), float("inf"), "ten", None])
def test_skeleton_graph_refuses_a_bad_min_branch_px(bad):
    with pytest.raises(ValueError, match="min_branch_px"):
        MZ.skeleton_graph(host_measures(), bad)


@pytest.mark.parametrize("bad", [-1, 1025, 2.0, True, None, "3"])
def test_skeleton_graph_refuses_a_bad_max_rounds(bad):
    with pytest.raises(ValueError, match="max_rounds"):
        MZ.skeleton_graph(host_measures(), 10.0, max_rounds=bad)


def test_skeleton_graph_refuses_other_bad_arguments():
    with pytest.raises(ValueError, match="mm_per_px"):
        MZ.skeleton_graph(host_measures(), 10.0, mm_per_px=0.0)
    with pytest.raises(ValueError, match="row_capacity"):
        MZ.skeleton_graph(host_measures(), 10.0, row_capacity=-1)
    m = host_measures()
    m.groups = None
    with pytest.raises(ValueError, match="measure_arena"):
        MZ.skeleton_graph(m, 10.0)


def test_instance_measures_keeps_what_it_had():
    m = host_measures()
    assert m.length_px.tolist() == [9.0] and m.table()[0]["length_px"] == 9.0 and m.groups_dev is None

"""The option matrix on the CPU: the table of tests/option_matrix.py covers every pair of option values, and every row that
is compared against the oracle gives it finite losses and a positive RoI (so the GPU comparison of that row is well-posed
before any GPU is involved)."""
import itertools

import numpy as np
import pytest
import torch

import disyolo_oracle as O
import option_matrix as OM
from disyolo_amd.net import YOLONet
from net_setup import perturb_variables
from test_gpu_class_list import class_batch


def _factors(row):
    return {"shape": (row.B, row.S), "C": row.C, "k": row.k, "m": row.m, "lock": OM.lock_kind(row)}


VALUES = {"shape": OM.SHAPES, "C": OM.CLASS_COUNTS, "k": OM.K_MAPS, "m": OM.MASK_STRIDES, "lock": OM.LOCK_KINDS}


def test_every_pair_of_option_values_occurs_in_a_row():
    rows = [_factors(r) for r in OM.VALUE_ROWS]
    missing = []
    for fa, fb in itertools.combinations(VALUES, 2):
        for va in VALUES[fa]:
            for vb in VALUES[fb]:
                if not any(r[fa] == va and r[fb] == vb for r in rows):
                    missing.append("%s=%s with %s=%s" % (fa, va, fb, vb))
    assert not missing, "pairs without a row: %s" % "; ".join(missing)


def test_the_extra_conditions_of_the_table():
    rows = OM.VALUE_ROWS
    assert len({r.name for r in OM.ROWS}) == len(OM.ROWS)
    assert any(r.C == 80 and r.k == 7 for r in rows) and any(r.C == 80 and r.m == 1 for r in rows)
    for shape in OM.SHAPES[1:]:
        assert any((r.B, r.S) == shape and OM.lock_kind(r) != "stage1" for r in rows), shape
    # the anchor, the evaluate row, two stage-1 rows for backbone_pair / fp8 that are not the configured mix, one S = 32 row
    anchor = [r for r in rows if "anchor" in r.extras]
    assert [(r.B, r.S, r.C, r.k, r.m, r.lock) for r in anchor] == [(2, 64, 3, 3, 2, "stage1")]
    assert [(r.C, r.k, r.m) for r in rows if "map" in r.extras] == [(6, 5, 4)]
    for what in ("pair", "fp8"):
        marked = [r for r in rows if what in r.extras]
        assert len(marked) == 2 and all(r.lock == "stage1" and (r.C, r.k, r.m) != (3, 3, 2) for r in marked)
    small = [r for r in OM.ROWS if not r.values]
    assert [(r.B, r.S) for r in small] == [(2, 32)]
    # every holed row's map has a hole, every map is one of its row's mask stride (lock_of_row asserts it)
    for r in OM.ROWS:
        assert bool(OM.expected_pass_through(r)) == (OM.lock_kind(r) == "holed"), r.name


def plan_net(row, training=True, seed=1):
    net = YOLONet(training=training, plan_only=True, seed=seed, **OM.net_kwargs(row))
    perturb_variables(net, seed)
    return net


@pytest.mark.parametrize("row", OM.VALUE_ROWS, ids=OM.ids(OM.VALUE_ROWS))
def test_oracle_is_finite_with_a_positive_roi_on_every_row(row):
    """the row's variables (a plan-only net, the perturbation of the GPU tests) through the oracle alone"""
    what = OM.describe(row)
    net = plan_net(row)
    assert net.pass_through_layers() == OM.expected_pass_through(row), what
    assert set(net.trainable_names()) == set(OM.trainable_names(row)), what
    b, perms = class_batch(row.B, row.S, row.seed, row.C)
    p = {k: v.detach().float().clone() for k, v in net.params.items()}
    with torch.no_grad():
        parts, det, yolos, mask_pos = OM.oracle_total_loss(row, p, b, perms, updates={})
    assert [tuple(y.shape[1:]) for y in yolos] == [(g, g, 3, 5 + row.C) for g in (row.S // 8, row.S // 16, row.S // 32)], what
    assert tuple(mask_pos.shape) == (row.B, row.S // row.m, row.S // row.m, row.k ** 2), what
    bad = [n for n, v in parts.items() if not np.isfinite(float(v))]
    assert not bad, "%s: oracle loss parts not finite: %s" % (what, bad)
    nroi = [len(O.select_mask_rois(det[i], b["true_boxes"].numpy()[i, 0, 0, 0], *perms[i])[0]) for i in range(row.B)]
    print("%s: oracle total %.5f mask %.5f, positive RoIs per image %s" % (row.name, float(parts["total"]), float(parts["mask"]), nroi))
    assert sum(nroi) > 0 and float(parts["mask"]) > 0, "%s: the oracle has no positive RoI (RoIs per image %s)" % (what, nroi)

"""K_MAP = 5 and 7 (yolo/config.py K_MAP; assemble_kmask_from_box's k = 3, 5, 7 list, yolo/yolo3_net_pos.py:808-823) on the
CPU side: the plan of a k x k net, the refusals of the mask-path entry points for any other k, the RoI row width, and
checkpoints of a k = 5 net.  No GPU: plan-only nets and host buffers that a launch would fault on."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import disyolo_oracle as O
from disyolo_amd import checkpoint as ck
from disyolo_amd import config as cfg
from disyolo_amd import lib as L
from disyolo_amd.net import YOLONet

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "disyolo.h")


def _check_plan(net, k):
    assert net.k == k and net.k_mapout == k * k
    assert tuple(net.params["yolo/convolutional82/weights"].shape) == (1, 1, 64, k * k)
    assert tuple(net.params["yolo/convolutional82/biases"].shape) == (k * k,)
    want = O.init_params(k=k, lock=O.default_lock(1))
    assert {n: tuple(t.shape) for n, t in net.params.items()} == {n: tuple(t.shape) for n, t in want.items()}
    lock = O.default_lock(1)
    assert sorted(net.trainable_names()) == sorted(O.trainable_names(lock))
    assert net.n_decay == sum(want[n].numel() for n in O.regularized_names(lock))
    assert net.n_params == sum(want[n].numel() for n in O.trainable_names(lock))


@pytest.mark.parametrize("k", [5, 7])
def test_plan_only_net_has_a_k_by_k_score_head(k):
    _check_plan(YOLONet(training=True, stage=1, plan_only=True, k_map=k), k)


def test_config_k_map_selects_the_grid(monkeypatch):
    monkeypatch.setattr(cfg, "K_MAP", 5)
    _check_plan(YOLONet(training=True, stage=1, plan_only=True), 5)


@pytest.mark.parametrize("k", [1, 2, 4, 6, 9])
def test_unsupported_k_map_is_refused_before_allocation(k, monkeypatch):
    with pytest.raises(ValueError, match="k_map"):
        YOLONet(training=True, plan_only=True, k_map=k)
    monkeypatch.setattr(cfg, "K_MAP", k)
    with pytest.raises(ValueError, match="k_map"):
        YOLONet(training=False, plan_only=True)


def test_mask_entry_points_refuse_other_k_before_any_launch():
    lib = L.load()
    buf = ctypes.create_string_buffer(1 << 16)
    p = ctypes.cast(buf, ctypes.c_void_p)
    B, sm = 2, 32
    assert lib.disyolo_psroi_loss_workspace(B, sm) <= len(buf)
    for k in (4, 6, 9):
        assert lib.disyolo_mask_rois_k(p, 30, p, 20, p, p, B, sm, k, 7, 3, 0.5, p, p, None) == -1
        assert b"k = 3" in lib.disyolo_last_error()
        assert lib.disyolo_psroi_loss(p, p, 20, p, p, B, sm, k, 5.0, p, p, p, len(buf), None) == -1
        assert b"k = 3" in lib.disyolo_last_error()
        assert lib.disyolo_psroi_assemble(p, p, B, 30, sm, k, p, p, None) == -1
        assert b"k = 3" in lib.disyolo_last_error()
    # the other argument checks still apply at the new k
    assert lib.disyolo_mask_rois_k(p, 30, p, 20, p, p, B, sm, 5, 9, 8, 0.5, p, p, None) == -1
    assert b"n_det + n_gt" in lib.disyolo_last_error()


def test_roi_row_width_matches_the_header():
    assert L.roi_w(3) == L.ROI_W == 12
    text = open(HEADER).read()
    m = re.search(r"#define DISYOLO_ROI_W_K\(k\)\s+(.+)", text)
    assert m, "DISYOLO_ROI_W_K missing from the header"
    expr = m.group(1).split("/*")[0].strip()
    for k in L.K_MAPS:
        assert eval(expr.replace("(k)", "(%d)" % k)) == L.roi_w(k)
    assert L.roi_w(5) == 16 and L.roi_w(7) == 20
    assert [L.block32_post(k) for k in L.K_MAPS] == [1, 2, 3]


def test_k5_checkpoint_round_trip_and_k3_mismatch(tmp_path):
    src = YOLONet(training=True, stage=1, seed=3, plan_only=True, k_map=5)
    with torch.no_grad():
        src.params["yolo/convolutional82/biases"].copy_(torch.arange(25, dtype=torch.float32) * 0.25 - 3.0)
    prefix = str(tmp_path / "model.ckpt-5")
    ck.save_net(src, prefix)
    assert ck.list_variables(prefix)["yolo/convolutional82/weights"] == ((1, 1, 64, 25), ck.DT_FLOAT)
    dst = YOLONet(training=True, stage=1, seed=9, plan_only=True, k_map=5)
    ck.restore_net(dst, prefix)
    assert all(torch.equal(dst.params[n], src.params[n]) for n in src.params)
    k3 = YOLONet(training=True, stage=1, seed=9, plan_only=True)
    with pytest.raises(ValueError, match="convolutional82"):
        ck.restore_net(k3, prefix)

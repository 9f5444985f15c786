"""The reference's three mask-subnet resolutions (m = 1/4, 1/2, 1: yolo/yolo3_net_pos.py:361-378, 380-412, 414-461) on the
CPU side: the layer table and the variables of each stride against a hand table read off the reference, cfg.MASK_STRIDE,
the refusals, checkpoints across strides, and the argument checks of the mask-loss entry at any stride.  No GPU:
plan-only nets and host buffers that a launch would fault on."""
import ctypes

import pytest
import torch

import disyolo_oracle as O
from disyolo_amd import checkpoint as ck
from disyolo_amd import config as cfg
from disyolo_amd import lib as L
from disyolo_amd.net import YOLONet, build_topology
from mask_stride_ref import MASK_LAYERS, SCORE_LAYER, default_lock, mask_layers, regularized_names, variable_shapes


def _spatial(layers, S):
    hw = {0: S}
    for l in layers:
        hw[l.idx] = -(-hw[l.src] // l.stride)
    return hw


@pytest.mark.parametrize("k", [3, 5])
@pytest.mark.parametrize("m", [4, 2, 1])
def test_layer_table_matches_the_reference_subnet(m, k):
    layers = build_topology(3, k, m)
    assert [l.idx for l in layers] == list(range(1, SCORE_LAYER[m] + 1))
    base = build_topology(3, k, 2)
    for a, b in zip(layers[:75], base[:75]):          # backbone and heads: the m = 1/2 table's
        assert (a.idx, a.cin, a.cout, a.k, a.stride, a.kind, a.src, a.src_up, a.shortcut) == \
               (b.idx, b.cin, b.cout, b.k, b.stride, b.kind, b.src, b.src_up, b.shortcut)
    got = [(l.idx, l.cin, l.cout, l.k, l.stride, l.kind, l.src, l.src_up) for l in layers[75:]]
    assert got == mask_layers(m, k)
    for l in layers[75:]:
        cin = layers[l.src - 1].cout + (layers[l.src_up - 1].cout if l.src_up else 0)
        assert l.cin == cin, "conv%d: %d input channels, its sources give %d" % (l.idx, l.cin, cin)
    for S in (576, 96):
        hw = _spatial(layers, S)
        assert hw[SCORE_LAYER[m]] == S // m                 # score maps at S/4, S/2, S
        for l in layers:
            if l.src_up is not None:
                assert hw[l.src] == 2 * hw[l.src_up], "conv%d: the upsampled source does not match the skip" % l.idx


@pytest.mark.parametrize("k", [3, 7])
@pytest.mark.parametrize("m", [4, 2, 1])
def test_plan_only_net_variables_per_stride(m, k):
    net = YOLONet(training=True, stage=1, plan_only=True, k_map=k, mask_stride=m)
    assert net.mask_stride == m and net.score_layer == SCORE_LAYER[m]
    assert {n: tuple(t.shape) for n, t in net.params.items()} == variable_shapes(m, k)
    sl = net.score_layer
    assert tuple(net.params["yolo/convolutional%d/weights" % sl].shape)[-1] == k * k
    assert "yolo/convolutional%d/biases" % sl in net.params
    if m != 2:
        assert "yolo/convolutional82/biases" not in net.params        # conv82 is gone (m = 1/4) or batch-normalised (m = 1)
    lock = default_lock(1, m)
    assert net.lock == lock
    # L2 covers the new score layer's bias and nothing that is batch-normalised
    reg = regularized_names(net.params, lock)
    assert "yolo/convolutional%d/biases" % sl in reg
    assert net.n_decay == sum(net.params[n].numel() for n in reg)
    trainable = [n for n in net.params if not lock[int(n.split("convolutional")[1].split("/")[0])]
                 and not n.endswith("moving_mean") and not n.endswith("moving_variance")]
    assert sorted(net.trainable_names()) == sorted(trainable)
    assert net.n_params == sum(net.params[n].numel() for n in trainable)
    # m = 1/2 is the oracle's own net
    if m == 2:
        want = O.init_params(k=k, lock=O.default_lock(1))
        assert {n: tuple(t.shape) for n, t in net.params.items()} == {n: tuple(t.shape) for n, t in want.items()}


def test_default_stride_is_the_m_half_net():
    assert cfg.MASK_STRIDE == 2
    net = YOLONet(training=True, stage=1, plan_only=True)
    assert net.mask_stride == 2 and net.score_layer == 82 and len(net.layers) == 82


@pytest.mark.parametrize("m", [4, 1])
def test_config_mask_stride_selects_the_subnet(m, monkeypatch):
    monkeypatch.setattr(cfg, "MASK_STRIDE", m)
    net = YOLONet(training=True, stage=1, plan_only=True)
    assert net.mask_stride == m and len(net.layers) == SCORE_LAYER[m]
    assert {n: tuple(t.shape) for n, t in net.params.items()} == variable_shapes(m, cfg.K_MAP)


@pytest.mark.parametrize("m", [0, 3, 8, -2])
def test_unsupported_stride_is_refused_before_allocation(m, monkeypatch):
    with pytest.raises(ValueError, match="mask_stride"):
        YOLONet(training=True, plan_only=True, mask_stride=m)
    with pytest.raises(ValueError, match="mask_stride"):
        build_topology(3, 3, m)
    monkeypatch.setattr(cfg, "MASK_STRIDE", m)
    with pytest.raises(ValueError, match="mask_stride"):
        YOLONet(training=False, plan_only=True)


def test_m1_fp8_with_an_e4m3_act1_is_refused(monkeypatch):
    """m = 1's conv83 reads act1 as a bf16 source: an fp8 backbone that starts at conv1 (DISYOLO_FP8_FROM=1) would hold it
    in e4m3 only -- refused with a clear error (the default fp8 range, conv10-52, keeps act1 bf16)"""
    from disyolo_amd.net import YOLONet as N
    net = N(training=False, plan_only=True, mask_stride=1, dtype="fp8")
    monkeypatch.setattr(N, "FP8_FROM", 1)
    with pytest.raises(L.DisyoloError, match="act1"):
        net._plan_fp8()


@pytest.mark.parametrize("m", [4, 1])
def test_checkpoint_round_trip_per_stride(m, tmp_path):
    src = YOLONet(training=True, stage=1, seed=3, plan_only=True, mask_stride=m)
    sl = src.score_layer
    with torch.no_grad():
        src.params["yolo/convolutional%d/biases" % sl].copy_(torch.arange(9, dtype=torch.float32) * 0.25 - 1.0)
        for n, t in src.params.items():
            if n.endswith("moving_variance"):
                t.uniform_(0.5, 2.0)
    prefix = str(tmp_path / ("model.ckpt-m%d" % m))
    ck.save_net(src, prefix)
    names = ck.list_variables(prefix)
    assert {n: v[0] for n, v in names.items()} == variable_shapes(m, 3)
    dst = YOLONet(training=True, stage=1, seed=9, plan_only=True, mask_stride=m)
    restored = ck.restore_net(dst, prefix)
    assert sorted(restored) == sorted(src.params)
    assert all(torch.equal(dst.params[n], src.params[n]) for n in src.params)


@pytest.mark.parametrize("m_from,m_to,var", [(4, 2, "convolutional79/weights"), (2, 4, "convolutional79/weights"),
                                             (1, 2, "convolutional82/weights"), (2, 1, "convolutional82/weights"),
                                             (4, 1, "convolutional79/weights"), (1, 4, "convolutional79/weights")])
def test_cross_stride_restore_names_the_variable(m_from, m_to, var, tmp_path):
    src = YOLONet(training=True, stage=1, seed=3, plan_only=True, mask_stride=m_from)
    prefix = str(tmp_path / "ck")
    ck.save_net(src, prefix)
    dst = YOLONet(training=True, stage=1, seed=9, plan_only=True, mask_stride=m_to)
    with pytest.raises(ValueError, match=var):
        ck.restore_net(dst, prefix)


@pytest.mark.parametrize("m_from", [4, 2, 1])
@pytest.mark.parametrize("m_to", [4, 2, 1])
def test_stage1_include_restores_layers_1_to_75_into_any_stride(m_from, m_to, tmp_path):
    src = YOLONet(training=True, stage=2, seed=3, plan_only=True, mask_stride=m_from)
    prefix = str(tmp_path / "coco")
    ck.save_net(src, prefix)
    dst = YOLONet(training=True, stage=1, seed=9, plan_only=True, mask_stride=m_to)
    before = {n: t.clone() for n, t in dst.params.items()}
    names = ck.restore_net(dst, prefix, stage1_include=True)
    assert len(names) == 72 * 5 + 3 * 2
    for n in dst.params:
        layer = int(n.split("convolutional")[1].split("/")[0])
        if layer >= 76 or layer in (59, 67, 75) and "BatchNorm" in n:
            assert torch.equal(dst.params[n], before[n]), n
        else:
            assert torch.equal(dst.params[n], src.params[n]), n


def test_psroi_loss_s_refuses_other_strides_before_any_launch():
    lib = L.load()
    buf = ctypes.create_string_buffer(1 << 16)
    p = ctypes.cast(buf, ctypes.c_void_p)
    B, sm = 2, 32
    assert lib.disyolo_psroi_loss_workspace(B, sm) <= len(buf)
    for s in (0, 3, 8, -1):
        assert lib.disyolo_psroi_loss_s(p, p, 20, p, p, B, sm, s, 3, 5.0, p, p, p, len(buf), None) == -1
        assert b"mask_stride" in lib.disyolo_last_error()
    # the other checks apply at every stride
    for s in L.MASK_STRIDES:
        assert lib.disyolo_psroi_loss_s(p, p, 20, p, p, B, sm, s, 4, 5.0, p, p, p, len(buf), None) == -1
        assert b"k = 3" in lib.disyolo_last_error()
        assert lib.disyolo_psroi_loss_s(p, p, 20, p, p, B, sm, s, 3, 5.0, p, p, p, 16, None) != 0
        assert b"workspace" in lib.disyolo_last_error()


def test_conv_takes_16_channel_sources_and_refuses_8_and_24():
    """sources of 16 * n channels are accepted (m = 1's conv83 / conv84 and their data gradients: the direct kernel, one
    statistics row per 64 pixels); C0 = 8 or 24, C1 = 8 are refused before any launch"""
    lib = L.load()
    for c0, c1 in ((8, 0), (24, 0), (32, 8)):
        x0 = torch.zeros(1, 8, 8, c0, dtype=torch.bfloat16)
        x1 = torch.zeros(1, 4, 4, c1, dtype=torch.bfloat16) if c1 else None
        w = torch.zeros(32, c0 + c1, dtype=torch.bfloat16)
        y = torch.zeros(1, 8, 8, 32, dtype=torch.bfloat16)
        d = L.make_conv_desc(x0, w, y, 1, 1, x1=x1)
        assert lib.disyolo_conv2d_fwd(ctypes.byref(d), None) == -1
        assert b"multiple of 16" in lib.disyolo_last_error()
    for c0, c1, ks in ((16, 0, 3), (32, 16, 1), (16, 0, 1), (48, 0, 3)):
        x0 = torch.zeros(2, 10, 6, c0, dtype=torch.bfloat16)
        x1 = torch.zeros(2, 5, 3, c1, dtype=torch.bfloat16) if c1 else None
        w = torch.zeros(32, ks * ks * (c0 + c1), dtype=torch.bfloat16)
        y = torch.zeros(2, 10, 6, 32, dtype=torch.bfloat16)
        d = L.make_conv_desc(x0, w, y, ks, 1, x1=x1)
        assert L.conv2d_tile(d)[0] == 30
        assert L.conv2d_stats_rows(d) == -(-2 * 10 * 6 // 64)
        assert L.conv2d_bn_bwd_stats_ok(d) is False or L.conv2d_bn_bwd_stats_ok(d) == 0
    # 32-channel shapes keep their kernels
    d = L.make_conv_desc(torch.zeros(2, 10, 6, 32, dtype=torch.bfloat16), torch.zeros(32, 288, dtype=torch.bfloat16),
                         torch.zeros(2, 10, 6, 32, dtype=torch.bfloat16), 3, 1)
    assert L.conv2d_tile(d)[0] != 30


"""The C-ABI shared library loads without a GPU and exports every symbol that
include/disyolo.h declares; the ctypes table in lib.py covers the same set."""
import ctypes
import os
import re

import pytest

from disyolo_amd import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_functions():
    src = open(os.path.join(ROOT, "include", "disyolo.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(disyolo_[a-z0-9_]+)\s*\(", src)))


def test_header_declares_the_expected_surface():
    names = declared_functions()
    for must in ("disyolo_conv2d_fwd", "disyolo_conv2d_wgrad", "disyolo_bn_finalize", "disyolo_bn_act_bwd",
                 "disyolo_detect", "disyolo_yolo_loss", "disyolo_psroi_loss", "disyolo_psroi_assemble",
                 "disyolo_adam_step", "disyolo_cmdlist_run", "disyolo_version"):
        assert must in names


def test_library_exports_every_declared_symbol():
    if not os.path.exists(L.LIB_PATH):
        pytest.fail("libdisyolo_hip.so is not built: run `python -c 'import __graft_entry__ as g; g.build()'`")
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in declared_functions():
        assert hasattr(lib, name), "%s declared in include/disyolo.h but not exported" % name


def test_ctypes_table_matches_header():
    assert sorted(L.EXPORTS) == declared_functions()
    assert L.load().disyolo_version() >= 100
    # 16 x int32/float + 8 pointers, + 6 pointers and a float of the batch-norm backward epilogue, + 2 floats (padded) and
    # 12 pointers of the in-launch batch norm (round 6)
    assert ctypes.sizeof(L.ConvDesc) == L.load().disyolo_conv_desc_size() == 288


def test_argument_errors_are_reported_not_thrown():
    # no GPU needed: validation happens before any launch
    lib = L.load()
    d = L.ConvDesc()
    assert lib.disyolo_conv2d_fwd(ctypes.byref(d), None) == -1
    assert b"conv" in lib.disyolo_last_error()
    assert lib.disyolo_cmdlist_run(None, 0, 0, None) == -1
    assert lib.disyolo_adam_step(None, None, None, None, 0, 0, 0.0, 0.0, 0.0, 0.0, 0.0, 0, 1.0, None) == -1
    assert lib.disyolo_detect_workspace(8, 576, 3) > 8 * 20412 * 24


def test_exchange_entry_points_validate_and_resolve_rccl_without_a_gpu():
    """csrc/comm.hip: RCCL is resolved at run time (no link-time dependency: the library above loaded without it being named),
    argument errors come back as codes, and nothing here computes or needs a device"""
    lib = L.load()
    assert L.comm_load() >= 20000                     # RCCL's version code (2.x.y -> 2xxyy), from the copy torch ships
    buf = ctypes.create_string_buffer(64)
    assert lib.disyolo_comm_allreduce_sum(None, buf, 16, 0, None) == -1 and b"comm_allreduce_sum" in lib.disyolo_last_error()
    assert lib.disyolo_comm_allreduce_sum(buf, buf, 16, 7, None) == -1              # unknown dtype code
    assert lib.disyolo_comm_init(buf, 3, 2, None) == -1                               # rank >= nranks / null output
    assert lib.disyolo_comm_destroy(None) == 0
    assert lib.disyolo_cast_f32_bf16(None, buf, 4, None) == -1
    assert lib.disyolo_cmdlist_count(None, 0, 0) == -1
    assert lib.disyolo_cmdlist_lane_stream(None, 1) is None


def test_cmdlist_describe_reports_argument_errors():
    """disyolo_cmdlist_describe reads a recorded list and nothing else: a null list, a null output and an index outside
    [0, size) come back as DISYOLO_E_ARG with a message; a recorded launch reads back as (0, lane, 0, 0)"""
    lib = L.load()
    out = (ctypes.c_int32 * 4)(7, 7, 7, 7)
    assert lib.disyolo_cmdlist_describe(None, 0, out) == -1 and b"cmdlist_describe" in lib.disyolo_last_error()
    prog = L.CmdList()
    assert lib.disyolo_cmdlist_describe(prog.h, 0, out) == -1 and b"outside [0,0)" in lib.disyolo_last_error()     # an empty list
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    with prog:
        L.set_lane(2)
        assert lib.disyolo_add_bf16(p, p, 16, 1, None) == 0          # (records itself: nothing is launched)
    assert prog.size() == 1
    assert lib.disyolo_cmdlist_describe(prog.h, 0, None) == -1 and b"null" in lib.disyolo_last_error()
    for bad in (-1, 1, 2 ** 31 - 1):
        assert lib.disyolo_cmdlist_describe(prog.h, bad, out) == -1 and b"cmdlist_describe: index" in lib.disyolo_last_error()
    assert list(out) == [7, 7, 7, 7]                                 # (a refused call writes nothing)
    assert lib.disyolo_cmdlist_describe(prog.h, 0, out) == 0 and list(out) == [0, 2, 0, 0]
    assert prog.describe() == [(0, 2, 0, 0)]


def test_loss_entry_points_reject_unsupported_arguments_before_any_launch():
    """csrc/loss.hip: each unsupported argument of the three loss kernels comes back as an error code with
    disyolo_last_error set, before anything touches a device (the pointers below are host buffers that a launch
    would fault on)"""
    lib = L.load()
    buf = ctypes.create_string_buffer(1 << 16)
    p = ctypes.cast(buf, ctypes.c_void_p)
    three = (ctypes.c_void_p * 3)(p, p, p)
    anchors = (ctypes.c_float * 18)(*([32.0] * 18))
    scales = (ctypes.c_float * 4)(2.0, 1.0, 1.0, 1.0)
    B, S = 2, 64
    need = lib.disyolo_yolo_loss_workspace(B, S, 3)
    assert 0 < need <= len(buf)

    def yolo(max_boxes=20, S=S, num_class=3, ws_bytes=len(buf)):
        return lib.disyolo_yolo_loss(three, three, p, max_boxes, B, S, num_class, anchors, 0.5, scales, three, p, p,
                                     ws_bytes, None)

    assert yolo(max_boxes=65) == -1 and b"max_boxes" in lib.disyolo_last_error()
    assert yolo(max_boxes=0) == -1 and b"max_boxes" in lib.disyolo_last_error()
    assert yolo(num_class=6) == -1 and b"bad sizes" in lib.disyolo_last_error()      # 3 * (5 + 6) > 32 padded channels
    assert yolo(num_class=0) == -1 and b"bad sizes" in lib.disyolo_last_error()
    assert yolo(S=80) == -1 and b"bad sizes" in lib.disyolo_last_error()             # not a multiple of 32
    assert yolo(ws_bytes=need - 1) == -2 and b"workspace" in lib.disyolo_last_error()   # DISYOLO_E_WORKSPACE

    def rois(n_det, n_gt):
        return lib.disyolo_mask_rois(p, 30, p, 20, p, p, B, S // 2, n_det, n_gt, 0.5, p, p, None)

    assert rois(9, 8) == -1 and b"n_det + n_gt" in lib.disyolo_last_error()           # 17 > DISYOLO_ROI_MAX
    assert rois(-1, 3) == -1

    def psroi(k):
        return lib.disyolo_psroi_loss(p, p, 20, p, p, B, S // 2, k, 5.0, p, p, p, len(buf), None)

    assert lib.disyolo_psroi_loss_workspace(B, S // 2) <= len(buf)
    for k in (2, 4):
        assert psroi(k) == -1 and b"k = 3" in lib.disyolo_last_error()

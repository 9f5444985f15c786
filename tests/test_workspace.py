"""The workspace contract without a GPU (include/disyolo.h, "Workspaces"): the test helper tests/workspace_guard.py checked on
the CPU before any entry-point test relies on it, and rule 4 -- one byte less than the size query's answer is refused with
DISYOLO_E_WORKSPACE before any launch -- for every entry point that takes a ``workspace`` / ``workspace_bytes`` pair.  Rules
1 to 3 need a device: tests/test_gpu_workspace.py."""
import ctypes
import os
import re

import pytest
import torch

from disyolo_amd import lib as L
from workspace_guard import GUARD_BYTE, GuardedWorkspace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_WORKSPACE = -2


def workspace_entry_points():
    """the functions of include/disyolo.h that take a ``workspace_bytes`` parameter"""
    src = open(os.path.join(ROOT, "include", "disyolo.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    found = re.findall(r"\b(disyolo_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", src, flags=re.S)
    return sorted(name for name, args in found if re.search(r"\bworkspace_bytes\b", args))


# ------------------------------------------------------------------------------------------------ the helper itself
def test_guarded_workspace_hands_out_exact_views_at_one_address():
    ws = GuardedWorkspace("cpu", poison=0xFF, guard=4096, capacity=1 << 16)
    sizes = (1000, 1, 4096, 777, 1 << 16)
    first = ws.get(sizes[0])
    for n in sizes:
        v = ws.get(n)
        assert v.dtype == torch.uint8 and v.numel() == n and v.is_contiguous()
        assert v.data_ptr() == first.data_ptr() and v.data_ptr() % 256 == 0
        assert bool((v == 0xFF).all())
    assert ws.high_water == 1 << 16 and ws.buf.numel() == 1 << 16
    ws.check()
    assert ws.interior_untouched()
    assert ws.get(0).numel() == 0


def test_guarded_workspace_keeps_its_guards_around_the_largest_request():
    ws = GuardedWorkspace("cpu", poison=0x3F, guard=512, capacity=8192)
    ws.get(100)
    assert ws.high_water == 100
    big = ws.get(3000)
    small = ws.get(40)
    assert ws.high_water == 3000 and small.numel() == 40
    # the bytes around the largest view hold the guard pattern, `guard` of them on either side, poison beyond
    s = ws._start
    assert bool((ws._all[s - 512:s] == GUARD_BYTE).all()) and bool((ws._all[s + 3000:s + 3512] == GUARD_BYTE).all())
    assert int(ws._all[s + 3512]) == 0x3F and int(ws._all[s + 100]) == 0x3F
    big[17] = 5                                       # a write INSIDE the view is what the workspace is for
    ws.check()
    assert not ws.interior_untouched()
    ws.repoison()
    assert ws.interior_untouched() and int(big[17]) == 0x3F
    ws.check()


def test_guarded_workspace_catches_one_byte_behind_and_one_in_front():
    for where, offset in (("behind", 0), ("behind", 511), ("in front of", -1), ("in front of", -512)):
        ws = GuardedWorkspace("cpu", poison=0xFF, guard=512, capacity=4096)
        ws.get(1000)
        at = ws._start + (1000 + offset if where == "behind" else offset)
        ws._all[at] = 0
        with pytest.raises(AssertionError) as e:
            ws.check()
        rel = at - (ws._start + 1000)
        assert where in str(e.value) and ("%+d .. %+d" % (rel, rel)) in str(e.value), str(e.value)
    # the first and the last offending byte are both named
    ws = GuardedWorkspace("cpu", poison=0xFF, guard=512, capacity=4096)
    ws.get(64)
    ws._all[ws._start + 64 + 3] = 1
    ws._all[ws._start + 64 + 200] = 1
    with pytest.raises(AssertionError, match=r"2 bytes .* \+3 \.\. \+200"):
        ws.check()
    # an over-run is not lost when a larger request moves the rear guard: the move looks at the guard first
    ws = GuardedWorkspace("cpu", poison=0xFF, guard=512, capacity=4096)
    ws.get(64)
    ws._all[ws._start + 64] = 9
    with pytest.raises(AssertionError, match="behind"):
        ws.get(2000)


def test_guarded_workspace_refuses_to_grow_past_its_capacity():
    ws = GuardedWorkspace("cpu", poison=0xFF, guard=256, capacity=4096)
    ws.get(4096)
    with pytest.raises(L.DisyoloError, match="never moves"):
        ws.get(4097)
    ws.check()
    with pytest.raises(ValueError):
        GuardedWorkspace("cpu", poison=GUARD_BYTE)


# ------------------------------------------------------------------------------------------------ rule 4
# Host buffers as pointers, as in tests/test_abi.py: a launch would fault on them, so a refusal here is a refusal before any
# launch.  Every entry point checks its arguments and its workspace on the host before it touches the device, so none is
# excluded (the list below is empty); disyolo_yolo_loss and disyolo_detect_x have this assertion already.
ASSERTED_ELSEWHERE = {
    "disyolo_yolo_loss": "tests/test_abi.py, test_loss_entry_points_reject_unsupported_arguments_before_any_launch",
    "disyolo_detect_x": "tests/test_limits.py, test_detect_x_rejects_bad_arguments_before_any_launch",
}
TOUCHES_THE_DEVICE_FIRST = {}     # entry point -> the source line that validates a pointer on the device before the size check


def _short_calls():
    """entry point -> (need, call(workspace_bytes) -> return code); ``need`` from the size query, or from the formula
    lib.py restates where the entry point has none"""
    lib = L.load()
    buf = ctypes.create_string_buffer(1 << 20)
    p = ctypes.cast(buf, ctypes.c_void_p)
    three = (ctypes.c_void_p * 3)(p, p, p)
    anchors = (ctypes.c_float * 18)(*([32.0] * 18))
    scales = (ctypes.c_float * 4)(2.0, 1.0, 1.0, 1.0)
    host = torch.zeros(4, dtype=torch.bfloat16)
    calls = {}

    def desc(B, H, W, Cin, Cout, k, s):
        x = torch.zeros(B, H, W, Cin, dtype=torch.bfloat16)
        y = torch.zeros(B, (H + s - 1) // s, (W + s - 1) // s, Cout, dtype=torch.bfloat16)
        return L.make_conv_desc(x, host, y, k, s)

    for tag, d in (("im2col", desc(2, 18, 18, 256, 24, 1, 1)), ("tap-fused", desc(2, 18, 18, 64, 128, 3, 1))):
        assert L.conv2d_wgrad_plan(d)[0] == (tag == "tap-fused")
        calls["disyolo_conv2d_wgrad/" + tag] = (
            lib.disyolo_conv2d_wgrad_workspace(ctypes.byref(d), 0),
            lambda n, d=d: lib.disyolo_conv2d_wgrad(ctypes.byref(d), p, d.Cout + (-d.Cout) % 8, p, p, n, 0, None))
    calls["disyolo_conv_first_wgrad"] = (lib.disyolo_conv_first_wgrad_workspace(2, 33, 128, 32),
                                         lambda n: lib.disyolo_conv_first_wgrad(p, p, p, 2, 33, 128, 32, p, n, None))
    rows, Cn = 777, 200
    calls["disyolo_bn_act_bwd"] = (lib.disyolo_bn_act_bwd_workspace(rows, Cn),
                                   lambda n: lib.disyolo_bn_act_bwd(p, p, p, p, p, p, p, p, p, rows, Cn, 0.1, None, 0, p, n, None))
    calls["disyolo_bn_act_bwd_partials"] = (
        lib.disyolo_bn_act_bwd_partials_workspace(Cn),
        lambda n: lib.disyolo_bn_act_bwd_partials(p, p, p, p, p, p, p, p, p, rows, Cn, 0.1, p, 4, None, 0, p, n, None))
    calls["disyolo_bn_bwd_reduce"] = (lib.disyolo_bn_bwd_reduce_rows(rows, Cn) * Cn * 2 * 4,      # lib.bn_bwd_reduce
                                      lambda n: lib.disyolo_bn_bwd_reduce(p, p, p, p, p, p, rows, Cn, 0.1, p, p, n, None))
    calls["disyolo_bn_bwd_apply_sums"] = (
        2 * Cn * 4,                                                                               # lib.bn_bwd_apply_sums
        lambda n: lib.disyolo_bn_bwd_apply_sums(p, p, p, p, p, p, p, p, 2 * rows, p, p, p, rows, Cn, 0.1, None, 0, p, n, None))
    calls["disyolo_colsum"] = (lib.disyolo_colsum_workspace(rows, Cn), lambda n: lib.disyolo_colsum(p, p, rows, Cn, 24, p, n, None))
    B, S = 2, 64
    for Cd in (3, 80):
        calls["disyolo_detect/C=%d" % Cd] = (
            lib.disyolo_detect_workspace(B, S, Cd),
            lambda n, Cd=Cd: lib.disyolo_detect(p, p, p, B, S, Cd, anchors, p, 0.25, 0.3, 64 if Cd > 16 else 30, p, p, p, n, None))
        calls["disyolo_detect_hw/C=%d" % Cd] = (
            lib.disyolo_detect_workspace_hw(B, S, 96, Cd),
            lambda n, Cd=Cd: lib.disyolo_detect_hw(p, p, p, B, S, 96, Cd, anchors, p, 0.25, 0.3, 30, p, p, p, n, None))
        for mode in (0, 1, 2):
            calls["disyolo_detect_nms_hw/C=%d,mode=%d" % (Cd, mode)] = (
                lib.disyolo_detect_workspace_hw(B, S, 96, Cd),
                lambda n, Cd=Cd, mode=mode: lib.disyolo_detect_nms_hw(p, p, p, B, S, 96, Cd, anchors, p, 0.25, 0.3, 30, mode, p, p, p,
                                                                      n, None))
    calls["disyolo_yolo_loss_wide"] = (
        lib.disyolo_yolo_loss_workspace(B, S, 80),
        lambda n: lib.disyolo_yolo_loss_wide(three, three, p, 20, B, S, 80, 256, anchors, 0.5, scales, three, p, p, n, None))
    for ld, Cl in ((0, 3), (256, 80)):
        calls["disyolo_yolo_loss_hw/ld=%d" % ld] = (
            lib.disyolo_yolo_loss_workspace_hw(B, S, 96, Cl),
            lambda n, ld=ld, Cl=Cl: lib.disyolo_yolo_loss_hw(three, three, p, 256, B, S, 96, Cl, ld, anchors, 0.5, scales, three, p,
                                                             p, n, None))
    calls["disyolo_psroi_loss"] = (lib.disyolo_psroi_loss_workspace(B, 32),
                                   lambda n: lib.disyolo_psroi_loss(p, p, 20, p, p, B, 32, 3, 5.0, p, p, p, n, None))
    calls["disyolo_psroi_loss_s"] = (lib.disyolo_psroi_loss_workspace(B, 32),
                                     lambda n: lib.disyolo_psroi_loss_s(p, p, 20, p, p, B, 32, 1, 5, 5.0, p, p, p, n, None))
    calls["disyolo_psroi_loss_hw"] = (lib.disyolo_psroi_loss_workspace_hw(B, 32, 48),
                                      lambda n: lib.disyolo_psroi_loss_hw(p, p, 20, p, p, B, 32, 48, 2, 7, 5.0, p, p, p, n, None))
    for cap in (17, 512):
        calls["disyolo_psroi_loss_x/cap=%d" % cap] = (
            lib.disyolo_psroi_loss_workspace_x(B, 32, 48, cap),
            lambda n, cap=cap: lib.disyolo_psroi_loss_x(p, p, 20, p, p, cap, B, 32, 48, 2, 3, 5.0, p, p, p, n, None))
    nw = 4096 * 3 + 5
    calls["disyolo_adam_step_fused"] = (
        lib.disyolo_adam_fused_workspace(nw),
        lambda n: lib.disyolo_adam_step_fused(p, p, p, p, nw, nw, p, 0.9, 0.999, 1e-8, 5e-4, p, 1.0, p, p, n, None))
    calls["disyolo_l2_loss"] = (lib.disyolo_l2_workspace(nw), lambda n: lib.disyolo_l2_loss(p, nw, 5e-4, p, p, n, None))
    return calls, len(buf), (buf, host)


_CALLS = None


def short_calls():
    global _CALLS
    if _CALLS is None:
        _CALLS = _short_calls()
    return _CALLS


CASES = (["disyolo_conv2d_wgrad/im2col", "disyolo_conv2d_wgrad/tap-fused", "disyolo_conv_first_wgrad", "disyolo_bn_act_bwd",
          "disyolo_bn_act_bwd_partials", "disyolo_bn_bwd_reduce", "disyolo_bn_bwd_apply_sums", "disyolo_colsum"] +
         ["disyolo_%s/C=%d" % (f, c) for f in ("detect", "detect_hw") for c in (3, 80)] +
         ["disyolo_detect_nms_hw/C=%d,mode=%d" % (c, m) for c in (3, 80) for m in (0, 1, 2)] +
         ["disyolo_yolo_loss_wide", "disyolo_yolo_loss_hw/ld=0", "disyolo_yolo_loss_hw/ld=256", "disyolo_psroi_loss",
          "disyolo_psroi_loss_s", "disyolo_psroi_loss_hw", "disyolo_psroi_loss_x/cap=17", "disyolo_psroi_loss_x/cap=512",
          "disyolo_adam_step_fused", "disyolo_l2_loss"])


def case_ids():
    return list(CASES)


def test_the_case_list_names_every_short_call():
    assert sorted(CASES) == sorted(short_calls()[0])


@pytest.mark.parametrize("case", CASES)
def test_one_byte_short_is_refused_before_any_launch(case):
    calls, room, _ = short_calls()
    need, call = calls[case]
    assert 0 < need <= room, "the size query of %s answers %d" % (case, need)
    lib = L.load()
    assert call(need - 1) == E_WORKSPACE, (case, lib.disyolo_last_error())
    assert b"workspace" in lib.disyolo_last_error(), (case, lib.disyolo_last_error())
    assert call(0) == E_WORKSPACE


def test_every_workspace_entry_point_of_the_header_is_held_to_rule_4():
    names = workspace_entry_points()
    assert len(names) >= 20 and "disyolo_conv2d_wgrad" in names and "disyolo_l2_loss" in names, names
    covered = {c.split("/")[0] for c in case_ids()}
    assert not covered & set(ASSERTED_ELSEWHERE) and not covered & set(TOUCHES_THE_DEVICE_FIRST)
    missing = [n for n in names if n not in covered and n not in ASSERTED_ELSEWHERE and n not in TOUCHES_THE_DEVICE_FIRST]
    assert not missing, "no one-byte-short test for %s" % missing
    unknown = [n for n in sorted(covered | set(ASSERTED_ELSEWHERE) | set(TOUCHES_THE_DEVICE_FIRST)) if n not in names]
    assert not unknown, "%s take no workspace_bytes in include/disyolo.h" % unknown

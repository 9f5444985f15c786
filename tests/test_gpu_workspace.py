"""The workspace contract on the GPU (include/disyolo.h, "Workspaces"), for every entry point that takes a ``workspace`` /
``workspace_bytes`` pair:

1. with ``workspace_bytes`` exactly what the size query (or lib.py's formula) answers, the call succeeds;
2. it writes nothing outside ``[workspace, workspace + need)``;
3. its outputs do not depend on what the workspace held before the call;
(4. one byte less is refused before any launch: tests/test_workspace.py, without a GPU).

``lib.Workspace`` hands out its whole buffer of at least 1 MiB, which a fresh allocation usually returns zeroed: with it an
under-reporting query, a carve past the reported size or a read of scratch nobody wrote cannot fail.  Every case below calls
its entry point three times on the same inputs -- (a) an ordinary zero-filled ``lib.Workspace``, (b) and (c) a
``workspace_guard.GuardedWorkspace`` of exactly the requested size between guard bands, filled with 0xFF (NaN as f32 / bf16,
-1 as int32) and with 0x3F (0.747 as f32, finite where a comparison would drop a NaN; 1061109567 as int32) -- and holds (b)
and (c) to (a) bit for bit: these paths all sum in a fixed order.  Agreement with float64 stays the business of the
per-kernel tests.  Nothing here passes less than the query's answer and nothing is meant to fault: an over-run lands in the
helper's own guard."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import disyolo_oracle as O
import limits_ref as LR
import mask_roi_ref as MR
from disyolo_amd import config as cfg
from disyolo_amd import lib as L
from disyolo_amd.net import YOLONet
from workspace_guard import GuardedWorkspace

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ANCH = np.asarray(cfg.ANCHORS, np.float32)
BF16, F32 = torch.bfloat16, torch.float32
POISONS = (0xFF, 0x3F)


def bits(t):
    """an integer view: NaN == NaN holds, and -0.0 != 0.0"""
    t = t.contiguous()
    if not t.is_floating_point():
        return t
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def nan(shape, dtype, dev):
    return torch.full(tuple(shape), float("nan"), dtype=dtype, device=dev)


def minus1(shape, dev, dtype=torch.int32):
    return torch.full(tuple(shape), -1, dtype=dtype, device=dev)


def vp(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ok(rc, what):
    assert rc == 0, "%s failed (%d): %s" % (what, rc, L.load().disyolo_last_error().decode())


class Case:
    """``run(ws)`` makes the call on fresh outputs (prefilled with NaN / -1 where the entry point defines every element) and
    returns them as a dict; ``need``: the size query's answer, which is what the call must request; ``entries``: the C entry
    points the call goes through; ``untouched``: the call must leave its workspace as it found it; ``no_workspace``: the call
    takes none (and ``run`` gets one it must not use)"""

    def __init__(self, run, need, entries, untouched=False, no_workspace=False):
        self.run, self.need, self.entries, self.untouched, self.no_workspace = run, int(need), tuple(entries), untouched, no_workspace


def rnd(g, *shape, dtype=BF16, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(dtype)


# ------------------------------------------------------------------------------------------------ weight gradients
def wgrad_case(B, H, W, Cin, Cout, k, s, kind, split, up=0):
    """``up``: channels of a half-resolution second input (the fused upsample + concat of the 1x1 layers)"""
    def build(dev):
        g = torch.Generator().manual_seed(B + H + W + Cin + Cout + k + s)
        x = rnd(g, B, H, W, Cin).to(dev)
        x1 = rnd(g, B, H // 2, W // 2, up).to(dev) if up else None
        Ho, Wo = (H + s - 1) // s, (W + s - 1) // s
        ld = ((Cout + 31) // 32) * 32 if Cout % 8 else Cout
        dy = torch.zeros(B, Ho, Wo, ld, dtype=BF16)
        dy[..., :Cout] = rnd(g, B, Ho, Wo, Cout)
        dy = dy.to(dev)
        d = L.make_conv_desc(x, torch.empty(1, dtype=BF16, device=dev), torch.empty(B, Ho, Wo, Cout, dtype=BF16, device=dev), k, s,
                             x1=x1)
        plan = L.conv2d_wgrad_plan(d)
        assert plan[0] == kind and (plan[3] > 1) == split, "the case left its branch: plan %s" % (plan,)

        def run(ws):
            dw = nan((k, k, Cin + up, Cout), F32, dev)
            L.conv2d_wgrad(d, dy, ld, dw, ws)
            return {"dw": dw}
        return Case(run, L.conv2d_wgrad_workspace(d), ["disyolo_conv2d_wgrad"], untouched=not split)
    return build


def first_wgrad_case(B, H, W, Cout=32):
    """Cout = 32 is the matrix-core kernel (the layer as the net builds it); any other count takes the direct kernel, whose
    slabs are carved as ceil(B H W / 1024) x 27 x Cout floats.  No other test runs that kernel, so its case also holds the
    result to float64: a thread adds at most 1024 products in f32, one after the other, and the slab pass adds the blocks'
    sums, so |error| <= (1024 + blocks + 1) 2^-24 sum |x dy| (the running-sum bound, first order), with the image in f32 as
    the kernel reads it and dy the bf16 values both sides share."""
    def build(dev):
        g = torch.Generator().manual_seed(B * 7 + H + W + Cout)
        img = torch.rand(B, H, W, 3, generator=g) * 2 - 1
        dy = rnd(g, B, H, W, Cout)
        imgd, dyd = img.to(dev), dy.to(dev)

        def run(ws):
            dw = nan((3, 3, 3, Cout), F32, dev)
            L.conv_first_wgrad(imgd, dyd, dw, ws)
            return {"dw": dw}
        case = Case(run, L.load().disyolo_conv_first_wgrad_workspace(B, H, W, Cout), ["disyolo_conv_first_wgrad"])
        if Cout != 32:
            def verify(out):
                def grad_of(x, d):
                    w = torch.zeros(3, 3, 3, Cout, dtype=torch.float64, requires_grad=True)
                    O.conv2d_same(x, w, 1).backward(d)
                    return w.grad
                want = grad_of(img.double(), dy.double())
                mag = grad_of(img.double().abs(), dy.double().abs())
                blocks = -(-B * H * W // 1024)
                assert blocks > 1
                err = (out["dw"].double().cpu() - want).abs()
                tol = (1024 + blocks + 1) * 2.0 ** -24 * mag
                print("direct first-layer weight gradient: max |err| %.3g, smallest bound %.3g, max |want| %.3g"
                      % (float(err.max()), float(tol.min()), float(want.abs().max())))
                assert (err <= tol).all(), "max |err| / bound %.3g" % float((err / tol).max())
            case.verify = verify
        return case
    return build


# ------------------------------------------------------------------------------------------------ batch norm backward, colsum
def bn_inputs(dev, rows, Cn, seed=0):
    g = torch.Generator().manual_seed(rows + Cn + seed)
    x = rnd(g, rows, Cn, scale=1.5).to(dev)
    dy = rnd(g, rows, Cn).to(dev)
    mean = x.float().mean(0)
    rstd = 1.0 / torch.sqrt(x.float().var(0, unbiased=False) + 1e-5)
    scale = torch.randn(Cn, generator=g).to(dev) * rstd
    shift = (torch.randn(Cn, generator=g) * 0.3).to(dev) - mean * scale
    return dy, x, scale.contiguous(), shift.contiguous(), mean.contiguous(), rstd.contiguous()


def bn_outputs(dev, rows, Cn, shortcut):
    out = {"dx": nan((rows, Cn), BF16, dev), "dgamma": nan((Cn,), F32, dev), "dbeta": nan((Cn,), F32, dev)}
    if shortcut:
        out["shortcut_grad"] = nan((rows, Cn), BF16, dev)      # (not accumulating: every element is written)
    return out


def bn_act_bwd_case(rows, Cn, shortcut):
    def build(dev):
        dy, x, scale, shift, mean, rstd = bn_inputs(dev, rows, Cn)

        def run(ws):
            o = bn_outputs(dev, rows, Cn, shortcut)
            L.bn_act_bwd(dy, x, scale, shift, mean, rstd, o["dx"], o["dgamma"], o["dbeta"], rows, Cn, ws, 0.1,
                         shortcut_grad=o.get("shortcut_grad"))
            return o
        return Case(run, L.load().disyolo_bn_act_bwd_workspace(rows, Cn), ["disyolo_bn_act_bwd"])
    return build


def bn_partials_case(B, H, W, Cin, Cout, tile):
    """the partial sums of a patch conv's epilogue, as tests/test_gpu_conv.py
    test_bn_act_bwd_from_conv_partials_matches_the_plain_path makes them"""
    def build(dev):
        g = torch.Generator().manual_seed(5)
        xin = rnd(g, B, H, W, Cin).to(dev)
        w = rnd(g, Cout, 9 * Cin, scale=1.0 / (9 * Cin) ** 0.5).to(dev)
        rows = B * H * W
        _, raw, scale, shift, mean, rstd = bn_inputs(dev, rows, Cout, seed=1)
        dy = torch.empty(B, H, W, Cout, dtype=BF16, device=dev)
        probe = L.make_conv_desc(xin, w, dy, 3, 1, tile=tile)
        assert L.conv2d_bn_bwd_stats_ok(probe)
        prow = L.conv2d_stats_rows(probe)
        part = nan((prow, Cout, 2), F32, dev)
        L.conv2d_fwd(L.make_conv_desc(xin, w, dy, 3, 1, tile=tile, bn_bwd=(raw, scale, shift, mean, rstd, part, 0.1)))
        torch.cuda.synchronize()
        assert torch.isfinite(part).all()

        def run(ws):
            o = bn_outputs(dev, rows, Cout, True)
            L.bn_act_bwd_partials(dy, raw, scale, shift, mean, rstd, o["dx"], o["dgamma"], o["dbeta"], rows, Cout, part, prow, ws,
                                  0.1, shortcut_grad=o["shortcut_grad"])
            return o
        return Case(run, L.load().disyolo_bn_act_bwd_partials_workspace(Cout), ["disyolo_bn_act_bwd_partials"])
    return build


def bn_reduce_case(rows, Cn):
    def build(dev):
        dy, x, scale, shift, mean, rstd = bn_inputs(dev, rows, Cn)

        def run(ws):
            sums = nan((Cn, 2), torch.float64, dev)
            L.bn_bwd_reduce(dy, x, scale, shift, mean, rstd, rows, Cn, sums, ws, 0.1)
            return {"sums": sums}
        # no size query: the formula lib.bn_bwd_reduce restates, here from the documented layout (rows x C x 2 floats)
        return Case(run, L.load().disyolo_bn_bwd_reduce_rows(rows, Cn) * Cn * 2 * 4, ["disyolo_bn_bwd_reduce"])
    return build


def bn_apply_sums_case(rows, Cn):
    def build(dev):
        dy, x, scale, shift, mean, rstd = bn_inputs(dev, rows, Cn)
        local = torch.zeros(Cn, 2, dtype=torch.float64, device=dev)
        L.bn_bwd_reduce(dy, x, scale, shift, mean, rstd, rows, Cn, local, L.Workspace(dev), 0.1)
        glob = local * 2.25                                     # "the other ranks": count = 2 x rows

        def run(ws):
            o = bn_outputs(dev, rows, Cn, True)
            L.bn_bwd_apply_sums(dy, x, scale, shift, mean, rstd, local, glob, 2 * rows, o["dx"], o["dgamma"], o["dbeta"], rows, Cn,
                                ws, 0.1, shortcut_grad=o["shortcut_grad"])
            return o
        return Case(run, 2 * Cn * 4, ["disyolo_bn_bwd_apply_sums"])      # cA / cC: 2 x C floats (include/disyolo.h)
    return build


def colsum_case(rows, Cn, out_C):
    def build(dev):
        g = torch.Generator().manual_seed(rows + Cn)
        x = rnd(g, rows, Cn).to(dev)

        def run(ws):
            out = nan((out_C,), F32, dev)
            L.colsum(x, out, rows, Cn, out_C, ws)
            return {"out": out}
        return Case(run, L.load().disyolo_colsum_workspace(rows, Cn), ["disyolo_colsum"])
    return build


# ------------------------------------------------------------------------------------------------ the detection filter
def rect_logits(Cn, H, W, B=2):
    """limits_ref.filter_logits on a rectangular net"""
    g = torch.Generator().manual_seed(300 + Cn + H + W)
    ys = [torch.randn(B, H // d, W // d, 3, 5 + Cn, generator=g) for d in (8, 16, 32)]
    for y in ys:
        y[..., 2:4] *= 0.3
        y[..., 4] = torch.round(y[..., 4] * 1.5) + 3.0
        y[..., 5:] = torch.round(y[..., 5:]) * 40.0
    return ys


def detect_case(Cn, D, mode="per_class", size=LR.FILTER_S, entry=None):
    """``entry`` None: lib.detect, which takes disyolo_detect_x or disyolo_detect_nms_hw by the sizes; else that C entry point"""
    def build(dev):
        lib = L.load()
        H, W = L.hw_of(size)
        B = LR.FILTER_B
        ys = LR.filter_logits(Cn) if H == W == LR.FILTER_S else rect_logits(Cn, H, W)
        logits = [y.reshape(B, y.shape[1], y.shape[2], 3 * (5 + Cn)).contiguous().to(dev) for y in ys]
        win = torch.as_tensor(LR.FILTER_WIN, device=dev).float()
        anc = LR.FILTER_ANCH.reshape(-1)
        canc = (C.c_float * 18)(*[float(v) for v in anc])
        takes_x = L.detect_takes_x(Cn, D)
        if entry is None:
            need = lib.disyolo_detect_workspace_x(B, H, W, Cn, D) if takes_x else lib.disyolo_detect_workspace_hw(B, H, W, Cn)
            entries = ["disyolo_detect_x" if takes_x else "disyolo_detect_nms_hw"]
            assert need == L.detect_workspace(B, (H, W), Cn, D)
        else:
            assert not takes_x and mode == "per_class"
            need = lib.disyolo_detect_workspace(B, H, Cn) if entry == "disyolo_detect" else lib.disyolo_detect_workspace_hw(B, H, W, Cn)
            entries = [entry]

        def run(ws):
            det, cnt = nan((B, D, 6), F32, dev), minus1((B,), dev)
            if entry is None:
                L.detect(logits[0], logits[1], logits[2], B, (H, W), Cn, anc, win, LR.FILTER_THR, LR.FILTER_NMS, D, det, cnt, ws,
                         nms=mode)
            else:
                buf = ws.get(need)
                size_args = (B, H, Cn) if entry == "disyolo_detect" else (B, H, W, Cn)
                ok(getattr(lib, entry)(vp(logits[0]), vp(logits[1]), vp(logits[2]), *size_args, canc, vp(win), LR.FILTER_THR,
                                       LR.FILTER_NMS, D, vp(det), vp(cnt), vp(buf), buf.numel(), stream()), entry)
            return {"detections": det, "det_count": cnt}
        case = Case(run, need, entries)
        case.min_count = min(D, 30)      # the logits put far more candidates than that above the threshold
        return case
    return build


# ------------------------------------------------------------------------------------------------ the YOLO loss
def rect_yolo_inputs(B, H, W, Cn, G, seed):
    """random heads, a few boxes in image 1 (none in image 0) and their dense labels on an H x W net"""
    rng = np.random.RandomState(seed)
    D = 5 + Cn
    grids = [(H // d, W // d) for d in (8, 16, 32)]
    heads = [rng.randn(B, gh, gw, 3, D).astype(np.float32) for gh, gw in grids]
    labels = [np.zeros((B, gh, gw, 3, D), np.float32) for gh, gw in grids]
    tb = np.zeros((B, G, 5), np.float32)
    for r in range(0, G, max(G // 12, 1)):
        w, h = rng.uniform(0.05, 0.5, size=2)
        xc, yc = rng.uniform(w / 2, 1 - w / 2), rng.uniform(h / 2, 1 - h / 2)
        c = rng.randint(0, Cn)
        tb[1, r] = [xc, yc, w, h, c]
        s, a = rng.randint(0, 3), rng.randint(0, 3)
        gh, gw = grids[s]
        cell = labels[s][1, min(int(yc * gh), gh - 1), min(int(xc * gw), gw - 1), a]
        cell[:] = 0
        cell[0:5] = [xc, yc, w, h, 1.0]
        cell[5 + c] = 1.0
    return heads, labels, tb


def yolo_case_of(Cn, size, G, ld, entry=None):
    """``entry`` None: lib.yolo_loss / lib.yolo_loss_wide (disyolo_yolo_loss_hw); else that C entry point, a square net"""
    def build(dev):
        lib = L.load()
        H, W = L.hw_of(size)
        B = 2
        if H == W and Cn == 3:
            from test_gpu_loss import yolo_case
            heads, labels, tb = yolo_case(B, H, Cn, G, 41, cfg.IGNORE_THRESH)
        else:
            heads, labels, tb = rect_yolo_inputs(B, H, W, Cn, G, 43)
        lg = [torch.from_numpy(h).to(dev).contiguous() for h in heads]
        lb = [torch.from_numpy(l).to(dev).contiguous() for l in labels]
        tbd = torch.from_numpy(tb).to(dev).contiguous()
        scales = (O.OBJECT_SCALE, O.NOOBJECT_SCALE, O.CLASS_SCALE, O.COORD_SCALE)
        need = lib.disyolo_yolo_loss_workspace_hw(B, H, W, Cn) if entry is None else lib.disyolo_yolo_loss_workspace(B, H, Cn)

        def run(ws):
            dl = [nan((B, h.shape[1], h.shape[2], ld or L.GRAD_LD), BF16, dev) for h in heads]
            losses = nan((8,), F32, dev)
            if entry is None and ld:
                L.yolo_loss_wide(lg, lb, tbd, G, B, (H, W), Cn, ld, ANCH.reshape(-1), cfg.IGNORE_THRESH, scales, dl, losses, ws)
            elif entry is None:
                L.yolo_loss(lg, lb, tbd, G, B, (H, W), Cn, ANCH.reshape(-1), cfg.IGNORE_THRESH, scales, dl, losses, ws)
            else:
                buf = ws.get(need)
                arr = lambda ts: (C.c_void_p * 3)(*[t.data_ptr() for t in ts])
                head = (arr(lg), arr(lb), vp(tbd), G, B, H, Cn) + ((ld,) if entry == "disyolo_yolo_loss_wide" else ())
                ok(getattr(lib, entry)(*head, (C.c_float * 18)(*[float(v) for v in ANCH.reshape(-1)]), cfg.IGNORE_THRESH,
                                       (C.c_float * 4)(*scales), arr(dl), vp(losses), vp(buf), buf.numel(), stream()), entry)
            return {"losses": losses, "dl3": dl[0], "dl2": dl[1], "dl1": dl[2]}
        return Case(run, need, [entry or "disyolo_yolo_loss_hw"])
    return build


# ------------------------------------------------------------------------------------------------ the mask loss
def psroi_case(nrow, map_size, k, st, entry=None, empty_image=False):
    """tables and inputs of tests/mask_roi_ref.py at B = 2.  ``entry`` None: lib.psroi_loss (disyolo_psroi_loss_hw) up to
    DISYOLO_ROI_MAX rows, lib.psroi_loss_x above; else that C entry point, a square map.  ``empty_image``: roi_count == 0 in
    the second image"""
    def build(dev):
        lib = L.load()
        Hm, Wm = L.hw_of(map_size)
        B = 2
        table, cnt = MR.loss_table(nrow, Hm, Wm, k, B=B)
        score, tm = MR.loss_inputs(Hm, Wm, k, st, B=B)
        cnt = np.array(cnt, np.int32)
        assert cnt[0] == nrow and cnt[1] > 0, "a full table in the first image"
        if empty_image:
            cnt[1] = 0
        wide = nrow > L.ROI_MAX
        assert table.shape == (B, nrow if wide else L.ROI_MAX, L.roi_w(k))
        td, cd = torch.as_tensor(table, device=dev).contiguous(), torch.as_tensor(cnt, device=dev)
        sd, md = score.to(dev), tm.to(dev)
        G = tm.shape[1]
        ld = (k * k + 31) // 32 * 32
        if wide:
            need, entries = lib.disyolo_psroi_loss_workspace_x(B, Hm, Wm, nrow), ["disyolo_psroi_loss_x"]
        elif entry is None:
            need, entries = lib.disyolo_psroi_loss_workspace_hw(B, Hm, Wm), ["disyolo_psroi_loss_hw"]
        else:
            need, entries = lib.disyolo_psroi_loss_workspace(B, Hm), [entry]

        def run(ws):
            dscore, loss = nan((B, Hm, Wm, ld), BF16, dev), nan((1,), F32, dev)
            if entry is None:
                (L.psroi_loss_x if wide else L.psroi_loss)(sd, md, G, td, cd, B, (Hm, Wm), k, cfg.MASK_SCALE, dscore, loss, ws,
                                                           mask_stride=st)
            else:
                buf = ws.get(need)
                mid = (B, Hm, k) if entry == "disyolo_psroi_loss" else (B, Hm, st, k)
                ok(getattr(lib, entry)(vp(sd), vp(md), G, vp(td), vp(cd), *mid, cfg.MASK_SCALE, vp(dscore), vp(loss), vp(buf),
                                       buf.numel(), stream()), entry)
            return {"loss": loss, "dscore": dscore}
        return Case(run, need, entries)
    return build


# ------------------------------------------------------------------------------------------------ the optimizer
def adam_case(n, with_reg):
    def build(dev):
        lib = L.load()
        g = torch.Generator().manual_seed(n)
        src = {nm: (torch.randn(n, generator=g) * sc).abs_() if nm == "v" else torch.randn(n, generator=g) * sc
               for nm, sc in (("w", 0.1), ("grad", 0.01), ("m", 0.01), ("v", 1e-4))}
        src = {nm: t.to(dev) for nm, t in src.items()}
        lr = torch.tensor([1e-3], device=dev)

        def run(ws):
            t = {nm: v.clone() for nm, v in src.items()}
            cnt = torch.tensor([6], dtype=torch.int64, device=dev)
            out = {"w": t["w"], "m": t["m"], "v": t["v"], "step_counter": cnt}
            if with_reg:
                out["reg_loss"] = nan((1,), F32, dev)
                L.adam_step_fused(t["w"], t["grad"], t["m"], t["v"], n, n - 100, lr, 0.9, 0.999, 1e-8, 5e-4, cnt, 0.5, out["reg_loss"], ws)
            else:       # no l2 term asked for: no workspace needed, none passed
                ok(lib.disyolo_adam_step_fused(vp(t["w"]), vp(t["grad"]), vp(t["m"]), vp(t["v"]), n, n - 100, vp(lr), 0.9, 0.999, 1e-8,
                                               5e-4, vp(cnt), 0.5, None, None, 0, stream()), "adam_step_fused")
            return out
        return Case(run, lib.disyolo_adam_fused_workspace(n) if with_reg else 0, ["disyolo_adam_step_fused"], no_workspace=not with_reg)
    return build


def l2_case(n):
    def build(dev):
        g = torch.Generator().manual_seed(n)
        w = torch.randn(n, generator=g).to(dev)

        def run(ws):
            out = nan((1,), F32, dev)
            L.l2_loss(w, n, 5e-4, out, ws)
            return {"out": out}
        return Case(run, L.load().disyolo_l2_workspace(n), ["disyolo_l2_loss"])
    return build


# ------------------------------------------------------------------------------------------------ the table
NW = 4096 * 3 + 5
# case -> (the C entry point it goes through, its builder)
TABLE = {
    # conv2d_wgrad: (B, H, W, Cin, Cout, k, s, plan kind, pixel splits > 1) -- the smallest shapes of
    # tests/test_gpu_conv.py's list (or next to them) at which disyolo_conv2d_wgrad_plan reports the branch
    "conv2d_wgrad/im2col-split": ("disyolo_conv2d_wgrad", wgrad_case(2, 17, 19, 96, 24, 1, 1, 0, True)),
    "conv2d_wgrad/tap-fused-split": ("disyolo_conv2d_wgrad", wgrad_case(2, 18, 18, 64, 128, 3, 1, 1, True)),
    # (one split: dw is written directly and the workspace must stay untouched)
    "conv2d_wgrad/tap-fused-one-split": ("disyolo_conv2d_wgrad", wgrad_case(5, 2, 2, 32, 64, 3, 1, 1, False)),
    "conv2d_wgrad/stride2": ("disyolo_conv2d_wgrad", wgrad_case(3, 36, 28, 96, 36, 3, 2, 1, True)),
    "conv2d_wgrad/stride2-one-split": ("disyolo_conv2d_wgrad", wgrad_case(1, 20, 20, 32, 64, 3, 2, 1, False)),
    "conv2d_wgrad/concat": ("disyolo_conv2d_wgrad", wgrad_case(2, 18, 18, 64, 32, 1, 1, 0, True, up=32)),
    "conv2d_wgrad/concat-one-split": ("disyolo_conv2d_wgrad", wgrad_case(2, 12, 12, 64, 32, 1, 1, 0, False, up=32)),
    "conv_first_wgrad/W=128": ("disyolo_conv_first_wgrad", first_wgrad_case(2, 33, 128)),
    "conv_first_wgrad/W=129": ("disyolo_conv_first_wgrad", first_wgrad_case(1, 130, 129)),
    "conv_first_wgrad/direct,Cout=16": ("disyolo_conv_first_wgrad", first_wgrad_case(2, 33, 40, Cout=16)),
    "bn_act_bwd/130x64": ("disyolo_bn_act_bwd", bn_act_bwd_case(130, 64, False)),
    "bn_act_bwd/130x64+shortcut": ("disyolo_bn_act_bwd", bn_act_bwd_case(130, 64, True)),
    "bn_act_bwd/777x200": ("disyolo_bn_act_bwd", bn_act_bwd_case(777, 200, False)),
    "bn_act_bwd/777x200+shortcut": ("disyolo_bn_act_bwd", bn_act_bwd_case(777, 200, True)),
    "bn_act_bwd/2592x1024": ("disyolo_bn_act_bwd", bn_act_bwd_case(2592, 1024, False)),
    "bn_act_bwd/2592x1024+shortcut": ("disyolo_bn_act_bwd", bn_act_bwd_case(2592, 1024, True)),
    "bn_act_bwd_partials": ("disyolo_bn_act_bwd_partials", bn_partials_case(2, 18, 18, 64, 128, 16)),
    "bn_bwd_reduce/1536x64": ("disyolo_bn_bwd_reduce", bn_reduce_case(1536, 64)),
    "bn_bwd_reduce/130x200": ("disyolo_bn_bwd_reduce", bn_reduce_case(130, 200)),
    "bn_bwd_apply_sums/1536x64": ("disyolo_bn_bwd_apply_sums", bn_apply_sums_case(1536, 64)),
    "bn_bwd_apply_sums/130x200": ("disyolo_bn_bwd_apply_sums", bn_apply_sums_case(130, 200)),
    "colsum/777x32->24": ("disyolo_colsum", colsum_case(777, 32, 24)),
    "colsum/130x200->200": ("disyolo_colsum", colsum_case(130, 200, 200)),
    # the filter, S = 96, B = 2 (tests/limits_ref.py): per class with the LDS rank merge; C * D > 512 (the k-way merge);
    # C = 80 (the bucketed layout with its WD_MAXC + 1 offsets) at 64 and 256 rows; the image-wide list; a rectangular net
    "detect/C=3,D=64": ("disyolo_detect_nms_hw", detect_case(3, 64)),
    "detect/C=3,D=256": ("disyolo_detect_x", detect_case(3, 256)),
    "detect/C=80,D=64": ("disyolo_detect_nms_hw", detect_case(80, 64)),
    "detect/C=80,D=256": ("disyolo_detect_x", detect_case(80, 256)),
    "detect/agnostic,D=256": ("disyolo_detect_x", detect_case(3, 256, "agnostic")),
    "detect/none,D=256": ("disyolo_detect_x", detect_case(3, 256, "none")),
    "detect/agnostic,C=80,D=64": ("disyolo_detect_nms_hw", detect_case(80, 64, "agnostic")),
    "detect/disyolo_detect": ("disyolo_detect", detect_case(3, 64, entry="disyolo_detect")),
    "detect/disyolo_detect_hw,64x96": ("disyolo_detect_hw", detect_case(3, 64, size=(64, 96), entry="disyolo_detect_hw")),
    "detect/64x96,C=80,D=256": ("disyolo_detect_x", detect_case(80, 256, size=(64, 96))),
    "yolo_loss/disyolo_yolo_loss": ("disyolo_yolo_loss", yolo_case_of(3, 64, 20, 0, entry="disyolo_yolo_loss")),
    "yolo_loss/disyolo_yolo_loss_wide": ("disyolo_yolo_loss_wide", yolo_case_of(3, 64, 20, 32, entry="disyolo_yolo_loss_wide")),
    "yolo_loss/hw,64x64": ("disyolo_yolo_loss_hw", yolo_case_of(3, 64, 20, 0)),
    "yolo_loss/hw,64x96,C=80": ("disyolo_yolo_loss_hw", yolo_case_of(80, (64, 96), 256, 256)),
    # (dlogits_ld = 0, the 32-channel rows, takes 5 classes at the most; 65 boxes: the 256-row instance)
    "yolo_loss/hw,64x96,C=5,ld=0": ("disyolo_yolo_loss_hw", yolo_case_of(5, (64, 96), 65, 0)),
    "psroi_loss/disyolo_psroi_loss": ("disyolo_psroi_loss", psroi_case(16, 32, 3, 2, entry="disyolo_psroi_loss")),
    "psroi_loss/disyolo_psroi_loss_s,stride2": ("disyolo_psroi_loss_s", psroi_case(16, 32, 3, 2, entry="disyolo_psroi_loss_s")),
    "psroi_loss/disyolo_psroi_loss_s,stride1,k=5": ("disyolo_psroi_loss_s", psroi_case(16, 32, 5, 1, entry="disyolo_psroi_loss_s")),
    "psroi_loss/hw,32x48,k=7": ("disyolo_psroi_loss_hw", psroi_case(16, (32, 48), 7, 2)),
    "psroi_loss/x,cap=40": ("disyolo_psroi_loss_x", psroi_case(40, 32, 3, 2)),
    "psroi_loss/x,cap=40,empty-image": ("disyolo_psroi_loss_x", psroi_case(40, 32, 3, 2, empty_image=True)),
    "psroi_loss/x,cap=512,32x48,k=7": ("disyolo_psroi_loss_x", psroi_case(512, (32, 48), 7, 2)),
    "adam_step_fused/reg_loss": ("disyolo_adam_step_fused", adam_case(NW, True)),
    "adam_step_fused/no-reg_loss": ("disyolo_adam_step_fused", adam_case(NW, False)),
    "l2_loss/n=1": ("disyolo_l2_loss", l2_case(1)),
    "l2_loss/n=%d" % NW: ("disyolo_l2_loss", l2_case(NW)),
}
# entry points with a workspace that no case above reaches, each with its reason
EXCLUDED = {}


def outputs_of(case, ws):
    out = case.run(ws)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("case", sorted(TABLE))
def test_exact_poisoned_workspace(dev, case):
    entry, build = TABLE[case]
    c = build(dev)
    assert c.entries == (entry,), "the case goes through %s, the table says %s" % (c.entries, entry)
    plain = L.Workspace(dev)
    plain.buf.zero_()
    a = outputs_of(c, plain)
    for name, t in a.items():
        if t.is_floating_point():
            assert not torch.isnan(t).any(), "%s: %s of the plain call holds NaN (not fully written?)" % (case, name)
        elif not t.is_floating_point():
            assert (t >= 0).all(), "%s: %s of the plain call not fully written" % (case, name)
    if hasattr(c, "verify"):
        c.verify(a)
    if hasattr(c, "min_count"):
        assert int(a["det_count"].min()) >= c.min_count, "the filter kept %s rows" % a["det_count"].tolist()
    for poison in POISONS:
        ws = GuardedWorkspace(dev, poison=poison)
        got = outputs_of(c, ws)                                                     # rule 1: the exact-size call succeeds
        ws.check()                                                                  # rule 2: nothing outside [ws, ws + need)
        assert ws.high_water == c.need, "%s asked for %d bytes, its size query answers %d" % (case, ws.high_water, c.need)
        if c.untouched or c.no_workspace:
            assert ws.interior_untouched(), "%s wrote into a workspace it has no use for" % case
        assert sorted(got) == sorted(a)
        for name in a:                                                              # rule 3: the poison does not show
            same = torch.equal(bits(got[name]), bits(a[name]))
            assert same, "%s: %s differs from the zero-filled call with the workspace poisoned 0x%02X (%d of %d elements)" % (
                case, name, poison, int((bits(got[name]) != bits(a[name])).sum()), a[name].numel())


def test_every_workspace_entry_point_of_the_header_has_a_case():
    src = open(os.path.join(ROOT, "include", "disyolo.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    found = re.findall(r"\b(disyolo_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", src, flags=re.S)
    names = sorted(name for name, args in found if re.search(r"\bworkspace_bytes\b", args))
    assert len(names) >= 20, names
    reached = {entry for entry, _ in TABLE.values()}
    missing = [n for n in names if n not in reached and n not in EXCLUDED]
    assert not missing, "no exact-size case for %s" % missing
    assert not [n for n in sorted(reached | set(EXCLUDED)) if n not in names]


# ------------------------------------------------------------------------------------------------ the whole step
def _net(dev, B, S, guarded):
    from test_gpu_fp8 import _heads
    net = YOLONet(training=True, device=dev, image_size=S, batch_size=B, stage=1, seed=4)
    if guarded:
        # right after construction: nothing is recorded yet, and what the constructor pre-sized is dropped with the old buffers
        cap = max(net.ws.buf.numel(), net.ws_aux.buf.numel(), net.ws_det.buf.numel(), 8 << 20)
        net.ws, net.ws_aux, net.ws_det = (GuardedWorkspace(dev, poison=0xFF, capacity=cap) for _ in range(3))
    _heads(net, 5)
    net.shuffle_seed = 2
    return net


def test_training_step_in_guarded_workspaces(dev):
    """Three steps of a stage-1 net at B = 2, 64^2 whose three workspaces are exact-size, guarded and poisoned again before
    every step: the same losses and the same variables, bit for bit, as the net on ordinary workspaces -- eager, and once more
    recorded (the command list holds the guarded views' fixed address).  In the step every kernel finds the previous kernel's
    data in its scratch; here it finds NaN patterns.  The views of one workspace share their start, so the rear guard sits
    behind the LARGEST request: a small request that over-runs into the room of a larger one is not caught here -- the
    per-entry-point cases above catch that."""
    B, S = 2, 64
    b = O.synthetic_batch(B, S, seed=23)
    plain = _net(dev, B, S, False)
    plain.set_batch(b)
    want = [float(plain.train_step(None, det_thresh=0.1).cpu()) for _ in range(3)]
    torch.cuda.synchronize()
    assert np.all(np.isfinite(want)), want
    for recorded in (False, True):
        net = _net(dev, B, S, True)
        guards = (net.ws, net.ws_aux, net.ws_det)
        net.set_batch(b)
        if recorded:
            net.build_program(det_thresh=0.1)
        got = []
        for _ in range(3):
            for w in guards:
                w.repoison()
            got.append(float((net.train_step(None) if recorded else net.train_step(None, det_thresh=0.1)).cpu()))
            torch.cuda.synchronize()
        for w in guards:
            w.check()
        assert (net.ws, net.ws_aux, net.ws_det) == guards, "the net replaced a workspace"
        assert net.ws.high_water > 0 and net.ws_det.high_water > 0
        np.testing.assert_array_equal(got, want, err_msg="recorded" if recorded else "eager")
        assert torch.equal(bits(net.arena), bits(plain.arena)), "recorded" if recorded else "eager"

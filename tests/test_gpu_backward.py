"""The training step's backward pass, layer by layer, against float64 references at the configured sizes.

Part A -- every trainable variable, teacher-forced one layer at a time.  One eager compute_losses + backward; then for
each trainable layer the reference is built in float64 from the kernels' own tensors one step downstream (the consumers'
output gradients and bf16 weights, the layer's own raw conv output and batch statistics), never from the reference's own
earlier results.  Checked element by element:
  * the output gradient g (l.grad, where the step materialises it whole): the consumers' transposed convolutions, the
    2x2 upsample-backward of a concat's src_up part, the residual layer's materialised gradient for a shortcut source;
  * the batch-norm + leaky backward (closed form with the kernel's mean / rstd / scale / shift / gamma / raw): dx, dgamma,
    dbeta -- in whichever form the step took (plain bn_act_bwd, partial sums from the patch-conv epilogue, in-launch);
  * the weight gradient (f64 correlation of the source activation with dx) and the linear layers' bias gradient;
  * all through grad_arena[o:o+c] by variable name, and the checked names must be net.trainable_names().
Bounds (the constants below; "twin" = the same f64 computation on |operands|):
  dW:               |err| <= C_DW * twin;   dbias: |err| <= C_DBIAS * sum|dx|
  g (bf16):         |err| <= C_G_REL*|want| + C_G_ACC*sum_contributions|c| + C_G_TWIN*twin
  dx (bf16):        |err| <= C_DX_REL*|want| + C_DX_FIRST*|gamma|*rstd*(|g'| + (|dbeta| + |xhat|*|dgamma|)/M)
                             (+ g's bound carried through the batch-norm backward in the in-launch form, whose g is the
                             reference's: backward_ref.bn_bounds)
  dgamma, dbeta:    |err| <= C_SUM_SQRT*sqrt(sum term^2) + C_SUM_ABS*sum|term|  (the *_OWN constants where the reference
                             reads the kernel's stored g)
The constants, and the worst ratios measured on an MI355X, are in backward_ref.

Part B -- every weight-gradient, data-gradient, upsample-backward and colsum launch of the step, on integer operands,
issued by the methods backward() itself calls for them (net._dgrad, net._wgrad, net._dgrad_final): f32 outputs bit-equal to the exact sum, bf16 outputs to the exact sum rounded
once to nearest-even.

Per-layer reports go to test_reports/backward_<config>.json and test_reports/backward_exact_<config>.json at the repository
root (kept out of git).
"""
import json
import os
import time

import numpy as np
import pytest
import torch

import backward_ref as R
from backward_ref import tuned_tables  # noqa: F401  (fixture)
from disyolo_amd import config as cfg
from disyolo_amd import lib as L
from disyolo_amd.net import YOLONet, var_name
from disyolo_amd.synth import synthetic_batch

pytestmark = pytest.mark.gpu

# bounds of Part A (see the module docstring; the values live in backward_ref, whose CPU tests plant defects against them)
from backward_ref import (C_DW, C_DBIAS, C_G_REL, C_G_ACC, C_G_TWIN, C_DX_REL, C_DX_FIRST, C_SUM_SQRT,  # noqa: E402
                          C_SUM_ABS, C_SUM_SQRT_OWN, C_SUM_ABS_OWN)

CONFIGS = {
    "stage1_576_b8": (1, 576, 8, False),            # BASELINE configs[1]: the step bench.py times
    "stage1_576_b8_inkernel_bwd": (1, 576, 8, True),
    "stage1_832_b4": (1, 832, 4, False),            # configs[4] per GPU
    "stage2_576_b8": (2, 576, 8, False),
    "stage1_576_b8_tuned": (1, 576, 8, False),      # ... with the tile table bench.py loads for it
}
# configurations that load a committed tile table (autotune(cache=...) only reads it) instead of the launcher's heuristic tiles
TABLES = {"stage1_576_b8_tuned": "tune_train_B8_576_stage1.json"}


REPORTS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "test_reports")


def _report(name, rep):
    os.makedirs(REPORTS, exist_ok=True)
    with open(os.path.join(REPORTS, name + ".json"), "w") as f:
        json.dump(rep, f, indent=1)


def _load_table(net, tag):
    if tag in TABLES:
        path = os.path.join(os.path.dirname(REPORTS), "profiles", TABLES[tag])
        assert os.path.exists(path), path        # (autotune(cache=) would time the candidates and write the file)
        net.autotune(cache=path)
        assert L.TUNED


def _net(dev, stage, S, B, inkernel_bwd=False):
    """the setup of test_gpu_loss.test_losses_inside_the_net_at_the_headline_configuration"""
    net = YOLONet(training=True, device=dev, image_size=S, batch_size=B, stage=stage, seed=0)
    with torch.no_grad():
        for i in (59, 67, 75, 82):
            net.params["yolo/convolutional%d/weights" % i].mul_(4.0)
    net.refresh_weights()
    b = synthetic_batch(B, S, seed=77)
    rng = np.random.RandomState(3)
    b["perm_det"] = np.stack([rng.permutation(cfg.MAX_DETECTION) for _ in range(B)]).astype(np.int32)
    b["perm_gt"] = np.stack([rng.permutation(cfg.MAX_BOX_PER_IMAGE) for _ in range(B)]).astype(np.int32)
    net.set_batch(b)
    net.bn_inkernel_bwd = inkernel_bwd
    return net


def _eager_backward(net):
    net.grad_arena.fill_(float("nan"))           # every variable's gradient must be written
    net.compute_losses(0.2)
    net.backward()
    torch.cuda.synchronize()
    assert int(net.roi_count.sum()) > 0, "no positive RoI: the mask subnet would get no gradient"


def _arena(net, name, shape):
    o, c = net.arena_slices[name]
    assert c == int(np.prod(shape)), name
    return net.grad_arena[o:o + c].view(shape)


def _bn_form(l):
    return "fused" if l.fused_bwd else ("partials" if l.bwd_part_rows else "plain")


def _collect(fails, fn, *args, **kw):
    """run a checker; a violation is recorded (the run goes on, so that the report covers every layer)"""
    try:
        return fn(*args, **kw)
    except AssertionError as e:
        fails.append(str(e))
        return float("inf")


def check_layer(net, l, checked):
    """Part A for one trainable layer; returns its report row"""
    t0 = time.perf_counter()
    by = net.by_idx
    row = {"layer": l.idx, "kind": l.kind, "k": l.k, "stride": l.stride, "cin": l.cin, "cout": l.cout, "hw": [l.Ho, l.Wo],
           "worst": {}, "failures": []}
    fails = row["failures"]
    dy = R.f64(l.dx[..., :l.cout])
    # ---- weight gradient: the source activation (bf16 image for layer 1) correlated with the layer's dx
    if l.idx == 1:
        x = R.layer_input(l, by, image_bf16=net.images.to(torch.bfloat16))
        row["wgrad_plan"] = "conv_first_wgrad"
    else:
        x = R.layer_input(l, by)
        row["wgrad_plan"] = list(L.conv2d_wgrad_plan(l.wgrad_desc))
    want = R.wgrad_ref(x, dy, l.k, l.stride)
    twin = R.wgrad_ref(x.abs(), dy.abs(), l.k, l.stride)
    del x
    name = var_name(l.idx, "weights")
    row["worst"]["dW"] = R.check_bounded(_arena(net, name, (l.k, l.k, l.cin, l.cout)), want, C_DW * twin,
                                         "layer %d dW" % l.idx, fails=fails)
    checked.append(name)
    del want, twin
    if l.kind == "lin":
        name = var_name(l.idx, "biases")
        row["worst"]["dbias"] = R.check_bounded(_arena(net, name, (l.cout,)), dy.sum((0, 1, 2)),
                                                C_DBIAS * dy.abs().sum((0, 1, 2)), "layer %d dbias" % l.idx, fails=fails)
        checked.append(name)
        row["seconds"] = round(time.perf_counter() - t0, 3)
        return row
    # ---- output gradient from the consumers (teacher-forced)
    row["bn_bwd"] = _bn_form(l)
    row["consumers"] = [[m.idx, how] for m, how in R.consumers(net.layers, l.idx)]
    wb = lambda m: m.w.to(torch.bfloat16)
    gw, gacc, gtwin = R.output_grad_ref(l, by, wb, lambda m: m.dx[..., :m.cout], lambda m: m.grad)
    gb = R.grad_bound(gw, gacc, gtwin, C_G_REL, C_G_ACC, C_G_TWIN)
    del gacc, gtwin
    if l.fused_bwd:
        g, g_err = gw, gb            # the in-launch form keeps its g in registers: the reference's own, and its bound
    else:
        row["worst"]["g"] = R.check_bounded(l.grad, gw, gb, "layer %d output gradient (%s)" % (l.idx, row["bn_bwd"]),
                                            fails=fails)
        g, g_err = l.grad, None
    # ---- batch norm + leaky backward
    r = R.bn_act_bwd_ref(g, l.raw, l.scale, l.shift, l.mean, l.rstd, l.gamma)
    del g, gw, gb
    if g_err is None:
        bdx, bdg, bdb = R.bn_bounds(r, C_DX_REL, C_DX_FIRST, C_SUM_SQRT_OWN, C_SUM_ABS_OWN)
    else:
        bdx, bdg, bdb = R.bn_bounds(r, C_DX_REL, C_DX_FIRST, C_SUM_SQRT, C_SUM_ABS, g_err)
    row["worst"]["dx"] = R.check_bounded(l.dx.reshape(-1, l.cout), r["dx"], bdx, "layer %d dx" % l.idx,
                                         alt=torch.where(r["amb"], r["dx_alt"], torch.full_like(r["dx"], float("nan"))), fails=fails)
    row["ambiguous_slopes"] = int(r["amb"].sum())
    for leaf, key, bound in (("BatchNorm/gamma", "dgamma", bdg), ("BatchNorm/beta", "dbeta", bdb)):
        name = var_name(l.idx, leaf)
        row["worst"][key] = R.check_bounded(_arena(net, name, (l.cout,)), r[key], bound, "layer %d %s" % (l.idx, key), fails=fails)
        checked.append(name)
    row["seconds"] = round(time.perf_counter() - t0, 3)
    return row


def run_part_a(net, tag):
    t0 = time.perf_counter()
    _eager_backward(net)
    t1 = time.perf_counter()
    checked, rows = [], []
    with torch.no_grad():
        for l in net.layers:
            if not l.lock:
                rows.append(check_layer(net, l, checked))
    torch.cuda.synchronize()
    assert sorted(checked) == sorted(net.trainable_names()) and len(checked) == len(set(checked))
    worst = {}
    for r_ in rows:
        for k, v in r_["worst"].items():
            worst[k] = max(worst.get(k, 0.0), v)
    rep = {"config": tag, "B": net.B, "S": net.S, "variables": len(checked), "step_seconds": round(t1 - t0, 2),
           "check_seconds": round(time.perf_counter() - t1, 2), "worst": worst,
           "forms": {f: [r_["layer"] for r_ in rows if r_.get("bn_bwd") == f] for f in ("plain", "partials", "fused")},
           "bounds": {"C_DW": C_DW, "C_DBIAS": C_DBIAS, "C_G_REL": C_G_REL, "C_G_ACC": C_G_ACC, "C_G_TWIN": C_G_TWIN,
                      "C_DX_REL": C_DX_REL, "C_DX_FIRST": C_DX_FIRST, "C_SUM_SQRT": C_SUM_SQRT, "C_SUM_ABS": C_SUM_ABS,
                      "C_SUM_SQRT_OWN": C_SUM_SQRT_OWN, "C_SUM_ABS_OWN": C_SUM_ABS_OWN},
           "layers": rows}
    _report("backward_" + tag, rep)
    fails = [f for r_ in rows for f in r_["failures"]]
    assert not fails, "%d checks failed:\n%s" % (len(fails), "\n".join(fails[:40]))
    return rep


@pytest.mark.parametrize("tag", list(CONFIGS))
def test_backward_matches_f64_layer_by_layer(dev, tag, tuned_tables):
    stage, S, B, inkernel = CONFIGS[tag]
    net = _net(dev, stage, S, B, inkernel)
    _load_table(net, tag)
    rep = run_part_a(net, tag)
    if inkernel and not rep["forms"]["fused"]:
        pytest.skip("no layer takes the in-launch batch-norm backward at %d^2, B = %d" % (S, B))


def test_recorded_step_gradients_are_bitwise_the_eager_ones(dev):
    """stage 1, 576^2, B = 8: grad_arena after one recorded pipelined train_step equals the eager backward's, bit for bit
    (same weights, same batch; the optimizer reads grad_arena, it does not write it)"""
    net = _net(dev, 1, 576, 8)
    _eager_backward(net)
    eager = net.grad_arena.clone()
    assert bool(torch.isfinite(eager).all())
    net.build_program(det_thresh=0.2, pipeline_backbone=True)
    net.prime_pipeline()
    net.grad_arena.fill_(float("nan"))
    net.train_step(None, want_loss=False)
    torch.cuda.synchronize()
    same = eager.view(torch.int32) == net.grad_arena.view(torch.int32)
    if not bool(same.all()):
        bad = [n for n, (o, c) in net.arena_slices.items() if not bool(same[o:o + c].all())]
        raise AssertionError("recorded step's gradients differ from the eager backward's in %s" % bad)


# ------------------------------------------------------------------------------------------------ Part B: integer operands
EXACT_CONFIGS = {"stage2_576_b8": (2, 576, 8), "stage1_832_b4": (1, 832, 4), "stage1_576_b8_tuned": (1, 576, 8)}


def _ints(t, lo, hi, gen):
    t.copy_(torch.randint(lo, hi + 1, t.shape, generator=gen, device=t.device).to(t.dtype))


def _bn_partials_ref(grad, tgt):
    """(sum g', sum g'*xhat) per channel of tgt's batch-norm backward from the stored gradient, and sum|term|"""
    r = R.bn_act_bwd_ref(grad, tgt.raw, tgt.scale, tgt.shift, tgt.mean, tgt.rstd, tgt.gamma)
    assert not bool(r["amb"].any())
    t1, t2 = r["gp"], r["gp"] * r["xh"]
    return torch.stack([t1.sum(0), t2.sum(0)], -1), torch.stack([t1.abs().sum(0), t2.abs().sum(0)], -1)


@pytest.mark.parametrize("tag", list(EXACT_CONFIGS))
def test_backward_launches_are_exact_on_integers(dev, tag, tuned_tables):
    stage, S, B = EXACT_CONFIGS[tag]
    net = YOLONet(training=True, device=dev, image_size=S, batch_size=B, stage=stage, seed=0)
    _load_table(net, tag)
    gen = torch.Generator(device=dev).manual_seed(11)
    t0 = time.perf_counter()
    launches, fails = [], []
    with torch.no_grad():
        # operands: weights in [-1, 1] (packed by the net itself), activations, dx and the image in [-2, 2]
        for l in net.layers:
            _ints(l.w, -1, 1, gen)
        net.refresh_weights()          # (also folds scale / shift from the moving statistics: the batch-norm state comes after)
        for l in net.layers:
            _ints(l.act, -2, 2, gen)
            if l.dx is not None:
                l.dx.zero_()
                _ints(l.dx[..., :l.cout], -2, 2, gen)
            if l.raw is not None:
                # batch-norm state read by the data-gradient conv that emits the backward sums: z = raw*scale + shift is never 0
                _ints(l.raw, -2, 2, gen)
                l.scale.copy_(torch.where(torch.rand(l.cout, generator=gen, device=dev) < 0.5, -0.5, 1.0))
                l.shift.fill_(0.25)
                _ints(l.mean, -1, 1, gen)
                l.rstd.copy_(torch.where(torch.rand(l.cout, generator=gen, device=dev) < 0.5, 0.5, 2.0))
        _ints(net.images, -2, 2, gen)
        visit = net.backward_order()
        final_of = net._final_writers(visit)
        for l in net.layers:
            l.grad_set = False
        for l in visit:
            if l.lock:
                continue
            dx, ld = net._dx_of(l)                           # (what backward() hands on from the layer's batch-norm step)
            dy = dx[..., :l.cout]
            # ---- the residual layer's batch-norm backward hands its gradient to the shortcut's source first
            if l.kind == "res" and net.by_idx[l.shortcut].grad is not None:
                sc = net.by_idx[l.shortcut]
                _ints(sc.grad, -2, 2, gen)
                sc.grad_set = True
            # ---- data gradients: backward()'s own step for each entry (net._dgrad), the net's own ``final`` predicate
            for entry in l.dgrad_descs:
                mode, tgt, kw = entry
                first = not tgt.grad_set
                if first:
                    tgt.grad.fill_(float("nan"))             # a first write must not read what was there
                    prev = None
                else:
                    _ints(tgt.grad, -2, 2, gen)
                    prev = R.f64(tgt.grad)
                w = R.f64(l.w)
                if mode == "direct":
                    final = net._dgrad_final(l, tgt, final_of)
                    lo = 0
                    tgt.bwd_part_rows = 0
                    net._dgrad(l, entry, dx, final_of)
                    exact = R.dgrad_ref(dy, w[:, :, lo:lo + tgt.cout, :], l.stride, l.H, l.W)
                    if prev is not None:
                        exact = exact + prev
                    what = "layer %d -> %d dgrad (%s%s%s)" % (l.idx, tgt.idx, "quad" if "quad" in kw else "direct",
                                                               ", accumulate" if prev is not None else "", ", final" if final else "")
                    _collect(fails, R.check_exact_bf16, tgt.grad, exact, what)
                    ent = {"layer": l.idx, "launch": "dgrad", "target": tgt.idx, "path": "quad" if "quad" in kw else "direct",
                           "accumulate": prev is not None, "final": final, "bn_partials": tgt.bwd_part_rows}
                    if tgt.bwd_part_rows:
                        got = tgt.bwd_part[:tgt.bwd_part_rows * tgt.cout * 2].view(tgt.bwd_part_rows, tgt.cout, 2)
                        want, absum = _bn_partials_ref(tgt.grad, tgt)
                        ent["bn_partials_worst"] = R.check_bounded(got.double().sum(0), want, 2.0 ** -20 * absum,
                                                                   what + " batch-norm partial sums", fails=fails)
                    launches.append(ent)
                else:
                    tmp = kw["tmp"]
                    tmp.fill_(float("nan"))
                    lo = net.by_idx[l.src].cout
                    net._dgrad(l, entry, dx, final_of)       # the conv into up_tmp, then upsample2x_bwd (which only reads it)
                    exact = R.dgrad_ref(dy, w[:, :, lo:lo + tgt.cout, :], 1, l.H, l.W)
                    what = "layer %d -> %d dgrad (concat, up_tmp)" % (l.idx, tgt.idx)
                    _collect(fails, R.check_exact_bf16, tmp, exact, what)
                    up = R.upsample2_bwd(R.f64(tmp))
                    if prev is not None:
                        up = up + prev
                    _collect(fails, R.check_exact_bf16, tgt.grad, up, "layer %d -> %d upsample2x_bwd%s" % (l.idx, tgt.idx,
                                                                                          ", accumulate" if prev is not None else ""))
                    launches.append({"layer": l.idx, "launch": "dgrad+upsample2x_bwd", "target": tgt.idx, "path": "up",
                                     "accumulate": prev is not None, "final": False})
            # ---- weight gradient (and the linear layers' bias gradient): backward()'s own step (net._wgrad), main lane
            l.dw.fill_(float("nan"))
            if l.kind == "lin":
                l.dbias.fill_(float("nan"))
            net._wgrad(l, dx, ld, False)
            if l.idx == 1:
                plan = "conv_first_wgrad"
                x = R.f64(net.images)
            else:
                plan = list(L.conv2d_wgrad_plan(l.wgrad_desc))
                x = R.layer_input(l, net.by_idx)
            _collect(fails, R.check_exact_f32, l.dw, R.wgrad_ref(x, dy, l.k, l.stride), "layer %d dW (plan %s)" % (l.idx, plan))
            del x
            launches.append({"layer": l.idx, "launch": "wgrad", "plan": plan})
            if l.kind == "lin":
                _collect(fails, R.check_exact_f32, l.dbias, R.f64(dy).sum((0, 1, 2)), "layer %d colsum" % l.idx)
                launches.append({"layer": l.idx, "launch": "colsum"})
        torch.cuda.synchronize()
    # every launch backward() would issue was issued here
    n_dgrad = sum(len(l.dgrad_descs) for l in net.layers if not l.lock)
    assert sum(1 for e in launches if e["launch"].startswith("dgrad")) == n_dgrad
    assert sum(1 for e in launches if e["launch"] == "wgrad") == sum(1 for l in net.layers if not l.lock)
    _report("backward_exact_" + tag, {"config": tag, "seconds": round(time.perf_counter() - t0, 2),
                                      "failures": fails, "launches": launches})
    assert not fails, "%d launches differ from their exact references:\n%s" % (len(fails), "\n".join(fails[:40]))

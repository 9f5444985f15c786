"""The forward pass, layer by layer, against float64 references at the configured sizes, with the tiles bench.py times.

Part A -- every layer 1...82 of each configuration, teacher-forced one layer (or one fused launch) at a time.  One eager
forward; then for each layer the reference is built in float64 from the kernels' own tensors one step upstream (the input
activation(s) as the layer reads them, the bf16 weights, the residual source) and every element is bounded
(tests/forward_ref.py holds the references, the bounds and their constants).  The forms:
  * inference-mode batch norm (the locked backbone, every layer of an inference net): act = leaky(conv*scale + shift)
    (+ residual) from the kernel's own scale / shift; scale / shift against bn_fold of gamma, beta and the moving moments;
  * training-mode batch norm, three-launch and in-launch: raw against the f64 conv; mean / rstd against the two-pass f64
    moments of the unrounded f64 conv over the batch (population variance); scale / shift from the kernel's mean / rstd;
    the moving mean / variance against a snapshot taken before the pass (decay 0.997, once); act from the kernel's
    coefficients applied to the bf16 raw output -- both forms read the bf16 raw values (the in-launch epilogue normalises
    the bf16 tile it staged in LDS, conv_igemm.hip), so one reference serves both;
  * the linear layers 59, 67, 75, 82: f32 conv + bias;
  * upsample + concat inputs (61, 69, 77, 80): the reference forms [src, up2(src_up)] itself (backward_ref.concat_input);
  * fused launches (conv1+2, conv3+4, conv6+7, conv8+9, conv80-82): the intermediates are computed in f64 and rounded to
    bf16 as the kernel does; the bound carries that rounding through the next conv to first order;
  * fp8 layers (conv10-52) and conv9's hand-over quantisation: every e4m3 code RNE(want / s_out), the adjacent code
    accepted only within the bound of a rounding midpoint (counted); the dual bf16 outputs (26, 43, 52) like the first form;
  * detection and mask assembly on the kernels' own logits and score maps (O.filter_detections, O.val_test).
The configurations load the tile tables bench.py loads (profiles/tune_<workload>.json; autotune(cache=...) only reads them).

Part B -- every distinct forward launch of four configurations (conv2d_fwd descriptors as the pass issues them, with
their statistics rows and in-launch batch norm; the five fused launches; conv_first_fwd; the e4m3 convs; quant_fp8) again
on integer operands: bf16 outputs equal the f32 epilogue (kernel order) rounded once, f32 outputs and statistics rows the
exact sums, the finalize outputs within 1 ulp of its f32 formula on the exact sums, e4m3 codes the torch rounding.  At
B = 32 inference every bf16 descriptor also runs under every tuner candidate the launcher accepts for its shape.

Bit-identity: a recorded pipelined train_step (stage 1, 576^2, B = 8) and the recorded inference graph (B = 32) give the
eager forward's tensors bit for bit.

Planted edges: channels with |mean|/std of 1, 16, 64 (and 256, reported only), zero weights, an all-negative output and a
negative gamma in four trainable layers (54, 57, 62, 65), in both batch-norm forms.

Reports go to test_reports/forward_<tag>.json at the repository root (kept out of git).
"""
import ctypes
import json
import os
import time

import numpy as np
import pytest
import torch

import disyolo_oracle as O
import forward_ref as FR
from backward_ref import tuned_tables  # noqa: F401  (fixture)
from forward_ref import check_bounded, f64, U_BF16, C_EPI
from disyolo_amd import config as cfg
from disyolo_amd import lib as L
from disyolo_amd.net import YOLONet
from disyolo_amd.synth import synthetic_batch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILES = os.path.join(ROOT, "profiles")
REPORTS = os.path.join(ROOT, "test_reports")
DET_THRESH = 0.2
CHUNK = 8           # images per f64 slice of the B = 32 inference layers

CONFIGS = {
    "train_s1_576_b8": dict(training=True, stage=1, S=576, B=8, table="tune_train_B8_576_stage1.json"),
    "train_s1_576_b8_threelaunch": dict(training=True, stage=1, S=576, B=8, table="tune_train_B8_576_stage1.json",
                                        bn_inkernel=False),
    "train_s1_832_b4": dict(training=True, stage=1, S=832, B=4, table="tune_train_B4_832_stage1.json"),
    "train_s2_576_b8": dict(training=True, stage=2, S=576, B=8, table="tune_train_B8_576_stage2.json"),
    "infer_576_b32": dict(training=False, S=576, B=32, table="tune_infer_B32_576.json"),
    "infer_576_b32_fp8": dict(training=False, S=576, B=32, table="tune_infer_B32_576.json", dtype="fp8"),
    "train_s1_832_b4_fp8": dict(training=True, stage=1, S=832, B=4, table="tune_train_B4_832_stage1_fp8.json", dtype="fp8"),
}
FUSED_GROUPS = ([1, 2], [3, 4], [6, 7], [8, 9], [80, 81, 82])
IN_LAUNCH_576_B8 = [53, 54, 55, 56, 57, 60, 61, 62, 63, 64, 65, 68]


def _report(name, rep):
    os.makedirs(REPORTS, exist_ok=True)
    with open(os.path.join(REPORTS, name + ".json"), "w") as f:
        json.dump(rep, f, indent=1)


def build(dev, c, k_map=None):
    """the configuration's net with the seeded heads of test_gpu_backward._net / test_gpu_configs.seeded_heads, its batch
    set and the tile table bench.py loads for the workload"""
    S, B, dtype = c["S"], c["B"], c.get("dtype", "bf16")
    table = os.path.join(PROFILES, c["table"])
    assert os.path.exists(table), table            # (autotune(cache=) would time the candidates and write the file)
    b = synthetic_batch(B, S, seed=77)
    if c["training"]:
        net = YOLONet(training=True, device=dev, image_size=S, batch_size=B, stage=c["stage"], seed=0, dtype=dtype)
        with torch.no_grad():
            for i in (59, 67, 75, 82):
                net.params["yolo/convolutional%d/weights" % i].mul_(4.0)
        net.refresh_weights()
        rng = np.random.RandomState(3)
        b["perm_det"] = np.stack([rng.permutation(cfg.MAX_DETECTION) for _ in range(B)]).astype(np.int32)
        b["perm_gt"] = np.stack([rng.permutation(cfg.MAX_BOX_PER_IMAGE) for _ in range(B)]).astype(np.int32)
        net.set_batch(b)
    else:
        net = YOLONet(training=False, device=dev, image_size=S, batch_size=B, stage=1, seed=0, dtype=dtype, k_map=k_map)
        g = torch.Generator().manual_seed(4242)
        with torch.no_grad():
            for i in (59, 67, 75, 82):
                net.params["yolo/convolutional%d/weights" % i].mul_(4.0)
                bias = net.params["yolo/convolutional%d/biases" % i]
                bias.copy_((torch.randn(bias.shape, generator=g) * 0.3).to(bias.device))
        net.refresh_weights()
        net._set_inputs(b["images"], b["clip_window"])
    net.bn_inkernel = c.get("bn_inkernel", True)
    net.autotune(cache=table)
    if dtype == "fp8":
        net.calibrate_fp8()
    return net, b


def train_bn(net, l):
    return net.training and not l.lock and l.kind != "lin"


def perturb_moving(net, seed=5):
    """non-trivial moving statistics in every training-mode layer (so that a wrong decay shows), and their snapshot"""
    g = torch.Generator(device=net.device).manual_seed(seed)
    snap = {}
    with torch.no_grad():
        for l in net.layers:
            if train_bn(net, l):
                l.mm.copy_(torch.randn(l.cout, generator=g, device=net.device) * 0.5)
                l.mv.copy_(torch.rand(l.cout, generator=g, device=net.device) + 0.5)
                snap[l.idx] = (l.mm.clone(), l.mv.clone())
    return snap


def eager(net, b):
    if net.training:
        net.compute_losses(DET_THRESH)
    else:
        net.forward(b["images"], b["clip_window"], [DET_THRESH], is_training=False)
    torch.cuda.synchronize()


def groups_of(net):
    """the fused launches of the pass: lists of layer indices, the launch at the last one"""
    plan = net._fusion_plan(net.training, 1, 82)
    out, cur = [], []
    for i in sorted(plan):
        cur.append(i)
        if plan[i] is not None:
            out.append(cur)
            cur = []
    return out


# ------------------------------------------------------------------------------------------------ Part A checks
class Row(dict):
    def __init__(self, l, form, **kw):
        super().__init__(layer=l.idx, form=form, k=l.k, stride=l.stride, cin=l.cin, cout=l.cout, hw=[l.Ho, l.Wo], worst={},
                         ambiguous=0, fp8_adjacent=0, failures=[], **kw)
        self.t0 = time.perf_counter()

    def bound(self, key, got, want, bound, what, alt=None):
        r = check_bounded(got, want, bound, what, alt=alt, fails=self["failures"])
        self["worst"][key] = max(self["worst"].get(key, 0.0), r)

    def e4m3(self, key, got, want, bound, s_out, what):
        bad, adj, worst = FR.check_e4m3(got, want, bound, s_out, what, fails=self["failures"])
        self["fp8_adjacent"] += adj
        self["worst"][key] = max(self["worst"].get(key, 0.0), worst if not bad else float("inf"))

    def done(self):
        self["seconds"] = round(time.perf_counter() - self.t0, 3)
        return self


def _w(l):
    """the weights as the kernel reads them: f32 for conv1 (conv_first_fwd, split bf16 in the fused launch), else bf16"""
    return l.w if l.idx == 1 else l.w.to(torch.bfloat16)


def _tile(l):
    try:
        return L.conv2d_tile(l.desc)[0] if l.desc is not None else None
    except L.DisyoloError:
        return None


def check_fold(row, l, what=""):
    sc, sh, bsc, bsh = FR.fold_bounds(l.gamma, l.beta, l.mm, l.mv)
    row.bound("scale", l.scale, sc, bsc, "layer %d scale%s" % (l.idx, what))
    row.bound("shift", l.shift, sh, bsh, "layer %d shift%s" % (l.idx, what))


def check_inference(net, l, chunks):
    """form 1 (and the linear layers): one conv launch with the folded batch norm / bias in its epilogue"""
    by = net.by_idx
    row = Row(l, "linear" if l.kind == "lin" else "inference", tile=_tile(l) if l.idx > 1 else "conv_first")
    if l.kind != "lin":
        check_fold(row, l)
    for sl in chunks:
        x = FR.layer_input_of(l, by, sl, net.images)
        if l.kind == "lin":
            s = FR.stage_ref(x, _w(l), l.stride, shift=l.bias, act=False)
            row.bound("act", l.act[sl], s["y"], s["bz"], "layer %d f32 output" % l.idx)
        else:
            res = by[l.shortcut].act[sl] if l.shortcut is not None else None
            s = FR.stage_ref(x, _w(l), l.stride, l.scale, l.shift, res)
            row.bound("act", l.act[sl], s["y"], FR.bf16_bound(s), "layer %d act" % l.idx)
            row["ambiguous"] += FR.ambiguous(s)
        del x, s
    return row.done()


def check_training(net, l, snap, skip_stats=None):
    """form 2: raw, batch statistics, coefficients, moving statistics and the activation of a training-mode layer.
    ``skip_stats``: channels whose statistics are reported, not bounded (the planted |mean|/std = 256 channel)"""
    by = net.by_idx
    form = "in-launch" if l.fused_fwd else ("colstats" if l.idx == 1 else "three-launch")
    row = Row(l, form, tile=_tile(l) if l.idx > 1 else "conv_first")
    x = FR.layer_input_of(l, by, slice(None), net.images)
    c, tw = FR.conv_ref(x, _w(l), l.stride)
    del x
    e = FR.C_ACC * tw
    del tw
    row.bound("raw", l.raw, c, U_BF16 * c.abs() + e, "layer %d raw" % l.idx)
    if l.idx == 1:
        e = e + U_BF16 * c.abs()         # conv1's statistics are column sums of its bf16 raw output (colstats)
    mean, var, bmean, bvar = FR.stats_bounds(c, e)
    del c, e
    rstd, brstd = FR.rstd_ref(var, bvar)
    keep = torch.ones(l.cout, dtype=torch.bool, device=mean.device)
    if skip_stats is not None:
        keep[skip_stats] = False
    mm0, mv0 = snap[l.idx]
    wmm, bmm = FR.moving_ref(mm0, mean, bmean)
    wmv, bmv = FR.moving_ref(mv0, var, bvar)
    for key, got, want, bound in (("mean", l.mean, mean, bmean), ("rstd", l.rstd, rstd, brstd), ("mm", l.mm, wmm, bmm),
                                  ("mv", l.mv, wmv, bmv)):
        row.bound(key, got[keep], want[keep], bound[keep], "layer %d %s (%s)" % (l.idx, key, form))
    sc, sh, bsc, bsh = FR.coeffs_from(l.gamma, l.beta, l.mean, l.rstd)
    row.bound("scale", l.scale, sc, bsc, "layer %d scale (%s)" % (l.idx, form))
    row.bound("shift", l.shift, sh, bsh, "layer %d shift (%s)" % (l.idx, form))
    raw = f64(l.raw)
    cs = raw * f64(l.scale)
    z = cs + f64(l.shift)
    y = FR.leaky(z)
    bz = C_EPI * (cs.abs() + f64(l.shift).abs())
    if l.shortcut is not None:
        r = f64(by[l.shortcut].act)
        y = y + r
        bz = bz + C_EPI * r.abs()
    row.bound("act", l.act, y, U_BF16 * y.abs() + bz, "layer %d act (%s)" % (l.idx, form))
    row["ambiguous"] += int((z.abs() <= bz).sum())
    row["stats"] = dict(mean=mean, var=var, rstd=rstd)          # (taken out of the row before the report is written)
    return row.done()


def check_group(net, members, chunks):
    """form 5: a fused launch; only the last member's output is stored"""
    by = net.by_idx
    ls = [by[i] for i in members]
    name = {1: "conv12_fused", 3: "block32_fused", 6: "block64_fused", 8: "block64_fused", 80: "block32_fused(mask head)"}
    row = Row(ls[-1], "fused", group=members, tile=name[members[0]])
    for m in ls:
        if m.kind != "lin":
            check_fold(row, m)
    for sl in chunks:
        x = FR.layer_input_of(ls[0], by, sl, net.images)
        err = None
        for j, m in enumerate(ls):
            if m.kind == "lin":
                s = FR.stage_ref(x, _w(m), m.stride, shift=m.bias, x_err=err, act=False)
            else:
                res = by[m.shortcut].act[sl] if m.shortcut is not None else None
                s = FR.stage_ref(x, _w(m), m.stride, m.scale, m.shift, res, x_err=err, split=(m.idx == 1))
                row["ambiguous"] += FR.ambiguous(s)
            if j < len(ls) - 1:
                x, err = FR.rounded_mid(s)
            elif m.kind == "lin":
                row.bound("act", m.act[sl], s["y"], s["bz"], "layers %s f32 output" % members)
            else:
                row.bound("act", m.act[sl], s["y"], FR.bf16_bound(s), "layers %s act" % members)
            del s
    return row.done()


def check_fp8(net, l, chunks):
    """form 6: an e4m3 conv (inputs, weights, residual and output in e4m3 with per-tensor scales)"""
    by = net.by_idx
    src = by[l.src]
    row = Row(l, "fp8", tile="conv_fp8", dual16=bool(l.dual16))
    check_fold(row, l)
    row.bound("escale", l.escale, f64(l.scale) * src.s_out * l.s_w, FR.C_COEF * f64(l.scale).abs() * src.s_out * l.s_w,
              "layer %d escale" % l.idx)
    wq = FR.fp8_weights(l.w8, l.k, l.cin, l.cout)
    # the packed codes: RNE_e4m3(w / s_w) exactly (the pack kernel multiplies by 1/s_w in f32: only a midpoint within that
    # rounding may go either way)
    wt = f64(l.w).permute(3, 0, 1, 2).reshape(l.cout, -1)
    row.e4m3("w8", l.w8, wt, torch.zeros_like(wt), l.s_w, "layer %d packed e4m3 weights" % l.idx)
    for sl in chunks:
        xq = FR.decode_e4m3(src.act8[sl])
        res = None
        if l.shortcut is not None:
            sc = by[l.shortcut]
            res = FR.decode_e4m3(sc.act8[sl]) * sc.s_out
        s = FR.stage_ref(xq, wq, l.stride, l.escale, l.shift, res, c_acc=FR.C_ACC8)
        row["ambiguous"] += FR.ambiguous(s)
        row.e4m3("act8", l.act8[sl], s["y"], s["bz"], l.s_out, "layer %d e4m3 output" % l.idx)
        if l.dual16:
            row.bound("act", l.act[sl], s["y"], FR.bf16_bound(s), "layer %d bf16 output" % l.idx)
        del xq, res, s
    return row.done()


def check_handover(net, chunks):
    q = net._fp8_entry
    row = Row(q, "fp8 hand-over (quant_fp8)", tile="quant_fp8")
    for sl in chunks:
        want = f64(q.act[sl])
        row.e4m3("act8", q.act8[sl], want, torch.zeros_like(want), q.s_out, "layer %d quant_fp8" % q.idx)
    return row.done()


def check_detection(net, window):
    """form 7: detection filter and mask assembly on the kernels' own logits / score maps (the tolerances of
    test_gpu_fullsize.test_config0_single_image_576_forward_matches_oracle)"""
    t0 = time.perf_counter()
    by, B = net.by_idx, net.B
    preds = [by[i].act.cpu().view(B, by[i].Ho, by[i].Wo, 3, 5 + net.num_class) for i in (75, 67, 59)]
    pred = O.interpret_output(preds)
    want = O.filter_detections(pred[2], pred[3], pred[5], np.asarray(window, np.float32).reshape(B, 4), DET_THRESH)
    det = net.detections.cpu().numpy()
    np.testing.assert_allclose(det, want, rtol=1e-5, atol=1e-6)
    Sm = net.S // 2
    masks = torch.zeros(B, cfg.MAX_DETECTION, Sm, Sm, dtype=torch.float32, device=net.device)
    keep = torch.zeros(B, cfg.MAX_DETECTION, dtype=torch.int32, device=net.device)
    L.psroi_assemble(by[82].act, net.detections, B, cfg.MAX_DETECTION, Sm, net.k, masks, keep)
    torch.cuda.synchronize()
    wb, wm = O.val_test(det, by[82].act.cpu()) if net.k == 3 else FR.val_test_k(det, by[82].act.cpu(), net.k)
    kp = keep.cpu().numpy().astype(bool)
    n = 0
    for i in range(B):
        np.testing.assert_array_equal(det[i][kp[i]], wb[i])
        if kp[i].any():
            np.testing.assert_allclose(masks[i][torch.from_numpy(kp[i]).to(net.device)].cpu().numpy(), wm[i], rtol=1e-5, atol=1e-6)
            n += int(kp[i].sum())
        else:
            assert np.ndim(wm[i]) == 0
    assert n > 0, "no detection to assemble"
    return {"detections": int((det[:, :, 5] > 0).sum()), "assembled": n, "seconds": round(time.perf_counter() - t0, 2)}


def run_part_a(net, b, tag, snap, layers=None):
    """every layer (or only ``layers``) of the pass just run; returns (rows, report)"""
    B = net.B
    chunks = [slice(i, min(i + CHUNK, B)) for i in range(0, B, CHUNK)] if not net.training else [slice(None)]
    fp8 = {l.idx for l in net._fp8_layers()} if (net.dtype == "fp8" and net.fp8_ready) else set()
    groups = groups_of(net)
    in_group = {i: g for g in groups for i in g}
    rows, covered = [], []
    t0 = time.perf_counter()
    with torch.no_grad():
        for l in net.layers:
            if layers is not None and l.idx not in layers:
                continue
            if l.idx in in_group:
                g = in_group[l.idx]
                if l.idx == g[-1]:
                    rows.append(check_group(net, g, chunks))
                    covered += g
            elif l.idx in fp8:
                rows.append(check_fp8(net, l, chunks))
                covered.append(l.idx)
            elif train_bn(net, l):
                rows.append(check_training(net, l, snap))
                covered.append(l.idx)
            else:
                rows.append(check_inference(net, l, chunks))
                covered.append(l.idx)
            if fp8 and getattr(net, "_fp8_entry", None) is not None and l.idx == net._fp8_entry.idx:
                rows.append(check_handover(net, chunks))
        torch.cuda.synchronize()
    for r in rows:
        r.pop("stats", None)
    worst = {}
    for r in rows:
        for k, v in r["worst"].items():
            worst[k] = max(worst.get(k, 0.0), v)
    forms = {}
    for r in rows:
        for i in (r.get("group") or [r["layer"]]):
            if r["form"].startswith("fp8 hand"):
                continue
            forms.setdefault(r["form"], []).append(i)
    rep = {"config": tag, "B": B, "S": net.S, "k_map": net.k, "check_seconds": round(time.perf_counter() - t0, 2),
           "worst": worst, "forms": forms, "groups": groups,
           "ambiguous": sum(r["ambiguous"] for r in rows), "fp8_adjacent": sum(r["fp8_adjacent"] for r in rows),
           "bounds": {"U_BF16": FR.U_BF16, "C_ACC": FR.C_ACC, "C_ACC8": FR.C_ACC8, "C_SPLIT": FR.C_SPLIT, "C_EPI": FR.C_EPI, "C_SUM": FR.C_SUM,
                      "C_COEF": FR.C_COEF}, "layers": rows}
    return covered, rep


@pytest.mark.parametrize("tag", list(CONFIGS))
def test_forward_matches_f64_layer_by_layer(dev, tag, tuned_tables):
    c = CONFIGS[tag]
    net, b = build(dev, c)
    snap = perturb_moving(net) if net.training else {}
    t0 = time.perf_counter()
    eager(net, b)
    step = time.perf_counter() - t0
    covered, rep = run_part_a(net, b, tag, snap)
    rep["step_seconds"] = round(step, 2)
    window = net.clip_window.cpu().numpy() if net.training else b["clip_window"]
    try:
        rep["detection"] = check_detection(net, window)
    except AssertionError as e:
        rep["detection"] = {"failure": str(e)[:2000]}
    _report("forward_" + tag, rep)
    fails = [f for r in rep["layers"] for f in r["failures"]]
    assert not fails, "%d checks failed:\n%s" % (len(fails), "\n".join(fails[:40]))
    assert "failure" not in rep["detection"], rep["detection"]["failure"]
    # every layer exactly once, on its own or inside its fused launch
    assert sorted(covered) == list(range(1, 83)), sorted(covered)
    forms = rep["forms"]
    if tag == "train_s1_576_b8":
        # every stride-1, non-residual, non-head trainable layer whose grid is resident at once with the table's tiles (or
        # a covering fallback tile): conv58 / 66 are head branches, the 72^2 and larger maps have grids too large
        assert sorted(forms.get("in-launch", [])) == IN_LAUNCH_576_B8, forms
    if tag == "train_s1_576_b8_threelaunch":
        assert not forms.get("in-launch"), forms
    if tag.startswith("infer_576_b32") and c.get("dtype", "bf16") == "bf16":
        assert rep["groups"] == [list(g) for g in FUSED_GROUPS], rep["groups"]
    if c.get("dtype") == "fp8":
        assert sorted(forms.get("fp8", [])) == list(range(10, 53)), forms


@pytest.mark.parametrize("k_map", [5, 7])
def test_fused_mask_head_at_batch_32_for_larger_grids(dev, k_map, tuned_tables):
    """B = 32 inference nets with 5x5 / 7x7 score-map grids: the fused conv80-82 launch and the mask assembly"""
    net, b = build(dev, CONFIGS["infer_576_b32"], k_map=k_map)
    eager(net, b)
    assert [80, 81, 82] in groups_of(net)
    covered, rep = run_part_a(net, b, "infer_576_b32_k%d" % k_map, {}, layers={80, 81, 82})
    rep["detection"] = check_detection(net, b["clip_window"])
    _report("forward_infer_576_b32_k%d" % k_map, rep)
    fails = [f for r in rep["layers"] for f in r["failures"]]
    assert not fails, "\n".join(fails[:40])
    assert covered == [80, 81, 82]


# ------------------------------------------------------------------------------------------------ planted edges
PLANT_LAYERS = (54, 57, 62, 65)     # in-launch layers (3x3 and 1x1, 18^2 and 36^2) whose source's output feeds them alone
PLANT_RATIOS = {0: 1.0, 1: 16.0, 2: 64.0, 3: 256.0}      # channel -> |mean|/std (256: reported only)
ZERO_CH, NEG_CH, NEG_GAMMA_CH = 4, 5, 6
CONST = 5.0                                             # the constant input channel planted in the source layer


def _plant(net, b, snap):
    """input channel 0 of every planted layer constant (its source layer: gamma 0, beta CONST), then per planted layer the
    weight of that channel's centre tap sets each ratio channel's mean to ratio * std of the rest of its conv"""
    by = net.by_idx
    with torch.no_grad():
        for p in PLANT_LAYERS:
            q = by[by[p].src]
            q.gamma[0], q.beta[0] = 0.0, CONST
        net.refresh_weights()
        for p in PLANT_LAYERS:
            l = by[p]
            w = l.w                    # f32 master [k,k,cin,cout]
            ctr = l.k // 2
            w[ctr, ctr, 0, :7] = 0.0
            w[..., ZERO_CH] = 0.0
            l.gamma[NEG_CH], l.beta[NEG_CH] = 0.1, -4.0
            l.gamma[NEG_GAMMA_CH] = -1.5
            net.refresh_weights()
            for q_, (mm0, mv0) in snap.items():
                by[q_].mm.copy_(mm0)
                by[q_].mv.copy_(mv0)
            eager(net, b)
            x = FR.layer_input_of(l, by, slice(None), net.images)
            assert bool((x[..., 0] == CONST).all()), "layer %d: input channel 0 is not constant" % p
            v = FR.conv_ref(x, _w(l)[..., :4], l.stride, twin=False)
            mean, var = FR.moments(v)
            for ch, r in PLANT_RATIOS.items():
                w[ctr, ctr, 0, ch] = float((r * var[ch].sqrt() - mean[ch]) / CONST)
            net.refresh_weights()
        for q_, (mm0, mv0) in snap.items():
            by[q_].mm.copy_(mm0)
            by[q_].mv.copy_(mv0)


def test_planted_statistics_and_leaky_edges(dev, tuned_tables):
    net, b = build(dev, CONFIGS["train_s1_576_b8"])
    snap = perturb_moving(net)
    _plant(net, b, snap)
    assert all(net.by_idx[p].fused_fwd for p in PLANT_LAYERS), [p for p in PLANT_LAYERS if not net.by_idx[p].fused_fwd]
    table, fails, rows = [], [], []
    for form in ("in-launch", "three-launch"):
        if form == "three-launch":
            net.bn_inkernel = False
            net._apply_tiles()
            assert not any(net.by_idx[p].fused_fwd for p in PLANT_LAYERS)
        with torch.no_grad():
            for q_, (mm0, mv0) in snap.items():
                net.by_idx[q_].mm.copy_(mm0)
                net.by_idx[q_].mv.copy_(mv0)
        eager(net, b)
        with torch.no_grad():
            for p in PLANT_LAYERS:
                l = net.by_idx[p]
                row = check_training(net, l, snap, skip_stats=[3])
                assert row["form"] == form
                st = row.pop("stats")
                fails += row["failures"]
                rows.append(row)
                for ch in range(7):
                    m, var, rs = float(st["mean"][ch]), float(st["var"][ch]), float(st["rstd"][ch])
                    table.append({"layer": p, "form": form, "channel": ch,
                                  "plant": {0: "ratio 1", 1: "ratio 16", 2: "ratio 64", 3: "ratio 256 (reported only)",
                                            4: "zero weights", 5: "all negative", 6: "negative gamma"}[ch],
                                  "mean_over_std": abs(m) / var ** 0.5 if var > 0 else None,
                                  "rstd_rel_err": abs(float(l.rstd[ch]) - rs) / rs,
                                  "mean_err": abs(float(l.mean[ch]) - m),
                                  "negative_outputs": float((l.act[..., ch].float() < 0).double().mean())})
    _report("forward_planted_train_s1_576_b8", {"channels": table, "layers": rows})
    assert not fails, "\n".join(fails[:40])
    for t in table:
        if t["channel"] in (1, 2):
            assert t["rstd_rel_err"] < FR.RSTD_LIMIT, t
        if t["channel"] in (0, 1, 2, 3):
            assert abs(t["mean_over_std"] / PLANT_RATIOS[t["channel"]] - 1) < 0.1, t       # the plant took
        if t["channel"] == ZERO_CH:
            assert t["mean_over_std"] is None and t["rstd_rel_err"] < 2.0 ** -20, t
        if t["channel"] == NEG_CH:
            assert t["negative_outputs"] == 1.0, t


# ------------------------------------------------------------------------------------------------ bit-identity
def _written(net):
    """layers whose output tensors the pass writes (not the intermediates of a fused launch, nor conv9's before fp8)"""
    inner = {i for g in groups_of(net) for i in g[:-1]}
    return [l for l in net.layers if l.idx not in inner]


def test_recorded_train_step_forward_is_bitwise_the_eager_one(dev, tuned_tables):
    net, b = build(dev, CONFIGS["train_s1_576_b8"])
    snap = perturb_moving(net)
    eager(net, b)
    names = ("act", "raw", "mean", "rstd", "mm", "mv")
    want = {(l.idx, n): getattr(l, n).clone() for l in _written(net) for n in names if getattr(l, n) is not None
            and (n in ("act",) or train_bn(net, l))}
    with torch.no_grad():
        for i, (mm0, mv0) in snap.items():
            net.by_idx[i].mm.copy_(mm0)
            net.by_idx[i].mv.copy_(mv0)
    net.build_program(det_thresh=DET_THRESH, pipeline_backbone=True)
    net.prime_pipeline()
    q = net._parity
    net.train_step(None, want_loss=False)
    torch.cuda.synchronize()
    # the double-buffered backbone outputs: parity q was written by prime_pipeline, the other one by the recorded step's own
    # backbone pass (for the next batch -- the same images here: the second input set is a copy of the first)
    xbuf = getattr(net, "_xbuf", {}) or {}
    assert xbuf, "no double-buffered backbone output"
    bad = []
    for (i, n), t in want.items():
        gots = [xbuf[i][q], xbuf[i][1 - q]] if (n == "act" and i in xbuf) else [getattr(net.by_idx[i], n)]
        for got in gots:
            if not torch.equal(got.view(torch.uint8), t.view(torch.uint8)):
                bad.append((i, n))
    assert not bad, "recorded step differs from the eager forward in %s" % bad


def test_inference_graph_forward_is_bitwise_the_eager_one(dev, tuned_tables):
    net, b = build(dev, CONFIGS["infer_576_b32"])
    eager(net, b)
    want = {l.idx: l.act.clone() for l in _written(net)}
    for l in net.layers:
        l.act.fill_(0)
    net.build_infer_program(det_thresh=DET_THRESH, graph=True)
    net.infer()
    torch.cuda.synchronize()
    bad = [i for i, t in want.items() if not torch.equal(t.view(torch.uint8), net.by_idx[i].act.view(torch.uint8))]
    assert not bad, "graph replay differs from the eager forward in layers %s" % bad


# ------------------------------------------------------------------------------------------------ Part B: integer operands
# Every distinct forward launch of a configuration is issued again with its own shape, flags and tile on fresh integer
# operands: every f32 partial sum is an integer below 2^24, so any summation order gives the exact sum.  bf16 outputs must
# be the epilogue emulated in f32 in the kernels' order (scale and shift, leaky 0.1f*v, residual add) rounded once to
# nearest-even; f32 outputs and statistics rows the exact values; the finalize outputs within 1 f32 ulp of the kernels' f32
# formula evaluated on the exact sums; e4m3 outputs the torch float8_e4m3fn rounding (power-of-two scales).
EXACT_CONFIGS = ("train_s1_576_b8", "train_s2_576_b8", "infer_576_b32", "infer_576_b32_fp8")
ALPHA32 = torch.tensor(cfg.ALPHA, dtype=torch.float32)


class Collector:
    """stands in for the tuner while one eager pass runs: every conv2d_fwd descriptor, by shape, flags and tile (launched
    without the in-launch batch norm, as the tuner does; the caller then issues the separate batch-norm launches)"""

    def __init__(self):
        self.descs, self.stats_rows = {}, {}

    def launch(self, d):
        key = L.conv_shape_key(d) + (d.flags, bool(d.residual), bool(d.scale), bool(d.shift), d.pad_t, d.pad_l, d.tile)
        if key not in self.descs:
            self.descs[key] = L.ConvDesc.from_buffer_copy(d)
        if d.stats:
            self.stats_rows[d.stats] = L.conv2d_stats_rows(d)
        keep = d.flags
        d.flags &= ~(L.CONV_BN_FUSED | L.CONV_BN_BWD_FUSED)
        rc = L.load().disyolo_conv2d_fwd(ctypes.byref(d), L._stream())
        d.flags = keep
        L._check(rc, "conv2d_fwd")


def _ints(shape, lo, hi, dev, g, dtype=torch.float32):
    return torch.randint(lo, hi + 1, tuple(shape), generator=g, device=dev).to(dtype)


def _pow2(n, dev, g):
    return torch.exp2(_ints((n,), -1, 1, dev, g))


def _dyadic(n, dev, g):
    return _ints((n,), -6, 6, dev, g) * 0.25


def _sparse_w(k, cin, cout, nz, dev, g):
    """HWIO weights with at most nz entries of +-1 per output channel (|conv| <= 2 nz on inputs in [-2, 2])"""
    K = k * k * cin
    w = torch.zeros(K, cout, device=dev)
    idx = torch.rand(K, cout, generator=g, device=dev).argsort(0)[:min(nz, K)]
    w.scatter_(0, idx, torch.where(torch.rand(idx.shape, generator=g, device=dev) < 0.5, -1.0, 1.0))
    return w.view(k, k, cin, cout)


def _pack(w_hwio):
    k, _, cin, cout = w_hwio.shape
    wp = torch.empty(cout, k * k * cin, dtype=torch.bfloat16, device=w_hwio.device)
    L.pack_weights(w_hwio.contiguous(), wp, None, k, cin, cout)
    return wp


def epilogue32(acc, scale=None, shift=None, leaky=False, res=None):
    """the conv epilogue in f32, in the kernels' order: acc*scale + shift, leaky (fmax(0.1f*v, v)), + residual"""
    v = acc.float()
    if scale is not None:
        v = v * scale.float()
    if shift is not None:
        v = v + shift.float()
    if leaky:
        v = torch.maximum(v * ALPHA32.to(v.device), v)
    if res is not None:
        v = v + res.float()
    return v


def _exact_bf16(got, want32, what, fails):
    """bf16 output == the f32 value rounded once to nearest-even"""
    w = want32.to(torch.bfloat16)
    ne = got.reshape(w.shape).view(torch.int16) != w.view(torch.int16)
    if bool(ne.any()):
        i = int(ne.flatten().nonzero()[0])
        fails.append("%s: %d of %d bf16 elements differ; first at flat %d: got %r want %r" % (
            what, int(ne.sum()), ne.numel(), i, float(got.flatten()[i]), float(w.flatten()[i])))


def _exact_f32(got, want32, what, fails):
    ne = got.reshape(want32.shape).view(torch.int32) != want32.view(torch.int32)
    if bool(ne.any()):
        i = int(ne.flatten().nonzero()[0])
        fails.append("%s: %d of %d f32 elements differ; first at flat %d: got %r want %r" % (
            what, int(ne.sum()), ne.numel(), i, float(got.flatten()[i]), float(want32.flatten()[i])))


def _ulps(got, wants, n, what, fails):
    """|got - want| <= n ulps of want (f32) for one of ``wants`` (the f32 evaluations a compiler may produce: with and
    without a fused multiply-add)"""
    err = ulp = None
    for w in (wants if isinstance(wants, (list, tuple)) else [wants]):
        e = (got.double() - w.double()).abs()
        u = torch.where(w != 0, w.abs().double() * 2.0 ** -23, torch.full_like(e, 2.0 ** -149))
        if err is None:
            err, ulp = e, u
        else:
            better = e / u < err / ulp
            err, ulp = torch.where(better, e, err), torch.where(better, u, ulp)
    bad = err > n * ulp
    if bool(bad.any()):
        i = int(bad.nonzero()[0])
        fails.append("%s: %d of %d beyond %d ulp; first at %d: got %r (err %.3g, ulp %.3g)" % (
            what, int(bad.sum()), bad.numel(), n, i, float(got[i]), float(err[i]), float(ulp[i])))


def _finalize_ref(s1, s2, M, gamma, beta, mm0, mv0):
    """the kernels' finalize (bn.hip bn_finalize_kernel, conv_common.h cl_bn_coeffs) on the exact f64 sums: mean and var in
    double, everything after in f32.  shift = beta - mean*scale and the moving averages are given both as separate f32
    operations and as one rounding of the exact expression (what a fused multiply-add gives)"""
    mean = s1 / M
    var = (s2 / M - mean * mean).clamp(min=0)
    meanf, varf = mean.float(), var.float()
    rstd = 1.0 / torch.sqrt(varf + torch.tensor(cfg.BN_EPSILON, dtype=torch.float32))
    sc = gamma * rstd
    d = torch.tensor(cfg.BN_DECAY, dtype=torch.float32, device=gamma.device)
    e = 1 - d
    D = lambda t: t.double()
    return dict(mean=meanf, rstd=rstd, scale=sc,
                shift=[beta - meanf * sc, (D(beta) - D(meanf) * D(sc)).float()],
                mm=[mm0 * d + meanf * e, (D(mm0) * D(d) + D(meanf) * D(e)).float()],
                mv=[mv0 * d + varf * e, (D(mv0) * D(d) + D(varf) * D(e)).float()])


def exact_conv_desc(d0, dev, g, fails, cands=(None,)):
    """one collected conv2d_fwd descriptor on integer operands, under its own tile (or each of ``cands``); returns the
    tiles that ran"""
    B, H, W, C0, C1, Cout, k = d0.B, d0.H, d0.W, d0.C0, d0.C1, d0.Cout, d0.ksize
    assert d0.in_div == 1
    Ho, pt = L.same_pads(H, k, d0.stride)
    Wo, pl = L.same_pads(W, k, d0.stride)
    assert (d0.Ho, d0.Wo, d0.pad_t, d0.pad_l) == (Ho, Wo, pt, pl)
    stats = bool(d0.flags & L.CONV_STATS)
    fused = bool(d0.flags & L.CONV_BN_FUSED)
    f32 = bool(d0.flags & L.CONV_OUT_F32)
    leaky = bool(d0.flags & L.CONV_LEAKY)
    x0 = _ints((B, H, W, C0), -2, 2, dev, g, torch.bfloat16)
    x1 = _ints((B, H // 2, W // 2, C1), -2, 2, dev, g, torch.bfloat16) if C1 else None
    # statistics: |conv| <= 64, so x^2 summed over any tile of pixels stays an integer below 2^24
    w = _sparse_w(k, C0 + C1, Cout, 32, dev, g) if stats else _ints((k, k, C0 + C1, Cout), -1, 1, dev, g)
    wp = _pack(w)
    scale = _pow2(Cout, dev, g) if d0.scale else None
    shift = _dyadic(Cout, dev, g) if d0.shift else None
    res = _ints((B, Ho, Wo, Cout), -3, 3, dev, g, torch.bfloat16) if d0.residual else None
    xin = torch.cat([x0.double(), FR.upsample2(x1.double())], -1) if C1 else x0.double()
    acc = FR.conv_ref(xin, w, d0.stride, twin=False)
    assert float(acc.abs().max()) < 2.0 ** 24
    want = epilogue32(acc, scale, shift, leaky, res)
    M = B * Ho * Wo
    ran = []
    for cand in cands:
        tile = d0.tile if cand is None else cand
        y = torch.full((B, Ho, Wo, Cout), float("nan"), dtype=torch.float32 if f32 else torch.bfloat16, device=dev)
        kw = dict(x1=x1, scale=scale, shift=shift, residual=res, leaky=leaky, out_f32=f32, alpha=d0.alpha, tile=tile)
        d = L.make_conv_desc(x0, wp, y, k, d0.stride, **kw)
        d.tile = tile
        tid = L.conv2d_tile(d)[0]
        what = "conv %s tile %#x (ran %#x)" % (list(L.conv_shape_key(d)), tile, tid)
        bn = None
        if stats:
            rows = L.conv2d_stats_rows(d)
            st = torch.full((rows, Cout, 2), float("nan"), device=dev)
            if fused:
                bn = dict(y_act=torch.full_like(y, float("nan")), gamma=torch.randn(Cout, generator=g, device=dev),
                          beta=torch.randn(Cout, generator=g, device=dev), mm=torch.randn(Cout, generator=g, device=dev),
                          mv=torch.rand(Cout, generator=g, device=dev) + 0.5, scale=torch.empty(Cout, device=dev),
                          shift=torch.empty(Cout, device=dev), mean=torch.empty(Cout, device=dev),
                          rstd=torch.empty(Cout, device=dev), decay=cfg.BN_DECAY, eps=cfg.BN_EPSILON,
                          sync=L.cluster_sync_buffer(Cout, dev))
                mm0, mv0 = bn["mm"].clone(), bn["mv"].clone()
            d = L.make_conv_desc(x0, wp, y, k, d0.stride, stats=st, bn_fused=bn, **kw)
            d.tile = tile
            if fused:
                assert L.conv2d_bn_fused_ok(d), what
        L.conv2d_fwd(d)
        torch.cuda.synchronize()
        ran.append(tid)
        (_exact_f32 if f32 else _exact_bf16)(y, want, what, fails)
        if stats:
            a = acc.reshape(-1, Cout)
            s1, s2 = a.sum(0), (a * a).sum(0)
            got = st.double()
            if not bool((got == got.round()).all()):
                fails.append(what + ": a statistics row is not an integer")
            # (every row an integer below 2^24: it is an exact partial sum; their f64 total is then exact too)
            tot = got.sum(0)
            for q, ex, n in ((0, s1, "sum x"), (1, s2, "sum x^2")):
                if not torch.equal(tot[:, q], ex):
                    fails.append("%s statistics rows (%s): %d channels differ from the exact sum" % (what, n,
                                                                                               int((tot[:, q] != ex).sum())))
            if fused:
                ref = _finalize_ref(s1, s2, M, bn["gamma"], bn["beta"], mm0, mv0)
                for n in ("mean", "rstd", "scale", "shift", "mm", "mv"):
                    _ulps(bn[n], ref[n], 1, what + " in-launch " + n, fails)
                # the activation from the launch's own coefficients, applied to the bf16 raw tile (exact: |raw| <= 64);
                # the product and the shift may be one fused multiply-add: either rounding is accepted
                raw = y.float().reshape(-1, Cout)
                fma = (raw.double() * bn["scale"].double() + bn["shift"].double()).float()
                sep = raw * bn["scale"] + bn["shift"]
                ya = bn["y_act"].reshape(-1, Cout)
                ok = torch.zeros_like(ya, dtype=torch.bool)
                for v in (fma, sep):
                    ok |= ya.view(torch.int16) == torch.maximum(v * ALPHA32.to(dev), v).to(torch.bfloat16).view(torch.int16)
                if not bool(ok.all()):
                    fails.append("%s: in-launch activation differs in %d elements" % (what, int((~ok).sum())))
            else:
                # the three-launch finalize on the rows this launch wrote
                gamma, beta = torch.randn(Cout, generator=g, device=dev), torch.randn(Cout, generator=g, device=dev)
                mm, mv = torch.randn(Cout, generator=g, device=dev), torch.rand(Cout, generator=g, device=dev) + 0.5
                ref = _finalize_ref(s1, s2, M, gamma, beta, mm.clone(), mv.clone())
                out = {n: torch.empty(Cout, device=dev) for n in ("scale", "shift", "mean", "rstd")}
                L.bn_finalize(st, rows, Cout, M, gamma, beta, mm, mv, cfg.BN_DECAY, cfg.BN_EPSILON, out["scale"], out["shift"],
                              out["mean"], out["rstd"])
                torch.cuda.synchronize()
                out.update(mm=mm, mv=mv)
                for n in ref:
                    _ulps(out[n], ref[n], 1, what + " bn_finalize " + n, fails)
    return ran


def exact_fused(net, members, dev, g, fails):
    """a fused launch on non-negative integer operands (its bf16 intermediates are integers, rounded as the kernel rounds)"""
    by, B = net.by_idx, net.B
    ls = [by[i] for i in members]
    first = ls[0]
    S = net.S
    if members[0] == 1:
        img = _ints((B, S, S, 3), 0, 1, dev, g)
        x, x1 = img, None
        xin = img.double()
    else:
        src = by[first.src]
        x = _ints(src.act.shape, 0, 1, dev, g, torch.bfloat16)
        x1 = _ints(by[first.src_up].act.shape, 0, 1, dev, g, torch.bfloat16) if first.src_up is not None else None
        xin = torch.cat([x.double(), FR.upsample2(x1.double())], -1) if x1 is not None else x.double()
    ws, scs, shs = [], [], []
    for j, m in enumerate(ls):
        cin = m.cin
        lo = 0 if j < len(ls) - 1 else -1      # the intermediates stay non-negative; the last conv has both signs
        ws.append(_ints((m.k, m.k, cin, m.cout), lo, 1, dev, g))
        scs.append(_pow2(m.cout, dev, g) if j == len(ls) - 1 and m.kind != "lin" else torch.ones(m.cout, device=dev))
        shs.append(_dyadic(m.cout, dev, g) if j == len(ls) - 1 else torch.zeros(m.cout, device=dev))
    cur = xin
    for j, m in enumerate(ls):
        acc = FR.conv_ref(cur, ws[j], m.stride, twin=False)
        assert float(acc.abs().max()) < 2.0 ** 24
        if j < len(ls) - 1:
            cur = acc.float().to(torch.bfloat16).double()          # (non-negative: the leaky side is never taken)
    last = ls[-1]
    res = x if last.shortcut is not None else None
    if last.kind == "lin":
        want = epilogue32(acc, None, shs[-1])
        y = torch.full(last.act.shape, float("nan"), device=dev)
    else:
        want = epilogue32(acc, scs[-1], shs[-1], True, res)
        y = torch.full(last.act.shape, float("nan"), dtype=torch.bfloat16, device=dev)
    if members[0] == 1:
        L.conv12_fused_fwd(img, ws[0], scs[0], shs[0], _pack(ws[1]), scs[1], shs[1], y, alpha=cfg.ALPHA)
    elif members[0] in (6, 8):
        L.block64_fused_fwd(x, _pack(ws[0]), scs[0], shs[0], _pack(ws[1]), scs[1], shs[1], y, alpha=cfg.ALPHA)
    elif members[0] == 3:
        L.block32_fused_fwd(x, None, _pack(ws[0]), scs[0], shs[0], _pack(ws[1]), scs[1], shs[1], y, post=0, alpha=cfg.ALPHA)
    else:
        L.block32_fused_fwd(x, x1, _pack(ws[0]), scs[0], shs[0], _pack(ws[1]), scs[1], shs[1], y, post=L.block32_post(net.k),
                            wC=_pack(ws[2]), biasC=shs[2], alpha=cfg.ALPHA)
    torch.cuda.synchronize()
    what = "fused launch %s" % members
    (_exact_f32 if last.kind == "lin" else _exact_bf16)(y, want, what, fails)


def exact_conv_first(net, dev, g, fails):
    l = net.by_idx[1]
    img = _ints(net.images.shape, -2, 2, dev, g)
    w = _ints((3, 3, 3, l.cout), -1, 1, dev, g)
    sc, sh = _pow2(l.cout, dev, g), _dyadic(l.cout, dev, g)
    y = torch.full(l.act.shape, float("nan"), dtype=torch.bfloat16, device=dev)
    L.conv_first_fwd(img, w, sc, sh, y, alpha=cfg.ALPHA)
    torch.cuda.synchronize()
    _exact_bf16(y, epilogue32(FR.conv_ref(img, w, 1, twin=False), sc, sh, True), "conv_first_fwd", fails)


def _e4m3_codes(v32):
    return v32.clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)


def exact_fp8(l, src, sc_layer, dev, g, fails):
    """an e4m3 conv: integer codes in and out, power-of-two scales"""
    B = src.act8.shape[0]
    x8 = _e4m3_codes(_ints(src.act8.shape, -2, 2, dev, g))
    wq = _ints((l.k, l.k, l.cin, l.cout), -1, 1, dev, g)
    w8 = _e4m3_codes(wq.permute(3, 0, 1, 2).reshape(l.cout, -1).contiguous())
    es, eh = _pow2(l.cout, dev, g) * 0.25, _dyadic(l.cout, dev, g)
    r8, rs = (_e4m3_codes(_ints(l.act8.shape, -3, 3, dev, g)), 0.5) if sc_layer is not None else (None, 0.0)
    y8 = torch.full(l.act8.shape, 0x7f, dtype=torch.uint8, device=dev)
    y16 = torch.full(l.act8.shape, float("nan"), dtype=torch.bfloat16, device=dev) if l.dual16 else None
    d = L.make_conv_desc(x8, w8, y8, l.k, l.stride, leaky=True, alpha=cfg.ALPHA)
    out_scale = 2.0
    L.conv2d_fp8_fwd(d, w8, es, eh, y8, out_scale, y16=y16, residual8=r8, residual_scale=rs)
    torch.cuda.synchronize()
    acc = FR.conv_ref(FR.decode_e4m3(x8), wq, l.stride, twin=False)
    assert float(acc.abs().max()) < 2.0 ** 24
    v = epilogue32(acc, es, eh, True, FR.decode_e4m3(r8).float() * rs if r8 is not None else None)
    what = "fp8 conv of layer %d (%s)" % (l.idx, [B] + list(src.act8.shape[1:]) + [l.cout, l.k, l.stride])
    ne = y8 != _e4m3_codes(v * (1.0 / out_scale))
    if bool(ne.any()):
        fails.append("%s: %d of %d e4m3 codes differ" % (what, int(ne.sum()), ne.numel()))
    if y16 is not None:
        _exact_bf16(y16, v, what + " bf16 output", fails)


def exact_quant(q, dev, g, fails):
    x = (_ints(q.act.shape, -1000, 1000, dev, g) * 0.25).to(torch.bfloat16)
    y8 = torch.full(q.act8.shape, 0x7f, dtype=torch.uint8, device=dev)
    L.quant_fp8(x, y8, 0.5)
    torch.cuda.synchronize()
    ne = y8 != _e4m3_codes(x.float() * 2.0)
    if bool(ne.any()):
        fails.append("quant_fp8: %d of %d codes differ" % (int(ne.sum()), ne.numel()))


@pytest.mark.parametrize("tag", EXACT_CONFIGS)
def test_forward_launches_are_exact_on_integers(dev, tag, tuned_tables):
    c = CONFIGS[tag]
    net, b = build(dev, c)
    t0 = time.perf_counter()
    col = Collector()
    L.TUNER = col
    try:
        eager(net, b)
    finally:
        L.TUNER = None
    g = torch.Generator(device=dev).manual_seed(21)
    fails, launches = [], []
    sweep = tag == "infer_576_b32"        # (the fp8 B = 32 benchmark tunes its bf16 layers live: any candidate may run)
    with torch.no_grad():
        for key, d0 in col.descs.items():
            cands = [None]
            if sweep:
                cands += [t for t in L.TUNE_CANDIDATES
                          if L.conv2d_tile(_retile(d0, t))[0] == (t & 0xff)]
            ran = exact_conv_desc(d0, dev, g, fails, cands)
            launches.append({"launch": "conv2d_fwd", "shape": list(L.conv_shape_key(d0)), "flags": d0.flags,
                             "tile": d0.tile, "ran": ran, "candidates": [t for t in cands if t is not None]})
        for grp in groups_of(net):
            exact_fused(net, grp, dev, g, fails)
            launches.append({"launch": "fused", "layers": grp})
        if net.training and not net.by_idx[1].lock:
            exact_conv_first(net, dev, g, fails)
            launches.append({"launch": "conv_first_fwd"})
        if net.dtype == "fp8":
            seen = set()
            for l in net._fp8_layers():
                src = net.by_idx[l.src]
                key = (tuple(src.act8.shape), l.cout, l.k, l.stride, l.shortcut is not None, bool(l.dual16))
                if key in seen:
                    continue
                seen.add(key)
                exact_fp8(l, src, net.by_idx[l.shortcut] if l.shortcut is not None else None, dev, g, fails)
                launches.append({"launch": "conv2d_fp8_fwd", "layer": l.idx})
            exact_quant(net._fp8_entry, dev, g, fails)
            launches.append({"launch": "quant_fp8", "layer": net._fp8_entry.idx})
    _report("forward_exact_" + tag, {"config": tag, "seconds": round(time.perf_counter() - t0, 2), "failures": fails,
                                     "launches": launches})
    assert not fails, "%d launches differ from their exact references:\n%s" % (len(fails), "\n".join(fails[:40]))
    n_conv = sum(1 for e in launches if e["launch"] == "conv2d_fwd")
    assert n_conv >= 10
    if tag.startswith("infer"):
        assert sum(1 for e in launches if e["launch"] == "fused") == 5
    if tag == "train_s1_576_b8":
        assert any(e.get("flags", 0) & L.CONV_BN_FUSED for e in launches)
    if tag == "train_s2_576_b8":
        assert any(e["launch"] == "conv_first_fwd" for e in launches)


def _retile(d0, t):
    d = L.ConvDesc.from_buffer_copy(d0)
    d.tile = t
    return d

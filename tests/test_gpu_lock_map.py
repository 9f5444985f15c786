"""Training with any lock map: the frozen batch-norm backward kernel against float64, whole steps of holed maps against
the CPU oracle (which differentiates through locked layers with autograd), the pass-through layers one by one against the
float64 references of tests/backward_ref.py, the recorded forms of the step, and the two reference stages left as they were.

The reference: ``lock`` is an argument of every conv_bn / conv call (yolo/yolo3_net_pos.py:71-146).  A locked layer
normalises with its moving statistics even when is_training is true (:76-81), trains nothing, and TF autodiff passes the loss
gradient through it: d conv = g * leaky'(z) * scale_c, z = scale_c * conv + shift_c."""
import json
import os

import numpy as np
import pytest
import torch

import backward_ref as R
import disyolo_oracle as O
import mask_stride_ref as MR
from backward_ref import C_G_REL, C_G_ACC, C_G_TWIN
from disyolo_amd import config as cfg
from disyolo_amd import lib as L
from disyolo_amd.net import YOLONet
from lock_maps import MAPS, inputs_of, lock_of, pass_through
from net_setup import perturb_variables

pytestmark = pytest.mark.gpu

REPORTS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "test_reports")
ALPHA = 0.1
U_BF16 = 2.0 ** -8          # one bf16 rounding of an f32 result, relative


# ------------------------------------------------------------------------------------------------ the kernel
SHAPES = [(1, 16), (777, 200), (1000, 32), (2, 1024), (4099, 16), (20736, 128)]


def _kernel_inputs(rows, C):
    g = torch.Generator().manual_seed(1000 * C + rows)
    x = torch.randn(rows, C, generator=g).to(torch.bfloat16)
    scale = 0.25 + 1.5 * torch.rand(C, generator=g)
    neg = torch.randperm(C, generator=g)[:C // 4]
    scale[neg] = -scale[neg]
    shift = 0.5 * torch.randn(C, generator=g)
    dy = torch.randn(rows, C, generator=g).to(torch.bfloat16)
    sc0 = torch.randn(rows, C, generator=g).to(torch.bfloat16)        # what the shortcut's gradient buffer holds before
    return x, scale, shift, dy, sc0


def frozen_bwd_f64(dy, x, scale, shift, alpha=ALPHA):
    """(want, decidable): dx = scale * dy * leaky'(z) in float64 on the kernel's own operands; ``decidable`` is False where
    z = x*scale + shift is within rounding of zero (either slope may be taken)"""
    dy, x, scale, shift = (t.detach().double().cpu() for t in (dy, x, scale, shift))
    z = x * scale + shift
    ok = z.abs() >= 1e-5 * ((x * scale).abs() + shift.abs())
    want = scale * (dy * torch.where(z > 0, torch.ones_like(z), torch.full_like(z, alpha)))
    return want, ok


def check_frozen_dx(got, dy, x, scale, shift, what):
    want, ok = frozen_bwd_f64(dy, x, scale, shift)
    left_out = int((~ok).sum())
    assert left_out <= 1e-3 * ok.numel(), "%s: %d of %d elements undecidable" % (what, left_out, ok.numel())
    err = (got.detach().double().cpu().reshape(want.shape) - want).abs()
    ratio = torch.where(ok, err / (U_BF16 * want.abs()).clamp_min(1e-300), torch.zeros_like(err))
    ratio = torch.where(ok & (want == 0), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)), ratio)
    worst = float(ratio.max())
    print("%s: worst |err| / (2^-8 |want|) = %.4f, %d left out" % (what, worst, left_out))
    assert worst <= 1.0, "%s: %d elements beyond 2^-8 |want| (worst ratio %.3g)" % (what, int((ratio > 1).sum()), worst)
    return worst


@pytest.mark.parametrize("mode", ["none", "set", "accumulate"])
@pytest.mark.parametrize("rows,C", SHAPES)
def test_bn_frozen_bwd_matches_f64(dev, rows, C, mode):
    x, scale, shift, dy, sc0 = _kernel_inputs(rows, C)
    xd, sd, hd, dyd = x.to(dev), scale.to(dev), shift.to(dev), dy.to(dev)
    outs = []
    for _ in range(2):
        dx = torch.full((rows, C), float("nan"), dtype=torch.bfloat16, device=dev)
        sc = sc0.to(dev).clone() if mode != "none" else None
        L.bn_frozen_bwd(dyd, xd, sd, hd, dx, rows, C, ALPHA, shortcut_grad=sc, shortcut_accumulate=(mode == "accumulate"))
        torch.cuda.synchronize()
        outs.append((dx, sc))
    dx, sc = outs[0]
    check_frozen_dx(dx, dy, x, scale, shift, "bn_frozen_bwd %dx%d %s" % (rows, C, mode))
    assert torch.equal(xd.cpu().view(torch.int16), x.view(torch.int16)) and torch.equal(dyd.cpu().view(torch.int16), dy.view(torch.int16))
    if mode == "set":
        assert torch.equal(sc.cpu().view(torch.int16), dy.view(torch.int16))
    elif mode == "accumulate":
        # disyolo_add_bf16: both operands widened to f32, added, rounded once to bf16
        want_sc = (dy.float() + sc0.float()).to(torch.bfloat16)
        assert torch.equal(sc.cpu().view(torch.int16), want_sc.view(torch.int16))
        via_add = sc0.to(dev).clone()
        L.add_bf16(dyd, via_add, True)
        assert torch.equal(sc.view(torch.int16), via_add.view(torch.int16))
    # deterministic
    assert torch.equal(outs[0][0].view(torch.int16), outs[1][0].view(torch.int16))
    if sc is not None:
        assert torch.equal(outs[0][1].view(torch.int16), outs[1][1].view(torch.int16))


@pytest.mark.parametrize("mode", ["none", "accumulate"])
def test_bn_frozen_bwd_in_place(dev, mode):
    rows, C = 20736, 128
    x, scale, shift, dy, sc0 = _kernel_inputs(rows, C)
    xd, sd, hd = x.to(dev), scale.to(dev), shift.to(dev)
    res = []
    for in_place in (False, True):
        g = dy.to(dev).clone()
        out = g if in_place else torch.empty_like(g)
        sc = sc0.to(dev).clone() if mode != "none" else None
        L.bn_frozen_bwd(g, xd, sd, hd, out, rows, C, ALPHA, shortcut_grad=sc, shortcut_accumulate=(mode == "accumulate"))
        torch.cuda.synchronize()
        res.append((out, sc))
    assert torch.equal(res[0][0].view(torch.int16), res[1][0].view(torch.int16))
    if mode != "none":
        assert torch.equal(res[0][1].view(torch.int16), res[1][1].view(torch.int16))
    check_frozen_dx(res[1][0], dy, x, scale, shift, "bn_frozen_bwd in place (%s)" % mode)


def test_bn_frozen_bwd_argument_errors_come_back_before_any_launch():
    """DY_REQUIRE: nothing below reaches a device (the pointers are host buffers)"""
    import ctypes
    lib = L.load()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.cast(buf, ctypes.c_void_p)
    call = lambda dy=p, x=p, scale=p, shift=p, dx=p, rows=4, C=16, sc=None: lib.disyolo_bn_frozen_bwd(
        dy, x, scale, shift, dx, rows, C, 0.1, sc, 0, None)
    for kw in (dict(dy=None), dict(x=None), dict(scale=None), dict(shift=None), dict(dx=None), dict(rows=0), dict(rows=-3),
               dict(C=12), dict(C=0), dict(sc=p)):
        assert call(**kw) == -1, kw
        assert b"bn_frozen_bwd" in lib.disyolo_last_error()


# ------------------------------------------------------------------------------------------------ nets with holed maps
def rel_err(got, want):
    got = torch.as_tensor(got).double().cpu().flatten()
    want = torch.as_tensor(want).detach().double().cpu().flatten()
    return float((got - want).norm() / (want.norm() + 1e-30)), float((got - want).abs().max()), float(want.abs().max())


def make_net(dev, name, B=2, S=64, seed=1, lock=None, m=None, perturb="scale", **kw):
    """tests/test_gpu_net.py make_net with a lock map: heads that produce non-trivial logits / detections, and the
    pass-through layers away from their initial batch-norm state.  ``perturb="scale"`` moves gamma and the moving variance
    (shift stays 0), ``"all"`` also beta and the moving mean.  The whole-step tests use "scale": the oracle normalises a
    locked layer's UNROUNDED conv output, a pass-through layer keeps its conv output in bf16 (like a trainable one), and
    with shift != 0 the two take different leaky branches where |z| is below the rounding of raw -- about 2^-10 of the
    elements per layer, each off by 0.9 g, i.e. 1-2 % relative l2 per pass-through layer, which is a property of the
    comparison and not of the step.  With shift = 0 the branch is the sign of raw * scale either way.  The per-layer test
    uses "all" and recomputes the coefficients from the variables in float64."""
    if name is not None:
        m, lock = lock_of(name)
    net = YOLONet(training=True, device=dev, image_size=S, batch_size=B, lock=lock, mask_stride=m, seed=seed, **kw)
    perturb_variables(net, seed, perturb)
    net.refresh_weights()
    return net


def _batch(B, S, seed):
    b = O.synthetic_batch(B, S, seed=seed)
    rng = np.random.RandomState(0)
    b["perm_det"] = np.stack([rng.permutation(cfg.MAX_DETECTION) for _ in range(B)]).astype(np.int32)
    b["perm_gt"] = np.stack([rng.permutation(cfg.MAX_BOX_PER_IMAGE) for _ in range(B)]).astype(np.int32)
    return b, [(b["perm_det"][i], b["perm_gt"][i]) for i in range(B)]


def oracle_params(net):
    return {k: v.detach().cpu().float().clone() for k, v in net.params.items()}


@pytest.mark.parametrize("name", list(MAPS))
def test_train_step_with_a_holed_map_matches_oracle(dev, name):
    """the recipe of tests/test_gpu_net.py::test_train_step_matches_oracle (same bounds), for a map with locked layers
    downstream of trainable ones"""
    B, S = 2, 64
    m, lock = lock_of(name)
    net = make_net(dev, name, B=B, S=S, seed=1)
    net.fuse_first_two = net.fuse_blocks = False      # (the per-layer comparison reads every layer's output)
    assert net.pass_through_layers() == pass_through(m, lock)
    b, perms = _batch(B, S, 11)
    p0 = oracle_params(net)
    net.set_batch(b)
    net.compute_losses(0.1)
    torch.cuda.synchronize()
    assert int(net.roi_count.sum()) > 0, "test needs at least one positive RoI"
    if m == 2:
        want_names = O.trainable_names(lock)
    else:       # (the oracle's list is the m = 1/2 net's: every variable of an unlocked layer but the moving statistics)
        want_names = [n for n in MR.variable_shapes(m, net.k) if not lock[int(n.split("convolutional")[1].split("/")[0])]
                      and not n.split("/")[-1].startswith("moving_")]
    tr = {n: p0[n].clone().requires_grad_(True) for n in want_names}
    pp = dict(p0)
    pp.update(tr)
    upd, taps = {}, {}
    force = {"act%d" % l.idx: l.act.float().cpu() for l in net.layers}
    if m == 2:
        parts, _, _, _ = O.total_loss(pp, b, lock, True, perms, upd, obj_thresh=0.1, quant=O.bf16_ste, taps=taps, force=force)
    else:
        parts, _, _, _ = MR.total_loss(pp, b, lock, m, net.k, perms, upd, obj_thresh=0.1, quant=O.bf16_ste, taps=taps,
                                       force=force)
    report = {"map": name, "forward": {}, "grad": {}}
    fails = []
    for l in net.layers:
        r, _, _ = rel_err(l.act, taps["act%d" % l.idx])
        report["forward"][l.idx] = r / 1.5e-2
        if not r < 1.5e-2:
            fails.append("layer %d forward (teacher-forced inputs): rel l2 err %.3g" % (l.idx, r))
    parts["total"].backward()
    total = float(net.total_loss().cpu())
    print("%s: total loss %.6f (oracle %.6f)" % (name, total, float(parts["total"])))
    assert abs(total - float(parts["total"])) < 1e-3 * abs(float(parts["total"]))
    net.backward()
    torch.cuda.synchronize()
    assert set(net.trainable_names()) == set(want_names)
    for nm, (o, cnt) in net.arena_slices.items():
        g = net.grad_arena[o:o + cnt].cpu()
        assert tr[nm].grad is not None, nm
        want_g = tr[nm].grad.flatten()
        if nm.endswith("weights") or nm.endswith("biases"):
            want_g = want_g - O.L2_WEIGHT * tr[nm].detach().flatten()   # (the kernel adds l2*w inside Adam)
        r, amax, wmax = rel_err(g, want_g)
        report["grad"][nm] = min(r / 0.03, amax / (1e-3 * max(wmax, 1e-6)))
        if not (r < 0.03 or amax < 1e-3 * max(wmax, 1e-6)):
            fails.append("grad %s: rel l2 err %.3g (max abs %.3g of %.3g)" % (nm, r, amax, wmax))
    report["worst_forward"] = max(report["forward"].values())
    report["worst_grad"] = max(report["grad"].values())
    print("%s: worst forward ratio %.3f, worst gradient ratio %.3f" % (name, report["worst_forward"], report["worst_grad"]))
    os.makedirs(REPORTS, exist_ok=True)
    with open(os.path.join(REPORTS, "lock_map_%s.json" % name), "w") as f:
        json.dump(report, f, indent=1)
    assert not fails, "%d checks failed:\n%s" % (len(fails), "\n".join(fails[:40]))
    # only trainable layers update their moving statistics
    locked = [l for l in net.layers if l.lock]
    assert {int(n.split("convolutional")[1].split("/")[0]) for n in upd} == {l.idx for l in net.layers if not l.lock and l.kind != "lin"}
    for nm, val in upd.items():
        r, amax, _ = rel_err(net.params[nm], val)
        assert r < 2e-2 or amax < 1e-4, "moving stat %s: rel err %.3g" % (nm, r)
    # a locked layer: variables and moving statistics bit-unchanged by the step
    before = {n: p0[n] for n in p0 if lock[int(n.split("convolutional")[1].split("/")[0])]}
    w_before = net.arena.clone()
    net.optimizer_step()
    torch.cuda.synchronize()
    assert locked and before
    for n, v in before.items():
        assert torch.equal(net.params[n].cpu(), v), "locked variable %s changed" % n
    assert not torch.equal(net.arena, w_before)


@pytest.mark.parametrize("name", ["hole_5_9", "frozen_heads"])
def test_pass_through_layers_one_by_one(dev, name):
    """teacher-forced, every pass-through layer: its output gradient from its consumers' dx as the kernels left them
    (tests/backward_ref.py, bounds C_G_*), its dx from its own grad / raw / scale / shift in closed form (the kernel test's
    bound)"""
    B, S = 2, 64
    net = make_net(dev, name, B=B, S=S, seed=2, perturb="all")
    b, _ = _batch(B, S, 12)
    net.set_batch(b)
    net.compute_losses(0.1)
    net.backward()
    torch.cuda.synchronize()
    assert int(net.roi_count.sum()) > 0
    by = net.by_idx
    wb = lambda mm: mm.w.to(torch.bfloat16)
    seen = 0
    with torch.no_grad():
        for l in net.layers:
            if not l.passthru or l.kind == "lin":
                continue
            seen += 1
            gw, gacc, gtwin = R.output_grad_ref(l, by, wb, lambda mm: mm.dx[..., :mm.cout], lambda mm: mm.grad)
            gb = R.grad_bound(gw, gacc, gtwin, C_G_REL, C_G_ACC, C_G_TWIN)
            worst = R.check_bounded(l.grad, gw, gb, "%s: layer %d output gradient" % (name, l.idx))
            assert float(gw.abs().max()) > 0, "layer %d: the reference gradient is all zero" % l.idx
            # the coefficients from the layer's own variables in float64, not the net's folded pair: a stale pair, another
            # layer's, or batch statistics in their place would show here
            scale = l.gamma.double() * torch.rsqrt(l.mv.double() + cfg.BN_EPSILON)
            shift = l.beta.double() - l.mm.double() * scale
            assert float((l.scale.double() - scale).abs().max()) <= 1e-6 * float(scale.abs().max())
            assert float(shift.abs().max()) > 0.05 and float((l.shift.double() - shift).abs().max()) <= 1e-6
            wdx = check_frozen_dx(l.dx.reshape(-1, l.cout), l.grad.reshape(-1, l.cout), l.raw.reshape(-1, l.cout), scale,
                                  shift, "%s: layer %d dx" % (name, l.idx))
            # ... and the forward used the same: act = leaky(raw * scale + shift) (+ the shortcut), one bf16 rounding
            z = l.raw.double().reshape(-1, l.cout) * scale + shift
            want_act = torch.maximum(z, ALPHA * z)
            if l.shortcut is not None:
                want_act = want_act + by[l.shortcut].act.double().reshape(-1, l.cout)
            err = (l.act.double().reshape(-1, l.cout) - want_act).abs()
            assert bool((err <= U_BF16 * want_act.abs() + 1e-6 * (z.abs() + 1)).all()), "layer %d forward" % l.idx
            print("%s layer %d: g %.3f dx %.3f of the bound" % (name, l.idx, worst, wdx))
    assert seen == len([i for i in pass_through(*lock_of(name)) if by[i].kind != "lin"])


@pytest.mark.parametrize("name", ["hole_5_9", "stage1_hole"])
def test_buffers_and_descriptors_follow_the_layer_roles(dev, name):
    """what _plan and _build_descs give a layer, at B = 1, 64^2 (the smallest net the kernels take): the kept conv output
    exactly where the layer keeps it, dx exactly for the linear layers and the layers the gradient crosses, and the output
    gradient, the flipped weights and the weight-gradient descriptor where the spelled-out conditions put them (which layer
    has a trainable layer at or above it comes from the test's own walk of the graph)"""
    m, lock = lock_of(name)
    net = YOLONet(training=True, device=dev, image_size=64, batch_size=1, lock=lock, mask_stride=m, seed=1)
    ins = inputs_of(m)

    def trainable_upto(i, seen=None):
        seen = set() if seen is None else seen
        if i == 0 or i in seen:
            return False
        seen.add(i)
        return (not lock[i]) or any(trainable_upto(j, seen) for j in ins[i])

    assert [l.idx for l in net.layers if l.passthru] == pass_through(m, lock)
    for l in net.layers:
        what = "%s, layer %d" % (name, l.idx)
        crossed = (not l.lock) or l.passthru
        assert l.on_path == crossed and l.keeps_raw == (crossed and l.kind != "lin"), what
        assert (l.raw is not None) == l.keeps_raw, what
        assert (l.dx is not None) == (l.kind == "lin" or l.on_path), what
        assert (l.grad is not None) == (trainable_upto(l.idx) and l.kind != "lin"), what
        srcs = [i for i in (l.src, l.src_up) if i is not None]
        assert (l.wdg is not None) == (crossed and l.idx > 1 and any(trainable_upto(i) for i in srcs)), what
        assert (l.wgrad_desc is not None) == (not l.lock and l.idx > 1), what
        assert bool(l.dgrad_descs) == (l.wdg is not None), what


# ------------------------------------------------------------------------------------------------ recorded forms
def _same_state(a, b):
    assert torch.equal(a.arena, b.arena) and torch.equal(a.adam_m, b.adam_m) and torch.equal(a.adam_v, b.adam_v)
    for nm in a.params:
        assert torch.equal(a.params[nm], b.params[nm]), nm


@pytest.mark.parametrize("name", ["hole_5_9", "frozen_heads", "stage1_hole"])
def test_recorded_and_overlapped_steps_equal_eager(dev, name):
    B, S = 2, 64
    batches = [O.synthetic_batch(B, S, seed=500 + t) for t in range(3)]
    nets = [make_net(dev, name, B=B, S=S, seed=4) for _ in range(3)]
    eager, rec, over = nets
    for n in nets:
        n.set_batch(batches[0])
    rec.build_program(det_thresh=0.1)
    over.build_program(det_thresh=0.1, overlap_tail=True)
    assert over._overlap
    losses = [[], [], []]
    for t in range(3):
        losses[0].append(float(eager.train_step(batches[t], det_thresh=0.1).cpu()))
        losses[1].append(float(rec.train_step(batches[t]).cpu()))
        if t == 1:
            over.train_step(batches[t], want_loss=False)        # (the tail stays open into the next call)
            assert over._tail_open
            losses[2].append(float(over.total_loss().cpu()))
        else:
            losses[2].append(float(over.train_step(batches[t]).cpu()))
    torch.cuda.synchronize()
    assert np.isfinite(losses[0]).sum() >= 2
    assert np.array_equal(np.asarray(losses[0]), np.asarray(losses[1]), equal_nan=True)
    assert np.array_equal(np.asarray(losses[1]), np.asarray(losses[2]), equal_nan=True)
    _same_state(eager, rec)
    _same_state(rec, over)
    assert eager.step_count == rec.step_count == over.step_count == 3


def test_pipelined_step_behind_a_holed_stage1_equals_plain_step(dev):
    """tests/test_gpu_net.py::test_pipelined_backbone_step_equals_plain_step with conv62-64 locked behind the pipelined
    prefix"""
    B, S = 2, 64
    batches = [O.synthetic_batch(B, S, seed=40 + t) for t in range(4)]
    plain = make_net(dev, "stage1_hole", B=B, S=S, seed=6)
    piped = make_net(dev, "stage1_hole", B=B, S=S, seed=6)
    assert piped._backbone_prefix() == 52
    plain.build_program(det_thresh=0.1)
    piped.build_program(det_thresh=0.1, pipeline_backbone=True)
    piped._set_inputs(batches[0]["images"], batches[0]["clip_window"])
    piped.prime_pipeline()
    lp, lq = [], []
    for t in range(3):
        plain.set_batch(batches[t])
        lp.append(float(plain.train_step(None).cpu()))
        mixed = dict(batches[t])
        mixed["images"] = batches[t + 1]["images"]        # labels of batch t, images of batch t+1
        piped.set_batch(mixed)
        lq.append(float(piped.train_step(None).cpu()))
    torch.cuda.synchronize()
    assert np.array_equal(np.asarray(lp), np.asarray(lq), equal_nan=True) and np.isfinite(lp).sum() >= 2
    _same_state(plain, piped)
    piped.check_cluster_sync()
    plain.check_cluster_sync()


def test_everything_up_to_the_heads_locked_records_and_steps(dev):
    """lock = {1..75}: the three detection heads are locked linear layers with nothing trainable upstream -- the loss kernels
    still write their dx -- and only the mask subnet trains"""
    net = make_net(dev, None, lock={i: True for i in range(1, 76)}, m=2, seed=3)
    assert net.pass_through_layers() == [] and net._backbone_prefix() == 75
    assert all(net.by_idx[i].dx is not None for i in (59, 67, 75, 82))
    b, _ = _batch(2, 64, 13)
    net.set_batch(b)
    net.build_program(det_thresh=0.1)
    w0 = net.arena.clone()
    loss = float(net.train_step(None).cpu())
    torch.cuda.synchronize()
    assert np.isfinite(loss) and not torch.equal(net.arena, w0)
    assert set(net.trainable_names()) == set(O.trainable_names({i: i <= 75 for i in range(1, 83)}))


# ------------------------------------------------------------------------------------------------ the two stages, unchanged
def _counts(prog):
    return {"%s/%d" % (what, lane): prog.count(what, lane) for what in ("launches", "records", "waits") for lane in range(4)}


@pytest.mark.parametrize("stage", [1, 2])
def test_reference_stages_keep_their_command_lists(dev, stage):
    """lock=None and lock={} are the stage's own map: the same packets per lane (launches, records, waits), bit-identical
    variables after two steps.  The counts are printed (and filed) so that they can be held against another commit's."""
    B, S = 2, 64
    b = O.synthetic_batch(B, S, seed=3)
    nets, counts = [], []
    for lock in (None, {}):
        net = YOLONet(training=True, device=dev, image_size=S, batch_size=B, stage=stage, seed=2, lock=lock)
        assert net.pass_through_layers() == [] and net.lock == O.default_lock(stage)
        net.set_batch(b)
        net.build_program(det_thresh=0.1, overlap_tail=True)
        counts.append(_counts(net._prog))
        nets.append(net)
    print("stage %d command list at B = 2, 64^2 (overlap_tail): %s" % (stage, json.dumps(counts[0], sort_keys=True)))
    os.makedirs(REPORTS, exist_ok=True)
    with open(os.path.join(REPORTS, "lock_map_stage%d_counts.json" % stage), "w") as f:
        json.dump(counts[0], f, indent=1, sort_keys=True)
    assert counts[0] == counts[1]
    for _ in range(2):
        for net in nets:
            net.train_step(None, want_loss=False)
    la, lb = float(nets[0].total_loss().cpu()), float(nets[1].total_loss().cpu())
    torch.cuda.synchronize()
    assert la == lb or (np.isnan(la) and np.isnan(lb))
    assert torch.equal(nets[0].arena, nets[1].arena) and torch.equal(nets[0].adam_v, nets[1].adam_v)

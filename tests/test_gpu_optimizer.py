"""The optimizer tail on the device, entry point by entry point, against the float64 references and the bounds of
tests/optimizer_ref.py (whose CPU tests hold the same inputs' f32 restatement to the same bounds):

  * adam_sweep on the capped grid (every thread makes two grid-stride iterations), at both slice alignments, with and
    without l2 partials, with the decay boundary inside a 16-byte vector; several slices that share one step counter and
    one partials buffer, finished once;
  * adam_finish / adam_finish_record: the double accumulation over more partials than the block has threads, the loss
    ring (slot, wrap, 64-bit step index, the reg_loss_in path);
  * l2_loss beyond its block cap, and against the sweep's own l2 term; adam_step_dev over three steps;
  * pack_all (one launch over a job table) bit for bit against the layout references and against pack_weights;
  * the network: after a step in every step mode the bf16 operands are the packed f32 masters, bit for bit, every
    arena element was swept exactly once with the right decay flag, and the job tables survive load_state_dict,
    autotune and repack.

Every output is judged from the device's own state before the step: the error measured is that of one step.
"""
import numpy as np
import pytest
import torch

import disyolo_oracle as O
import optimizer_ref as OR
from backward_ref import tuned_tables  # noqa: F401  (fixture: clears the tile table autotune fills)
from disyolo_amd import config as cfg
from disyolo_amd import lib as L
from test_gpu_net import make_net

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
PRE, POST = 4, 5                       # guard elements around a slice (PRE keeps the slice's offset modulo 16 bytes)
SENTINEL = {"w": -1234.5, "g": 4321.25, "m": -77.125, "v": 99.0625}


def bits(t: torch.Tensor) -> torch.Tensor:
    """the raw bits, so that NaNs and signed zeros compare"""
    t = t.detach().contiguous()
    return t.view({4: torch.int32, 2: torch.int16, 8: torch.int64}[t.element_size()]).cpu()


def same_bits(a, b) -> bool:
    return torch.equal(bits(a), bits(b))


class Slices:
    """w, g, m, v as equal-offset slices [PRE + off, PRE + off + n) of four 16-byte aligned buffers full of sentinels"""

    def __init__(self, dev, n, off, w, g, m, v):
        self.n, self.lo = n, PRE + off
        self.host = {}
        for name, a in zip("wgmv", (w, g, m, v)):
            h = torch.full((PRE + off + n + POST,), SENTINEL[name], dtype=torch.float32)
            h[self.lo:self.lo + n] = torch.from_numpy(np.array(a, np.float32))
            self.host[name] = h
        self.dev = {k: h.to(dev) for k, h in self.host.items()}
        assert all(t.data_ptr() % 16 == 0 for t in self.dev.values())

    def __getitem__(self, name):
        return self.dev[name][self.lo:self.lo + self.n]

    def args(self):
        return self["w"], self["g"], self["m"], self["v"]

    def restore(self):
        for k, h in self.host.items():
            self.dev[k].copy_(h)

    def fetch(self):
        """host copies of the whole buffers; guards and g must be what they were"""
        out = {k: t.cpu() for k, t in self.dev.items()}
        for k, t in out.items():
            assert same_bits(t[:self.lo], self.host[k][:self.lo]), "%s: guard in front of the slice overwritten" % k
            assert same_bits(t[self.lo + self.n:], self.host[k][self.lo + self.n:]), "%s: guard behind the slice overwritten" % k
        assert same_bits(out["g"], self.host["g"]), "the sweep wrote the gradient"
        return out

    def inner(self, fetched, name):
        return fetched[name][self.lo:self.lo + self.n].numpy()


def nan_parts(dev, nparts):
    """partials buffer of NaNs with one guard entry on each side; (whole buffer, the slice the kernel gets)"""
    buf = torch.full((nparts + 2,), float("nan"), dtype=torch.float32, device=dev)
    return buf, buf[1:1 + nparts]


def sweep(S, n, n_decay, lr, cnt, parts):
    L.adam_sweep(*S.args(), n, n_decay, lr, OR.B1, OR.B2, OR.EPS, OR.L2, cnt, OR.GRAD_SCALE, parts)


def check_parts(buf, nparts, sumsq, rel, what):
    """the guards still NaN, every entry written, their float64 sum within the per-thread bound of the float64 sum"""
    p = buf.cpu().numpy()
    assert np.isnan(p[0]) and np.isnan(p[-1]), "%s: partials written outside their range" % what
    inner = p[1:1 + nparts]
    assert np.isfinite(inner).all() and (inner >= 0).all(), "%s: %d partials not written" % (what, int(np.isnan(inner).sum()))
    got = float(inner.astype(np.float64).sum())
    print("%s: partials sum %.17g, float64 %.17g, rel err %.3g (bound %.3g)" % (what, got, sumsq, abs(got - sumsq) / sumsq, rel))
    assert abs(got - sumsq) <= rel * sumsq, "%s: l2 partials %.3g off relative (bound %.3g)" % (what, abs(got - sumsq) / sumsq, rel)
    return inner


# ------------------------------------------------------------------------------------------------ sweep: capped grid
INSIDE = 4 * (2048 * 256 + 1000) + 2       # + head: inside a 16-byte vector of the second grid-stride iteration


@pytest.mark.parametrize("t", [1, 7])
@pytest.mark.parametrize("decay", ["all", "none", "inside"])
@pytest.mark.parametrize("off", [0, 1])
def test_sweep_on_the_capped_grid(dev, off, decay, t):
    n = OR.CAP_N
    head = (4 - off) % 4                                           # leading scalars of the slice
    n_decay = {"all": n, "none": 0, "inside": INSIDE + head}[decay]
    assert L.adam_sweep_parts(n) == OR.sweep_blocks(n) == 2048 and n > 2048 * 1024 * 2 - 4
    if decay == "inside":
        assert (n_decay - head) % 4 == 2 and (n_decay - head) // 4 >= 2048 * 256
    w, g, m, v = OR.adam_inputs(n, 0)
    S = Slices(dev, n, off, w, g, m, v)
    assert S["w"].data_ptr() % 16 == 4 * off
    lr = torch.tensor([OR.LR], dtype=torch.float32, device=dev)
    cnt = torch.tensor([t - 1], dtype=torch.int64, device=dev)
    nparts = 0 if decay == "none" else L.adam_sweep_parts(n)
    pbuf, parts = nan_parts(dev, nparts) if nparts else (None, None)
    sweep(S, n, n_decay, lr, cnt, parts)
    torch.cuda.synchronize()
    assert int(cnt.cpu()) == t - 1, "a sweep must not touch the step counter"
    out = S.fetch()
    r = OR.adam_ref(w, g, m, v, t, n_decay)
    OR.assert_step_within_bounds(S.inner(out, "w"), S.inner(out, "m"), S.inner(out, "v"), r, "sweep")
    if nparts:
        check_parts(pbuf, nparts, OR.l2_sumsq(w, n_decay), OR.thread_sum_rel(n, nparts), "sweep")
    # again from the restored state: bit-identical
    S.restore()
    if nparts:
        first = pbuf.clone()
        pbuf.fill_(float("nan"))
    sweep(S, n, n_decay, lr, cnt, parts)
    torch.cuda.synchronize()
    again = S.fetch()
    for k in "wmv":
        assert same_bits(out[k], again[k]), "%s differs between two runs from the same state" % k
    if nparts:
        assert same_bits(first, pbuf), "l2 partials differ between two runs from the same state"


# ------------------------------------------------------------------------------------------------ several slices, one finish
def test_slices_share_one_counter_and_one_partials_buffer(dev):
    lens = OR.SLICES
    offs = [sum(lens[:i]) for i in range(len(lens))]
    total = sum(lens)
    assert [o % 4 for o in offs] == [0, 0, 3]
    ins = [OR.adam_inputs(c, 10 + i) for i, c in enumerate(lens)]
    w, g, m, v = (np.concatenate([x[j] for x in ins]) for j in range(4))
    S = Slices(dev, total, 0, w, g, m, v)
    lr = torch.tensor([OR.LR], dtype=torch.float32, device=dev)
    cnt = torch.tensor([1], dtype=torch.int64, device=dev)
    reg = torch.full((3,), -5.0, dtype=torch.float32, device=dev)
    np_of = [L.adam_sweep_parts(c) for c in lens]
    assert np_of == [OR.sweep_blocks(c) for c in lens] == [5, 1075, 1]
    nparts = sum(np_of)

    def run():
        pbuf, parts = nan_parts(dev, nparts)
        po = 0
        for o, c, k in zip(offs, lens, np_of):
            L.adam_sweep(*(a[o:o + c] for a in S.args()), c, c, lr, OR.B1, OR.B2, OR.EPS, OR.L2, cnt, OR.GRAD_SCALE,
                         parts[po:po + k])
            po += k
        L.adam_finish(cnt, parts, nparts, OR.L2, reg[1:2])
        torch.cuda.synchronize()
        return pbuf, S.fetch()

    pbuf, out = run()
    assert int(cnt.cpu()) == 2, "the finish advances the counter once for all slices"
    # every slice ran at t = 2: the next bias correction moves w by far more than the bound (tests/test_optimizer_ref.py)
    p = pbuf.cpu().numpy()
    assert np.isnan(p[0]) and np.isnan(p[-1]) and np.isfinite(p[1:-1]).all()
    budget, po = 0.0, 1
    for i, (o, c, k) in enumerate(zip(offs, lens, np_of)):
        r = OR.adam_ref(w[o:o + c], g[o:o + c], m[o:o + c], v[o:o + c], 2, c)
        OR.assert_step_within_bounds(*(S.inner(out, x)[o:o + c] for x in "wmv"), r, "slice %d" % i)
        ss, rel = OR.l2_sumsq(w[o:o + c], c), OR.thread_sum_rel(c, k)
        got = float(p[po:po + k].astype(np.float64).sum())
        assert abs(got - ss) <= rel * ss, "slice %d: l2 partials %.3g off relative (bound %.3g)" % (i, abs(got - ss) / ss, rel)
        budget += rel * ss
        po += k
    regv = reg.cpu().numpy()
    assert regv[0] == -5.0 and regv[2] == -5.0
    fin = OR.finish_ref(p[1:-1])
    assert abs(float(regv[1]) - fin) <= OR.FINISH_REL * fin
    want = OR.l2_term(w, total)
    assert abs(float(regv[1]) - want) <= 0.5 * OR.L2 * budget + OR.FINISH_REL * want
    # again from the restored state
    S.restore()
    cnt.fill_(1)
    pbuf2, again = run()
    assert same_bits(pbuf, pbuf2) and all(same_bits(out[k], again[k]) for k in "wmv")
    assert same_bits(reg, torch.from_numpy(regv))


# ------------------------------------------------------------------------------------------------ finish
@pytest.mark.parametrize("nparts", OR.FINISH_NPARTS)
def test_finish_adds_the_partials_in_double(dev, nparts):
    p = OR.finish_parts(nparts)
    pbuf, parts = nan_parts(dev, nparts)
    parts.copy_(torch.from_numpy(np.array(p)))
    before = pbuf.clone()
    cnt = torch.tensor([41], dtype=torch.int64, device=dev)
    reg = torch.full((3,), -5.0, dtype=torch.float32, device=dev)
    L.adam_finish(cnt, parts, nparts, OR.L2, reg[1:2])
    torch.cuda.synchronize()
    got = reg.cpu().numpy()
    want = OR.finish_ref(p)
    print("nparts %d: reg %.9g, float64 %.17g, rel err %.3g" % (nparts, got[1], want, abs(float(got[1]) - want) / want))
    assert got[0] == -5.0 and got[2] == -5.0 and int(cnt.cpu()) == 42
    assert abs(float(got[1]) - want) <= OR.FINISH_REL * want
    assert same_bits(pbuf, before), "the finish wrote the partials"
    L.adam_finish(cnt, parts, nparts, OR.L2, reg[1:2])
    torch.cuda.synchronize()
    assert same_bits(reg, torch.from_numpy(got)) and int(cnt.cpu()) == 43


def test_finish_without_partials_still_advances_the_counter(dev):
    cnt = torch.tensor([6, -9], dtype=torch.int64, device=dev)
    L.adam_finish(cnt, None, 0, OR.L2, None)
    torch.cuda.synchronize()
    assert cnt.cpu().tolist() == [7, -9]


# ------------------------------------------------------------------------------------------------ finish + loss ring
@pytest.mark.parametrize("mode,start", [("parts", 3), ("reg_in", 3), ("none", 3), ("parts", 2 ** 33 + 1)])
def test_finish_record_files_the_loss_in_the_ring(dev, mode, start):
    ring_len, f = 5, np.float32
    rbuf = torch.full((ring_len + 2,), -3.0, dtype=torch.float32, device=dev)
    ring = rbuf[1:1 + ring_len]
    want_ring = np.full(ring_len + 2, -3.0, np.float32)
    cnt = torch.tensor([start], dtype=torch.int64, device=dev)
    rng = np.random.RandomState(9)
    nparts = 300
    losses8 = torch.zeros(8, dtype=torch.float32, device=dev)
    mask_loss = torch.zeros(1, dtype=torch.float32, device=dev)
    reg = torch.full((1,), -5.0, dtype=torch.float32, device=dev)
    reg_in = torch.zeros(1, dtype=torch.float32, device=dev)
    parts = torch.zeros(nparts, dtype=torch.float32, device=dev)
    for i in range(12):
        t = start + i                                              # the counter before its increment
        l8 = rng.uniform(0.5, 40.0, 8).astype(f)
        ml = rng.uniform(0.01, 3.0, 1).astype(f)
        losses8.copy_(torch.from_numpy(l8))
        mask_loss.copy_(torch.from_numpy(ml))
        if mode == "parts":
            parts.copy_(torch.from_numpy(rng.uniform(0.0, 50.0, nparts).astype(f)))
            L.adam_finish(cnt, parts, nparts, OR.L2, reg, record=(losses8, mask_loss, None, ring))
            torch.cuda.synchronize()
            regv = reg.cpu().numpy()[0]                            # (its value has a test of its own above)
            fin = OR.finish_ref(parts.cpu().numpy())
            assert abs(float(regv) - fin) <= OR.FINISH_REL * fin
        elif mode == "reg_in":
            regv = f(rng.uniform(0.1, 2.0))
            reg_in.fill_(float(regv))
            L.adam_finish(cnt, None, 0, OR.L2, None, record=(losses8, mask_loss, reg_in, ring))
        else:
            regv = f(0)
            L.adam_finish(cnt, None, 0, OR.L2, None, record=(losses8, mask_loss, None, ring))
        torch.cuda.synchronize()
        want_ring[1 + t % ring_len] = f(f(l8[7] + ml[0]) + regv)
        assert int(cnt.cpu()) == t + 1
        assert same_bits(rbuf, torch.from_numpy(want_ring)), "finish %d (step index %d): ring %s, expected %s" % (
            i, t, rbuf.cpu().numpy(), want_ring)
    if mode != "parts":
        assert float(reg.cpu()) == -5.0                            # no partials: reg_loss_out is not written


# ------------------------------------------------------------------------------------------------ l2_loss
@pytest.mark.parametrize("n", OR.L2_NS)
def test_l2_loss_and_the_sweeps_l2_term(dev, n):
    w, g, m, v = OR.adam_inputs(n, 20)
    S = Slices(dev, n, 0, w, g, m, v)
    ws = L.Workspace(dev)
    out = torch.full((3,), -5.0, dtype=torch.float32, device=dev)
    L.l2_loss(S["w"], n, OR.L2, out[1:2], ws)
    torch.cuda.synchronize()
    S.fetch()
    got = out.cpu().numpy()
    want = OR.l2_term(w, n)
    rel = OR.thread_sum_rel(n, OR.l2_blocks(n)) + OR.FINISH_REL    # the per-thread sums, then the double finish
    print("n %d: l2_loss %.9g, float64 %.17g, rel err %.3g (bound %.3g)" % (n, got[1], want, abs(float(got[1]) - want) / want, rel))
    assert got[0] == -5.0 and got[2] == -5.0
    assert abs(float(got[1]) - want) <= rel * want
    # the l2 term a sweep + finish over the same weights produces
    lr = torch.tensor([OR.LR], dtype=torch.float32, device=dev)
    cnt = torch.zeros(1, dtype=torch.int64, device=dev)
    nparts = L.adam_sweep_parts(n)
    pbuf, parts = nan_parts(dev, nparts)
    reg = torch.zeros(1, dtype=torch.float32, device=dev)
    sweep(S, n, n, lr, cnt, parts)
    L.adam_finish(cnt, parts, nparts, OR.L2, reg)
    torch.cuda.synchronize()
    rel2 = OR.thread_sum_rel(n, nparts) + OR.FINISH_REL
    assert abs(float(reg.cpu()) - want) <= rel2 * want
    assert abs(float(reg.cpu()) - float(got[1])) <= (rel + rel2) * want


# ------------------------------------------------------------------------------------------------ adam_step_dev
def test_adam_step_dev_three_steps(dev):
    n, n_decay = OR.STEP_DEV_N, OR.STEP_DEV_DECAY
    w, g, m, v = OR.step_dev_inputs()
    S = Slices(dev, n, 0, w, g, m, v)
    cnt = torch.zeros(1, dtype=torch.int64, device=dev)
    for t in (1, 2, 3):
        before = {k: S.inner(S.fetch(), k).copy() for k in "wmv"}
        L.adam_step_dev(*S.args(), n, n_decay, OR.LR, OR.B1, OR.B2, OR.EPS, OR.L2, cnt, OR.GRAD_SCALE)
        torch.cuda.synchronize()
        assert int(cnt.cpu()) == t
        out = S.fetch()
        r = OR.adam_ref(before["w"], g, before["m"], before["v"], t, n_decay)
        OR.assert_step_within_bounds(S.inner(out, "w"), S.inner(out, "m"), S.inner(out, "v"), r, "step %d" % t)


# ------------------------------------------------------------------------------------------------ pack table
GAP = 7       # bf16 elements between two outputs (odd: the outputs start at every 2-byte alignment)


def run_pack_table(dev, order):
    """one launch over the jobs PACK_JOBS[i], i in order; every output a slice of one NaN-filled bf16 buffer"""
    jobs = [OR.PACK_JOBS[i] for i in order]
    sizes = []
    for k, cin, cout, pad, dg in jobs:
        sizes.append((cout * k * k * cin, cin * k * k * pad if dg else 0))
    total = GAP + sum(a + GAP + (b + GAP if b else 0) for a, b in sizes)
    buf = torch.full((total,), float("nan"), dtype=BF16, device=dev)
    ws = [OR.pack_weights_for(i).to(dev) for i in order]
    table, spans, pos = [], [], GAP
    for (k, cin, cout, pad, dg), (a, b), w in zip(jobs, sizes, ws):
        wf = buf[pos:pos + a]
        pos += a + GAP
        wd = buf[pos:pos + b] if b else None
        pos += b + GAP if b else 0
        table.append((w, wf, wd, k, cin, cout, pad))
        spans.append((wf, wd))
    assert pos == total
    T = L.PackTable(table, dev)
    assert T.blocks == OR.pack_blocks(jobs)
    before = bits(buf)
    T.run()
    torch.cuda.synchronize()
    written = torch.zeros(total, dtype=torch.bool)
    for i, (k, cin, cout, pad, dg), (wf, wd), w in zip(order, jobs, spans, ws):
        what = "job %d (k %d, %d -> %d, pad %d)" % (i, k, cin, cout, pad)
        w_host = OR.pack_weights_for(i)
        assert same_bits(wf, OR.fwd_layout(w_host).to(BF16).flatten()), what + ": forward operand"
        wf2 = torch.full((cout, k * k * cin), float("nan"), dtype=BF16, device=dev)
        wd2 = torch.full((cin, k * k * pad), float("nan"), dtype=BF16, device=dev) if dg else None
        L.pack_weights(w, wf2, wd2, k, cin, cout, pad)
        torch.cuda.synchronize()
        assert same_bits(wf, wf2.flatten()), what + ": forward operand differs from pack_weights'"
        if dg:
            assert same_bits(wd, OR.dgrad_layout(w_host, pad).to(BF16).flatten()), what + ": data-gradient operand"
            assert same_bits(wd, wd2.flatten()), what + ": data-gradient operand differs from pack_weights'"
            assert (bits(wd).view(cin, k * k, pad)[..., cout:] == 0).all(), what + ": pad channels must be +0"
        for s in (wf, wd):
            if s is not None:
                o = (s.data_ptr() - buf.data_ptr()) // 2
                written[o:o + s.numel()] = True
    assert int((~written).sum()) == GAP * (1 + sum(1 + (1 if b else 0) for _, b in sizes))
    assert torch.equal(bits(buf)[~written], before[~written]), "pack_all wrote between its outputs"
    assert not torch.isnan(buf.float().cpu()[written]).any(), "pack_all left an output element unwritten"


@pytest.mark.parametrize("order", ["table", "reversed"] + ["only%d" % i for i in range(len(OR.PACK_JOBS))])
def test_pack_table_matches_layouts_and_pack_weights(dev, order):
    n = len(OR.PACK_JOBS)
    idx = {"table": list(range(n)), "reversed": list(range(n))[::-1]}.get(order) or [int(order[4:])]
    run_pack_table(dev, idx)


# ------------------------------------------------------------------------------------------------ the network
def assert_operands_fresh(net):
    """wp / wdg of every layer that owns them are its f32 master packed now, bit for bit (locked layers too: they never move)"""
    n = 0
    for l in net.layers:
        if getattr(l, "wp", None) is None:
            continue
        wp = torch.full_like(l.wp, float("nan"))
        wdg = torch.full_like(l.wdg, float("nan")) if l.wdg is not None else None
        L.pack_weights(l.w, wp, wdg, l.k, l.cin, l.cout, l.cout_pad)
        torch.cuda.synchronize()
        assert torch.equal(l.wp.view(torch.int16), wp.view(torch.int16)), "conv%d: wp is not its packed f32 master" % l.idx
        if wdg is not None:
            assert torch.equal(l.wdg.view(torch.int16), wdg.view(torch.int16)), "conv%d: wdg is not its packed f32 master" % l.idx
            n += 1
    assert n > 0


def assert_swept_once(net, w_before, grad_scale=1.0):
    """after the first step from zero moments: m = (1-b1)*g', v = (1-b2)*g'^2 with g' = g*grad_scale + l2*w on [0, n_decay)
    and g*grad_scale beyond, within the m' and v' bounds of tests/optimizer_ref.py (written out for zero moments, in
    float64 on the device); a slice swept twice has 0.19*g', one never swept 0"""
    assert net.step_count == 1
    l2 = OR.f32v(net.l2)
    b1, b2 = OR.f32v(cfg.ADAM_BETA1), OR.f32v(cfg.ADAM_BETA2)
    g = net.grad_arena.double() * float(grad_scale)
    dec = torch.zeros_like(g)
    dec[:net.n_decay] = l2 * w_before[:net.n_decay].double()
    gp = g + dec
    c = (g.abs() + dec.abs() - gp.abs()).clamp_(min=0)
    want_m = (1.0 - b1) * gp
    want_v = (1.0 - b2) * gp * gp
    bm = 2.0 ** -21 * want_m.abs() + (1.0 - b1) * OR.U * c
    bv = 2.0 ** -21 * want_v + (1.0 - b2) * (2.0 * OR.U * gp.abs() * c + OR.U ** 2 * (2.0 * gp.abs() + c) ** 2 * (c > 0))
    assert float(gp.abs().max()) > 0 and int((gp[net.n_decay:] != 0).sum()) > 0
    for name, got, want, bound in (("adam_m", net.adam_m, want_m, bm), ("adam_v", net.adam_v, want_v, bv)):
        bad = (got.double() - want).abs() > bound
        nbad = int(bad.sum())
        if nbad:
            i = int(bad.nonzero()[0])
            ci = [k for k, ch in enumerate(net.opt_chunks) if ch["off"] <= i < ch["off"] + ch["cnt"]]
            raise AssertionError("%s: %d elements outside the bound, first at %d (slice %s; n_decay %d): got %r, float64 %r" % (
                name, nbad, i, ci or "gamma/beta", net.n_decay, float(got[i]), float(want[i])))


def table_pointers(net):
    return [(t.data_ptr() if t is not None else 0) for ch in net.opt_chunks if ch["pack"] is not None
            for job in ch["pack"].keep for t in job[:3]]


def layer_pointers(net):
    return [(t.data_ptr() if t is not None else 0) for l in net.layers if getattr(l, "wp", None) is not None and not l.lock
            for t in (l.w, l.wp, l.wdg)]


def batch(seed):
    return O.synthetic_batch(2, 64, seed=seed)


MODES = [(s, m) for s in (1, 2) for m in ("eager", "program", "graph", "overlap")] + [(1, "pipeline")]


@pytest.mark.parametrize("stage,mode", MODES)
def test_a_step_leaves_the_operands_fresh_and_sweeps_every_element_once(dev, stage, mode):
    net = make_net(dev, True, stage, B=2, S=64, seed=8)
    batches = [batch(60 + t) for t in range(4)]
    net.set_batch(batches[0])
    if mode == "program":
        net.build_program(det_thresh=0.1)
    elif mode == "graph":
        net.build_program(det_thresh=0.1, graph=True)
    elif mode == "overlap":
        net.build_program(det_thresh=0.1, overlap_tail=True)
    elif mode == "pipeline":
        net.build_program(det_thresh=0.1, pipeline_backbone=True)
        net._set_inputs(batches[0]["images"], batches[0]["clip_window"])
        net.prime_pipeline()

    def step(t):
        b = dict(batches[t])
        if mode == "pipeline":
            b["images"] = batches[t + 1]["images"]                 # labels of batch t, images of batch t + 1
        net.set_batch(b)
        if mode == "eager":
            net.train_step(None, det_thresh=0.1, want_loss=False)
        else:
            net.train_step(None, want_loss=False)                  # (overlap: the tail stays open, sync_lanes joins it)

    w_before = net.arena.clone()
    assert float(net.adam_m.abs().max()) == 0.0 and float(net.adam_v.abs().max()) == 0.0
    step(0)
    net.sync_lanes()
    torch.cuda.synchronize()
    assert len(net.opt_chunks) >= 2
    assert_operands_fresh(net)
    assert_swept_once(net, w_before, 1.0)
    assert not torch.equal(net.arena, w_before)
    step(1)
    step(2)
    net.sync_lanes()
    torch.cuda.synchronize()
    assert net.step_count == 3
    assert_operands_fresh(net)


@pytest.mark.parametrize("change", ["load_state_dict", "autotune", "repack"])
def test_job_tables_survive_state_changes(dev, change, tuned_tables):  # noqa: F811
    """the tables hold raw pointers: nothing may move l.w / l.wp / l.wdg, and one more recorded step after the change
    leaves the operands fresh"""
    net = make_net(dev, True, 1, B=2, S=64, seed=8)
    net.set_batch(batch(70))
    if change == "autotune":
        net.train_step(None, det_thresh=0.1, want_loss=False)      # eager: plans the slices and their tables
    else:
        net.build_program(det_thresh=0.1)
        net.train_step(None, want_loss=False)
    net.sync_lanes()
    assert len(net.opt_chunks) >= 2
    tp, lp = table_pointers(net), layer_pointers(net)
    assert len(tp) > 0 and sorted(tp) == sorted(lp)
    if change == "load_state_dict":
        other = make_net(dev, True, 1, B=2, S=64, seed=9)
        assert not torch.equal(other.arena, net.arena)
        net.load_state_dict(other.state_dict())
        assert torch.equal(other.arena[:net.n_decay], net.arena[:net.n_decay])
    elif change == "autotune":
        net.autotune(reps=1, candidates=(3,), det_thresh=0.1)
        net.build_program(det_thresh=0.1)
    else:
        with torch.no_grad():
            net.arena[:net.n_decay].mul_(1.25)
        net.repack()
    torch.cuda.synchronize()
    assert table_pointers(net) == tp and layer_pointers(net) == lp
    assert_operands_fresh(net)
    before = net.arena.clone()
    net.train_step(None, want_loss=False)
    net.sync_lanes()
    torch.cuda.synchronize()
    assert table_pointers(net) == tp and layer_pointers(net) == lp
    assert not torch.equal(net.arena[:net.n_decay], before[:net.n_decay])
    assert_operands_fresh(net)

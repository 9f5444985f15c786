"""Are the hand-placed event edges of the recorded programs SUFFICIENT?

Every other test of the lanes replays a program at the timing the hardware happens to give; a missing edge whose producer
usually wins the race passes them all.  Here a recorded program is replayed one command at a time, in an order that the
test chooses among those the edges allow (tests/lane_order.py), with the device synchronised after every command: the
host order is the execution order, nothing depends on how long anything takes, and no extra stream, priority or delay
kernel is involved.  If the edges are sufficient every such order gives the eager step's bits.  For two lanes the two
extreme orders ("main lane as early as legal", "side lane as early as legal") cover every missing producer -> consumer
or reader -> overwriter edge (tests/test_lane_order.py proves that against brute force); three-lane programs run all six
priority orders, and every program four seeded random ones.

A failure names the policy and, by a bisect over hybrid orders (the first k nodes of the failing order, the rest as
recorded -- each legal, each a deterministic replay), the command whose early run changes the result."""
import math

import pytest
import torch

import disyolo_oracle as O
import lane_order as LO
from disyolo_amd import lib as L
from disyolo_amd.net import YOLONet
from lock_maps import lock_of

pytestmark = pytest.mark.gpu

B, S, R = 2, 64, 3
THRESH = 0.1


def policies_of(graph):
    pols = LO.all_policies(graph)
    assert len(pols) == 1 + math.factorial(len(graph.lanes)) + 4
    return pols


def check_schedule(order, graph, policy):
    """conditions on the test, not measurements: the order is legal and issues every command exactly once"""
    assert LO.is_legal(order, graph), LO.policy_name(policy)
    issued = sorted((graph.nodes[n].replay, graph.nodes[n].index) for n in order if LO.issues_command(graph.nodes[n]))
    assert issued == [(r, i) for r, rep in enumerate(graph.replays) for i in range(len(rep.cmds))], LO.policy_name(policy)


def check_extremes_differ(graph, recorded_is_side_first=False):
    """the two extreme priority orders must each swap at least one pair of launches on different lanes against the recorded
    order: a program where they do not would hide everything.  ``recorded_is_side_first``: a list that records every
    side-lane launch right behind the edge that releases it IS the "side lane as early as legal" order -- that extreme
    cannot differ from it and is run as ``recorded``; the other extreme must swap pairs all the same."""
    lanes = sorted(graph.lanes)
    assert len(lanes) >= 2
    inv = [LO.launch_inversions(LO.schedule(graph, LO.priority(perm)), graph) for perm in (tuple(lanes), tuple(reversed(lanes)))]
    assert inv[0] > 0, "priority%r runs every pair of launches as recorded" % (tuple(lanes),)
    if recorded_is_side_first:
        launches = lambda o: [n for n in o if graph.nodes[n].what == "launch"]
        assert inv[1] == 0 and launches(LO.schedule(graph, LO.priority(tuple(reversed(lanes))))) == launches(LO.schedule(graph, LO.recorded()))
    else:
        assert inv[1] > 0, "priority%r runs every pair of launches as recorded" % (tuple(reversed(lanes)),)
    assert LO.launch_inversions(LO.schedule(graph, LO.recorded()), graph) == 0


def bits(t):
    t = t.detach().contiguous()
    if t.dtype == torch.float32:
        return t.view(torch.int32)
    if t.dtype == torch.bfloat16:
        return t.view(torch.int16)
    return t


def first_difference(got, want):
    """name of the first tensor of ``got`` whose bits differ from ``want``'s (NaN equals NaN: bit patterns), or None"""
    assert list(got) == list(want)
    for name in want:
        if not torch.equal(bits(got[name]), bits(want[name])):
            return name
    return None


# ---------------------------------------------------------------------------------------------------- a. the toy
def test_the_harness_sees_a_wrong_order(dev):
    """lane 1: B = A;  sync(1, 0);  lane 0: C += B.  Replayed by the true model every policy gives C0 + A; with the sync
    taken out of the MODEL only (the recorded list keeps it), the main lane first runs the consumer in front of its
    producer and C stays C0 (B is 0 then) -- the harness would see a missing edge of this kind.  The only deliberately
    mis-ordered run of the suite: three dense, initialised vectors and nothing else."""
    n = 4096
    g = torch.Generator().manual_seed(11)
    A = torch.randn(n, generator=g).to(dev, torch.bfloat16)
    C0 = torch.randn(n, generator=g).to(dev, torch.bfloat16)
    Bv = torch.zeros(n, dtype=torch.bfloat16, device=dev)
    C = C0.clone()
    want = (C0.float() + A.float()).to(torch.bfloat16)
    assert not torch.equal(want, C0)
    prog = L.CmdList()
    with prog:
        L.set_lane(1)
        L.add_bf16(A, Bv, False)
        L.lane_sync(1, 0)
        L.set_lane(0)
        L.add_bf16(Bv, C, True)
    cmds = prog.describe()
    assert cmds == [(LO.LAUNCH, 1, 0, 0), (LO.SYNC, 0, 1, 0), (LO.LAUNCH, 0, 0, 0)]

    def run(graph, policy, full_prog_index=None):
        Bv.zero_()
        C.copy_(C0)
        torch.cuda.synchronize()
        order = LO.schedule(graph, policy)
        assert LO.is_legal(order, graph)
        # (the mis-modelled list has one command less: its launches keep the RECORDED list's indices)
        for node in (graph.nodes[i] for i in order):
            if LO.issues_command(node):
                i = node.index if full_prog_index is None else full_prog_index[node.index]
                prog.run(i, i + 1, fork=False, join=False)
            torch.cuda.synchronize()
        return C.clone()

    true = LO.Graph([LO.Replay(cmds, True, True)])
    for pol in policies_of(true):
        # (the sync leaves one order of the two launches: no policy can swap them)
        assert LO.launch_inversions(LO.schedule(true, pol), true) == 0
        assert torch.equal(bits(run(true, pol)), bits(want)), LO.policy_name(pol)
    # the same replay with the edge taken out of the model: nothing orders the two launches any more
    loose = LO.Graph([LO.Replay([cmds[0], cmds[2]], True, True)])
    got = run(loose, LO.priority((0, 1)), full_prog_index=[0, 2])
    assert torch.equal(bits(got), bits(C0)), "the consumer ran in front of its producer and the harness did not notice"
    assert torch.equal(bits(run(loose, LO.priority((1, 0)), full_prog_index=[0, 2])), bits(want))
    assert torch.equal(bits(run(true, LO.recorded())), bits(want))


def test_describe_round_trip_with_all_six_kinds(dev):
    got = LO.describe_round_trip(all_kinds=True)
    assert sorted({d[0] for d in got}) == [0, 1, 2, 3, 4, 5]


# ------------------------------------------------------------------------------- b. recorded steps under every policy
def train_net(dev, stage, seed, lock_map=None):
    if lock_map is not None:
        m, lock = lock_of(lock_map)
        net = YOLONet(training=True, device=dev, image_size=S, batch_size=B, lock=lock, mask_stride=m, seed=seed)
    else:
        net = YOLONet(training=True, device=dev, image_size=S, batch_size=B, stage=stage, seed=seed)
    net.shuffle_seed = 5
    return net


def training_state(net):
    """what a step leaves behind: variables, Adam moments, step counter, moving statistics, the loss, state_dict()"""
    torch.cuda.synchronize()
    st = {"arena": net.arena, "adam_m": net.adam_m, "adam_v": net.adam_v, "step": net.step_dev}
    for l in net.layers:
        if l.kind != "lin":
            st["mm%d" % l.idx], st["mv%d" % l.idx] = l.mm, l.mv
    st["total_loss"] = net.total_loss().reshape(1)
    for k, v in net.state_dict().items():
        st["state_dict/" + k] = v
    return {k: v.detach().clone() for k, v in st.items()}


def saved_tensors(net):
    # what build_program(graph=True) saves and restores around its warm-up replay
    return [net.arena, net.adam_m, net.adam_v, net.step_dev] + [t for l in net.layers if l.kind != "lin" for t in (l.mm, l.mv)]


class Scheduled:
    """a net with a recorded program, driven by lane_order.execute only -- never by train_step / run_program.  Mirrors
    what YOLONet._run_program does for the list executor without data parallelism and without a graph: replay r runs
    ``_progs[parity]`` and flips the parity (the pipelined step), forks, and joins unless the tail is overlapped."""

    def __init__(self, net, batches, per_replay, host_joins=False, reset=None):
        assert net._graph is None and net.dp is None and not net.pair
        self.net, self.batches, self.per_replay, self.reset = net, batches, per_replay, reset
        self.saved = [t.clone() for t in saved_tensors(net)]
        if net._progs is not None:
            self.progs = [net._progs[(net._parity + r) % 2][0] for r in range(R)]
        else:
            self.progs = [net._prog] * R
        self.hosts = [(lambda r=r: net.set_batch(batches[r])) if per_replay else None for r in range(R)]
        self.graph = LO.Graph([LO.Replay(self.progs[r].describe(), True, not net._overlap, self.hosts[r], host_joins)
                               for r in range(R)])

    def restore(self):
        net = self.net
        torch.cuda.synchronize()
        for t, v in zip(saved_tensors(net), self.saved):
            t.copy_(v)
        net.refresh_weights()
        net.set_batch(self.batches[0])
        if self.reset is not None:
            self.reset()
        torch.cuda.synchronize()

    def run(self, order):
        net = self.net
        self.restore()
        parity = net._parity if net._progs is not None else None
        issued = LO.execute(order, self.graph, self.progs, self.hosts)
        assert set(issued.values()) == {1} and len(issued) == sum(len(rep.cmds) for rep in self.graph.replays)
        if parity is not None:
            net._parity = (parity + R) % 2
            net._prog, net._prog_marks, net._bwd_end = net._progs[(parity + R - 1) % 2]
        assert not net._tail_open           # (the executor ends with a device synchronise: nothing is left open)
        return training_state(net)

    def locate(self, order, want):
        """the first node of ``order`` whose run in that place changes the result: the smallest k for which the first k
        nodes of ``order`` followed by the rest in recorded order differ from ``want``"""
        lo, hi = 0, len(order)              # hybrid(lo) agrees (it is the recorded order), hybrid(hi) differs
        while hi - lo > 1:
            mid = (lo + hi) // 2
            o = LO.hybrid(order, mid, self.graph)
            assert LO.is_legal(o, self.graph)
            if first_difference(self.run(o), want) is None:
                lo = mid
            else:
                hi = mid
        return self.graph.nodes[order[hi - 1]]

    def check_every_policy(self, want, note=""):
        graph = self.graph
        check_extremes_differ(graph)
        for pol in policies_of(graph):
            order = LO.schedule(graph, pol)
            check_schedule(order, graph, pol)
            got = self.run(order)
            diff = first_difference(got, want)
            print("%-20s %5d nodes, %6d swapped launch pairs, %5d across replays: %s"
                  % (LO.policy_name(pol), len(order), LO.launch_inversions(order, graph), LO.cross_replay_inversions(order, graph),
                     "same bits" if diff is None else "DIFFERS in " + diff))
            if diff is None:
                continue
            name = LO.policy_name(pol)
            if pol == LO.recorded():
                pytest.fail("the recorded order itself differs from the eager steps in %s: not an ordering matter%s" % (diff, note))
            node = self.locate(order, want)
            pytest.fail("policy %s: %s differs from the eager steps.  First command whose run in this order changes the result: "
                        "replay %d, list index %s, lane %d (%s, kind %s)%s"
                        % (name, diff, node.replay, node.index, node.lane, node.what, node.kind, note))


def eager_reference(dev, make, batches, per_replay):
    ref = make()
    ref.set_batch(batches[0])
    for r in range(R):
        ref.train_step(batches[r] if per_replay else None, det_thresh=THRESH, want_loss=False)
    st = training_state(ref)
    assert int(st["step"].item()) == R
    return st


def overlap_run_ahead(graph):
    """replays without a join in between: under "main lane first" the next replay's head runs in front of the previous
    replay's side-lane tail wherever the slots allow.  Number of (lane-0 launch of replay r + 1, lane-1 launch of replay r)
    pairs scheduled in that order."""
    return LO.cross_replay_inversions(LO.schedule(graph, LO.priority(tuple(sorted(graph.lanes)))), graph)


@pytest.mark.parametrize("stage", [1, 2])
def test_joined_step_under_every_policy(dev, stage):
    """cases 1 and 2: the two-lane step of build_program(), resident batch, three replays"""
    batches = [O.synthetic_batch(B, S, seed=700)]
    make = lambda: train_net(dev, stage, 21)
    want = eager_reference(dev, make, batches, False)
    net = make()
    net.set_batch(batches[0])
    net.build_program(det_thresh=THRESH)
    sch = Scheduled(net, batches, False)
    assert sorted(sch.graph.lanes) == [0, 1]
    assert overlap_run_ahead(sch.graph) == 0            # (joined: no replay runs into the one before)
    sch.check_every_policy(want)


@pytest.mark.parametrize("stage,feed", [(1, "resident"), (1, "per_replay"), (2, "resident"), (2, "per_replay")])
def test_overlapped_tail_under_every_policy(dev, stage, feed):
    """cases 3, 4 and 5: build_program(overlap_tail=True) -- the three replays are ONE schedule with no join in between,
    only the cross-replay slots keep replay r + 1's locked-backbone forward off replay r's tail.  ``per_replay``:
    set_batch(batches[r]) is a host node in front of replay r that orders behind the side lane only where the net says
    its inputs are NOT free of the tail (stage 2); in stage 1 "main lane first" lands the new inputs before the previous
    tail has run, which is what _inputs_free_of_tail() promises is harmless."""
    per_replay = feed == "per_replay"
    batches = [O.synthetic_batch(B, S, seed=700 + t) for t in range(R if per_replay else 1)]
    make = lambda: train_net(dev, stage, 21)
    want = eager_reference(dev, make, batches, per_replay)
    net = make()
    net.set_batch(batches[0])
    net.build_program(det_thresh=THRESH, overlap_tail=True)
    assert net._overlap
    # would set_batch join a tail that is open?  (asked of the recorded net; the executor itself never leaves one open)
    net._tail_open = True
    host_joins = not net._inputs_free_of_tail()
    net._tail_open = False
    assert host_joins == (stage == 2)
    sch = Scheduled(net, batches, per_replay, host_joins=host_joins)
    assert sorted(sch.graph.lanes) == [0, 1]
    ahead = overlap_run_ahead(sch.graph)
    if stage == 1:
        # otherwise the case would test nothing about the slots
        assert ahead > 0, "no launch of a replay is scheduled in front of the previous replay's tail"
    if per_replay:
        # main lane first: in stage 1 the new inputs land while side-lane launches of the replay before are still to run; in
        # stage 2 set_batch joins and nothing of the replay before is left
        g = sch.graph
        at = {n: p for p, n in enumerate(LO.schedule(g, LO.priority((0, 1))))}
        for host in (n for n in g.nodes if n.what == "host" and n.replay > 0):
            late = sum(1 for n in g.nodes if n.what == "launch" and n.replay == host.replay - 1 and at[n.seq] > at[host.seq])
            assert (late > 0) == (stage == 1), (host.replay, late)
    sch.check_every_policy(want, note=" (cross-replay inversions under main-lane-first: %d)" % ahead)


def test_overlapped_tail_behind_a_holed_lock_map_under_every_policy(dev):
    """case 6: _plan_overlap depends on the lock map -- conv62-64 locked behind the locked backbone"""
    batches = [O.synthetic_batch(B, S, seed=700)]
    make = lambda: train_net(dev, 1, 4, lock_map="stage1_hole")
    want = eager_reference(dev, make, batches, False)
    net = make()
    net.set_batch(batches[0])
    net.build_program(det_thresh=THRESH, overlap_tail=True)
    sch = Scheduled(net, batches, False)
    ahead = overlap_run_ahead(sch.graph)
    assert ahead > 0
    sch.check_every_policy(want, note=" (cross-replay inversions under main-lane-first: %d)" % ahead)


def test_pipelined_step_under_every_policy(dev):
    """case 7: build_program(pipeline_backbone=True) after prime_pipeline, resident inputs (nothing is pending on the feed
    stream: no torch event is involved).  Three lanes -- the next batch's backbone on lane 2 -- hence all six priority
    orders; the schedule alternates the two lists, and every replay joins.  With the same batch in both input sets the
    pipelined step computes what the plain step computes (test_pipelined_backbone_step_equals_plain_step)."""
    batches = [O.synthetic_batch(B, S, seed=40)]
    make = lambda: train_net(dev, 1, 6)
    want = eager_reference(dev, make, batches, False)
    net = make()
    net.set_batch(batches[0])
    net.build_program(det_thresh=THRESH, pipeline_backbone=True)
    net.prime_pipeline()
    assert net._fed_pending == [False, False] and net._parity == 0
    sch = Scheduled(net, batches, False, reset=net.prime_pipeline)
    assert sch.progs[0] is net._progs[0][0] and sch.progs[1] is net._progs[1][0] and sch.progs[2] is sch.progs[0]
    assert sorted(sch.graph.lanes) == [0, 1, 2]
    sch.check_every_policy(want)
    assert net._parity == R % 2


def test_inference_list_under_every_policy(dev):
    """case 8: build_infer_program(graph=False), whose head branches run on lane 1 -- logits, score maps, detections,
    counts, kept flags and assembled masks of every policy against the eager forward + assembly of a twin"""
    batch = O.synthetic_batch(B, S, seed=3)

    def make():
        net = YOLONet(training=False, device=dev, image_size=S, batch_size=B, stage=1, seed=0)
        g = torch.Generator().manual_seed(7919)
        with torch.no_grad():                       # heads that produce non-trivial logits / detections
            for i in (59, 67, 75, 82):
                net.params["yolo/convolutional%d/weights" % i].mul_(6.0)
                b = net.params["yolo/convolutional%d/biases" % i]
                b.copy_((torch.randn(b.shape, generator=g) * 0.5).to(b.device))
        net.refresh_weights()
        return net

    def outputs(net):
        torch.cuda.synchronize()
        out = {"logits%d" % i: net.by_idx[i].act for i in (75, 67, 59)}
        out.update(score=net.by_idx[net.score_layer].act, detections=net.detections, det_count=net.det_count, keep=net.keep,
                   masks=net.masks)
        return {k: v.detach().clone() for k, v in out.items()}

    ref = make()
    ref.evaluation_device(batch["images"], batch["clip_window"], THRESH)
    want = outputs(ref)
    assert int(want["keep"].sum()) > 0 and float(want["masks"].abs().sum()) > 0
    net = make()
    net.build_infer_program(det_thresh=THRESH, graph=False)
    prog = net._infer_prog
    n_rep = 2
    graph = LO.Graph([LO.Replay(prog.describe(), True, True) for _ in range(n_rep)])
    assert sorted(graph.lanes) == [0, 1]
    # every head branch is recorded right behind the sync that releases it, and every replay joins: the recorded order is
    # the side-lane-first order itself
    check_extremes_differ(graph, recorded_is_side_first=True)
    for pol in policies_of(graph):
        order = LO.schedule(graph, pol)
        check_schedule(order, graph, pol)
        net._set_inputs(batch["images"], batch["clip_window"])
        for t in (net.detections, net.det_count, net.keep, net.masks) + tuple(net.by_idx[i].act for i in (75, 67, 59, net.score_layer)):
            t.zero_()                               # (nothing of the policy before is left to agree by accident)
        LO.execute(order, graph, [prog] * n_rep)
        diff = first_difference(outputs(net), want)
        assert diff is None, "policy %s: %s differs from the eager forward" % (LO.policy_name(pol), diff)

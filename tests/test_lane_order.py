"""tests/lane_order.py on the CPU: the happens-before model of the command-list executor against hand-written lists with
known answers, the two-lane exhaustiveness claim that tests/test_gpu_lane_order.py rests on (by brute force), and the
round trip of ``disyolo_cmdlist_describe`` through a list recorded without a device."""
import random

import pytest

import lane_order as LO
from lane_order import LAUNCH, SYNC, MARK, WAIT, MARK_SLOT, WAIT_SLOT

launch = lambda lane: (LAUNCH, lane, 0, 0)
sync = lambda src, dst: (SYNC, 0, src, dst)
mark = lambda lane: (MARK, 0, lane, 0)
wait = lambda index, lane: (WAIT, 0, index, lane)
mark_slot = lambda lane, slot: (MARK_SLOT, 0, lane, slot)
wait_slot = lambda slot, lane: (WAIT_SLOT, 0, slot, lane)


def graph_of(cmds, replays=1, fork=False, join=False):
    return LO.Graph([LO.Replay(cmds, fork, join) for _ in range(replays)])


def at(graph, order, replay, index, what=None):
    """position in ``order`` of the node of command ``index`` of ``replay`` (``what`` picks a half of a sync)"""
    hits = [p for p, n in enumerate(order) if graph.nodes[n].replay == replay and graph.nodes[n].index == index
            and (what is None or graph.nodes[n].what == what)]
    assert len(hits) == 1, hits
    return hits[0]


def test_two_lanes_without_an_edge_run_one_after_the_other_under_a_priority():
    cmds = [launch(0), launch(1), launch(0), launch(1), launch(1), launch(0)]
    g = graph_of(cmds)
    lane_of = lambda order: [g.nodes[n].lane for n in order]
    assert lane_of(LO.schedule(g, LO.priority((0, 1)))) == [0, 0, 0, 1, 1, 1]
    assert lane_of(LO.schedule(g, LO.priority((1, 0)))) == [1, 1, 1, 0, 0, 0]
    assert LO.schedule(g, LO.recorded()) == list(range(6))
    assert lane_of(LO.schedule(g, LO.recorded())) == [0, 1, 0, 1, 1, 0]
    for s in range(8):
        o = LO.schedule(g, LO.random(s))
        assert LO.is_legal(o, g) and o == LO.schedule(g, LO.random(s))          # (seeded: a failure can be replayed)
    assert len({tuple(LO.schedule(g, LO.random(s))) for s in range(8)}) > 1
    with pytest.raises(ValueError):
        LO.schedule(g, LO.priority((0, 2)))


def test_a_sync_forces_the_order():
    # lane 1 produces, lane 0 consumes behind sync(1, 0): no policy may run the consumer first
    cmds = [launch(1), launch(1), sync(1, 0), launch(0), launch(1)]
    g = graph_of(cmds)
    for pol in LO.all_policies(g):
        o = LO.schedule(g, pol)
        assert LO.is_legal(o, g)
        assert at(g, o, 0, 1) < at(g, o, 0, 2, "record") < at(g, o, 0, 2, "wait") < at(g, o, 0, 3), pol
    # ... and the main lane waits for nothing recorded BEHIND the sync: with the main lane first, command 4 runs last
    o = LO.schedule(g, LO.priority((0, 1)))
    assert at(g, o, 0, 3) < at(g, o, 0, 4)
    # the other direction: lane 1 waits for lane 0
    g = graph_of([launch(0), sync(0, 1), launch(1), launch(0)])
    o = LO.schedule(g, LO.priority((1, 0)))
    assert [(g.nodes[n].index, g.nodes[n].what) for n in o] == [(0, "launch"), (1, "record"), (1, "wait"), (2, "launch"), (3, "launch")]


def test_a_wait_waits_for_its_mark_only():
    # lane 1: a, mark, b.  lane 0 waits for the mark: it must follow a, and may overtake b
    cmds = [launch(1), mark(1), launch(1), wait(1, 0), launch(0)]
    g = graph_of(cmds)
    o = LO.schedule(g, LO.priority((0, 1)))
    assert at(g, o, 0, 0) < at(g, o, 0, 1) < at(g, o, 0, 3) < at(g, o, 0, 4) < at(g, o, 0, 2)
    # the same list with a sync in the wait's place: b comes first
    g2 = graph_of([launch(1), mark(1), launch(1), sync(1, 0), launch(0)])
    o2 = LO.schedule(g2, LO.priority((0, 1)))
    assert at(g2, o2, 0, 2) < at(g2, o2, 0, 4)
    for pol in LO.all_policies(g):
        assert LO.is_legal(LO.schedule(g, pol), g)


def test_a_slot_wait_in_front_of_its_mark_binds_to_the_previous_replay():
    # the shape of overlap_tail: the main lane's head waits for the slot that the side lane's tail marks at the END
    cmds = [wait_slot(3, 0), launch(0), launch(1), mark_slot(1, 3)]
    g = graph_of(cmds, replays=3)
    waits = [n for n in g.nodes if n.kind == WAIT_SLOT]
    marks = [n for n in g.nodes if n.kind == MARK_SLOT]
    assert g.deps[waits[0].seq] == []                       # first replay: slot_recorded is false, nothing is enqueued
    assert g.deps[waits[1].seq] == [marks[0].seq] and g.deps[waits[2].seq] == [marks[1].seq]
    o = LO.schedule(g, LO.priority((0, 1)))
    # the main lane runs replay 0 and stops at replay 1's wait until the side lane has finished replay 0
    assert at(g, o, 0, 1) < at(g, o, 0, 2) < at(g, o, 0, 3) < at(g, o, 1, 0) < at(g, o, 1, 1) < at(g, o, 1, 2)
    # a mark earlier in the same replay wins over the previous replay's
    g = graph_of([mark_slot(1, 3), launch(1), wait_slot(3, 0), launch(0), mark_slot(1, 3)], replays=2)
    w = [n for n in g.nodes if n.kind == WAIT_SLOT]
    m = [n for n in g.nodes if n.kind == MARK_SLOT]
    assert g.deps[w[0].seq] == [m[0].seq] and g.deps[w[1].seq] == [m[2].seq]
    # another slot is another event
    g = graph_of([mark_slot(1, 2), wait_slot(3, 0), launch(0)], replays=2)
    assert all(g.deps[n.seq] == [] for n in g.nodes if n.kind == WAIT_SLOT)


def test_fork_and_join_every_policy_is_legal_and_complete():
    cmds = [launch(0), launch(1), launch(2), sync(1, 0), launch(0), launch(2), mark(0), launch(0), wait(6, 2), launch(2)]
    g = LO.Graph([LO.Replay(cmds, True, True, (lambda: None) if r == 1 else None, r == 1) for r in range(3)])
    assert sorted(g.lanes) == [0, 1, 2]
    pols = LO.all_policies(g)
    assert len(pols) == 1 + 6 + 4
    for pol in pols:
        o = LO.schedule(g, pol)
        assert LO.is_legal(o, g), pol
        assert sorted(o) == list(range(len(g.nodes)))
        issued = [(g.nodes[n].replay, g.nodes[n].index) for n in o if LO.issues_command(g.nodes[n])]
        assert sorted(issued) == [(r, i) for r in range(3) for i in range(len(cmds))], pol
        pos = {n: p for p, n in enumerate(o)}
        for r in range(3):
            nodes = [n for n in g.nodes if n.replay == r]
            join = [n for n in nodes if n.what == "join"]
            forks = [n for n in nodes if n.what == "fork"]
            assert len(join) == 1 and sorted(f.lane for f in forks) == [1, 2]
            # join: behind everything of this replay and the ones before; fork: behind lane 0's part of the replays before
            assert all(pos[n.seq] < pos[join[0].seq] for n in g.nodes if n.replay <= r and n.seq != join[0].seq)
            for f in forks:
                assert all(pos[n.seq] < pos[f.seq] for n in g.nodes if n.lane == 0 and n.seq < f.seq)
        host = [n for n in g.nodes if n.what == "host"]
        assert len(host) == 1 and all(pos[n.seq] < pos[host[0].seq] for n in g.nodes if n.replay == 0)
    # without a join the side lanes' tails may run into the next replay: the main lane first puts replay 1 in front of them
    g = LO.Graph([LO.Replay([launch(0), launch(1), launch(1)], True, False) for _ in range(2)])
    o = LO.schedule(g, LO.priority((0, 1)))
    assert at(g, o, 1, 0) < at(g, o, 0, 1) and LO.cross_replay_inversions(o, g) == 2
    assert LO.cross_replay_inversions(LO.schedule(g, LO.recorded()), g) == 0
    # a host node that does not join stays where lane 0 has it; one that joins waits for the side lane
    for joins, first in ((False, "host"), (True, "launch")):
        g = LO.Graph([LO.Replay([launch(1)], False, False), LO.Replay([launch(0)], False, False, lambda: None, joins)])
        assert g.nodes[LO.schedule(g, LO.priority((0, 1)))[0]].what == first


def test_illegal_orders_are_rejected():
    cmds = [launch(1), sync(1, 0), launch(0), mark(0), launch(0), wait(3, 1), launch(1)]
    g = graph_of(cmds, fork=True, join=True)
    good = LO.schedule(g, LO.recorded())
    assert good == list(range(len(g.nodes))) and LO.is_legal(good, g)
    name = lambda n: (g.nodes[n].index, g.nodes[n].what)
    pos = {name(n): p for p, n in enumerate(good)}

    def swapped(a, b):
        o = list(good)
        o[pos[a]], o[pos[b]] = o[pos[b]], o[pos[a]]
        return o
    assert not LO.is_legal(swapped((1, "record"), (1, "wait")), g)            # a wait in front of its own record
    assert not LO.is_legal(swapped((0, "launch"), (2, "launch")), g)          # the consumer in front of the producer
    assert not LO.is_legal(swapped((2, "launch"), (4, "launch")), g)          # lane 0 out of FIFO order
    assert not LO.is_legal(swapped((3, "record"), (5, "wait")), g)            # a wait in front of its mark
    assert not LO.is_legal(swapped((None, "fork"), (0, "launch")), g)         # the side lane in front of its fork
    assert not LO.is_legal(swapped((None, "join"), (6, "launch")), g)         # the join in front of the side lane's end
    assert not LO.is_legal(good[:-1], g) and not LO.is_legal(good + [good[0]], g)      # a node missing, a node twice
    assert not LO.is_legal(good[:-1] + [good[0]], g)
    # every hybrid of a legal order and the recorded one is legal (what a failing GPU case bisects over)
    for pol in LO.all_policies(g):
        o = LO.schedule(g, pol)
        assert LO.hybrid(o, 0, g) == good and LO.hybrid(o, len(o), g) == o
        assert all(LO.is_legal(LO.hybrid(o, k, g), g) for k in range(len(o) + 1))
    # swapping two nodes that nothing orders stays legal: (4, launch) on lane 0 and (5, wait) on lane 1
    assert LO.is_legal(swapped((4, "launch"), (5, "wait")), g)


def test_an_unsatisfiable_wait_raises():
    # lane 0 waits for a mark that lane 1 makes behind a wait for lane 0's NEXT command: neither head can ever go
    g = graph_of([wait(2, 0), sync(0, 1), mark(1)])
    for pol in LO.all_policies(g):
        with pytest.raises(LO.OrderError):
            LO.schedule(g, pol)
    assert list(LO.linearisations(g)) == []
    with pytest.raises(LO.OrderError):
        graph_of([launch(0), wait(0, 1)])                   # what it waits for is not a mark
    with pytest.raises(LO.OrderError):
        graph_of([wait(5, 1)])
    with pytest.raises(LO.OrderError):
        graph_of([sync(1, 1)])


def random_two_lane_list(rng):
    """what the recorder accepts: up to 10 commands on lanes 0 and 1, waits for marks made earlier"""
    cmds, marks = [], []
    for i in range(rng.randint(2, 10)):
        k = rng.choice((LAUNCH, LAUNCH, LAUNCH, SYNC, MARK, WAIT, MARK_SLOT, WAIT_SLOT))
        a = rng.randint(0, 1)
        if k == WAIT and not marks:
            k = LAUNCH
        if k == LAUNCH:
            cmds.append(launch(a))
        elif k == SYNC:
            cmds.append(sync(a, 1 - a))
        elif k == MARK:
            marks.append(i)
            cmds.append(mark(a))
        elif k == WAIT:
            cmds.append(wait(rng.choice(marks), a))
        elif k == MARK_SLOT:
            cmds.append(mark_slot(a, rng.randint(0, 1)))
        else:
            cmds.append(wait_slot(rng.randint(0, 1), a))
    return cmds


def test_two_priority_schedules_are_exhaustive_for_two_lanes():
    """The claim the GPU test rests on.  For nodes a on lane 0 and b on lane 1: if ANY legal linearisation runs b in front
    of a, one of the two extreme priority schedules does, and likewise for a in front of b -- so a missing producer ->
    consumer or reader -> overwriter edge between two lanes is exercised by one of two replays.  Checked against every
    legal linearisation of small random lists (one replay, forked and joined or not, and two replays without a join in
    between, where slot waits bind to the previous replay)."""
    rng = random.Random(20240611)
    lists = pairs = orders = 0
    for t in range(48):
        cmds = random_two_lane_list(rng)
        shape = t % 3
        if shape == 2:
            g = LO.Graph([LO.Replay(cmds[:5], True, False), LO.Replay(cmds[:5], True, t % 2 == 0)])
        else:
            g = graph_of(cmds, fork=shape == 1, join=shape == 1)
        if sorted(g.lanes) != [0, 1]:
            continue
        lane0, lane1 = g.lanes[0], g.lanes[1]
        b_first, a_first = set(), set()           # (a, b) that some linearisation runs as b < a / as a < b
        n_lin = 0
        for o in LO.linearisations(g):
            n_lin += 1
            pos = {n: p for p, n in enumerate(o)}
            for a in lane0:
                for b in lane1:
                    (b_first if pos[b] < pos[a] else a_first).add((a, b))
        assert n_lin >= 1
        ext = []
        for perm in ((0, 1), (1, 0)):
            o = LO.schedule(g, LO.priority(perm))
            assert LO.is_legal(o, g)
            ext.append({n: p for p, n in enumerate(o)})
        for a, b in b_first:
            assert any(pos[b] < pos[a] for pos in ext), (cmds, g.nodes[a], g.nodes[b])
        for a, b in a_first:
            assert any(pos[a] < pos[b] for pos in ext), (cmds, g.nodes[a], g.nodes[b])
        lists += 1
        pairs += len(lane0) * len(lane1)
        orders += n_lin
    print("exhaustiveness: %d lists, %d lane-0 x lane-1 node pairs, %d legal linearisations" % (lists, pairs, orders))
    assert lists >= 36 and pairs >= 500




def test_describe_round_trip_through_the_library():
    """describe() returns what was recorded and count() agrees with it.  Without a device the recorder cannot create the
    HIP event of a sync, a mark or a slot mark and refuses them, so here the list holds launches on both lanes and slot
    waits; all six kinds go through the same check on the GPU (tests/test_gpu_lane_order.py) and, with the HIP calls
    stubbed, through tools/asan_driver.cpp."""
    import torch
    LO.describe_round_trip(all_kinds=torch.cuda.is_available())
